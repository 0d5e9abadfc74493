"""`-m "not gpu"`: the scalar steps of the preconditioned conjugate-gradient operator (csrc/ks_pcg_plan.hpp through ks_host_pcg_step)
against hand-computed values, the numpy model of its recurrence (tests/pcg_model.py) on the very cases
tests/test_gpu_pcg_operator.py runs on the device -- so the bounds and counts asserted there are known to hold for the reference
alone --, and the host-only helpers of extras: grid_line_terms bit for bit against the host matrices, jacobi_preconditioner's
refusals."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import cg_cases as cc
import cg_model
import pcg_cases as cases
import pcg_model as model
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

INF, NAN = float("inf"), float("nan")
CURV, PREC, RESID = model.FAIL_CURVATURE, model.FAIL_PRECONDITIONER, model.FAIL_RESIDUAL


# ------------------------------------------------------------------------------------------------ the scalar steps
def test_host_pcg_step_hand_computed_values():
    # tau = 6, pq = 3 -> alpha = 2; rho' = 1.5 > stop; tau' = 1.5 -> beta = 0.25
    assert pkg.host_pcg_step(6.0, 3.0, 1.5, 1e-6, 1.5) == (2.0, 0.25, False, 0)
    # alpha and beta are the correctly rounded quotients, and beta is tau' / tau, not rho' / anything
    assert pkg.host_pcg_step(1.0, 3.0, 0.7, 0.0, 0.1) == (1.0 / 3.0, 0.1 / 1.0, False, 0)
    assert pkg.host_pcg_step(7.0, 3.0, 0.7, 0.0, 0.1) == (7.0 / 3.0, 0.1 / 7.0, False, 0)
    # rho' <= stop (equality included) -> done, beta = 0; one ulp above: not done
    assert pkg.host_pcg_step(6.0, 3.0, 1e-6, 1e-6, 1.5) == (2.0, 0.0, True, 0)
    assert pkg.host_pcg_step(6.0, 3.0, 5e-7, 1e-6, 1.5) == (2.0, 0.0, True, 0)
    assert pkg.host_pcg_step(6.0, 3.0, np.nextafter(1e-6, 1.0), 1e-6, 1.5) == (2.0, 0.25, False, 0)


def test_host_pcg_step_zero_residual_is_done_and_never_looks_at_the_new_tau():
    """rho' == 0 makes tau' == 0 too (z = M 0): done comes first, without a division and whatever tau' holds."""
    with np.errstate(all="raise"):
        for tau_new in (0.0, -1.0, NAN, INF, 1.5):
            assert pkg.host_pcg_step(6.0, 3.0, 0.0, 0.0, tau_new) == (2.0, 0.0, True, 0)
            assert pkg.host_pcg_step(6.0, 3.0, 0.0, 1e-30, tau_new) == (2.0, 0.0, True, 0)


@pytest.mark.parametrize("tau_new", [0.0, -0.0, -1.0, -1e-300, NAN, INF, -INF])
def test_host_pcg_step_fails_on_a_preconditioner_that_is_not_positive_and_finite(tau_new):
    """tau' == 0 with rho' > stop included: r != 0 and r^H M r == 0 is a semidefinite M.  alpha stands (r has taken the step)."""
    assert pkg.host_pcg_step(6.0, 3.0, 1.0, 1e-6, tau_new) == (2.0, 0.0, False, PREC)


def test_host_pcg_step_fails_on_a_beta_that_overflows():
    assert pkg.host_pcg_step(1e-300, 1e-300, 1.0, 1e-6, 1e300) == (1.0, 0.0, False, PREC)


@pytest.mark.parametrize("pq", [0.0, -0.0, -1.0, -1e-300, NAN, INF, -INF])
def test_host_pcg_step_fails_on_a_curvature_that_is_not_positive_and_finite(pq):
    assert pkg.host_pcg_step(6.0, pq, 1.0, 1e-6, 1.5) == (0.0, 0.0, False, CURV)
    # ... whatever the residual and the preconditioner say
    assert pkg.host_pcg_step(6.0, pq, 0.0, 1e-6, -1.0) == (0.0, 0.0, False, CURV)
    assert pkg.host_pcg_step(6.0, pq, NAN, 1e-6, 1.5) == (0.0, 0.0, False, CURV)


def test_host_pcg_step_fails_on_values_that_are_not_finite():
    assert pkg.host_pcg_step(6.0, 3.0, NAN, 1e-6, 1.5) == (0.0, 0.0, False, RESID)
    assert pkg.host_pcg_step(6.0, 3.0, INF, 1e-6, 1.5) == (0.0, 0.0, False, RESID)
    assert pkg.host_pcg_step(1e300, 1e-300, 1.0, 1e-6, 1.5) == (0.0, 0.0, False, CURV)      # alpha overflows
    assert pkg.host_pcg_step(NAN, 3.0, 1.0, 1e-6, 1.5) == (0.0, 0.0, False, CURV)
    # the residual is looked at before the preconditioner
    assert pkg.host_pcg_step(6.0, 3.0, NAN, 1e-6, -1.0) == (0.0, 0.0, False, RESID)


def test_numpy_step_is_the_library_step():
    rng = np.random.default_rng(0)
    special = [0.0, -1.0, 1.0, 1e-300, 1e300, NAN, INF, 3.0]
    quints = [tuple(rng.random(5) * 10.0 ** rng.integers(-8, 8, 5)) for _ in range(200)]
    quints += [(a, b, c, 1e-6, e) for a in special for b in special for c in special for e in special]
    for q in quints:
        want, got = model.pcg_step(*q), pkg.host_pcg_step(*q)
        assert want == got, (q, want, got)


def test_with_the_identity_the_step_is_the_conjugate_gradient_step():
    """M = I: tau = rho and tau' = rho', and (alpha, beta, done) are ks_host_cg_step's."""
    rng = np.random.default_rng(1)
    for _ in range(200):
        rho, pq, rho_new = rng.random(3) * 10.0 ** rng.integers(-6, 6, 3)
        for stop in (0.0, rho_new, 2 * rho_new):
            a, b, done, fail = pkg.host_cg_step(rho, pq, rho_new, stop)
            assert pkg.host_pcg_step(rho, pq, rho_new, stop, rho_new) == (a, b, done, int(fail))


# ------------------------------------------------------------------------------------------------ the model on the device's cases
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
@pytest.mark.parametrize("n", cc.DIAG_SIZES)
def test_diag3_takes_two_iterations_with_two_clusters_and_one_with_the_inverse(n, dtype):
    A, b, d = cc.diag3(n, dtype), cc.rhs(n, dtype), cases.diag3_entries(n)
    assert cg_model.solve(A, b, tol=cc.TOL)[1] == 3
    m2 = cases.two_cluster_diagonal(n)
    assert sorted(set(m2 * d)) == [1.0, 2.0]
    y, its, relres = model.solve(A, lambda r: m2 * r, b, tol=cc.TOL)
    print("n = %d, two clusters: relres %s" % (n, relres))
    assert its == 2 and relres[1] > 1e-3 and relres[2] < 1e-14
    assert np.linalg.norm(A @ y - b) <= 2 * cc.TOL * np.linalg.norm(b)
    y, its, relres = model.solve(A, lambda r: r / d, b, tol=cc.TOL)
    assert its == 1 and relres[1] < 1e-14
    assert np.max(np.abs(y - b / d) / np.abs(b / d)) <= 4 * np.finfo(np.float64).eps


def test_identity_preconditioner_is_conjugate_gradients():
    for A in (cc.laplace_v(), cc.mass()):
        b = cc.rhs(A.shape[0], np.float64)
        y, its, relres = model.solve(A, lambda r: r, b, tol=cc.TOL)
        y0, its0, relres0 = cg_model.solve(A, b, tol=cc.TOL)
        assert its == its0 and np.array_equal(y, y0) and relres == relres0


@pytest.fixture(scope="module")
def jump():
    c = cases.jump_coeff()
    taps, d = extras.diffusion_terms(cases.SHAPE, c, 1.0, None)
    A = pkg.host_grid_variable_matrix(cases.SHAPE, taps, c, d)
    assert np.array_equal(A.diagonal(), d) and abs(A - A.T).max() == 0
    return A, d, cc.rhs(A.shape[0], np.float64)


@pytest.fixture(scope="module")
def aniso():
    t, v = cases.aniso_terms()
    A = pkg.host_grid_matrix(cases.SHAPE, t, v)
    T = sp.diags(list(extras.grid_line_terms(cases.SHAPE, t, v)), [-1, 0, 1]).tocsc()
    return A, spl.splu(T).solve, cc.rhs(A.shape[0], np.float64)


def _recorded(case, A, M, b):
    n = A.shape[0]
    ystar = np.linalg.solve(A.toarray(), b)
    its_cg = cg_model.solve(A, b, tol=cases.TOL, maxit=5000)[1]
    counts = []
    for seed in cases.PERMUTATION_SEEDS:
        y, its, _ = model.solve(A, M, b, tol=cases.TOL, order=cases.order(n, seed))
        res, res_bound, err, err_bound = cc.bounds(A, y, ystar, b, cases.TOL)
        print("%s, order %s: %d iterations (cg %d), residual %.3g <= %.3g, error %.3g <= %.3g" % (case, seed, its, its_cg, res, res_bound, err, err_bound))
        assert res <= res_bound and err <= err_bound
        assert abs(its - cases.MODEL_ITS[case]) <= cases.band(case)
        counts.append(its)
    # the record itself: numpy's summation differs from build to build, so it is held to the band, not to equality
    assert abs(counts[0] - cases.MODEL_ITS[case]) <= cases.band(case), (counts, cases.MODEL_ITS[case])
    assert abs(its_cg - cases.CG_ITS[case]) <= max(cases.CG_ITS[case] // 20, 2), (its_cg, cases.CG_ITS[case])
    assert 3 * (cases.MODEL_ITS[case] + cases.band(case)) <= its_cg, "the preconditioner does not save two thirds of the iterations"


def test_recorded_counts_and_spread_jacobi_on_a_coefficient_jump(jump):
    A, d, b = jump
    ev = np.linalg.eigvalsh(A.toarray())
    assert ev[0] > 0 and 1e3 < ev[-1] / ev[0] < 1e4
    _recorded("jump", A, lambda r: r / d, b)


def test_a_larger_jump_moves_only_the_plain_count():
    """A jump of 1e4 in c (the figure README quotes): the Jacobi count stays within the band of the count at 100, the plain count
    almost triples.  Both are held to the record of pcg_cases like the counts of "jump"."""
    c = cases.jump_coeff(jump=cases.JUMP_HARD)
    taps, d = extras.diffusion_terms(cases.SHAPE, c, 1.0, None)
    A = pkg.host_grid_variable_matrix(cases.SHAPE, taps, c, d)
    b = cc.rhs(A.shape[0], np.float64)
    its = model.solve(A, lambda r: r / d, b, tol=cases.TOL)[1]
    its_cg = cg_model.solve(A, b, tol=cases.TOL, maxit=20000)[1]
    print("jump of %g: %d iterations, plain conjugate gradients %d" % (cases.JUMP_HARD, its, its_cg))
    assert abs(its - cases.HARD_ITS["pcg"]) <= cases.band("jump"), its
    assert abs(its_cg - cases.HARD_ITS["cg"]) <= cases.HARD_ITS["cg"] // 20, its_cg
    assert abs(its - cases.MODEL_ITS["jump"]) <= 3 and its_cg >= 2 * cases.CG_ITS["jump"]


def test_recorded_counts_and_spread_line_solve_on_an_anisotropic_grid(aniso):
    A, M, b = aniso
    assert np.linalg.eigvalsh(A.toarray())[0] > 0
    _recorded("aniso", A, M, b)
    # the diagonal alone does nothing here
    assert model.solve(A, lambda r: r / A.diagonal(), b, tol=cases.TOL)[1] > 3 * cases.MODEL_ITS["aniso"]


@pytest.mark.parametrize("shift", [-2.0])
def test_shifted_solve_with_a_preconditioner_built_for_the_shifted_operator(shift):
    A = cc.laplace_v()
    b = cc.rhs(A.shape[0], np.float64)
    d = A.diagonal() - shift
    y, its, _ = model.solve(A, lambda r: r / d, b, shift=shift, tol=cc.TOL)
    ystar = np.linalg.solve(A.toarray() - shift * np.eye(A.shape[0]), b)
    res, res_bound, err, err_bound = cc.bounds(A, y, ystar, b, cc.TOL, shift)
    assert res <= res_bound and err <= err_bound


def test_model_reports_both_kinds_of_indefiniteness_and_a_zero_right_hand_side():
    A, b = cc.indefinite(37)
    with pytest.raises(model.NotPositiveDefinite, match="at iteration 1"):
        model.solve(A, lambda r: r, b, tol=cc.TOL)
    with pytest.raises(model.PreconditionerNotPositiveDefinite, match="at iteration 0"):
        model.solve(cc.diag3(37), lambda r: -r, cc.rhs(37, np.float64), tol=cc.TOL)
    y, its, relres = model.solve(cc.diag3(37), lambda r: r, np.zeros(37), tol=cc.TOL)
    assert its == 0 and not y.any()
    with pytest.raises(model.DidNotConverge):
        model.solve(cc.mass(), lambda r: r, cc.rhs(cc.size(cc.MASS_SHAPE), np.float64), tol=cc.TOL, maxit=2)


# ------------------------------------------------------------------------------------------------ extras, host only
def _diagonals(H):
    return H.diagonal(-1), H.diagonal(0), H.diagonal(1)


LINE_SHAPES = [(7,), (1,), (5, 4), (3, 1), (4, 3, 2), (12, 10, 8)]
LINE_CASES = [(s, p) for s in LINE_SHAPES for p in (False, True) if not p or s[0] >= 3]   # (a periodic axis needs three points)


@pytest.mark.parametrize("shape, periodic_x", LINE_CASES, ids=["%s-%s" % ("x".join(map(str, s)), "periodic-x" if p else "open") for s, p in LINE_CASES])
@pytest.mark.parametrize("variable", [False, True], ids=["const", "variable"])
def test_grid_line_terms_are_the_bits_of_the_host_matrix(shape, periodic_x, variable):
    ndim, n = len(shape), cc.size(shape)
    rng = np.random.default_rng(5 + n)
    taps, v, c = rng.random(2 * ndim + 1) - 0.5, rng.random(n), rng.random(n) + 0.5
    per = tuple([True] + [False] * (ndim - 1)) if periodic_x else None
    for pot in (v, None):
        if variable:
            H = pkg.host_grid_variable_matrix(shape, taps, c, pot, periodic=per)
            got = extras.grid_line_terms(shape, taps, pot, coeff=c)
        else:
            H = pkg.host_grid_matrix(shape, taps, pot, periodic=per)
            got = extras.grid_line_terms(shape, taps, pot)
        for g, w in zip(got, _diagonals(H)):
            assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), np.ascontiguousarray(w).view(np.uint64))
        # the lines do not touch
        ends = np.arange(shape[0] - 1, n - 1, shape[0])
        assert not got[0][ends].any() and not got[2][ends].any()
    # the shift goes to the main diagonal only, as one subtraction from the matrix entry
    base = extras.grid_line_terms(shape, taps, v, coeff=c if variable else None)
    sh = extras.grid_line_terms(shape, taps, v, coeff=c if variable else None, shift=0.3)
    assert np.array_equal(sh[0], base[0]) and np.array_equal(sh[2], base[2]) and np.array_equal(sh[1], base[1] - 0.3)


def test_grid_line_terms_complex_taps_and_refusals():
    shape = (4, 3)
    t = np.array([-1.0, -1.0 + 0.5j, 4.0, -1.0 - 0.5j, -1.0])
    H = pkg.host_grid_matrix(shape, t)
    got = extras.grid_line_terms(shape, t)
    for g, w in zip(got, _diagonals(H)):
        assert g.dtype == np.complex128 and np.array_equal(g, w)
    with pytest.raises(pkg.DimensionMismatch):
        extras.grid_line_terms(shape, t[:3])
    with pytest.raises(pkg.ArgumentError):
        extras.grid_line_terms((4, 0), t)
    with pytest.raises(pkg.ArgumentError, match="shift"):
        extras.grid_line_terms(shape, t, shift=NAN)
    with pytest.raises(pkg.DimensionMismatch):
        extras.grid_line_terms(shape, t.real, coeff=np.ones(5))


@pytest.mark.parametrize("diagonal, shift", [([1.0, 2.0, 0.0], 0.0), ([1.0, 2.0, 3.0], 1.0), ([1.0, -2.0, 3.0], 0.0), ([1.0, NAN, 3.0], 0.0),
                                             ([1.0, INF, 3.0], 0.0), ([1.0, 2.0], 5.0)])
def test_jacobi_preconditioner_refuses_a_diagonal_that_is_not_positive(diagonal, shift):
    with pytest.raises(pkg.ArgumentError, match="must be positive and finite"):
        extras.jacobi_preconditioner(diagonal, shift=shift)


def test_jacobi_preconditioner_refuses_malformed_input():
    with pytest.raises(pkg.ArgumentError, match="1-D"):
        extras.jacobi_preconditioner(np.ones((2, 2)))
    with pytest.raises(pkg.ArgumentError, match="shift"):
        extras.jacobi_preconditioner([1.0, 2.0], shift=INF)
    with pytest.raises(pkg.ArgumentError, match="real"):
        extras.jacobi_preconditioner(np.array([1.0 + 1j, 2.0]))
    with pytest.raises(pkg.ArgumentError):
        extras.jacobi_preconditioner(["a", "b"])


def test_diagonal_operator_refuses_without_a_device():
    with pytest.raises(pkg.ArgumentError, match="finite"):
        pkg.diagonal_operator([1.0, NAN], ctx=object())
    with pytest.raises(pkg.ArgumentError, match="1-D"):
        pkg.diagonal_operator(np.ones((2, 2)), ctx=object())
    with pytest.raises(pkg.ArgumentError, match="real"):
        pkg.diagonal_operator(np.array([1j, 2.0]), ctx=object())
    with pytest.raises(pkg.ArgumentError):
        pkg.pcg_operator(sp.identity(3), sp.identity(3))


def test_the_new_entries_are_declared_and_exported():
    for sym, nargs in (("ks_operator_pcg", 8), ("ks_operator_pcg_info", 8), ("ks_operator_diagonal", 5), ("ks_host_pcg_step", 9)):
        assert len(pkg._lib.PROTOTYPES[sym]) == nargs and hasattr(pkg._lib.load(), sym)
    assert math.isfinite(cases.TOL)
