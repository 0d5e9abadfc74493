"""`-m "not gpu"`: the scalar steps of the BiCGStab(2) operator (csrc/ks_bicgstab_plan.hpp through ks_host_bicgstab_coef and
ks_host_bicgstab_mr) against hand-computed values and against the numpy steps, and the numpy model of the recurrence
(tests/bicgstab_model.py) on the very cases tests/test_gpu_bicgstab_operator.py runs on the device -- so the bounds asserted there
are known to hold for the reference alone, and the band its iteration counts get is measured here (tests/bicgstab_cases.py)."""
import numpy as np
import pytest

import bicgstab_cases as cases
import bicgstab_model as model
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

INF, NAN = float("inf"), float("nan")
TOL = cases.TOL


# ------------------------------------------------------------------------------------------------ the scalar steps
def test_host_coef_real_by_hand():
    """rho0 = 4, rho1 = 6, alpha = 0.5, gamma = 8: beta = 0.5 * 6 / 4 = 0.75, alpha' = 6 / 8 = 0.75 (all exact)."""
    assert pkg.host_bicgstab_coef(4.0, 6.0, 0.5, 8.0) == (0.75, 0.75, 0)
    # the first iteration: rho0 = -1, alpha = 0 -> beta = -0 (u0 is not read), alpha' = rho1 / gamma
    beta, alpha, fail = pkg.host_bicgstab_coef(-1.0, 10.0, 0.0, 4.0)
    assert (beta, alpha, fail) == (0.0, 2.5, 0)
    # the two calls of a kernel: beta with gamma = 1, alpha' with rho0 = 1 and alpha = 0
    assert pkg.host_bicgstab_coef(4.0, 6.0, 0.5, 1.0)[0] == 0.75 and pkg.host_bicgstab_coef(1.0, 6.0, 0.0, 8.0)[1:] == (0.75, 0)
    assert isinstance(beta, float)


def test_host_coef_complex_by_hand():
    """alpha rho1 = (1 + i)(2 - i) = 3 + i; / rho0 = 2i: (3 + i)(-2i) / 4 = (2 - 6i) / 4 = 0.5 - 1.5i.
    alpha' = rho1 / gamma = (2 - i) / (1 + i) = (2 - i)(1 - i) / 2 = (1 - 3i) / 2."""
    beta, alpha, fail = pkg.host_bicgstab_coef(2.0j, 2.0 - 1.0j, 1.0 + 1.0j, 1.0 + 1.0j)
    assert (beta, alpha, fail) == (0.5 - 1.5j, 0.5 - 1.5j, 0)
    # complex arithmetic on real values gives the real result in the real part
    assert pkg.host_bicgstab_coef(4.0, 6.0, 0.5, 8.0, complex_scalars=True) == (0.75 + 0j, 0.75 + 0j, 0)


@pytest.mark.parametrize("rho0", [0.0, -0.0, NAN, INF, -INF])
def test_host_coef_breaks_down_on_rho(rho0):
    assert pkg.host_bicgstab_coef(rho0, 6.0, 0.5, 8.0) == (0.0, 0.0, 1)
    assert pkg.host_bicgstab_coef(complex(rho0, 0.0), 6.0, 0.5, 8.0) == (0j, 0j, 1)
    assert model.bicg_coef(rho0, 6.0, 0.5, 8.0)[2] == 1 and model.bicg_coef(complex(rho0, 0.0), 6.0, 0.5, 8.0)[2] == 1


def test_host_coef_breaks_down_on_a_rho1_or_alpha_that_is_not_finite():
    for rho1, alpha in ((NAN, 0.5), (INF, 0.5), (6.0, NAN), (1e308, 1e308)):
        assert pkg.host_bicgstab_coef(4.0, rho1, alpha, 8.0)[2] == 1, (rho1, alpha)
        assert model.bicg_coef(4.0, rho1, alpha, 8.0)[2] == 1
    assert pkg.host_bicgstab_coef(4.0, complex(1.0, NAN), 0.5, 8.0)[2] == 1


@pytest.mark.parametrize("gamma", [0.0, -0.0, NAN, INF, -INF, 0j, complex(0.0, NAN), complex(INF, 1.0)])
def test_host_coef_breaks_down_on_gamma(gamma):
    beta, alpha, fail = pkg.host_bicgstab_coef(4.0, 6.0, 0.5, gamma)
    assert beta == 0.75 and alpha == 0 and fail == 2
    assert model.bicg_coef(4.0, 6.0, 0.5, gamma)[2] == 2
    # an alpha' that overflows
    assert pkg.host_bicgstab_coef(1.0, 1e308, 0.0, 1e-10)[2] == 2


def test_host_mr_real_by_hand():
    """G = [4 1; 1 3], h = (9, 5): det = 11, g1 = (3 * 9 - 1 * 5) / 11 = 2, g2 = (4 * 5 - 1 * 9) / 11 = 1."""
    assert pkg.host_bicgstab_mr(4.0, 3.0, 1.0, 9.0, 5.0) == (2.0, 1.0, 11.0, 0)
    # a diagonal G: two independent quotients
    assert pkg.host_bicgstab_mr(4.0, 8.0, 0.0, 2.0, 2.0) == (0.5, 0.25, 32.0, 0)


def test_host_mr_complex_by_hand():
    """G = [2 i; -i 1] (Hermitian, det = 2 - 1 = 1), g = (1 + i, 2): h1 = 2 (1 + i) + 2 i = 2 + 4 i, h2 = -i (1 + i) + 2 = 3 - i."""
    g1, g2, det, fail = pkg.host_bicgstab_mr(2.0, 1.0, 1.0j, 2.0 + 4.0j, 3.0 - 1.0j)
    assert (g1, g2, det, fail) == (1.0 + 1.0j, 2.0 + 0.0j, 1.0, 0)


def test_host_mr_determinant_is_one_fused_multiply_add():
    """g11 g22 - g12^2 with g11 = g22 = 1 + 2^-30 and g12 = 1: the product 1 + 2^-29 + 2^-60 is not a double; the fused form keeps
    the 2^-60, two roundings lose it."""
    a = 1.0 + 2.0 ** -30
    det = pkg.host_bicgstab_mr(a, a, 1.0, 1.0, 1.0)[2]
    assert det == 2.0 ** -29 + 2.0 ** -60 and a * a - 1.0 == 2.0 ** -29


@pytest.mark.parametrize("g", [(1.0, 1.0, 1.0), (4.0, 1.0, 2.0), (0.0, 0.0, 0.0), (NAN, 1.0, 0.0), (1.0, INF, 0.0), (1.0, 1.0, NAN), (1e200, 1e200, 0.0)])
def test_host_mr_breaks_down_on_a_singular_or_not_finite_g(g):
    g11, g22, g12 = g
    g1, g2, det, fail = pkg.host_bicgstab_mr(g11, g22, g12, 1.0, 1.0)
    assert (g1, g2, fail) == (0.0, 0.0, 1) and (det == 0.0 or not np.isfinite(det))
    assert model.mr_solve(g11, g22, g12, 1.0, 1.0)[3] == 1
    g1, g2, det, fail = pkg.host_bicgstab_mr(g11, g22, complex(g12, 0.0), 1.0j, 1.0)
    assert (g1, g2, fail) == (0j, 0j, 1)
    # a right-hand side that is not finite
    assert pkg.host_bicgstab_mr(4.0, 3.0, 1.0, NAN, 5.0)[3] == 1 and pkg.host_bicgstab_mr(4.0, 3.0, 1.0j, 1.0, complex(INF, 0.0))[3] == 1


def _close(a, b, scale):
    return abs(a - b) <= 4 * np.spacing(scale)


def test_numpy_steps_are_the_library_steps_within_4_ulp():
    """2 000 random inputs, real and complex: the library's steps (explicit fma, a conj(b) / |b|^2 for a complex quotient) against
    numpy's.  beta and alpha' are products and quotients: 4 ulp of the result's modulus.  g1 and g2 are differences that may cancel:
    4 ulp of the larger term over |det|, with a G whose determinant is at least a tenth of g11 g22."""
    rng = np.random.default_rng(0)
    for trial in range(2000):
        cplx = trial % 2 == 1
        draw = (lambda: complex(*(rng.random(2) - 0.5))) if cplx else (lambda: float(rng.random() - 0.5))
        rho0, rho1, alpha, gamma = (draw() * 10.0 ** rng.integers(-3, 4) for _ in range(4))
        want, got = model.bicg_coef(rho0, rho1, alpha, gamma), pkg.host_bicgstab_coef(rho0, rho1, alpha, gamma)
        assert want[2] == 0 and got[2] == 0
        assert _close(want[0], got[0], abs(want[0])) and _close(want[1], got[1], abs(want[1])), (rho0, rho1, alpha, gamma, want, got)
        g11, g22 = rng.random(2) + 0.5
        g12 = draw() * 1.3 * np.sqrt(g11 * g22)      # |g12|^2 <= 0.85 g11 g22 (real: 0.43)
        h1, h2 = draw(), draw()
        want, got = model.mr_solve(g11, g22, g12, h1, h2), pkg.host_bicgstab_mr(g11, g22, g12, h1, h2)
        assert want[3] == 0 and got[3] == 0 and _close(want[2], got[2], g11 * g22)
        for j, terms in ((0, (g22 * abs(h1), abs(g12) * abs(h2))), (1, (g11 * abs(h2), abs(g12) * abs(h1)))):
            # (the determinants differ by 4 ulp of g11 g22 at most: that relative change of the quotient comes on top)
            scale = max(terms) / abs(want[2]) + abs(want[j]) * g11 * g22 / abs(want[2])
            assert _close(want[j], got[j], scale), (g11, g22, g12, h1, h2, want, got)


# ------------------------------------------------------------------------------------------------ the model on the device's cases
@pytest.mark.parametrize("case", list(cases.SOLVES))
def test_model_holds_the_bounds_and_permutations_record_the_spread(case):
    """The model on every case of the device's solve test, in every ordering: the recurrence's residual below tol, the TRUE residual
    below 1.25 tol ||b|| (a condition on the inputs: no residual replacement, so a case whose true residual drifts further does not
    belong here), the count within the band of the recorded one -- and the same record whether the stage tests fire where the
    recurrence states them or late, where a kernel that derives them from partial sums sees them."""
    A, b, shift = cases.host_case(case)
    assert abs(A - A.conj().T).max() > 0.1      # not Hermitian
    counts, worst = [], 0.0
    for seed in cases.PERMUTATION_SEEDS:
        Ap, bp = cases.permuted(A, b, seed)
        y, its, stage, relres = model.solve(Ap, bp, shift=shift, tol=TOL)
        y2, its2, stage2, relres2 = model.solve(Ap, bp, shift=shift, tol=TOL, late_stage_tests=True)
        assert (its2, stage2, relres2) == (its, stage, relres) and np.array_equal(y, y2)
        assert relres[-1] <= TOL and stage in (1, 2, 3)
        res = cases.true_residual(Ap, y, bp, shift)
        worst = max(worst, res / (TOL * np.linalg.norm(b)))
        assert res <= 1.25 * TOL * np.linalg.norm(b), (case, seed, res)
        counts.append(its)
    print("%s: counts under %s = %s, spread %d (recorded %s, spread %d), band %d, worst true residual %.3f tol ||b||" %
          (case, cases.PERMUTATION_SEEDS, counts, max(counts) - min(counts), cases.PERMUTED_ITS[case], cases.SPREAD[case], cases.band(case), worst))
    for its in counts:
        assert abs(its - cases.MODEL_ITS[case]) <= cases.band(case), (case, counts)


def test_recorded_spreads_give_the_bands_the_device_test_uses():
    assert set(cases.MODEL_ITS) == set(cases.PERMUTED_ITS) == set(cases.SOLVES)
    for case, counts in cases.PERMUTED_ITS.items():
        assert counts[0] == cases.MODEL_ITS[case] and len(counts) == len(cases.PERMUTATION_SEEDS)
    assert cases.band("swirl-2.0") == 4 and cases.band("convdiff-c64") == 10 and cases.band("convdiff-0") == 2


def test_the_test_operators_are_what_their_names_say():
    ev = np.linalg.eigvals(cases.grid_matrix("convdiff").toarray())
    assert np.abs(ev.imag).max() < 1e-9 and abs(ev.real.min() - 1.0436) < 1e-4 and abs(ev.real.max() - 11.99) < 1e-2
    ev = np.linalg.eigvals(cases.grid_matrix("swirl").toarray())
    assert abs(np.abs(ev.imag).max() - 2.42) < 1e-2 and abs(ev.real.min() - 2.81) < 1e-2
    # the library's host matrix is the same matrix
    H = pkg.host_grid_matrix(cases.SHAPE, cases.taps("swirl"), cases.V)
    assert abs(H - cases.grid_matrix("swirl")).max() == 0


def test_twice_the_identity_ends_in_the_half_step():
    """A = 2 I: alpha = 1/2 exactly, r0 = b - b = 0 after the first BiCG step; everything behind it would be 0 / 0."""
    b = cases.rhs(37, np.float64)
    y, its, stage, relres = model.solve(2.0 * np.eye(37), b, tol=TOL)
    assert (its, stage, relres[-1]) == (1, 1, 0.0) and np.array_equal(y, b / 2)
    y, its, stage, relres = model.solve(2.0 * np.eye(37), b, tol=TOL, late_stage_tests=True)
    assert (its, stage, relres[-1]) == (1, 1, 0.0) and np.array_equal(y, b / 2)


@pytest.mark.parametrize("n", cases.DIAG_SIZES)
@pytest.mark.parametrize("values,dtype", [(cases.THREE, np.float64), (cases.THREE, np.complex128), (cases.THREE_C, np.complex128)],
                         ids=["three-f64", "three-c64", "complex-c64"])
def test_three_eigenvalues_end_within_eight_iterations(values, dtype, n):
    """Three distinct eigenvalues: BiCGStab(2) ends in the second iteration in exact arithmetic.  Finite termination is not exact
    in floating point: an upper bound only."""
    A, b = cases.cyclic_diag(values, n, dtype), cases.rhs(n, dtype)
    y, its, stage, relres = model.solve(A, b, tol=TOL)
    print("n = %d: %d iterations, stage %d, relres %s" % (n, its, stage, relres))
    assert its <= cases.DIAG_MAX_ITS and relres[-1] <= TOL
    assert cases.true_residual(A, y, b) <= 1.25 * TOL * np.linalg.norm(b)


def test_model_reports_failures():
    b = cases.rhs(8, np.float64)
    y, its, stage, relres = model.solve(np.eye(8), np.zeros(8), tol=TOL)
    assert its == 0 and stage == 0 and not y.any()
    with pytest.raises(model.Breakdown, match="gamma = 0.0 at iteration 1"):
        model.solve(np.eye(8), b, shift=1.0, tol=TOL)
    with pytest.raises(model.NotFinite):
        model.solve(np.eye(8), np.array([1.0, NAN] + [0.0] * 6), tol=TOL)
    A, bb, shift = cases.host_case("swirl-2.0")
    with pytest.raises(model.DidNotConverge, match="after 2 iterations"):
        model.solve(A, bb, shift=shift, tol=TOL, maxit=2)


def test_interior_eigenvalues_maps_complex_pairs_and_complex_shifts():
    lam = np.array([2.84436439 + 0.29708184j, 2.84436439 - 0.29708184j, 3.05478566 + 0.29834683j])
    mu = 1.0 / (lam - 2.0)
    got = extras.interior_eigenvalues(mu, 2.0)
    assert got.dtype == np.complex128 and np.allclose(got, lam, rtol=0, atol=1e-15)
    sigma = 2.0 + 0.5j
    assert np.allclose(extras.interior_eigenvalues(1.0 / (lam - sigma), sigma), lam, rtol=0, atol=1e-15)
    # real input stays real, bit for bit what it was
    mur = np.array([-13.2972, 9.41234])
    out = extras.interior_eigenvalues(mur, 1.2)
    assert out.dtype == np.float64 and np.array_equal(out, 1.2 + 1.0 / mur)
