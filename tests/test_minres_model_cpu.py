"""`-m "not gpu"`: the scalar step of the MINRES operator (csrc/ks_minres_plan.hpp through ks_host_minres_step) against hand-computed
values and against the numpy step, and the numpy model of the recurrence (tests/minres_model.py) on the very cases
tests/test_gpu_minres_operator.py runs on the device -- so the bounds asserted there are known to hold for the reference alone, and
the band its iteration counts get is measured here (tests/minres_cases.py)."""
import math

import numpy as np
import pytest

import cg_cases
import cg_model
import minres_cases as cases
import minres_model as model
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

INF, NAN = float("inf"), float("nan")
TOL = cases.TOL
IDENTITY = (1.0, 0.0, 1.0, 0.0)      # (c, s, c_prev, s_prev) before there is a rotation


# ------------------------------------------------------------------------------------------------ the scalar step
def test_host_minres_step_first_step_3_4_5():
    """alpha = 3, beta' = 4 under the identity rotations: gbar = 3, gamma = 5 (formed as 4 sqrt(0.75^2 + 1), exact), c' = 3/5,
    s' = 4/5, phi = c' phibar, phibar' = -s' phibar."""
    eps, delta, gamma, c, s, phi, phibar, done, fail = pkg.host_minres_step(3.0, 0.0, 4.0, *IDENTITY, 10.0, 1e-12)
    assert (eps, delta, gamma, c, s) == (0.0, 0.0, 5.0, 0.6, 0.8)
    assert (phi, phibar, done, fail) == (0.6 * 10.0, -(0.8 * 10.0), False, False)
    # a later step: the column (beta, alpha) = (4, 1) through (c_, s_) = (0, 1) and (c, s) = (0.6, 0.8):
    # eps = 4, dbar = 0, delta = 0.8, gbar = 0.6, beta' = 0.8 -> gamma = 1
    eps, delta, gamma, c, s, phi, phibar, done, fail = pkg.host_minres_step(1.0, 4.0, 0.8, 0.6, 0.8, 0.0, 1.0, -8.0, 1e-12)
    assert (eps, delta, gamma, c, s) == (4.0, 0.8, 1.0, 0.6, 0.8) and (phi, phibar) == (0.6 * -8.0, 0.8 * 8.0) and not done and not fail


def test_host_minres_step_without_progress():
    """gbar = 0 (alpha = 0 in the first step): c' = 0, phi = 0, s' = 1 -- y does not move and |phibar| stays."""
    eps, delta, gamma, c, s, phi, phibar, done, fail = pkg.host_minres_step(0.0, 0.0, 1.0, *IDENTITY, 7.0, 1e-12)
    assert (gamma, c, s, phi, phibar, done, fail) == (1.0, 0.0, 1.0, 0.0, -7.0, False, False)
    # beta' = 0: s' = 0, phibar' = 0, done for every stop >= 0
    out = pkg.host_minres_step(2.0, 0.0, 0.0, *IDENTITY, 7.0, 0.0)
    assert out[2:] == (2.0, 1.0, 0.0, 7.0, 0.0, True, False) and math.copysign(1.0, out[6]) in (1.0, -1.0)
    # a negative gbar: gamma stays positive, c' carries the sign
    out = pkg.host_minres_step(-3.0, 0.0, 4.0, *IDENTITY, 10.0, 1e-12)
    assert out[2:5] == (5.0, -0.6, 0.8)


def test_host_minres_step_stops_on_the_right_side():
    """|phibar'| == stop is done, the next float above it is not.  s' = 0.8, phibar = 10: |phibar'| = fl(0.8 * 10) = 8."""
    assert pkg.host_minres_step(3.0, 0.0, 4.0, *IDENTITY, 10.0, 8.0)[7] is True
    assert pkg.host_minres_step(3.0, 0.0, 4.0, *IDENTITY, 10.0, np.nextafter(8.0, 0.0))[7] is False
    assert pkg.host_minres_step(3.0, 0.0, 4.0, *IDENTITY, -10.0, 8.0)[7] is True      # (the sign of phibar does not matter)
    assert pkg.host_minres_step(3.0, 0.0, 4.0, *IDENTITY, np.nextafter(10.0, 11.0), 8.0)[7] is False


def test_host_minres_step_gamma_does_not_overflow_early():
    big = 1e308
    eps, delta, gamma, c, s, phi, phibar, done, fail = pkg.host_minres_step(big, 0.0, big, *IDENTITY, 1.0, 1e-12)
    assert not fail and abs(gamma - math.sqrt(2.0) * big) <= 2 * np.spacing(gamma) and abs(c - math.sqrt(0.5)) <= 1e-15
    tiny = 1e-300
    out = pkg.host_minres_step(3 * tiny, 0.0, 4 * tiny, *IDENTITY, 1.0, 1e-12)
    assert not out[8] and abs(out[2] - 5 * tiny) <= np.spacing(5 * tiny) and abs(out[3] - 0.6) <= 2e-16


@pytest.mark.parametrize("alpha,beta_new", [(0.0, 0.0), (-0.0, 0.0), (NAN, 1.0), (1.0, NAN), (INF, 1.0), (-INF, 1.0), (1.0, INF), (1.7e308, 1.7e308)])
def test_host_minres_step_fails_on_a_gamma_that_is_zero_or_not_finite(alpha, beta_new):
    out = pkg.host_minres_step(alpha, 0.0, beta_new, *IDENTITY, 10.0, 1e-12)
    assert out[7] is False and out[8] is True and out[:2] == (0.0, 0.0) and out[3:7] == (0.0, 0.0, 0.0, 0.0)
    assert out[2] == 0.0 or not math.isfinite(out[2])
    assert model.minres_step(alpha, 0.0, beta_new, *IDENTITY, 10.0, 1e-12)[8] is True


def _ulps(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


def test_numpy_step_is_the_library_step_within_4_ulp():
    """3 000 random inputs with genuine rotations (c^2 + s^2 = 1): every output within 4 ulp (the library forms gamma by scaling, numpy
    by its hypot; delta and gbar are one fused multiply-add against two roundings); done and fail equal wherever |phibar'| is not
    within those ulps of stop.  delta = c dbar + s alpha and gbar = -s dbar + c alpha are the two rows of one rotation, so for any
    signs one of them is a difference that may cancel: alpha takes the sign that makes gbar a sum (everything downstream depends on
    gbar), and delta, the difference, is held to 4 ulp of its larger term, the only scale a cancelling sum has."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(3000):
        th, th2 = rng.random(2) * 0.5 * np.pi
        sgn = 1.0 if rng.random() < 0.5 else -1.0
        c, s, c_prev, s_prev = math.cos(th), sgn * math.sin(th), math.cos(th2), math.sin(th2)
        alpha = -sgn * (rng.random() + 0.01) * 10.0 ** rng.integers(-3, 4)
        beta, beta_new = (rng.random(2) + 0.01) * 10.0 ** rng.integers(-3, 4, 2)
        phibar = (rng.random() - 0.5) * 10.0 ** rng.integers(-12, 3)
        args = (alpha, beta, beta_new, c, s, c_prev, s_prev, phibar, 1e-6)
        want, got = model.minres_step(*args), pkg.host_minres_step(*args)
        assert got[8] is False and want[8] is False, args
        for i in range(7):
            if i == 1:
                err = abs(want[i] - got[i]) / np.spacing(max(abs(c * c_prev * beta), abs(s * alpha)))
            else:
                err = _ulps(want[i], got[i])
            worst = max(worst, err)
            assert err <= 4, (i, args, want, got)
        if abs(abs(want[6]) - 1e-6) > 8 * np.spacing(1e-6):
            assert got[7] == want[7], args
    print("largest difference: %.2f ulp" % worst)


def test_numpy_step_is_the_library_step_within_4_ulp_of_every_output_without_a_previous_column():
    """beta = 0 (dbar = eps = 0: the first iteration, under any rotation): delta = s alpha and gbar = c alpha are single products,
    nothing cancels, and all seven outputs are held to 4 ulp of themselves on 2 000 random inputs with rotations from the whole
    circle and either sign of alpha and phibar."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(2000):
        th, th2 = rng.random(2) * 2.0 * np.pi
        alpha = (rng.random() - 0.5) * 10.0 ** rng.integers(-3, 4)
        beta_new = (rng.random() + 0.01) * 10.0 ** rng.integers(-3, 4)
        phibar = (rng.random() - 0.5) * 10.0 ** rng.integers(-12, 3)
        args = (alpha, 0.0, beta_new, math.cos(th), math.sin(th), math.cos(th2), math.sin(th2), phibar, 1e-6)
        want, got = model.minres_step(*args), pkg.host_minres_step(*args)
        assert got[8] is False and want[8] is False, args
        for i in range(7):
            err = _ulps(want[i], got[i])
            worst = max(worst, err)
            assert err <= 4, (i, args, want, got)
        if abs(abs(want[6]) - 1e-6) > 8 * np.spacing(1e-6):
            assert got[7] == want[7], args
    print("largest difference: %.2f ulp" % worst)


# ------------------------------------------------------------------------------------------------ the model on the device's cases
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
@pytest.mark.parametrize("n", cases.DIAG_SIZES)
@pytest.mark.parametrize("values", [cases.THREE, cases.FIVE], ids=["three", "five"])
def test_distinct_eigenvalues_take_exactly_that_many_iterations(values, n, dtype):
    A, b = cases.cyclic_diag(values, n, dtype), cg_cases.rhs(n, dtype)
    y, its, relres = model.solve(A, b, tol=TOL)
    # (the count says that relres[-2] > tol >= relres[-1]; how far the last step undershoots is a rounding residue that depends on
    # how the dot products are split, printed only)
    print("n = %d: relres %s" % (n, relres))
    assert its == len(values) and relres[-2] > TOL >= relres[-1]
    assert np.linalg.norm(A @ y - b) <= 2 * TOL * np.linalg.norm(b)


@pytest.mark.parametrize("n", cases.PM_SIZES)
def test_a_step_without_progress(n):
    """diag(1, -1, ...) with b = ones: alpha_1 = b^T A b / n = 0, so the first step leaves y = 0 and the residual where it was
    (conjugate gradients divide by that zero); the second solves."""
    A, b = cases.cyclic_diag(cases.PLUS_MINUS, n), np.ones(n)
    y, its, relres = model.solve(A, b, tol=TOL)
    # alpha_1 = O(eps): c' = O(eps), s' = 1 - O(eps^2), so the first step leaves the residual norm where it was to all printed digits
    assert its == 2 and relres[1] > 1.0 - 1e-12 and relres[2] <= TOL
    assert np.linalg.norm(A @ y - b) <= 2 * TOL * np.linalg.norm(b)
    with pytest.raises(cg_model.NotPositiveDefinite):
        cg_model.solve(A, b, tol=TOL)


def _bloch_host():
    t = cg_cases.LAPLACE.astype(np.complex128)
    w = extras.bloch_wrap(t, (0.7, -0.4, 1.1))
    v = cg_cases.potential(lo=1.0).astype(np.complex128)
    return pkg.host_grid_matrix(cg_cases.GRID_SHAPE, t, v, periodic=(True, True, True), wrap=w)


def host_case(case):
    """(A, b) of a case of minres_cases.SOLVES on the host."""
    if case.startswith("laplace-v"):
        A = cg_cases.laplace_v()
    elif case == "random-csr":
        A = cg_cases.random_spd()
    elif case == "bloch-c64":
        A = _bloch_host()
    else:
        A = cg_cases.mass()
    return A, cg_cases.rhs(A.shape[0], A.dtype)


@pytest.mark.parametrize("case", list(cases.SOLVES))
def test_model_holds_the_bounds_and_permutations_record_the_spread(case):
    """The model on every case of the device's solve test: eigenvalues below the shift as recorded, true residual and error within
    their bounds, a monotone residual history (asserted inside the model too), the count within the band of the recorded one -- and
    the same under the six symmetric permutations, whose spread is what the band is made of."""
    shift, below = cases.SOLVES[case]
    A, b = host_case(case)
    assert abs(A - A.conj().T).max() == 0
    ystar = np.linalg.solve(np.asarray(A.todense()) - shift * np.eye(A.shape[0]), b)
    counts = []
    for seed in cases.PERMUTATION_SEEDS:
        Ap, bp = cases.permuted(A, b, seed)
        y, its, relres = model.solve(Ap, bp, shift=shift, tol=TOL)
        assert all(r1 <= r0 for r0, r1 in zip(relres, relres[1:])) and relres[-1] <= TOL
        res = float(np.linalg.norm(Ap @ y - shift * y - bp))
        assert res <= 2 * TOL * np.linalg.norm(b), (case, seed, res)
        counts.append(its)
        if seed is None:
            res, res_bound, err, err_bound, nbelow = cases.bounds(A, y, ystar, b, TOL, shift)
            print("%s: %d iterations, %d eigenvalues below %g, residual %.3g <= %.3g, error %.3g <= %.3g" % (case, its, nbelow, shift, res, res_bound, err, err_bound))
            assert nbelow == below and res <= res_bound and err <= err_bound
    print("%s: counts under %s = %s, spread %d (recorded %s, spread %d), band %d" %
          (case, cases.PERMUTATION_SEEDS, counts, max(counts) - min(counts), cases.PERMUTED_ITS[case], cases.SPREAD[case], cases.band(case)))
    for its in counts:
        assert abs(its - cases.MODEL_ITS[case]) <= cases.band(case), (case, counts)


def test_recorded_spreads_give_the_bands_the_device_test_uses():
    assert sorted(cases.PERMUTED_ITS["laplace-v-1.2"]) == [148, 153, 153, 154, 154, 154]
    assert cases.band("laplace-v-1.2") == 12 and cases.band("laplace-v-3.0") == 16 and cases.band("mass-box") == 2
    assert cases.BLOCH_BELOW >= 5 and cases.MODEL_ITS["bloch-c64"] <= 400


def test_mass_matrix_count_equals_conjugate_gradients():
    """Positive definite: MINRES and conjugate gradients stop on different residual norms of the same Krylov space; here both take 61."""
    A, b = host_case("mass-box")
    _, its, _ = model.solve(A, b, tol=TOL)
    _, cg_its, _ = cg_model.solve(A, b, tol=TOL)
    assert its == cg_its == 61


def test_model_solves_what_conjugate_gradients_refuse_and_reports_failures():
    A, b = cg_cases.indefinite(37)
    with pytest.raises(cg_model.NotPositiveDefinite):
        cg_model.solve(A, b, tol=TOL)
    y, its, _ = model.solve(A, b, tol=TOL)
    assert its == 4 and np.linalg.norm(A @ y - b) <= 2 * TOL * np.linalg.norm(b)      # four distinct eigenvalues: 1, 2, 4, -3
    y, its, relres = model.solve(A, np.zeros(37), tol=TOL)
    assert its == 0 and not y.any()
    with pytest.raises(model.Singular, match="gamma = 0 at iteration 1"):
        model.solve(np.eye(8), np.ones(8), shift=1.0, tol=TOL)
    with pytest.raises(model.NotFinite):
        model.solve(np.eye(8), np.array([1.0, NAN] + [0.0] * 6), tol=TOL)
    L, bl = host_case("laplace-v-1.2")
    with pytest.raises(model.DidNotConverge, match="after 10 iterations"):
        model.solve(L, bl, shift=1.2, tol=TOL, maxit=10)


def test_interior_eigenvalues_is_the_back_transformation():
    lam = np.array([1.12478146, 1.30622545])
    mu = 1.0 / (lam - 1.2)
    assert np.allclose(extras.interior_eigenvalues(mu, 1.2), lam, rtol=0, atol=1e-15)
    assert extras.interior_eigenvalues(mu, 1.2).dtype == np.float64
