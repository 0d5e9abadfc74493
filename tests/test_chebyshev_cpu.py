"""`-m "not gpu"`: the host side of the Chebyshev polynomial filter -- the Clenshaw schedule (`ks_host_chebyshev_plan`,
csrc/ks_cheb_plan.hpp) against literal tables and against exact rational arithmetic, its refusals, and the coefficient makers of
`extras` (chebyshev_window, chebyshev_damping, grid_spectrum_bounds).  No device: the schedule is a host function."""
from fractions import Fraction

import numpy as np
import pytest

import chebyshev_cases as cc
import grid_cases as gc
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

EPS = np.finfo(np.float64).eps
X0, Y, NONE = -1, -1, -2


def _rows(steps):
    return [(s["in"], s["out"], s["w"], s["sigma"], s["gamma"]) for s in steps]


def test_plan_tables_for_degrees_1_2_3_5():
    """The schedule, written out: slots (-1 = x0 / y, -2 = none, b_k in temporary (m - 1 - k) mod 3) and the scalars as the issue's
    table forms them, h = fl(2 / e), h1 = fl(1 / e); c and e are no powers of two, so a scalar formed in another way differs."""
    c, e = 3.0, 0.7
    g = (0.3, -1.1, 0.7, 2.3, -0.9, 1.7)
    h, h1 = 2.0 / e, 1.0 / e
    want = {
        1: ([(X0, Y, NONE, g[1] * h1, g[0])], 0),
        2: ([(X0, 0, NONE, g[2] * h, g[1]), (0, Y, NONE, h1, g[0] - g[2])], 1),
        3: ([(X0, 0, NONE, g[3] * h, g[2]), (0, 1, NONE, h, g[1] - g[3]), (1, Y, 0, h1, g[0])], 2),
        5: ([(X0, 0, NONE, g[5] * h, g[4]), (0, 1, NONE, h, g[3] - g[5]), (1, 2, 0, h, g[2]), (2, 0, 1, h, g[1]), (0, Y, 2, h1, g[0])], 3),
    }
    for m, (table, ntmp) in want.items():
        steps, nt = pkg.host_chebyshev_plan(m, c, e, g[: m + 1])
        assert nt == ntmp, (m, nt)
        assert _rows(steps) == table, (m, _rows(steps), table)


def test_no_step_writes_a_vector_it_reads():
    """m = 1 ... 12: `out` is none of `in`, `w`, x0 (x0 and y are different vectors; temporaries by their slot), every step but
    the last writes a temporary that the next step reads, temporaries = min(m - 1, 3), theta-independent."""
    for m in range(1, 13):
        steps, nt = pkg.host_chebyshev_plan(m, 0.25, 1.5, np.linspace(-1.0, 2.0, m + 1))
        assert len(steps) == m and nt == min(m - 1, 3)
        for i, s in enumerate(steps):
            vec = lambda slot, role: ("x0" if role == "in" else "y") if slot == -1 else ("tmp", slot)  # noqa: E731
            out = vec(s["out"], "out")
            reads = {vec(s["in"], "in"), "x0"} | ({("tmp", s["w"])} if s["w"] != NONE else set())
            assert out not in reads, (m, i, s)
            assert s["in"] >= -1 and s["out"] >= -1 and s["in"] < nt and s["out"] < nt and -2 <= s["w"] < nt and s["w"] != -1
            assert (s["out"] == -1) == (i == m - 1) and (s["in"] == -1) == (i == 0)
            if i > 0:
                assert s["in"] == steps[i - 1]["out"]
            if i > 1:
                assert s["w"] == steps[i - 2]["out"]
            else:
                assert s["w"] == NONE


@pytest.mark.parametrize("degree", [1, 2, 3, 4, 6])
def test_plan_in_exact_arithmetic(degree):
    """The plan run with Fractions on the 5 x 4 x 3 integer case equals sum_k gamma_k T_k(Ahat) x by the three-term recurrence,
    exactly; and the same plan run in Float64 equals the Fraction result exactly (every intermediate is a dyadic rational that
    Float64 holds: tests/chebyshev_cases.py)."""
    shape = cc.EXACT_SHAPES[0]
    _v, x, A = cc.exact_case(shape)
    g = cc.EXACT_GAMMA[: degree + 1]
    steps, _ = pkg.host_chebyshev_plan(degree, cc.EXACT_CENTER, cc.EXACT_HALFWIDTH, g)
    want = cc.series(A, x, cc.EXACT_CENTER, cc.EXACT_HALFWIDTH, g)
    got = cc.run_plan(steps, A, cc.to_fractions(x), cc.EXACT_CENTER)
    assert all(a == b for a, b in zip(got, want)), degree
    y64 = cc.run_plan(steps, A, x, cc.EXACT_CENTER)
    assert y64.dtype == np.float64
    assert all(Fraction(float(a)) == b for a, b in zip(y64, want)), degree
    if degree == 6:
        print("largest entry of the exact result: %g" % float(max(abs(t) for t in want)))
        assert np.array_equal(cc.fraction_bits(want), y64)


def test_plan_refuses_bad_arguments():
    ok = (0.5, 1.0, -0.25)
    plan = pkg.host_chebyshev_plan
    with pytest.raises(pkg.ArgumentError, match="degree = 0"):
        plan(0, 0.0, 1.0, ok[:1])
    with pytest.raises(pkg.ArgumentError, match="degree = 257"):
        plan(257, 0.0, 1.0, np.ones(258))
    plan(256, 0.0, 1.0, np.ones(257))
    for e in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(pkg.ArgumentError, match="halfwidth"):
            plan(2, 0.0, e, ok)
    for c in (np.inf, -np.inf, np.nan):
        with pytest.raises(pkg.ArgumentError, match="center"):
            plan(2, c, 1.0, ok)
    for k in range(3):
        for bad in (np.nan, np.inf):
            g = list(ok)
            g[k] = bad
            with pytest.raises(pkg.ArgumentError, match="coefficient %d " % k):
                plan(2, 0.0, 1.0, g)
    with pytest.raises(pkg.DimensionMismatch):
        plan(3, 0.0, 1.0, ok)
    with pytest.raises(pkg.ArgumentError):
        plan(2, 0.0, 1.0, np.array([1.0, 2.0, 3.0j]))


# ------------------------------------------------------------------------------------------------ coefficients
WINDOWS = [((0.0651, 16.83), 1.9, 2.06, 80), ((-1.0, 1.0), -0.3, 0.1, 40), ((2.0, 50.0), 2.0, 7.5, 64), ((0.0, 10.0), 9.0, 10.0, 41)]


@pytest.mark.parametrize("bounds,lo,hi,degree", WINDOWS)
def test_window_coefficients_are_the_cosine_integrals(bounds, lo, hi, degree):
    """Undamped: gamma_k = (2 / pi) int_{t2}^{t1} cos(k t) dt (k = 0: 1 / pi) by 64-node Gauss-Legendre, k <= 40, to 1e-13
    absolute: the integrand is entire and |gamma_k| <= 2, the closed form's own rounding is about k eps, the quadrature error
    (k (t1 - t2) / 2 <= 63 against 64 nodes) far below that."""
    c, e, g = extras.chebyshev_window(lo, hi, bounds, degree, damping=None)
    assert c == 0.5 * (bounds[0] + bounds[1]) and e == 0.5 * (bounds[1] - bounds[0]) and g.shape == (degree + 1,)
    t1, t2 = np.arccos((lo - c) / e), np.arccos((hi - c) / e)
    node, wt = np.polynomial.legendre.leggauss(64)
    th = 0.5 * (t1 + t2) + 0.5 * (t1 - t2) * node
    for k in range(min(degree, 40) + 1):
        quad = (1.0 if k == 0 else 2.0) / np.pi * 0.5 * (t1 - t2) * np.sum(wt * np.cos(k * th))
        assert abs(g[k] - quad) <= 1e-13, (k, g[k], quad)


@pytest.mark.parametrize("bounds,lo,hi,degree", WINDOWS)
def test_jackson_window_stays_in_0_1_and_peaks_in_the_window(bounds, lo, hi, degree):
    """Jackson-damped: the kernel is positive, so 0 <= p <= 1 mathematically: -1e-13 <= p(t) <= 1 + 1e-13 on 4001 mesh points of
    [a, b]; and p at the window's midpoint exceeds p at every mesh point outside [lo - w, hi + w], w the window's width."""
    c, e, g = extras.chebyshev_window(lo, hi, bounds, degree)
    t = np.linspace(bounds[0], bounds[1], 4001)
    p = cc.cheb_series(c, e, g, t)
    assert p.min() >= -1e-13 and p.max() <= 1 + 1e-13, (float(p.min()), float(p.max()))
    w = hi - lo
    outside = (t < lo - w) | (t > hi + w)
    mid = cc.cheb_series(c, e, g, 0.5 * (lo + hi))
    assert np.any(outside) and mid > p[outside].max(), (float(mid), float(p[outside].max()))
    # the helper users map eigenvalues with agrees with the reference evaluation
    assert np.abs(extras.chebyshev_eval(c, e, g, t) - p).max() <= 64 * degree * EPS


def test_window_refusals():
    with pytest.raises(pkg.ArgumentError, match="inside the bounds"):
        extras.chebyshev_window(-0.1, 0.5, (0.0, 1.0), 10)
    with pytest.raises(pkg.ArgumentError, match="inside the bounds"):
        extras.chebyshev_window(0.5, 0.5, (0.0, 1.0), 10)
    with pytest.raises(pkg.ArgumentError, match="degree"):
        extras.chebyshev_window(0.2, 0.5, (0.0, 1.0), 0)
    with pytest.raises(pkg.ArgumentError, match="bounds"):
        extras.chebyshev_window(0.2, 0.5, (1.0, 0.0), 10)
    with pytest.raises(pkg.ArgumentError, match="damping"):
        extras.chebyshev_window(0.2, 0.5, (0.0, 1.0), 10, damping="lanczos")


@pytest.mark.parametrize("bounds,below,degree", [((0.0651, 16.83), 0.0651, 12), ((2.5, 16.83), 0.8, 12), ((1.0, 3.0), 3.5, 7), ((-2.0, 5.0), -2.25, 40)])
def test_damping_polynomial(bounds, below, degree):
    """p = T_m((t - c) / e) / T_m((below - c) / e): only the top coefficient is non-zero; p(below) = 1 to 4 ulp (the reciprocal and
    the product round once each, T_m is evaluated in extended precision on both sides); |p| <= 1 / |T_m((below - c) / e)| on
    [a, b] -- |T_m| <= 1 there, so |p| <= |gamma_m|, and gamma_m is that reciprocal to an ulp (bound x (1 + 4 eps))."""
    c, e, g = extras.chebyshev_damping(bounds, below, degree)
    assert np.count_nonzero(g) == 1 and g[degree] != 0 and g.shape == (degree + 1,)
    sb = (np.longdouble(below) - np.longdouble(c)) / np.longdouble(e)
    top = cc.cheb_t(degree, sb)
    assert abs(np.longdouble(g[degree]) * top - 1) <= 4 * EPS, float(np.longdouble(g[degree]) * top - 1)
    t = np.linspace(bounds[0], bounds[1], 4001)
    s = np.clip((t.astype(np.longdouble) - np.longdouble(c)) / np.longdouble(e), -1, 1)
    p = np.longdouble(g[degree]) * cc.cheb_t(degree, s)
    assert np.abs(p).max() <= (1 + 4 * EPS) / abs(top)
    assert abs(top) >= 1
    with pytest.raises(pkg.ArgumentError, match="beyond an end"):
        extras.chebyshev_damping(bounds, 0.5 * (bounds[0] + bounds[1]), degree)


@pytest.mark.parametrize("radius", [1, 2])
def test_gershgorin_bounds_contain_the_spectrum(radius):
    shape = (6, 5, 4)
    t = gc.taps(3, np.float64, symmetric=True) if radius == 1 else -extras.fd_laplacian_taps(3, 4)
    v = gc.harmonic(shape)
    A = pkg.host_grid_matrix(shape, t, v, radius=radius)
    assert abs(A - A.T).max() == 0
    ev = np.linalg.eigvalsh(A.toarray())
    a, b = extras.grid_spectrum_bounds(t, v, radius=radius)
    assert a <= ev[0] and ev[-1] <= b, (a, ev[0], ev[-1], b)
    off = np.abs(t).sum() - abs(t[t.size // 2])
    assert a == t[t.size // 2] + v.min() - off and b == t[t.size // 2] + v.max() + off
    a0, b0 = extras.grid_spectrum_bounds(t, radius=radius)
    ev0 = np.linalg.eigvalsh(pkg.host_grid_matrix(shape, t, radius=radius).toarray())
    assert a0 <= ev0[0] and ev0[-1] <= b0
    with pytest.raises(pkg.ArgumentError):
        extras.grid_spectrum_bounds(t[:-1], v, radius=radius)
    with pytest.raises(pkg.ArgumentError, match="Hermitian"):
        extras.grid_spectrum_bounds(t, v + 1j, radius=radius)
