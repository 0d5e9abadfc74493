"""Data and exact references shared by tests/test_chebyshev_cpu.py and tests/test_gpu_chebyshev.py (the Chebyshev polynomial filter,
csrc/ks_cheb_plan.hpp, csrc/ks_cheb.hpp).  Plain numpy / scipy / fractions: no device, no library.

THE EXACT CASE.  The 7-point matrix with off-diagonals -1 and diagonal 6 + an integer in 0 ... 3, an integer x in -8 ... 8, centre
c = 8, half-width e = 8 and dyadic coefficients: 2 / e = 1/4 and 1 / e = 1/8 are powers of two, so every number a Clenshaw step forms
is a dyadic rational with a few fractional bits more than its inputs (degree 6: below 2^-20) and a magnitude far below 2^10 -- exactly
representable in Float64, whatever the order of the additions and whether or not a product is contracted into an addition.  The
filter's result must therefore carry the BITS of sum_k gamma_k T_k((A - c) / e) x evaluated in rational arithmetic."""
from fractions import Fraction

import numpy as np

import grid_cases as gc

EXACT_SHAPES = [(5, 4, 3), (33, 5, 9)]
EXACT_TAPS = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
EXACT_CENTER, EXACT_HALFWIDTH = 8.0, 8.0
EXACT_GAMMA = (0.5, -0.25, 0.75, 1.0, -0.5, 0.25, 1.5)


def exact_case(shape, seed=0):
    """(potential, x, A): integers as Float64; A the scipy CSR matrix assembled by grid_cases.kron_matrix (no library)."""
    rng = np.random.default_rng(41 + seed + gc.size(shape))
    v = rng.integers(0, 4, gc.size(shape)).astype(np.float64)
    x = rng.integers(-8, 9, gc.size(shape)).astype(np.float64)
    return v, x, gc.kron_matrix(shape, EXACT_TAPS, v)


def to_fractions(a):
    """Float64 array -> object array of Fractions (exact: every double is a rational)."""
    return np.array([Fraction(float(t)) for t in np.asarray(a).ravel()], dtype=object)


def matvec(A, v):
    """A v for a CSR matrix without empty rows, in the arithmetic of v (Float64, or Fractions in an object array)."""
    data = to_fractions(A.data) if v.dtype == object else A.data
    return np.add.reduceat(data * v[A.indices], A.indptr[:-1])


def series(A, x, center, halfwidth, gamma):
    """sum_k gamma_k T_k(Ahat) x, Ahat = (A - c) / e, by the three-term recurrence T_{k+1} = 2 Ahat T_k - T_{k-1} on vectors of
    Fractions: the definition, with no Clenshaw in it."""
    c, e = Fraction(center), Fraction(halfwidth)
    g = [Fraction(float(t)) for t in gamma]
    hat = lambda v: (matvec(A, v) - c * v) / e  # noqa: E731
    t0 = to_fractions(x)
    y = g[0] * t0
    if len(g) > 1:
        t1 = hat(t0)
        y = y + g[1] * t1
        for k in range(2, len(g)):
            t0, t1 = t1, 2 * hat(t1) - t0
            y = y + g[k] * t1
    return y


def run_plan(steps, A, x, center):
    """The schedule of host_chebyshev_plan executed step by step, out = ((sigma (A in - c in)) - w) + gamma x0, in the arithmetic
    of x (Float64: one rounding per operation; an object array of Fractions: exact, with the plan's Float64 scalars taken as the
    rationals they are)."""
    exact = x.dtype == object
    num = (lambda t: Fraction(float(t))) if exact else float
    tmp, y = {}, None
    for s in steps:
        vin = x if s["in"] == -1 else tmp[s["in"]]
        t = num(s["sigma"]) * (matvec(A, vin) - num(center) * vin)
        if s["w"] != -2:
            t = t - tmp[s["w"]]
        t = t + num(s["gamma"]) * x
        if s["out"] == -1:
            y = t
        else:
            tmp[s["out"]] = t
    return y


def fraction_bits(v):
    """An object array of Fractions as Float64, asserting that every entry is exactly representable."""
    out = np.array([float(t) for t in v])
    assert all(Fraction(float(o)) == t for o, t in zip(out, v)), "the exact result is not a Float64 vector"
    return out


def cheb_t(m, s):
    """T_m(s) in np.longdouble: cos(m acos s) inside [-1, 1], +-cosh(m acosh |s|) outside."""
    s = np.asarray(s, dtype=np.longdouble)
    inside = np.abs(s) <= 1
    a = np.abs(s)
    out = np.where(inside, np.cos(m * np.arccos(np.clip(s, -1, 1))), np.cosh(m * np.arccosh(np.where(inside, 1, a))))
    return np.where(~inside & (s < 0) & (m % 2 == 1), -out, out)


def cheb_series(center, halfwidth, gamma, t):
    """p(t) = sum_k gamma_k T_k((t - c) / e) in np.longdouble through numpy's Chebyshev class evaluation (chebval)."""
    s = (np.asarray(t, dtype=np.longdouble) - np.longdouble(center)) / np.longdouble(halfwidth)
    return np.polynomial.chebyshev.chebval(s, np.asarray(gamma, dtype=np.longdouble))
