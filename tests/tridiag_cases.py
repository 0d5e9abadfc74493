"""Shared by tests/test_tridiag_solve_cpu.py and tests/test_gpu_tridiag_solve.py: the seeded matrix families of the tridiagonal
shift-invert operator (csrc/ks_tridiag_plan.hpp), the normwise backward error both files assert, LAPACK's figure for the same
input, and a small model of how many levels the DEFAULT split (no shortened block) gives.

Families (dl, d, du, sigma):
  a   laplace1d(n) - sigma I, real, sigma in {1.7, 1.0, 2.0}: indefinite (sigma = 2: zero diagonal)
  b   BASELINE config 4: laplace1d + i diag(0.3 rand), sigma = 1.7 + 0.1i, default_rng(3); Float64 twin: + diag(0.3 rand), sigma = 1.7
  c   zero diagonal, dl = du = 1, n even: every pivot needs an interchange, every odd block is singular
  d   random, diagonally dominant
  e   random, not dominant: standard_normal on all three diagonals
"""
import numpy as np

EPS = np.finfo(np.float64).eps
ETA_BOUND = 64 * EPS   # measured margin: ~40 x the worst case of the numpy prototype of the scheme (3.3e-16), LAPACK 7.3e-17


def _normal(rng, n, cplx):
    x = rng.standard_normal(n)
    return (x + 1j * rng.standard_normal(n)) if cplx else x


def family(name, n, cplx=False, sigma=None):
    """-> (dl, d, du, sigma) of the named family."""
    m = max(n - 1, 0)
    if name == "a":
        return -np.ones(m), 2.0 * np.ones(n), -np.ones(m), float(sigma)
    if name == "b":
        rng = np.random.default_rng(3)
        r = 0.3 * rng.random(n)
        if cplx:
            return -np.ones(m, dtype=complex), 2.0 + 1j * r, -np.ones(m, dtype=complex), 1.7 + 0.1j
        return -np.ones(m), 2.0 + r, -np.ones(m), 1.7
    if name == "c":
        assert n % 2 == 0 or sigma == "odd"
        return np.ones(m), np.zeros(n), np.ones(m), 0.0
    rng = np.random.default_rng(1000 + n + (7 if cplx else 0) + (13 if name == "e" else 0))
    dl, du, d = _normal(rng, m, cplx), _normal(rng, m, cplx), _normal(rng, n, cplx)
    if name == "d":
        dom = np.zeros(n)
        dom[1:] += np.abs(dl)
        dom[:-1] += np.abs(du)
        ph = d / np.maximum(np.abs(d), 1e-300)
        d = ph * (dom + 1.0 + np.abs(d))
    return dl, d, du, (0.25 + 0.5j if cplx else 0.25)


def rhs(n, cplx, seed=0):
    rng = np.random.default_rng(4242 + seed + n)
    return _normal(rng, n, cplx)


def matvec(dl, d, du, sigma, x):
    y = (np.asarray(d) - sigma) * x
    if len(x) > 1:
        y[1:] += np.asarray(dl) * x[:-1]
        y[:-1] += np.asarray(du) * x[1:]
    return y


def norm1(dl, d, du, sigma):
    col = np.abs(np.asarray(d) - sigma).astype(float)
    if len(col) > 1:
        col[:-1] += np.abs(dl)
        col[1:] += np.abs(du)
    return float(col.max())


def eta(dl, d, du, sigma, x, b):
    """normwise backward error ||M x - b||_2 / (||M||_1 ||x||_2 + ||b||_2)"""
    if not np.all(np.isfinite(x)):
        return float("inf")
    r = matvec(dl, d, du, sigma, x) - b
    return float(np.linalg.norm(r) / (norm1(dl, d, du, sigma) * np.linalg.norm(x) + np.linalg.norm(b)))


def lapack_solve(dl, d, du, sigma, b):
    from scipy.linalg import solve_banded

    n = len(d)
    dt = np.result_type(np.asarray(dl).dtype, np.asarray(d).dtype, np.asarray(du).dtype, type(sigma), np.asarray(b).dtype)
    ab = np.zeros((3, n), dtype=dt)
    ab[0, 1:] = du
    ab[1, :] = np.asarray(d) - sigma
    ab[2, :-1] = dl
    return solve_banded((1, 1), ab, np.asarray(b, dtype=dt))


def default_levels(n, block_rows):
    """Levels of the default split: blocks of m rows, one separator each -> n // (m + 1) separators; a level of at most 2 m rows
    is solved directly."""
    m = block_rows or 64
    levels, rows = 1, n
    while rows > 2 * m:
        rows //= m + 1
        levels += 1
    return levels
