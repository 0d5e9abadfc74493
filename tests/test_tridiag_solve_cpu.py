"""`-m "not gpu"`: the host side of the tridiagonal shift-invert operator (csrc/ks_tridiag_plan.hpp) through
ks_host_tridiag_solve / ks_host_tridiag_info -- partition, block factors, spikes, the reduced levels and the apply that walks the
arrays the device kernels read.  Every case asserts the normwise backward error

    eta = ||M x - b||_2 / (||M||_1 ||x||_2 + ||b||_2)  <=  64 eps  (1.4e-14)

of the returned x (the bound is about 40 times the worst case measured on a numpy prototype of the scheme, 3.3e-16; LAPACK's banded
solve gave 7.3e-17 on the same inputs) and prints LAPACK's figure next to it; `levels` must be what the default split gives."""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import import_package
from tridiag_cases import ETA_BOUND, default_levels, eta, family, lapack_solve, rhs

pkg = import_package()
_lib = pkg._lib

SMALL_N = [1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25, 26, 340, 341, 400]
DEFAULT_N = [63, 64, 65, 66, 67, 129, 130, 131, 4225, 4226, 70000]
FAMILIES = [("b", False), ("b", True), ("c", False), ("d", False), ("d", True), ("e", False), ("e", True)]


def _cases(ns, block_rows, a_n):
    out = []
    for n in ns:
        for name, cplx in FAMILIES:
            if name == "c" and n % 2:
                continue
            out.append(pytest.param(name, cplx, n, None, block_rows, id=f"{name}-{'c128' if cplx else 'f64'}-n{n}-m{block_rows}"))
    for sigma in (1.7, 1.0, 2.0):
        out.append(pytest.param("a", False, a_n, sigma, block_rows, id=f"a-f64-n{a_n}-sigma{sigma}-m{block_rows}"))
    return out


def _check(name, cplx, n, sigma, block_rows):
    dl, d, du, sg = family(name, n, cplx, sigma)
    b = rhs(n, cplx)
    x, info = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=block_rows)
    e = eta(dl, d, du, sg, x, b)
    e_lapack = eta(dl, d, du, sg, lapack_solve(dl, d, du, sg, b), b)
    print(f"{name} {'c128' if cplx else 'f64'} n={n} m={block_rows}: eta {e:.2e}  LAPACK {e_lapack:.2e}  levels {info['levels']} "
          f"rows {info['level_rows']} shortened {info['shortened_blocks']} growth {info['max_growth']:.2e} check {info['residual']:.2e}")
    assert e <= ETA_BOUND, (e, e_lapack)
    assert info["levels"] == default_levels(n, block_rows), info
    assert info["level_rows"][0] == n and len(info["level_rows"]) == info["levels"]
    assert info["residual"] <= ETA_BOUND and 0.0 <= info["max_growth"] <= 1e6
    return info


@pytest.mark.parametrize("name,cplx,n,sigma,block_rows", _cases(SMALL_N, 4, 400))
def test_block_size_4(name, cplx, n, sigma, block_rows):
    """Three levels are reached by n ~ 125, four at 340: every path of the recursion on sizes around the block and the direct limit."""
    _check(name, cplx, n, sigma, block_rows)


@pytest.mark.parametrize("name,cplx,n,sigma,block_rows", _cases(DEFAULT_N, 0, 70000))
def test_default_block_size(name, cplx, n, sigma, block_rows):
    _check(name, cplx, n, sigma, block_rows)


def _raw(n, dtype, dl, d, du, sre, sim, block_rows, nrhs, b, ldb, x, ldx):
    L = _lib.load()
    lv, gr, res = C.c_int(), C.c_double(), C.c_double()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    rc = L.ks_host_tridiag_solve(n, dtype, ptr(dl), ptr(d), ptr(du), sre, sim, block_rows, nrhs, ptr(b), ldb, ptr(x), ldx, C.byref(lv),
                                 C.byref(gr), C.byref(res))
    return rc, lv.value


@pytest.mark.parametrize("cplx", [False, True])
def test_three_right_hand_sides_with_a_leading_dimension(cplx):
    """nrhs = 3, ldb != n and ldx != n: the same columns as three single calls, bit for bit."""
    n = 341
    dl, d, du, sg = family("e", n, cplx)
    dt = np.complex128 if cplx else np.float64
    dl, d, du = (np.ascontiguousarray(a, dtype=dt) for a in (dl, d, du))
    sg = complex(sg)
    ldb, ldx = n + 5, n + 2
    B = np.zeros((3, ldb), dtype=dt)
    for k in range(3):
        B[k, :n] = rhs(n, cplx, seed=k)
    X = np.full((3, ldx), np.nan, dtype=dt)
    rc, _ = _raw(n, _lib.KS_C64 if cplx else _lib.KS_F64, dl, d, du, sg.real, sg.imag, 4, 3, B, ldb, X, ldx)
    assert rc == _lib.KS_OK, _lib.load().ks_last_error_string()
    for k in range(3):
        xk, _ = pkg.host_tridiagonal_solve(dl, d, du, B[k, :n].copy(), sigma=sg if cplx else sg.real, block_rows=4)
        assert np.array_equal(X[k, :n], xk)
        assert np.all(np.isnan(X[k, n:]))  # the padding of x is not written
        assert eta(dl, d, du, sg if cplx else sg.real, X[k, :n], B[k, :n]) <= ETA_BOUND


def test_shortened_blocks_are_reported():
    """Zero diagonal, block size 5: every 5-row block is singular, so the planner has to shorten every block -- and the result
    still meets the bound."""
    n = 400
    dl, d, du, sg = family("c", n)
    b = rhs(n, False)
    x, info = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=5)
    e = eta(dl, d, du, sg, x, b)
    print(f"c n={n} m=5: eta {e:.2e} LAPACK {eta(dl, d, du, sg, lapack_solve(dl, d, du, sg, b), b):.2e} {info}")
    assert info["shortened_blocks"] > 0
    assert e <= ETA_BOUND
    # the default split of a matrix that needs none reports none
    dl, d, du, sg = family("d", n)
    _, info = pkg.host_tridiagonal_solve(dl, d, du, rhs(n, False), sigma=sg, block_rows=5)
    assert info["shortened_blocks"] == 0


def test_backtracking_partition_of_the_zero_diagonal_matrix():
    """n = 26 at block size 4: five default blocks leave a singular one-row tail, so do four; the planner must go back and shorten
    two blocks (a greedy planner without backtracking fails here)."""
    dl, d, du, sg = family("c", 26)
    b = rhs(26, False)
    x, info = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=4)
    assert info["shortened_blocks"] >= 2 and info["levels"] == 2
    assert eta(dl, d, du, sg, x, b) <= ETA_BOUND


def test_refusals():
    f64, c64 = _lib.KS_F64, _lib.KS_C64
    ERR = _lib.KS_ERR_ARGUMENT
    last = lambda: _lib.load().ks_last_error_string().decode()  # noqa: E731

    def solve(n, dl, d, du, sre=0.0, sim=0.0, block_rows=0, dtype=f64):
        dt = np.complex128 if dtype == c64 else np.float64
        b = np.ones(max(n, 1), dtype=dt)
        x = np.zeros(max(n, 1), dtype=dt)
        return _raw(n, dtype, dl.astype(dt), d.astype(dt), du.astype(dt), sre, sim, block_rows, 1, b, max(n, 1), x, max(n, 1))[0]

    # the zero-diagonal matrix of odd order is exactly singular (in integer arithmetic: nothing rounds)
    n = 401
    assert solve(n, np.ones(n - 1), np.zeros(n), np.ones(n - 1)) == ERR
    assert "tridiagonal solve" in last()
    assert solve(n, np.ones(n - 1), np.zeros(n), np.ones(n - 1), block_rows=4) == ERR
    # a NaN entry, in each diagonal
    n = 300
    dl, d, du, _ = family("d", n)
    for which in range(3):
        arrs = [dl.copy(), d.copy(), du.copy()]
        arrs[which][17] = np.nan
        assert solve(n, *arrs) == ERR
        assert "non-finite" in last()
    assert solve(n, dl, d, du, sre=np.inf) == ERR
    # a complex shift of a real matrix
    assert solve(n, dl, d, du, sre=0.3, sim=0.1) == ERR
    assert solve(n, dl, d, du, sre=0.3, sim=0.1, dtype=c64) == _lib.KS_OK
    # block sizes outside 2...64
    for m in (1, 65, -3):
        assert solve(n, dl, d, du, block_rows=m) == ERR
    assert solve(n, dl, d, du, block_rows=2) == _lib.KS_OK and solve(n, dl, d, du, block_rows=64) == _lib.KS_OK
    # n = 0
    assert solve(0, np.zeros(0), np.zeros(0), np.zeros(0)) == ERR
    # the Python mirror raises the reference's exception kind
    with pytest.raises(pkg.ArgumentError):
        pkg.host_tridiagonal_solve(np.ones(400), np.zeros(401), np.ones(400), np.ones(401))
