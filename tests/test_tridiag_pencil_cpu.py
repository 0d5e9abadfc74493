"""`-m "not gpu"`: the HOST path of the fused tridiagonal pencil operator y = (K - sigma M)^-1 M x
(`api.host_tridiagonal_pencil_solve`: T = K - sigma M and t = M b formed in numpy, then `ks_host_tridiag_solve` on (T, t) with
shift 0) -- the reference the GPU tests of `ks_operator_tridiag_pencil` compare with.  The reference side is the `ShiftAndInvert`
LinearMap of docs/src/index.md:273-287 (`mul!(temp, B, x); ldiv!(y, A_lu, temp)`) on a 1-D pencil.

Checked against the pencil itself: the normwise backward error of (K - sigma M) y = M b stays within 64 eps (the bound of
tests/tridiag_cases.py; measured on these families <= 8.9e-16), the planner takes the default number of levels, and with M = I the
path is the plain shift-invert solve bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import ROOT, import_package
from pencil_cases import ETA_BOUND, FAMILIES, IDS, SIZES, default_levels, family, mass, pencil, pencil_eta, rhs

pkg = import_package()


@pytest.mark.parametrize("kname,mname,cplx,sigma", FAMILIES, ids=IDS)
@pytest.mark.parametrize("n,block_rows", SIZES)
def test_host_pencil_solve_is_backward_stable(kname, mname, cplx, sigma, n, block_rows):
    K, M, sg = pencil(kname, mname, n, cplx, sigma)
    b = rhs(n, cplx)
    y, info = pkg.host_tridiagonal_pencil_solve(*K, *M, b, sigma=sg, block_rows=block_rows)
    e = pencil_eta(K, M, sg, y, b)
    print(f"{kname} {mname} {'c128' if cplx else 'f64'} n={n} m={block_rows}: eta {e:.2e} {info}")
    assert y.dtype == (np.complex128 if cplx else np.float64) and y.shape == b.shape
    assert e <= ETA_BOUND
    assert info["levels"] == default_levels(n, block_rows)
    assert info["level_rows"][0] == n


@pytest.mark.parametrize("kname,sigma", [("a", 1.7), ("b", None), ("d", None)])
@pytest.mark.parametrize("n,block_rows", [(1, 4), (2, 4), (26, 4), (341, 4), (131, 0), (4226, 0)])
def test_identity_mass_is_the_plain_solve_bit_for_bit(kname, sigma, n, block_rows):
    """M = I: T = K - sigma I is what the plain path forms itself and M b = b, so nothing may differ (real families)."""
    dl, d, du, sg = family(kname, n, False, sigma)
    b = rhs(n, False)
    want, winfo = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=block_rows)
    got, info = pkg.host_tridiagonal_pencil_solve(dl, d, du, *mass("identity", n), b, sigma=sg, block_rows=block_rows)
    assert np.array_equal(got, want) and info == winfo


def test_several_right_hand_sides_and_promotion():
    n = 131
    K, M, sg = pencil("a", "fem", n, False, 1.0)
    B = np.stack([rhs(n, False, seed=s) for s in range(3)], axis=1)
    Y, _ = pkg.host_tridiagonal_pencil_solve(*K, *M, B, sigma=sg)
    for k in range(3):
        y, _ = pkg.host_tridiagonal_pencil_solve(*K, *M, B[:, k], sigma=sg)
        assert np.array_equal(Y[:, k], y)
    # a complex shift, or a complex diagonal of M alone, makes the whole pencil ComplexF64 (as _tridiag_args promotes)
    y, _ = pkg.host_tridiagonal_pencil_solve(*K, *M, B[:, 0], sigma=1.0 + 0.5j)
    assert y.dtype == np.complex128 and pencil_eta(K, M, 1.0 + 0.5j, y, B[:, 0]) <= ETA_BOUND
    Mc = (M[0], M[1] + 0.1j, M[2])
    y, _ = pkg.host_tridiagonal_pencil_solve(*K, *Mc, B[:, 0], sigma=1.0)
    assert y.dtype == np.complex128 and pencil_eta(K, Mc, 1.0, y, B[:, 0]) <= ETA_BOUND


def test_wrong_lengths_are_refused_before_the_library_is_called():
    K, M, sg = pencil("a", "fem", 20, False, 1.0)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.host_tridiagonal_pencil_solve(*K, M[0], M[1][:-1], M[2], rhs(20, False), sigma=sg)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.host_tridiagonal_pencil_solve(*K, M[0][:-1], M[1], M[2], rhs(20, False), sigma=sg)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.host_tridiagonal_pencil_solve(K[0], K[1], K[2][:-2], *M, rhs(20, False), sigma=sg)


def test_a_singular_shifted_matrix_is_refused_like_the_plain_solve():
    """Family c (zero diagonal) at an ODD size is singular; with M's diagonal zero the shift does not move it."""
    n = 401
    dl, d, du, _ = family("c", n, sigma="odd")
    with pytest.raises(pkg.ArgumentError):
        pkg.host_tridiagonal_pencil_solve(dl, d, du, np.full(n - 1, 1.0 / 6.0), np.zeros(n), np.full(n - 1, 1.0 / 6.0), rhs(n, False), sigma=0.0)


def test_header_and_prototype_table_carry_both_operators():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kschur.h")).read(), flags=re.S)
    L = pkg._lib.load()
    for name, nargs in (("ks_operator_product", 4), ("ks_operator_tridiag_pencil", 11)):
        m = re.search(r"^int\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/kschur.h"
        assert len(m.group(1).split(",")) == nargs
        assert len(pkg._lib.PROTOTYPES[name]) == nargs
        assert isinstance(getattr(L, name), C._CFuncPtr)
    for name in ("product_operator", "tridiagonal_pencil_operator", "host_tridiagonal_pencil_solve"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
