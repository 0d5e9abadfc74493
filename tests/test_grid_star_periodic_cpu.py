"""`-m "not gpu"`: the definition of the star-stencil grid operator of radius 2-4 with PERIODIC axes
(`ks_operator_grid_star_periodic`, csrc/ks_grid.hpp) -- mul!(y, A, x), src/expansion.jl:121, for central differences of order 4, 6,
8 on a crystal cell, with Bloch phases on the links that cross the boundary -- through its host function
`ks_host_grid_matrix_star_periodic` / `host_grid_star_matrix`, and `extras.bloch_wrap(..., radius=R)`: no device is touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_star_periodic_cases.py: Kronecker sums of 1-D parts with diagonals at +-1 ... +-R and the R (R + 1) / 2 corner entries
per side of a periodic axis), for every case the device tests use; the place of every wrapped entry inside its row is checked
against the row order of include/kschur.h (x-b) entry by entry."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_periodic_cases as gp
import grid_star_cases as sc
import grid_star_periodic_cases as sp_
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_matrix(A, B):
    assert A.shape == B.shape and A.nnz == B.nnz, (A.shape, B.shape, A.nnz, B.nnz)
    assert A.dtype == B.dtype
    assert np.array_equal(A.indptr, B.indptr)
    assert np.array_equal(A.indices, B.indices)
    assert np.array_equal(_bits(A.data), _bits(B.data))


def _all_cases(R):
    return [c for g in sp_.GROUPS.values() for c in g(R)] + sp_.EDGE_CASES_X


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", sc.RADII)
def test_matrix_is_the_kronecker_assembly_entry_for_entry(R, dtype):
    """Distinct taps and wrap values in every slot; with and without a potential, wrap = None and given; columns ascend strictly;
    nnz by the formula; wrap = None is wrap = the taps without the centre."""
    for shape, per in _all_cases(R):
        ndim = len(shape)
        t, w = sc.taps(ndim, R, dtype), sp_.wrap(ndim, R, dtype)
        assert len(set(t.tolist()) | set(w.tolist())) == 4 * ndim * R + 1
        for pot in (None, sc.potential(shape, dtype)):
            for wv in (None, w):
                A = pkg.host_grid_star_matrix(shape, t, R, pot, periodic=per, wrap=wv)
                want = sp_.kron_matrix(shape, per, R, t, wv, pot)
                assert want.nnz == sp_.nnz(shape, per, R), (shape, per)      # (nothing cancelled or merged in the reference assembly)
                _same_matrix(A, want)
                assert A.dtype == np.dtype(dtype)
                rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
                same_row = rows[1:] == rows[:-1]
                assert np.all(np.diff(A.indices.astype(np.int64))[same_row] > 0), (shape, per)
                if all(per):
                    assert np.all(np.diff(A.indptr) == 2 * ndim * R + 1)
            _same_matrix(pkg.host_grid_star_matrix(shape, t, R, pot, periodic=per),
                         pkg.host_grid_star_matrix(shape, t, R, pot, periodic=per, wrap=sp_.taps_as_wrap(t, ndim, R)))


def _row_by_definition(shape, per, R, t, w, r):
    """(columns, values) of row r without its diagonal value, in the order the header defines: before the centre the axes z, y, x,
    each with its wrapped +d links (d ascending) and then its interior -d links (d = R ... 1); after it the axes x, y, z, each with
    its interior +d links (d = 1 ... R) and then its wrapped -d links (d = R ... 1)."""
    ndim = len(shape)
    ext = list(shape) + [1] * (3 - ndim)
    pr = list(per) + [False] * (3 - ndim)
    stride = [1, ext[0], ext[0] * ext[1]]
    idx = [r % ext[0], (r // ext[0]) % ext[1], r // (ext[0] * ext[1])]
    c = ndim * R
    cols, vals = [], []
    for a in (2, 1, 0):
        if a >= ndim:
            continue
        m, i = ext[a], idx[a]
        if pr[a]:
            for d in range(1, R + 1):
                if i + d >= m:
                    cols.append(r + (d - m) * stride[a]); vals.append(w[c + a * R + d - 1])
        for d in range(R, 0, -1):
            if i - d >= 0:
                cols.append(r - d * stride[a]); vals.append(t[c - a * R - d])
    cols.append(r); vals.append(None)
    for a in (0, 1, 2):
        if a >= ndim:
            continue
        m, i = ext[a], idx[a]
        for d in range(1, R + 1):
            if i + d < m:
                cols.append(r + d * stride[a]); vals.append(t[c + a * R + d])
        if pr[a]:
            for d in range(R, 0, -1):
                if i - d < 0:
                    cols.append(r + (m - d) * stride[a]); vals.append(w[c - a * R - d])
    return cols, vals


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", sc.RADII)
def test_every_wrapped_entry_stands_at_its_defined_place_in_the_row(R, dtype):
    m = 2 * R + 1
    for shape, per in [((m, m, m), sp_.ALL), ((2 * R + 2, m + 2, 3), (True, True, False)), ((m, m + 1), (False, True))]:
        t, w = sc.taps(len(shape), R, dtype), sp_.wrap(len(shape), R, dtype)
        A = pkg.host_grid_star_matrix(shape, t, R, periodic=per, wrap=w)
        for r in range(A.shape[0]):
            cols, vals = _row_by_definition(shape, per, R, t, w, r)
            lo, hi = A.indptr[r], A.indptr[r + 1]
            assert A.indices[lo:hi].tolist() == cols, (shape, r)
            for got, want in zip(A.data[lo:hi], vals):
                assert want is None or np.array_equal(_bits(np.asarray([got], dtype=dtype)), _bits(np.asarray([want], dtype=dtype))), (shape, r)
            assert A.data[lo + cols.index(r)] == t[len(shape) * R]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", sc.RADII)
def test_reductions_to_the_open_star_and_to_the_radius_one_periodic_matrix(R, dtype):
    for shape in [(7,), (5, 4), (6, 5, 4), (1, 5, 3), (33, 34, 9)]:
        ndim = len(shape)
        t, v = sc.taps(ndim, R, dtype), sc.potential(shape, dtype)
        for pot in (None, v):
            want = pkg.host_grid_matrix(shape, t, pot, radius=R)
            for kw in (dict(), dict(periodic=False), dict(periodic=(False,) * ndim, wrap=sp_.wrap(ndim, R, dtype))):
                _same_matrix(pkg.host_grid_star_matrix(shape, t, R, pot, **kw), want)
    for shape, per in gp.CASES_ALL[:2] + gp.CASES_MIXED[1:] + gp.CASES_2D[:1] + [((7,), (True,))]:
        ndim = len(shape)
        t, v, w = gc.taps(ndim, dtype), gc.potential(shape, dtype), gp.wrap(ndim, dtype)
        for pot in (None, v):
            for wv in (None, w):
                _same_matrix(pkg.host_grid_star_matrix(shape, t, 1, pot, periodic=per, wrap=wv),
                             pkg.host_grid_matrix(shape, t, pot, periodic=per, wrap=wv))


@pytest.mark.parametrize("R", (1,) + sc.RADII)
def test_bloch_wraps_give_an_exactly_hermitian_matrix(R):
    theta = (0.7, 1.1, 1.9)
    for shape in [(11,), (2 * R + 1, 12), (12, 10, 9)]:
        ndim = len(shape)
        t = extras.fd_laplacian_taps(ndim, 2 * R)
        w = extras.bloch_wrap(t, theta[:ndim], radius=R)
        assert w.shape == (2 * ndim * R,) and w.dtype == np.complex128
        A = pkg.host_grid_star_matrix(shape, t, R, gc.harmonic(shape), periodic=True, wrap=w)
        assert A.dtype == np.complex128
        assert (A != A.conj().T).nnz == 0
        # theta = 0: the plain torus, bit for bit
        w0 = extras.bloch_wrap(t, np.zeros(ndim), radius=R)
        assert np.array_equal(_bits(w0), _bits(sp_.taps_as_wrap(t, ndim, R).astype(np.complex128)))
        _same_matrix(pkg.host_grid_star_matrix(shape, t.astype(np.complex128), R, periodic=True, wrap=w0),
                     pkg.host_grid_star_matrix(shape, t.astype(np.complex128), R, periodic=True))


def test_bloch_ring_has_the_analytic_eigenvalues():
    """1-D ring, m = 11, R = 4: w_0 + 2 sum_d w_d cos(d (2 pi k + theta) / m), to 1e-12 relative to ||A||."""
    m, R, theta = 11, 4, 0.7
    t = extras.fd_laplacian_taps(1, 8)
    A = pkg.host_grid_star_matrix((m,), t, R, periodic=True, wrap=extras.bloch_wrap(t, [theta], radius=R)).toarray()
    q = (2 * np.pi * np.arange(m) + theta) / m
    want = np.sort(t[R] + 2 * sum(t[R + d] * np.cos(d * q) for d in range(1, R + 1)))
    got = np.linalg.eigvalsh(A)
    assert np.abs(got - want).max() <= 1e-12 * np.linalg.norm(A, 2)


def test_bloch_wrap_of_radius_one_has_the_bits_of_the_existing_function():
    theta = (0.7, 1.1, 1.9)
    for ndim in (1, 2, 3):
        for dtype in DTYPES:
            t = gc.taps(ndim, dtype)
            old = extras.bloch_wrap(t, theta[:ndim])
            want = np.empty(2 * ndim, dtype=np.complex128)
            for a in range(ndim):
                want[ndim - 1 - a] = t[ndim - 1 - a] * np.exp(-1j * theta[a])
                want[ndim + a] = t[ndim + 1 + a] * np.exp(1j * theta[a])
            assert np.array_equal(_bits(old), _bits(want))
            assert np.array_equal(_bits(extras.bloch_wrap(t, theta[:ndim], radius=1)), _bits(want))
    # the radius is never inferred from the length: 13 taps are a 3-D star of radius 2 or a 2-D star of radius 3
    t13 = np.arange(13.0)
    assert extras.bloch_wrap(t13, theta, radius=2).shape == (12,)
    assert extras.bloch_wrap(t13, theta[:2], radius=3).shape == (12,)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        extras.bloch_wrap(t13, theta)
    with pytest.raises(pkg.DimensionMismatch, match="theta"):
        extras.bloch_wrap(t13, theta, radius=3)
    with pytest.raises(pkg.ArgumentError, match="radius"):
        extras.bloch_wrap(t13, theta, radius=5)
    # every +-d link of an axis carries the same phase
    w = extras.bloch_wrap(np.ones(13), theta, radius=2)
    assert np.array_equal(w[:6], np.exp(-1j * np.repeat(theta[::-1], 2))) and np.array_equal(w[6:], np.exp(1j * np.repeat(theta, 2)))


def test_refusals_name_their_cause():
    for R in sc.RADII:
        t = sc.taps(3, R, np.float64)
        m = 2 * R + 1
        for a, shape in enumerate([(2 * R, m, m), (m, 2 * R, m), (m, m, 2 * R)]):
            with pytest.raises(pkg.ArgumentError, match=r"(?s)periodic axis %d.*extent %d.*radius %d" % (a, 2 * R, R)):
                pkg.host_grid_star_matrix(shape, t, R, periodic=True)
            per = tuple(b != a for b in range(3))
            assert pkg.host_grid_star_matrix(shape, t, R, periodic=per).shape == (2 * R * m * m,) * 2   # (the short axis is open)
        for bad in (np.ones(6 * R - 1), np.ones(6), np.ones((6, R))):
            if bad.shape != (6 * R,):
                with pytest.raises(pkg.DimensionMismatch, match="wrap"):
                    pkg.host_grid_star_matrix((m, m, m), t, R, periodic=True, wrap=bad)
        # a non-finite wrap value of a periodic axis, by its index; of an open axis: neither read nor checked
        for k in (0, 2 * R, 3 * R - 1, 3 * R, 6 * R - 1):
            w = sp_.wrap(3, R, np.float64)
            w[k] = np.nan
            with pytest.raises(pkg.ArgumentError, match=r"wrap value %d\b.*not finite" % k):
                pkg.host_grid_star_matrix((m, m, m), t, R, periodic=True, wrap=w)
        w = sp_.wrap(3, R, np.float64)
        w[3 * R - 1] = w[3 * R] = np.inf       # -1 x and +1 x
        assert pkg.host_grid_star_matrix((m, m, m), t, R, periodic=(False, True, True), wrap=w).nnz == sp_.nnz((m, m, m), (False, True, True), R)
        # an imaginary wrap with a pinned Float64; a complex wrap promotes otherwise
        wc = sp_.wrap(3, R, np.complex128)
        with pytest.raises(pkg.ArgumentError, match="imaginary"):
            pkg.host_grid_star_matrix((m, m, m), t, R, dtype=np.float64, periodic=True, wrap=wc)
        assert pkg.host_grid_star_matrix((m, m, m), t, R, periodic=True, wrap=wc).dtype == np.complex128
        assert pkg.host_grid_star_matrix((m, m, m), t, R, dtype=np.float64, periodic=True, wrap=wc.real + 0j).dtype == np.float64
    t2 = sc.taps(3, 2, np.float64)
    for radius in (0, 5, -1, 2.0, "2", None, True):
        with pytest.raises(pkg.ArgumentError, match="radius"):
            pkg.host_grid_star_matrix((5, 5, 5), t2, radius, periodic=True)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_star_matrix((5, 5, 5), t2, 3, periodic=True)
    with pytest.raises(pkg.DimensionMismatch, match="periodic"):
        pkg.host_grid_star_matrix((5, 5, 5), t2, 2, periodic=(True, True))
    # ... and at the C ABI: the radius, and a cap that is too small still reports nnz
    L = pkg._lib.load()
    dims = np.array([5, 6, 7], dtype=np.int64)
    flags = np.array([1, 0, 1], dtype=np.int32)
    want = sp_.nnz((5, 6, 7), (True, False, True), 2)
    rowptr, col, val = np.zeros(211, dtype=np.int64), np.zeros(want, dtype=np.int32), np.zeros(want)
    for radius in (0, 5):
        got = C.c_int64(-1)
        rc = L.ks_host_grid_matrix_star_periodic(3, dims.ctypes.data, radius, pkg._lib.KS_F64, np.ones(31).ctypes.data, None, flags.ctypes.data, None,
                                                 rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, want, C.byref(got))
        assert rc == pkg._lib.KS_ERR_ARGUMENT and "radius" in L.ks_last_error_string().decode()
    got = C.c_int64(-1)
    rc = L.ks_host_grid_matrix_star_periodic(3, dims.ctypes.data, 2, pkg._lib.KS_F64, t2.ctypes.data, None, flags.ctypes.data, None,
                                             rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, want - 1, C.byref(got))
    assert rc == pkg._lib.KS_ERR_ARGUMENT and got.value == want and "cap" in L.ks_last_error_string().decode()
    assert not rowptr.any() and not col.any() and not val.any()
    got = C.c_int64(-1)
    rc = L.ks_host_grid_matrix_star_periodic(3, dims.ctypes.data, 2, pkg._lib.KS_F64, t2.ctypes.data, None, flags.ctypes.data, None,
                                             rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, want, C.byref(got))
    assert rc == pkg._lib.KS_OK and got.value == want == rowptr[-1]
    # the existing functions still refuse periodic axes above radius 1, and say where to go
    with pytest.raises(pkg.ArgumentError, match="(?s)periodic.*radius.*grid_star_operator"):
        pkg.host_grid_matrix((5, 5, 5), t2, radius=2, periodic=True)
