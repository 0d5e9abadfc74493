"""`-m "not gpu"`: the definition of the matrix-free grid operator (`ks_operator_grid`, csrc/ks_grid.hpp) -- mul!(y, A, x),
src/expansion.jl:121, for a constant-coefficient stencil plus a per-point diagonal -- through its host function
`ks_host_grid_matrix` / `host_grid_matrix`: no device is touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_cases.py: Kronecker sums plus diags(centre + potential)); the refusals carry the reference's exception kinds."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import spmv_reference as ref
from __graft_entry__ import import_package

pkg = import_package()
EPS = ref.EPS
DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]

# 1-, 2- and 3-D, extents including 1 and 2
SHAPES = [(1,), (2,), (7,), (1, 1), (2, 1), (1, 2), (5, 4), (2, 9), (1, 1, 1), (2, 2, 2), (1, 5, 3), (4, 1, 3), (4, 3, 1), (6, 5, 4), (3, 2, 7)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64)


def _same_matrix(A, B):
    assert A.shape == B.shape and A.nnz == B.nnz, (A.shape, B.shape, A.nnz, B.nnz)
    assert A.dtype == B.dtype
    assert np.array_equal(A.indptr, B.indptr)
    assert np.array_equal(A.indices, B.indices)
    assert np.array_equal(_bits(A.data), _bits(B.data))


def _nnz(shape):
    nx, ny, nz = list(shape) + [1] * (3 - len(shape))
    return nx * ny * nz + 2 * ((nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix_is_the_kronecker_assembly_entry_for_entry(shape, dtype):
    """Seven distinct, non-symmetric taps; with and without a potential; the potential flat and as an array in C order."""
    t = gc.taps(len(shape), dtype)
    assert len(set(t.tolist())) == 2 * len(shape) + 1
    v = gc.potential(shape, dtype)
    for pot in (None, v, v.reshape(shape[::-1])):
        A = pkg.host_grid_matrix(shape, t, pot)
        want = gc.kron_matrix(shape, t, None if pot is None else v)
        assert want.nnz == _nnz(shape)      # (nothing cancelled in the reference assembly)
        _same_matrix(A, want)
        assert A.has_sorted_indices and A.dtype == np.dtype(dtype)


def test_element_type_is_promoted_like_the_tridiagonal_operator():
    t = np.array([-1, 2, -1])                                  # integers -> Float64
    assert pkg.host_grid_matrix((5,), t).dtype == np.float64
    assert pkg.host_grid_matrix((5,), t, np.zeros(5, dtype=np.complex128)).dtype == np.complex128
    assert pkg.host_grid_matrix((5,), t + 0j).dtype == np.complex128
    assert pkg.host_grid_matrix((5,), t, dtype=np.complex128).dtype == np.complex128
    # a pinned Float64 accepts complex input whose imaginary parts are zero
    _same_matrix(pkg.host_grid_matrix((5,), t + 0j, dtype=np.float64), pkg.host_grid_matrix((5,), t))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_zero_diagonal_entries_stay_stored(dtype):
    shape = (4, 3, 2)
    n = gc.size(shape)
    t = gc.taps(3, dtype)
    v = gc.potential(shape, dtype)
    v[[0, 5, n - 1]] = -t[3]             # centre + potential == 0 exactly
    A = pkg.host_grid_matrix(shape, t, v)
    assert A.nnz == _nnz(shape)
    d = A.diagonal()
    for r in range(n):
        row = A.indices[A.indptr[r] : A.indptr[r + 1]]
        assert np.count_nonzero(row == r) == 1, r
    assert np.all(d[[0, 5, n - 1]] == 0) and np.count_nonzero(d == 0) == 3
    assert np.array_equal(_bits(d), _bits(np.add(t[3], v)))
    # a zero TAP is stored as well: the pattern depends on the shape alone
    t0 = t.copy()
    t0[4] = 0
    B = pkg.host_grid_matrix(shape, t0, v)
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)


def _call(ndim, dims, dtype_code, taps, pot, cap):
    L = pkg._lib.load()
    dims = np.asarray(dims, dtype=np.int64)
    n = int(np.prod(dims[:ndim])) if 1 <= ndim <= 3 else 1
    rowptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int32), np.zeros(2 * max(cap, 1))
    nnz = C.c_int64(-1)
    rc = L.ks_host_grid_matrix(ndim, dims.ctypes.data, dtype_code, taps.ctypes.data, None if pot is None else pot.ctypes.data,
                               rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, cap, C.byref(nnz))
    return rc, nnz.value, L.ks_last_error_string().decode()


def test_too_small_capacity_reports_the_required_size():
    shape = (6, 5, 4)
    t = gc.taps(3, np.float64)
    need = _nnz(shape)
    rc, nnz, msg = _call(3, shape, pkg._lib.KS_F64, t, None, need - 1)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need and "cap" in msg and str(need) in msg
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, None, 0)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, None, need)
    assert rc == pkg._lib.KS_OK and nnz == need


def test_refusals_name_their_cause():
    t3, t1 = gc.taps(3, np.float64), gc.taps(1, np.float64)
    # ndim outside 1 ... 3: at the C ABI and through the Python layer
    for ndim in (0, 4, -1):
        rc, _, msg = _call(ndim, (3, 3, 3, 3), pkg._lib.KS_F64, np.ones(9), None, 1000)
        assert rc == pkg._lib.KS_ERR_ARGUMENT and "ndim" in msg, (ndim, msg)
    with pytest.raises(pkg.ArgumentError, match="ndim"):
        pkg.host_grid_matrix((2, 2, 2, 2), np.ones(9))
    with pytest.raises(pkg.ArgumentError, match="ndim"):
        pkg.host_grid_matrix((), np.ones(1))
    # an extent < 1
    for shape in ((0,), (4, 0, 3), (4, 3, -2)):
        with pytest.raises(pkg.ArgumentError, match="extent"):
            pkg.host_grid_matrix(shape, gc.taps(len(shape), np.float64))
    with pytest.raises(pkg.ArgumentError, match="extent"):
        pkg.host_grid_matrix((4, 0, 3), t3, np.zeros(5))
    # n, or the plane stride, beyond the 32-bit row index (refused before anything of that size is allocated)
    for shape in ((2 ** 31,), (2 ** 16, 2 ** 15), (2 ** 16, 2 ** 16, 1), (2 ** 11, 2 ** 10, 2 ** 10), (2 ** 40, 1, 1)):
        with pytest.raises(pkg.ArgumentError, match="32-bit"):
            pkg.host_grid_matrix(shape, gc.taps(len(shape), np.float64))
    # non-finite tap / potential entry
    for bad in (np.nan, np.inf, -np.inf):
        t = t3.copy()
        t[5] = bad
        with pytest.raises(pkg.ArgumentError, match="tap 5"):
            pkg.host_grid_matrix((3, 3, 3), t)
        v = np.zeros(27)
        v[13] = bad
        with pytest.raises(pkg.ArgumentError, match="potential entry 13"):
            pkg.host_grid_matrix((3, 3, 3), t3, v)
    tc = gc.taps(2, np.complex128)
    tc[0] = complex(1.0, np.nan)
    with pytest.raises(pkg.ArgumentError, match="tap 0"):
        pkg.host_grid_matrix((3, 3), tc)
    # an imaginary part where the element type is Float64
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.host_grid_matrix((3, 3), gc.taps(2, np.complex128), dtype=np.float64)
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.host_grid_matrix((3,), t1, np.array([0.0, 1.0j, 0.0]), dtype=np.float64)
    with pytest.raises(pkg.ArgumentError, match="float64 or complex128"):
        pkg.host_grid_matrix((3,), t1, dtype=np.float32)
    # shape or length mismatches
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((3, 3), t3)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((3, 3, 3), t3.reshape(7, 1))
    with pytest.raises(pkg.DimensionMismatch, match="potential"):
        pkg.host_grid_matrix((4, 3, 2), t3, np.zeros(23))
    with pytest.raises(pkg.DimensionMismatch, match="potential"):
        pkg.host_grid_matrix((4, 3, 2), t3, np.zeros((4, 3, 2)))     # (nz, ny, nx) is (2, 3, 4)
    assert pkg.host_grid_matrix((4, 3, 2), t3, np.zeros((2, 3, 4))).shape == (24, 24)


def test_sequential_product_of_a_symmetric_case_agrees_with_the_dense_product():
    """8 x 7 x 6, symmetric taps and a real harmonic potential: A is symmetric, and seq_matvec -- the bits the device product
    promises -- agrees with the dense product within the bound of two sums of L = 7 rounded products, 2 (L + 1) eps |A| |x|."""
    shape = (8, 7, 6)
    t = gc.taps(3, np.float64, symmetric=True)
    A = pkg.host_grid_matrix(shape, t, gc.harmonic(shape))
    assert (A - A.T).nnz == 0 and A.nnz == _nnz(shape)
    x = gc.vector(shape, np.float64)
    y = ref.seq_matvec(A, x)
    assert np.array_equal(y, ref.seq_matvec_loop(A, x))
    D = A.toarray()
    w = np.abs(D) @ np.abs(x)
    assert np.all(np.abs(y - D @ x) <= 2 * 8 * EPS * w)
    # the harmonic potential is laid out as documented: it depends on the distance from the centre only
    V = gc.harmonic(shape).reshape(shape[::-1])
    assert V[0, 0, 0] == V[-1, -1, -1] == V[0, -1, 0] == V.max() and V[2, 3, 3] == V.min()
