"""`-m "not gpu"`: the definition of the star-stencil grid operator of radius 2-4 (`ks_operator_grid_star`, csrc/ks_grid.hpp) --
mul!(y, A, x), src/expansion.jl:121, for central differences of order 4, 6, 8 plus a per-point diagonal -- through its host
function `ks_host_grid_matrix_star` / `host_grid_matrix(..., radius=R)`, and the taps of `extras.fd_laplacian_taps`: no device is
touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_star_cases.py: Kronecker sums of 1-D parts with diagonals at +-1 ... +-R plus diags(centre + potential)), for every
shape the device tests use."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import grid_cases as gc
import grid_star_cases as sc
import spmv_reference as ref
from __graft_entry__ import import_package

pkg = import_package()
EPS = ref.EPS
DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
SMALL = [(1,), (2,), (7,), (2, 1), (1, 2), (5, 4), (2, 9), (1, 1, 1), (2, 2, 2), (1, 5, 3), (4, 1, 3), (6, 5, 4), (3, 2, 7), (9, 9, 9)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_matrix(A, B):
    assert A.shape == B.shape and A.nnz == B.nnz, (A.shape, B.shape, A.nnz, B.nnz)
    assert A.dtype == B.dtype
    assert np.array_equal(A.indptr, B.indptr)
    assert np.array_equal(A.indices, B.indices)
    assert np.array_equal(_bits(A.data), _bits(B.data))


def _all_shapes(R):
    return list(dict.fromkeys(SMALL + sc.shapes_1d(R) + sc.shapes_2d(R) + sc.shapes_3d(R) + sc.EDGE_SHAPES))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", sc.RADII)
def test_matrix_is_the_kronecker_assembly_entry_for_entry(R, dtype):
    """Distinct, non-symmetric taps in every slot; with and without a potential; columns ascend strictly; nnz by the formula."""
    for shape in _all_shapes(R):
        t = sc.taps(len(shape), R, dtype)
        assert len(set(t.tolist())) == 2 * len(shape) * R + 1
        v = sc.potential(shape, dtype)
        for pot in (None, v):
            A = pkg.host_grid_matrix(shape, t, pot, radius=R)
            want = sc.kron_matrix(shape, R, t, pot)
            assert want.nnz == sc.nnz(shape, R), shape      # (nothing cancelled in the reference assembly)
            _same_matrix(A, want)
            assert A.dtype == np.dtype(dtype)
            rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
            same_row = rows[1:] == rows[:-1]
            assert np.all(np.diff(A.indices.astype(np.int64))[same_row] > 0), shape
    # the potential as an array in C order
    shape = (6, 5, 4)
    t, v = sc.taps(3, R, dtype), sc.potential(shape, dtype)
    _same_matrix(pkg.host_grid_matrix(shape, t, v.reshape(shape[::-1]), radius=R), pkg.host_grid_matrix(shape, t, v, radius=R))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radius_one_returns_the_arrays_of_the_existing_call(dtype):
    L = pkg._lib.load()
    for shape in [(7,), (5, 4), (6, 5, 4), (1, 5, 3)]:
        t, v = gc.taps(len(shape), dtype), gc.potential(shape, dtype)
        for pot in (None, v):
            A = pkg.host_grid_matrix(shape, t, pot)
            _same_matrix(pkg.host_grid_matrix(shape, t, pot, radius=1), A)
            # ... and the new symbol itself with radius 1
            dims = np.asarray(shape, dtype=np.int64)
            rowptr, col, val = np.zeros(A.shape[0] + 1, dtype=np.int64), np.zeros(A.nnz, dtype=np.int32), np.zeros(A.nnz, dtype=dtype)
            got = C.c_int64(-1)
            rc = L.ks_host_grid_matrix_star(len(shape), dims.ctypes.data, 1, pkg._lib.KS_F64 if np.dtype(dtype).kind == "f" else pkg._lib.KS_C64,
                                            t.ctypes.data, None if pot is None else pot.ctypes.data, rowptr.ctypes.data, col.ctypes.data,
                                            val.ctypes.data, A.nnz, C.byref(got))
            assert rc == pkg._lib.KS_OK and got.value == A.nnz
            assert np.array_equal(rowptr, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(_bits(val), _bits(A.data))


@pytest.mark.parametrize("R", sc.RADII)
def test_zero_diagonal_entries_and_zero_taps_stay_stored(R):
    shape = (6, 5, 4)
    n = gc.size(shape)
    t = sc.taps(3, R, np.float64)
    v = sc.potential(shape, np.float64)
    v[[0, 5, n - 1]] = -t[3 * R]
    A = pkg.host_grid_matrix(shape, t, v, radius=R)
    assert A.nnz == sc.nnz(shape, R)
    d = A.diagonal()
    assert np.all(d[[0, 5, n - 1]] == 0) and np.array_equal(_bits(d), _bits(np.add(t[3 * R], v)))
    t0 = t.copy()
    t0[0] = t0[3 * R + 2] = 0
    B = pkg.host_grid_matrix(shape, t0, v, radius=R)
    assert np.array_equal(B.indptr, A.indptr) and np.array_equal(B.indices, A.indices)


@pytest.mark.parametrize("R", sc.RADII)
def test_sequential_product_of_a_symmetric_case_agrees_with_the_dense_product(R):
    """9 x 9 x 9 (the centre point has all its 6 R + 1 taps at every radius), symmetric taps and a real harmonic potential:
    A is symmetric, and seq_matvec -- the bits the device product promises -- agrees with the dense product within the bound of two
    sums of L = 6 R + 1 rounded products, 2 (L + 1) eps |A| |x|."""
    shape = (9, 9, 9)
    t = sc.taps(3, R, np.float64, symmetric=True)
    A = pkg.host_grid_matrix(shape, t, gc.harmonic(shape), radius=R)
    assert (A - A.T).nnz == 0 and A.nnz == sc.nnz(shape, R)
    assert np.diff(A.indptr).max() == 6 * R + 1
    x = gc.vector(shape, np.float64)
    y = ref.seq_matvec(A, x)
    assert np.array_equal(y, ref.seq_matvec_loop(A, x))
    D = A.toarray()
    w = np.abs(D) @ np.abs(x)
    L = 6 * R + 1
    assert np.all(np.abs(y - D @ x) <= 2 * (L + 1) * EPS * w)


def test_refusals_name_their_cause():
    t2 = sc.taps(3, 2, np.float64)
    for radius in (0, 5, -1, 2.0, "2", None, True):
        with pytest.raises(pkg.ArgumentError, match="radius"):
            pkg.host_grid_matrix((5, 5, 5), t2, radius=radius)
    # ... and at the C ABI
    L = pkg._lib.load()
    dims = np.array([5, 5, 5], dtype=np.int64)
    for radius in (0, 5):
        rowptr, col, val, got = np.zeros(126, dtype=np.int64), np.zeros(4000, dtype=np.int32), np.zeros(4000), C.c_int64(-1)
        rc = L.ks_host_grid_matrix_star(3, dims.ctypes.data, radius, pkg._lib.KS_F64, np.ones(31).ctypes.data, None, rowptr.ctypes.data,
                                        col.ctypes.data, val.ctypes.data, 4000, C.byref(got))
        assert rc == pkg._lib.KS_ERR_ARGUMENT and "radius" in L.ks_last_error_string().decode()
    # the tap count follows the radius and is never inferred from it
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((5, 5, 5), t2)                               # 13 taps, radius 1
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((5, 5, 5), t2, radius=3)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((5, 5, 5), gc.taps(3, np.float64), radius=2)  # 7 taps
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_matrix((5, 5), t2, radius=2)
    # a non-finite tap, by its index in the new layout
    for R in sc.RADII:
        for k in (0, 3 * R, 6 * R):
            t = sc.taps(3, R, np.float64)
            t[k] = np.inf
            with pytest.raises(pkg.ArgumentError, match=r"tap %d is not finite" % k):
                pkg.host_grid_matrix((5, 5, 5), t, radius=R)
    v = np.zeros(125)
    v[13] = np.nan
    with pytest.raises(pkg.ArgumentError, match="potential entry 13"):
        pkg.host_grid_matrix((5, 5, 5), t2, v, radius=2)
    with pytest.raises(pkg.ArgumentError, match="extent"):
        pkg.host_grid_matrix((5, 0, 5), t2, radius=2)
    # periodic axes take radius 1
    for kw in (dict(periodic=True), dict(periodic=(True, False, False)), dict(wrap=np.ones(6)), dict(periodic=False)):
        with pytest.raises(pkg.ArgumentError, match="(?s)(periodic.*radius)|(radius.*periodic)"):
            pkg.host_grid_matrix((5, 5, 5), t2, radius=2, **kw)


# ------------------------------------------------------------------------------------------------ fd_laplacian_taps
WEIGHTS = {
    2: [Fraction(2), Fraction(-1)],
    4: [Fraction(5, 2), Fraction(-4, 3), Fraction(1, 12)],
    6: [Fraction(49, 18), Fraction(-3, 2), Fraction(3, 20), Fraction(-1, 90)],
    8: [Fraction(205, 72), Fraction(-8, 5), Fraction(1, 5), Fraction(-8, 315), Fraction(1, 560)],
}


@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_fd_taps_are_the_exact_rational_weights(order):
    from arnoldimethod_jl_amd import extras  # noqa: F401
    ex = pkg.extras if hasattr(pkg, "extras") else extras
    R, w = order // 2, WEIGHTS[order]
    assert sum(w[1:]) * 2 + w[0] == 0                    # a constant has no second derivative
    assert sum(2 * d * d * w[d] for d in range(1, R + 1)) == -2   # ... and x^2 has -(x^2)'' = -2
    for ndim in (1, 2, 3):
        t = ex.fd_laplacian_taps(ndim, order)
        assert t.shape == (2 * ndim * R + 1,) and t.dtype == np.float64
        c = ndim * R
        for a in range(ndim):
            for d in range(1, R + 1):
                assert t[c - a * R - d] == t[c + a * R + d] == float(w[d])        # spacing 1: the rational, rounded once
        assert abs(t[c] - ndim * float(w[0])) <= 2 * EPS * ndim * float(w[0])
    # per-axis spacing (powers of two: exact), and a scale
    h = (0.5, 0.25, 2.0)
    t = ex.fd_laplacian_taps(3, order, spacing=h, scale=0.5)
    c = 3 * R
    for a in range(3):
        for d in range(1, R + 1):
            assert t[c - a * R - d] == t[c + a * R + d] == 0.5 * float(w[d]) / h[a] ** 2
    assert abs(t[c] - 0.5 * float(w[0]) * sum(1 / x ** 2 for x in h)) <= 4 * EPS * abs(t[c])
    assert np.array_equal(ex.fd_laplacian_taps(2, order, spacing=0.25), ex.fd_laplacian_taps(2, order, spacing=(0.25, 0.25)))
    with pytest.raises(pkg.ArgumentError, match="order"):
        ex.fd_laplacian_taps(3, order + 1)
    with pytest.raises(pkg.DimensionMismatch, match="spacing"):
        ex.fd_laplacian_taps(3, order, spacing=(1.0, 2.0))


@pytest.mark.parametrize("order,bound", [(2, 2.5e-3), (4, 5e-5), (6, 2e-6), (8, 1e-7)])
def test_fd_taps_converge_on_the_harmonic_oscillator(order, bound):
    """1/2 (-d^2/dx^2) + 1/2 x^2 on n = 64 points with h = 0.25: the lowest eigenvalue of the host matrix misses 1/2 by the
    truncation error of the order (computed with numpy: 1.96e-3, 3.99e-5, 1.37e-6, 6.6e-8)."""
    from arnoldimethod_jl_amd import extras
    n, h = 64, 0.25
    xs = (np.arange(n) - (n - 1) / 2.0) * h
    A = pkg.host_grid_matrix((n,), extras.fd_laplacian_taps(1, order, spacing=h, scale=0.5), 0.5 * xs * xs, radius=order // 2)
    lam = np.linalg.eigvalsh(A.toarray())[0]
    print("order %d: lowest eigenvalue %.12f, error %.3e" % (order, lam, abs(lam - 0.5)))
    assert abs(lam - 0.5) < bound
