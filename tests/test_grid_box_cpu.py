"""`-m "not gpu"`: the definition of the matrix-free box-stencil grid operator (`ks_operator_grid_box`, csrc/ks_grid_box.hpp) --
mul!(y, A, x), src/expansion.jl:121, for the 3-, 9- or 27-point stencil with the diagonal neighbours -- through its host function
`ks_host_grid_box_matrix` / `host_grid_box_matrix`, and the two tap helpers `extras.tensor_laplacian_taps` and `extras.q1_fem_taps`:
no device is touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_box_cases.py: a sum over the slots of Kronecker products of 1-D shift matrices); in 1-D, and with the taps of a 7-point
stencil embedded, it must be the matrix of `host_grid_matrix`; the refusals carry the reference's exception kinds."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import grid_box_cases as bc
import grid_cases as gc
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

EPS = np.finfo(np.float64).eps
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


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shapes", [bc.SHAPES_1D, bc.SHAPES_2D, bc.SHAPES_3D], ids=["1d", "2d", "3d"])
def test_matrix_is_the_independent_assembly_entry_for_entry(shapes, dtype):
    """Distinct non-symmetric taps, with and without a potential; the nnz formula; strictly ascending columns in every row; taps
    flat and of shape (3,) * ndim, the potential flat and in C order."""
    for shape in shapes:
        ndim = len(shape)
        t, v = bc.taps(ndim, dtype), gc.potential(shape, dtype)
        for pot in (None, v):
            want = bc.assemble(shape, t, pot)
            assert want.nnz == bc.nnz(shape)
            A = pkg.host_grid_box_matrix(shape, t, pot)
            _same_matrix(A, want)
            assert A.dtype == np.dtype(dtype)
            ascending = np.diff(A.indices.astype(np.int64)) > 0
            ascending[A.indptr[1:-1] - 1] = True          # (between the last entry of a row and the first of the next: no claim)
            assert np.all(ascending)
        B = pkg.host_grid_box_matrix(shape, t.reshape((3,) * ndim), v.reshape(shape[::-1]))
        _same_matrix(B, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_dimension_is_the_matrix_of_host_grid_matrix(dtype):
    for shape in bc.SHAPES_1D:
        t, v = bc.taps(1, dtype), gc.potential(shape, dtype)
        for pot in (None, v):
            _same_matrix(pkg.host_grid_box_matrix(shape, t, pot), pkg.host_grid_matrix(shape, t, pot))


def test_a_zero_tap_is_stored():
    for shape in [(5, 4), (6, 5, 4), (1, 5, 3)]:
        ndim = len(shape)
        t = bc.taps(ndim, np.float64)
        t[0] = 0.0                                          # a corner
        A = pkg.host_grid_box_matrix(shape, t)
        assert A.nnz == bc.nnz(shape) == pkg.host_grid_box_matrix(shape, bc.taps(ndim, np.float64)).nnz
        t[:] = 0.0                                          # ... and all of them, the centre included
        A = pkg.host_grid_box_matrix(shape, t)
        assert A.nnz == bc.nnz(shape) and not A.data.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_star_taps_embedded_give_the_star_matrix_after_eliminate_zeros(dtype):
    for shape in [(7,), (5, 4), (6, 5, 4), (1, 5, 3), (33, 5, 9)]:
        ndim = len(shape)
        t7, v = gc.taps(ndim, dtype), gc.potential(shape, dtype)
        for pot in (None, v):
            A = pkg.host_grid_box_matrix(shape, bc.embed_star(t7, ndim), pot)
            assert A.nnz == bc.nnz(shape)
            A.eliminate_zeros()
            _same_matrix(A, pkg.host_grid_matrix(shape, t7, pot))


def _call(ndim, dims, dtype_code, taps, pot, cap):
    L = pkg._lib.load()
    dims = np.asarray(dims, dtype=np.int64)
    n = int(np.prod(dims[:ndim])) if 1 <= ndim <= 3 else 1
    rowptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int32), np.zeros(2 * max(cap, 1))
    nnz = C.c_int64(-1)
    rc = L.ks_host_grid_box_matrix(ndim, dims.ctypes.data, dtype_code, taps.ctypes.data, None if pot is None else pot.ctypes.data,
                                   rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, cap, C.byref(nnz))
    return rc, nnz.value, L.ks_last_error_string().decode()


def test_nnz_follows_the_formula_and_a_too_small_capacity_reports_it():
    for shape in [(7,), (1,), (5, 4), (1, 9), (6, 5, 4), (4, 1, 3), (2, 2, 2), (1, 1, 1)]:
        assert pkg.host_grid_box_matrix(shape, bc.taps(len(shape), np.float64)).nnz == bc.nnz(shape)
    assert bc.nnz((6, 5, 4)) == 16 * 13 * 10 and bc.nnz((2, 2, 2)) == 64
    shape = (6, 5, 4)
    t = bc.taps(3, np.float64)
    need = bc.nnz(shape)
    rc, nnz, msg = _call(3, shape, pkg._lib.KS_F64, t, None, need - 1)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need and "cap" in msg and str(need) in msg
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, None, 0)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, None, need)
    assert rc == pkg._lib.KS_OK and nnz == need


def test_refusals_name_their_cause():
    t3 = bc.taps(3, np.float64)
    # the wrong number of taps: a star stencil's 7, the 2-D 9 on a 3-D grid, a (3, 3) array on a 3-D grid
    for shape, t in (((3, 3, 3), gc.taps(3, np.float64)), ((3, 3, 3), bc.taps(2, np.float64)), ((3, 3), t3),
                     ((3, 3, 3), np.ones((3, 3))), ((4,), np.ones(5))):
        with pytest.raises(pkg.DimensionMismatch, match="taps"):
            pkg.host_grid_box_matrix(shape, t)
    # a non-finite tap by its index (every one of the 27), a non-finite potential entry by its index
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 6, 7, 13, 26):
            t = t3.copy()
            t[k] = bad
            with pytest.raises(pkg.ArgumentError, match="tap %d is not finite" % k):
                pkg.host_grid_box_matrix((3, 3, 3), t)
        t = bc.taps(2, np.complex128)
        t[8] = complex(1.0, bad)
        with pytest.raises(pkg.ArgumentError, match="tap 8 is not finite"):
            pkg.host_grid_box_matrix((3, 3), t)
        v = np.zeros(27)
        v[13] = bad
        with pytest.raises(pkg.ArgumentError, match="potential entry 13"):
            pkg.host_grid_box_matrix((3, 3, 3), t3, v)
    # an extent of 0, ndim outside 1 ... 3, a potential of the wrong shape, an imaginary part under a pinned Float64
    for shape in ((0,), (4, 0, 3)):
        with pytest.raises(pkg.ArgumentError, match="extent"):
            pkg.host_grid_box_matrix(shape, bc.taps(len(shape), np.float64))
    with pytest.raises(pkg.ArgumentError, match="ndim"):
        pkg.host_grid_box_matrix((2, 2, 2, 2), np.ones(81))
    with pytest.raises(pkg.DimensionMismatch, match="potential"):
        pkg.host_grid_box_matrix((3, 3, 3), t3, np.ones(26))
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.host_grid_box_matrix((3, 3), bc.taps(2, np.complex128), dtype=np.float64)


# ------------------------------------------------------------------------------------------------ extras.tensor_laplacian_taps
TENSOR = np.array([[1.0, 0.3, 0.2], [0.3, 1.5, 0.25], [0.2, 0.25, 2.0]])


def test_tensor_laplacian_matrix_is_symmetric_also_with_a_spacing_per_axis():
    for shape, h in [((12, 10, 9), 1.0), ((7, 6, 5), (0.5, 0.75, 1.25)), ((9, 6), (0.3, 1.0)), ((11,), 0.1)]:
        ndim = len(shape)
        t = extras.tensor_laplacian_taps(TENSOR[:ndim, :ndim], spacing=h)
        assert t.shape == (3 ** ndim,) and np.array_equal(t, t[::-1])     # the slot of -d is the mirror image of the slot of d
        A = pkg.host_grid_box_matrix(shape, t, gc.harmonic(shape))
        assert (A - A.T).nnz == 0 and A.nnz == bc.nnz(shape)


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_tensor_laplacian_of_a_diagonal_tensor_is_the_star_laplacian(ndim):
    h = (0.5, 0.75, 1.25)[:ndim]
    assert np.array_equal(_bits(extras.tensor_laplacian_taps(np.eye(ndim), spacing=h, scale=0.5)),
                          _bits(bc.embed_star(extras.fd_laplacian_taps(ndim, 2, spacing=h, scale=0.5), ndim).ravel()))
    d = np.array([1.0, 1.5, 2.0])[:ndim]
    t = extras.tensor_laplacian_taps(np.diag(d))
    per_axis = [extras.fd_laplacian_taps(1, 2, scale=d[a]) for a in range(ndim)]
    star = np.concatenate([[per_axis[a][0] for a in range(ndim - 1, -1, -1)], [sum(p[1] for p in per_axis)], [per_axis[a][2] for a in range(ndim)]])
    assert np.array_equal(t, bc.embed_star(star, ndim).ravel())


def test_tensor_laplacian_mixed_term_is_exact_on_x_times_y():
    """u = x y: -div(D grad u) = -2 D_xy, and second central differences are exact on it.  |row| <= 27 eps max|t| max|u| bounds the
    rounding of a 27-term sum whose terms are at most max|t| max|u|."""
    shape, h = (9, 8, 7), (0.5, 0.75, 1.25)
    t = extras.tensor_laplacian_taps(TENSOR, spacing=h)
    A = pkg.host_grid_box_matrix(shape, t)
    z, y, x = np.meshgrid(*[np.arange(m) * hh for m, hh in zip(shape[::-1], h[::-1])], indexing="ij")
    u = (x * y).ravel()
    iz, iy, ix = np.meshgrid(*[np.arange(m) for m in shape[::-1]], indexing="ij")
    interior = ((ix > 0) & (ix < shape[0] - 1) & (iy > 0) & (iy < shape[1] - 1) & (iz > 0) & (iz < shape[2] - 1)).ravel()
    err = np.abs((A @ u)[interior] + 2.0 * TENSOR[0, 1])
    bound = 27 * EPS * np.abs(t).max() * np.abs(u).max()
    print("largest error of the mixed term:", err.max(), "bound", bound)
    assert interior.sum() == 7 * 6 * 5 and err.max() <= bound
    # ... and likewise x z and y z
    for (a, b), w in (((0, 2), x * z), ((1, 2), y * z)):
        assert np.abs((A @ w.ravel())[interior] + 2.0 * TENSOR[a, b]).max() <= 27 * EPS * np.abs(t).max() * np.abs(w).max()


def test_tensor_laplacian_spectrum_of_the_solve_case_is_well_separated():
    """12 x 10 x 9 with the harmonic potential: the matrix tests/test_gpu_grid_box.py solves."""
    shape = (12, 10, 9)
    A = pkg.host_grid_box_matrix(shape, extras.tensor_laplacian_taps(TENSOR), gc.harmonic(shape))
    w = np.linalg.eigvalsh(A.toarray())[:5]
    assert np.allclose(w[:4], [1.2605, 1.8938, 2.0971, 2.2998], atol=5e-4), w
    assert (np.diff(w[:4]) / w[1:4]).min() >= 0.08 and w[4] > w[3]


def test_tensor_laplacian_refusals():
    with pytest.raises(pkg.ArgumentError, match="symmetric"):
        extras.tensor_laplacian_taps([[1.0, 0.5], [0.25, 1.0]])
    for bad in (np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="finite"):
            extras.tensor_laplacian_taps([[1.0, bad], [bad, 1.0]])
    with pytest.raises(pkg.DimensionMismatch, match="D"):
        extras.tensor_laplacian_taps(np.eye(4))
    with pytest.raises(pkg.DimensionMismatch, match="D"):
        extras.tensor_laplacian_taps(np.ones((2, 3)))
    with pytest.raises(pkg.DimensionMismatch, match="spacing"):
        extras.tensor_laplacian_taps(np.eye(2), spacing=(1.0, 1.0, 1.0))
    for h in (0.0, -1.0, np.nan):
        with pytest.raises(pkg.ArgumentError, match="spacing"):
            extras.tensor_laplacian_taps(np.eye(2), spacing=h)


# ------------------------------------------------------------------------------------------------ extras.q1_fem_taps
def _q1_1d(m, h):
    K = sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1]) / h
    M = sp.diags([np.ones(m - 1), 4 * np.ones(m), np.ones(m - 1)], [-1, 0, 1]) * (h / 6.0)
    return K.tocsr(), M.tocsr()


@pytest.mark.parametrize("shape,h", [((7,), 0.3), ((6, 5), (0.5, 0.75)), ((6, 5, 4), (0.5, 0.75, 1.25)), ((5, 4, 3), 1.0)], ids=["1d", "2d", "3d", "3d-unit"])
def test_q1_matrices_are_the_kronecker_products_of_the_1d_matrices(shape, h):
    """Entries are products of up to three 1-D entries (and K a sum of three such): 8 eps relative to the largest entry covers the
    different association of the products here and in sp.kron."""
    ndim = len(shape)
    hh = np.full(ndim, h) if np.ndim(h) == 0 else np.asarray(h)
    kt, mt = extras.q1_fem_taps(ndim, spacing=h)
    assert kt.shape == mt.shape == (3 ** ndim,)
    K, M = pkg.host_grid_box_matrix(shape, kt), pkg.host_grid_box_matrix(shape, mt)
    one = [_q1_1d(m, x) for m, x in zip(shape, hh)]     # axis 0 = x is the fastest: the LAST Kronecker factor

    def kron(parts):
        out = parts[ndim - 1]
        for a in range(ndim - 2, -1, -1):
            out = sp.kron(out, parts[a])
        return out.toarray()

    Mref = kron([one[a][1] for a in range(ndim)])
    Kref = sum(kron([one[b][0] if b == a else one[b][1] for b in range(ndim)]) for a in range(ndim))
    assert np.abs(M.toarray() - Mref).max() <= 8 * EPS * np.abs(Mref).max()
    assert np.abs(K.toarray() - Kref).max() <= 8 * EPS * np.abs(Kref).max()
    assert (K - K.T).nnz == 0 and (M - M.T).nnz == 0
    # the mass taps sum to the cell volume, the stiffness taps to zero: interior rows of K sum to zero
    assert abs(mt.sum() - np.prod(hh)) <= 27 * EPS * np.prod(hh)
    assert abs(kt.sum()) <= 27 * EPS * np.abs(kt).max()
    idx = np.meshgrid(*[np.arange(m) for m in shape[::-1]], indexing="ij")
    interior = np.all([(i > 0) & (i < m - 1) for i, m in zip(idx, shape[::-1])], axis=0).ravel()
    assert interior.any() and np.abs((K @ np.ones(K.shape[0]))[interior]).max() <= 27 * EPS * np.abs(kt).max()


def test_q1_lowest_generalized_eigenvalue_is_the_closed_form():
    """6 x 5 x 4: the eigenvectors of the pair are products of sines, lambda = sum_a 6 (1 - cos th_a) / ((2 + cos th_a) h_a^2) with
    th_a = pi / (m_a + 1).  1e-12 relative: a dense 120 x 120 eigh against a closed form."""
    shape, h = (6, 5, 4), (0.5, 0.75, 1.25)
    kt, mt = extras.q1_fem_taps(3, spacing=h)
    K, M = pkg.host_grid_box_matrix(shape, kt).toarray(), pkg.host_grid_box_matrix(shape, mt).toarray()
    w = scipy.linalg.eigh(K, M, eigvals_only=True)
    th = [np.pi / (m + 1) for m in shape]
    exact = sum(6.0 * (1.0 - np.cos(t)) / ((2.0 + np.cos(t)) * x * x) for t, x in zip(th, h))
    print("lowest generalized Q1 eigenvalue:", w[0], "closed form", exact)
    assert abs(w[0] - exact) <= 1e-12 * exact


def test_q1_refusals():
    for nd in (0, 4, 2.0, True):
        with pytest.raises(pkg.ArgumentError, match="ndim"):
            extras.q1_fem_taps(nd)
    with pytest.raises(pkg.DimensionMismatch, match="spacing"):
        extras.q1_fem_taps(2, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(pkg.ArgumentError, match="spacing"):
        extras.q1_fem_taps(2, spacing=0.0)
