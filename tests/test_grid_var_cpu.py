"""`-m "not gpu"`: the definition of the matrix-free variable-coefficient grid operator (`ks_operator_grid_var`,
csrc/ks_grid_var.hpp) -- mul!(y, A, x), src/expansion.jl:121, for A = -div(c(x) grad) + V(x) -- through its host function
`ks_host_grid_var_matrix` / `host_grid_variable_matrix`, and `extras.diffusion_terms`: no device is touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_var_cases.py: index masks per direction, h[k] * (c[r] + c[s]) on real arrays); with c == 1 it must be the matrix of
`host_grid_matrix`; the refusals carry the reference's exception kinds."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_var_cases as vc
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
@pytest.mark.parametrize("shapes", [gc.SHAPES_1D, gc.SHAPES_2D, gc.SHAPES_3D], ids=["1d", "2d", "3d"])
def test_matrix_is_the_independent_assembly_entry_for_entry(shapes, dtype):
    """Non-symmetric taps, the random coefficient, with and without a potential; coefficient and potential flat and in C order."""
    for shape in shapes:
        t = gc.taps(len(shape), dtype)
        c, v = vc.random_coeff(shape), gc.potential(shape, dtype)
        for pot in (None, v):
            want = vc.assemble(shape, t, c, pot)
            assert want.nnz == vc.nnz(shape)
            A = pkg.host_grid_variable_matrix(shape, t, c, pot)
            _same_matrix(A, want)
            assert A.has_sorted_indices and A.dtype == np.dtype(dtype)
        B = pkg.host_grid_variable_matrix(shape, t, c.reshape(shape[::-1]), v.reshape(shape[::-1]))
        _same_matrix(B, want)


def test_the_smooth_field_with_a_jump_and_a_real_coefficient_of_any_sign():
    shape = (12, 10, 9)
    c = vc.coeff(shape)
    assert c.min() >= 0.5 and c.max() <= 3.0 and np.count_nonzero(c > 2.0) > 0
    t = gc.taps(3, np.complex128)
    _same_matrix(pkg.host_grid_variable_matrix(shape, t, c), vc.assemble(shape, t, c))
    cn = c - 1.25                                    # no sign requirement
    assert cn.min() < 0 < cn.max()
    _same_matrix(pkg.host_grid_variable_matrix(shape, t.real.copy(), cn), vc.assemble(shape, t.real.copy(), cn))
    # integers are taken as Float64; a complex operator keeps a real coefficient
    A = pkg.host_grid_variable_matrix((5,), np.array([-1, 0, -1]), np.arange(1, 6), dtype=np.complex128)
    assert A.dtype == np.complex128 and np.array_equal(A.diagonal(1), -0.5 * (np.arange(1, 5) + np.arange(2, 6)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unit_coefficient_gives_the_bits_of_the_constant_coefficient_matrix(dtype):
    for shape in [(7,), (5, 4), (6, 5, 4), (1, 5, 3), (33, 5, 9)]:
        t, v = gc.taps(len(shape), dtype), gc.potential(shape, dtype)
        for pot in (None, v):
            _same_matrix(pkg.host_grid_variable_matrix(shape, t, np.ones(gc.size(shape)), pot), pkg.host_grid_matrix(shape, t, pot))


def _call(ndim, dims, dtype_code, taps, coeff, pot, cap):
    L = pkg._lib.load()
    dims = np.asarray(dims, dtype=np.int64)
    n = int(np.prod(dims[:ndim])) if 1 <= ndim <= 3 else 1
    rowptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int32), np.zeros(2 * max(cap, 1))
    nnz = C.c_int64(-1)
    rc = L.ks_host_grid_var_matrix(ndim, dims.ctypes.data, dtype_code, taps.ctypes.data, None if coeff is None else coeff.ctypes.data,
                                   None if pot is None else pot.ctypes.data, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, cap,
                                   C.byref(nnz))
    return rc, nnz.value, L.ks_last_error_string().decode()


def test_nnz_follows_the_formula_and_a_too_small_capacity_reports_it():
    for shape in [(7,), (1,), (5, 4), (1, 9), (6, 5, 4), (4, 1, 3), (2, 2, 2)]:
        assert pkg.host_grid_variable_matrix(shape, gc.taps(len(shape), np.float64), vc.coeff(shape)).nnz == vc.nnz(shape)
    shape = (6, 5, 4)
    t, c = gc.taps(3, np.float64), vc.coeff(shape)
    need = vc.nnz(shape)
    rc, nnz, msg = _call(3, shape, pkg._lib.KS_F64, t, c, None, need - 1)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need and "cap" in msg and str(need) in msg
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, c, None, 0)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need
    rc, nnz, _ = _call(3, shape, pkg._lib.KS_F64, t, c, None, need)
    assert rc == pkg._lib.KS_OK and nnz == need


def test_refusals_name_their_cause():
    t3 = gc.taps(3, np.float64)
    c27 = np.ones(27)
    # a coefficient of the wrong shape, a complex one, a missing one (at the C ABI)
    with pytest.raises(pkg.DimensionMismatch, match="coeff"):
        pkg.host_grid_variable_matrix((4, 3, 2), t3, np.ones(23))
    with pytest.raises(pkg.DimensionMismatch, match="coeff"):
        pkg.host_grid_variable_matrix((4, 3, 2), t3, np.ones((4, 3, 2)))     # (nz, ny, nx) is (2, 3, 4)
    assert pkg.host_grid_variable_matrix((4, 3, 2), t3, np.ones((2, 3, 4))).shape == (24, 24)
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, c27 + 0j)
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        pkg.host_grid_variable_matrix((3, 3, 3), gc.taps(3, np.complex128), c27 * (1 + 1j))
    rc, _, msg = _call(3, (3, 3, 3), pkg._lib.KS_F64, t3, None, None, 1000)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and "coeff" in msg
    # non-finite coefficient, tap, potential entry: by index
    for bad in (np.nan, np.inf, -np.inf):
        c = c27.copy()
        c[13] = bad
        with pytest.raises(pkg.ArgumentError, match="coefficient entry 13 is not finite"):
            pkg.host_grid_variable_matrix((3, 3, 3), t3, c)
        t = t3.copy()
        t[5] = bad
        with pytest.raises(pkg.ArgumentError, match="tap 5"):
            pkg.host_grid_variable_matrix((3, 3, 3), t, c27)
        v = np.zeros(27)
        v[13] = bad
        with pytest.raises(pkg.ArgumentError, match="potential entry 13"):
            pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, v)
    # an extent of 0, ndim outside 1 ... 3, the wrong number of taps, an imaginary part under a pinned Float64
    for shape in ((0,), (4, 0, 3)):
        with pytest.raises(pkg.ArgumentError, match="extent"):
            pkg.host_grid_variable_matrix(shape, gc.taps(len(shape), np.float64), np.ones(0))
    with pytest.raises(pkg.ArgumentError, match="ndim"):
        pkg.host_grid_variable_matrix((2, 2, 2, 2), np.ones(9), np.ones(16))
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_variable_matrix((3, 3), t3, np.ones(9))
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.host_grid_variable_matrix((3, 3, 3), np.ones(13), c27)
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.host_grid_variable_matrix((3, 3), gc.taps(2, np.complex128), np.ones(9), dtype=np.float64)


# ------------------------------------------------------------------------------------------------ extras.diffusion_terms
@pytest.mark.parametrize("shape", [(9,), (6, 5), (6, 5, 4)], ids=["1d", "2d", "3d"])
def test_diffusion_terms_of_a_unit_coefficient_are_the_laplacian_exactly(shape):
    ndim, n = len(shape), gc.size(shape)
    taps, diag = extras.diffusion_terms(shape, np.ones(n))
    lap = extras.fd_laplacian_taps(ndim, 2)
    assert taps[ndim] == 0.0 and np.array_equal(np.delete(taps, ndim), np.delete(lap, ndim))
    assert diag.shape == (n,) and np.array_equal(_bits(diag), _bits(np.full(n, lap[ndim])))
    _same_matrix(pkg.host_grid_variable_matrix(shape, taps, np.ones(n), diag), pkg.host_grid_matrix(shape, lap))
    # a potential is added once, on top; flat or in C order
    V = gc.harmonic(shape)
    _t, dv = extras.diffusion_terms(shape, np.ones(shape[::-1]), potential=V.reshape(shape[::-1]))
    assert np.array_equal(_bits(dv), _bits(lap[ndim] + V))


def _diffusion(shape, boundary, spacing=1.0):
    c = vc.coeff(shape)
    taps, diag = extras.diffusion_terms(shape, c, spacing=spacing, boundary=boundary)
    return taps, pkg.host_grid_variable_matrix(shape, taps, c, diag)


@pytest.mark.parametrize("boundary", ["dirichlet", "neumann"])
def test_diffusion_matrix_is_symmetric_also_with_a_spacing_per_axis(boundary):
    for shape, h in [((12, 10, 9), 1.0), ((12, 10, 9), (0.5, 0.75, 1.25)), ((17, 6), (0.3, 1.0)), ((11,), 0.1)]:
        taps, A = _diffusion(shape, boundary, h)
        ndim = len(shape)
        hh = np.full(ndim, h) if np.ndim(h) == 0 else np.asarray(h)
        assert np.array_equal(taps[ndim + 1 :], -1.0 / (hh * hh)) and np.array_equal(taps[:ndim], taps[ndim + 1 :][::-1])
        assert (A - A.T).nnz == 0            # c[r] + c[s] is commutative: the two entries of a link are the same bits
        assert np.all(A.diagonal() > 0) and A.nnz == vc.nnz(shape)


def test_diffusion_spectrum_of_the_solve_case_is_well_separated():
    """12 x 10 x 9, Dirichlet: the matrix tests/test_gpu_grid_var.py solves, without its harmonic term.  (With the jump at
    x > nx // 2 = 6 as vc.coeff places it; at x > 5 the lowest five are 0.322, 0.554, 0.602, 0.645, 0.787.)"""
    _taps, A = _diffusion((12, 10, 9), "dirichlet")
    w = np.linalg.eigvalsh(A.toarray())[:5]
    assert np.allclose(w, [0.2954, 0.5247, 0.5615, 0.6043, 0.7517], atol=5e-4), w
    assert np.diff(w).min() > 0.03


@pytest.mark.parametrize("shape", [(9,), (6, 5), (12, 10, 9)], ids=["1d", "2d", "3d"])
def test_neumann_rows_sum_to_zero_up_to_rounding(shape):
    """|A 1|[r] <= 2 ndim eps sum_k |e_k|: the diagonal is a rounded sum of at most 2 ndim terms, and A 1 adds them back."""
    _taps, A = _diffusion(shape, "neumann", 0.7)
    off = abs(A).sum(axis=1).A1 - np.abs(A.diagonal())
    rows = np.abs(A @ np.ones(A.shape[0]))
    print("largest |A 1| / (eps sum |e_k|):", (rows / np.maximum(off, 1e-300)).max() / EPS)
    assert np.all(rows <= 2 * len(shape) * EPS * off)
    import math

    exact = np.array([abs(math.fsum(A.data[A.indptr[r] : A.indptr[r + 1]])) for r in range(A.shape[0])])   # the diagonal's own rounding
    assert np.all(exact <= 2 * len(shape) * EPS * off)
    # Dirichlet keeps the ghost links on the diagonal: boundary rows do not sum to zero
    _taps, D = _diffusion(shape, "dirichlet", 0.7)
    assert (D @ np.ones(D.shape[0])).max() > 0.1


def test_diffusion_terms_refusals():
    c = np.ones(20)
    with pytest.raises(pkg.ArgumentError, match="boundary"):
        extras.diffusion_terms((5, 4), c, boundary="periodic")
    with pytest.raises(pkg.ArgumentError, match="boundary"):
        extras.diffusion_terms((5, 4), c, boundary=None)
    for h in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="spacing"):
            extras.diffusion_terms((5, 4), c, spacing=h)
    with pytest.raises(pkg.DimensionMismatch, match="spacing"):
        extras.diffusion_terms((5, 4), c, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(pkg.DimensionMismatch, match="coeff"):
        extras.diffusion_terms((5, 4), np.ones(19))
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        extras.diffusion_terms((5, 4), c + 0j)
    with pytest.raises(pkg.DimensionMismatch, match="potential"):
        extras.diffusion_terms((5, 4), c, potential=np.ones(19))
    with pytest.raises(pkg.ArgumentError, match="ndim"):
        extras.diffusion_terms((2, 2, 2, 2), np.ones(16))
