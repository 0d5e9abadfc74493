"""`-m "not gpu"`: the definition of the matrix-free variable-coefficient grid operator with periodic axes
(`ks_operator_grid_var_periodic`, csrc/ks_grid_var.hpp) -- mul!(y, A, x), src/expansion.jl:121, for A = -div(c(x) grad) + V(x) on a
torus or with Bloch phases on the links that cross the cell boundary -- through its host function
`ks_host_grid_var_matrix_periodic` / `host_grid_variable_matrix(..., periodic=, wrap=)`, and `extras.diffusion_terms(...,
periodic=)`: no device is touched.

The matrix is compared entry for entry (pattern, order, value BITS) with an assembly that shares nothing with the library
(tests/grid_var_periodic_cases.py: index masks per direction for the interior and the wrapped links, h * (c[r] + c[s]) on real arrays,
rows sorted into ascending columns)."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_periodic_cases as gp
import grid_var_cases as vc
import grid_var_periodic_cases as vp
from __graft_entry__ import import_package
from test_grid_operator_cpu import _bits, _same_matrix

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

EPS = np.finfo(np.float64).eps
DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]


def _check_matrix(shape, per, dtype):
    ndim = len(shape)
    t, w = gc.taps(ndim, dtype), gp.wrap(ndim, dtype)
    c, v = vc.random_coeff(shape), gc.potential(shape, dtype)
    for wv in (None, w):
        for pot in (None, v):
            want = vp.assemble(shape, per, t, c, wv, pot)
            assert want.nnz == gp.nnz(shape, per)
            A = pkg.host_grid_variable_matrix(shape, t, c, pot, periodic=per, wrap=wv)
            _same_matrix(A, want)
            assert A.has_sorted_indices and A.dtype == np.dtype(dtype)
    B = pkg.host_grid_variable_matrix(shape, t, c.reshape(shape[::-1]), v.reshape(shape[::-1]), periodic=list(per), wrap=w)
    _same_matrix(B, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(4, 3, 5), (5, 3), (7,)], ids=["3d", "2d", "1d"])
def test_matrix_is_the_independent_assembly_for_every_mask(shape, dtype):
    for per in gp.masks(len(shape)):
        _check_matrix(shape, per, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_matrix_with_short_open_axes_and_at_a_tile_edge(dtype):
    for shape, per in [((1, 3, 4), (False, True, True)), ((4, 2, 3), (True, False, True)), ((2, 9), (False, True)), ((33, 5, 9), gp.ALL),
                       ((5, 17, 3), gp.Y)]:
        _check_matrix(shape, per, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_periodic_axis_gives_the_arrays_of_the_open_matrix(dtype):
    """... whatever `wrap` holds (values of axes that do not wrap are neither read nor checked), also for extents below 3."""
    for shape in ((1,), (2,), (7,), (5, 4), (2, 2, 2), (4, 1, 3), (6, 5, 4)):
        ndim = len(shape)
        t, c = gc.taps(ndim, dtype), vc.random_coeff(shape)
        bad = np.full(2 * ndim, np.nan, dtype=dtype)
        for pot in (None, gc.potential(shape, dtype)):
            want = pkg.host_grid_variable_matrix(shape, t, c, pot)
            for per, wv in ((False, None), ((False,) * ndim, None), (None, gp.wrap(ndim, dtype)), (False, bad)):
                _same_matrix(pkg.host_grid_variable_matrix(shape, t, c, pot, periodic=per, wrap=wv), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unit_coefficient_gives_the_bits_of_the_constant_coefficient_periodic_matrix(dtype):
    """0.5 w * 2 is exact."""
    for shape, per in [((7,), (True,)), ((5, 4), (True, False)), ((6, 5, 4), gp.ALL), ((1, 5, 3), (False, True, True)), ((33, 5, 9), gp.X)]:
        ndim = len(shape)
        t, v = gc.taps(ndim, dtype), gc.potential(shape, dtype)
        for wv in (None, gp.wrap(ndim, dtype)):
            for pot in (None, v):
                _same_matrix(pkg.host_grid_variable_matrix(shape, t, np.ones(gc.size(shape)), pot, periodic=per, wrap=wv),
                             pkg.host_grid_matrix(shape, t, pot, periodic=per, wrap=wv))


def test_bloch_wrap_with_a_real_coefficient_is_exactly_hermitian():
    shape, theta = (5, 4, 3), (0.7, 1.1, 1.9)
    t = gc.taps(3, np.float64, symmetric=True)
    c = vc.random_coeff(shape)
    assert np.unique(c).size == c.size
    w = extras.bloch_wrap(t, theta)
    for per in (gp.ALL, (True, False, True)):
        A = pkg.host_grid_variable_matrix(shape, t, c, gc.harmonic(shape), periodic=per, wrap=w)
        assert A.dtype == np.complex128 and np.any(A.data.imag != 0)
        assert (A - A.conj().T).nnz == 0
    # taps with t_{-a} = conj(t_{+a})
    tc = t.astype(np.complex128)
    tc[4:] += 1j * np.array([0.25, -0.5, 0.125])
    tc[:3] = np.conj(tc[4:][::-1])
    A = pkg.host_grid_variable_matrix(shape, tc, c, periodic=True, wrap=extras.bloch_wrap(tc, theta))
    assert (A - A.conj().T).nnz == 0 and np.any(A.data.imag != 0)


def _call(ndim, dims, dtype_code, taps, coeff, periodic, wrap, cap):
    L = pkg._lib.load()
    dims = np.asarray(dims, dtype=np.int64)
    n = int(np.prod(dims[:ndim]))
    flags = None if periodic is None else np.asarray(periodic, dtype=np.int32)
    rowptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int32), np.zeros(2 * max(cap, 1))
    nnz = C.c_int64(-1)
    rc = L.ks_host_grid_var_matrix_periodic(ndim, dims.ctypes.data, dtype_code, taps.ctypes.data, coeff.ctypes.data, None,
                                            None if flags is None else flags.ctypes.data, None if wrap is None else wrap.ctypes.data,
                                            rowptr.ctypes.data, col.ctypes.data, val.ctypes.data, cap, C.byref(nnz))
    return rc, nnz.value, L.ks_last_error_string().decode(), (rowptr, col, val)


def test_nnz_formula_capacity_and_null_flags():
    t = gc.taps(3, np.float64)
    for shape in ((3, 3, 3), (5, 4, 3), (7, 1, 4), (2, 6, 3)):
        c = vc.coeff(shape)
        for per in gp.masks(3):
            if any(p and m < 3 for p, m in zip(per, shape)):
                continue
            n = gc.size(shape)
            want = n * (1 + 2 * sum(per)) + 2 * sum((m - 1) * n // m for m, p in zip(shape, per) if not p)
            assert pkg.host_grid_variable_matrix(shape, t, c, periodic=per).nnz == want == gp.nnz(shape, per)
    shape = (5, 4, 3)
    c = vc.coeff(shape)
    open_ = pkg.host_grid_variable_matrix(shape, t, c)
    rc, nnz, _, (rowptr, col, val) = _call(3, shape, pkg._lib.KS_F64, t, c, None, None, open_.nnz)       # periodic == NULL: all open
    assert rc == pkg._lib.KS_OK and nnz == open_.nnz
    assert np.array_equal(rowptr, open_.indptr) and np.array_equal(col[:nnz], open_.indices) and np.array_equal(_bits(val[:nnz]), _bits(open_.data))
    need = gp.nnz(shape, (True, False, True))
    rc, nnz, msg, _ = _call(3, shape, pkg._lib.KS_F64, t, c, (1, 0, 1), None, need - 1)
    assert rc == pkg._lib.KS_ERR_ARGUMENT and nnz == need and "cap" in msg and str(need) in msg
    rc, nnz, _, _ = _call(3, shape, pkg._lib.KS_F64, t, c, (1, 0, 1), None, need)
    assert rc == pkg._lib.KS_OK and nnz == need


def test_refusals_name_their_cause():
    t3, t1 = gc.taps(3, np.float64), gc.taps(1, np.float64)
    # a periodic axis of extent < 3: the message names the axis
    for shape, per, axis in (((2, 4, 4), (True, False, False), "axis 0"), ((4, 1, 4), (True, True, True), "axis 1"), ((4, 4, 2), True, "axis 2")):
        with pytest.raises(pkg.ArgumentError, match="periodic " + axis + ".*extent"):
            pkg.host_grid_variable_matrix(shape, t3, np.ones(gc.size(shape)), periodic=per)
    with pytest.raises(pkg.ArgumentError, match="periodic axis 0"):
        pkg.host_grid_variable_matrix((2,), t1, np.ones(2), periodic=True)
    assert pkg.host_grid_variable_matrix((2, 4, 4), t3, np.ones(32), periodic=(False, True, True)).shape == (32, 32)
    # a non-finite wrap value on a periodic axis: the message names the index; on an open axis it is not read
    c27 = np.ones(27)
    for bad in (np.nan, np.inf, -np.inf):
        w = gp.wrap(3, np.float64)
        w[4] = bad                                                                                   # +y
        with pytest.raises(pkg.ArgumentError, match="wrap value 4"):
            pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, periodic=True, wrap=w)
        assert pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, periodic=(True, False, True), wrap=w).nnz == gp.nnz((3, 3, 3), (True, False, True))
    # a complex coefficient; a pinned Float64 with a complex wrap; the refusals of the open matrix stay
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, c27 + 0j, periodic=True)
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, dtype=np.float64, periodic=True, wrap=gp.wrap(3, np.complex128))
    assert pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, periodic=True, wrap=gp.wrap(3, np.complex128)).dtype == np.complex128
    bad = c27.copy()
    bad[13] = np.nan
    with pytest.raises(pkg.ArgumentError, match="coefficient entry 13 is not finite"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, bad, periodic=True)
    with pytest.raises(pkg.DimensionMismatch, match="periodic"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, periodic=(True, True))
    with pytest.raises(pkg.DimensionMismatch, match="wrap"):
        pkg.host_grid_variable_matrix((3, 3, 3), t3, c27, periodic=True, wrap=np.ones(7))


# ------------------------------------------------------------------------------------------------ extras.diffusion_terms(periodic=)
@pytest.mark.parametrize("shape", [(9,), (6, 5), (6, 5, 4)], ids=["1d", "2d", "3d"])
def test_periodic_diffusion_terms_of_a_unit_coefficient_are_the_periodic_laplacian_exactly(shape):
    ndim, n = len(shape), gc.size(shape)
    taps, diag = extras.diffusion_terms(shape, np.ones(n), periodic=True)
    lap = extras.fd_laplacian_taps(ndim, 2)
    assert taps[ndim] == 0.0 and np.array_equal(np.delete(taps, ndim), np.delete(lap, ndim))
    assert np.array_equal(_bits(diag), _bits(np.full(n, 2.0 * ndim)))
    A = pkg.host_grid_variable_matrix(shape, taps, np.ones(n), diag, periodic=True)
    _same_matrix(A, pkg.host_grid_matrix(shape, lap, periodic=True))
    assert np.all(np.diff(A.indptr) == 2 * ndim + 1) and set(A.data.tolist()) == {-1.0, 2.0 * ndim}


def _diffusion(shape, per, boundary="dirichlet", spacing=1.0):
    c = vc.coeff(shape)
    taps, diag = extras.diffusion_terms(shape, c, spacing=spacing, boundary=boundary, periodic=per)
    return taps, pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=per)


def test_periodic_diffusion_matrix_is_symmetric_also_with_a_spacing_per_axis():
    for shape, h, per in [((12, 10, 9), 1.0, True), ((12, 10, 9), (0.5, 0.75, 1.25), True), ((12, 10, 9), (0.5, 0.75, 1.25), (True, False, True)),
                          ((17, 6), (0.3, 1.0), (False, True)), ((11,), 0.1, True)]:
        _taps, A = _diffusion(shape, per, spacing=h)
        flags = (per,) * len(shape) if isinstance(per, bool) else per
        assert (A - A.T).nnz == 0 and np.all(A.diagonal() > 0) and A.nnz == gp.nnz(shape, flags)


@pytest.mark.parametrize("shape", [(9,), (6, 5), (12, 10, 9)], ids=["1d", "2d", "3d"])
def test_rows_of_the_torus_sum_to_zero_up_to_rounding(shape):
    """The bound of the Neumann test of tests/test_grid_var_cpu.py: |A 1|[r] <= 2 ndim eps sum_k |e_k|."""
    _taps, A = _diffusion(shape, True, spacing=0.7)
    off = abs(A).sum(axis=1).A1 - np.abs(A.diagonal())
    rows = np.abs(A @ np.ones(A.shape[0]))
    print("largest |A 1| / (eps sum |e_k|):", (rows / np.maximum(off, 1e-300)).max() / EPS)
    assert np.all(rows <= 2 * len(shape) * EPS * off)


def test_open_axes_of_a_mixed_grid_follow_the_boundary():
    shape, per = (6, 5, 4), (True, False, True)
    c = vc.coeff(shape)
    ones = np.ones(gc.size(shape))
    iy = (np.arange(gc.size(shape)) // shape[0]) % shape[1]
    edge = (iy == 0) | (iy == shape[1] - 1)
    _tn, N = _diffusion(shape, per, "neumann")
    off = abs(N).sum(axis=1).A1 - np.abs(N.diagonal())
    assert np.all(np.abs(N @ ones) <= 6 * EPS * off)                      # no flux through the open faces
    _td, D = _diffusion(shape, per, "dirichlet")
    rows = D @ ones
    assert np.all(np.abs(rows[~edge]) <= 6 * EPS * off[~edge])
    assert np.allclose(rows[edge], c[edge])                               # the ghost link of the open y axis: 0.5 (c + c) / h^2
    assert np.array_equal(_bits(D.diagonal()[~edge]), _bits(N.diagonal()[~edge]))


def test_diffusion_terms_periodic_refusals():
    with pytest.raises(pkg.ArgumentError, match="periodic axis 1 .y. has extent 2 .*at least 3"):
        extras.diffusion_terms((5, 2), np.ones(10), periodic=True)
    with pytest.raises(pkg.ArgumentError, match="periodic axis 0"):
        extras.diffusion_terms((1,), np.ones(1), periodic=(True,))
    assert extras.diffusion_terms((5, 2), np.ones(10), periodic=(True, False))[1].shape == (10,)
    with pytest.raises(pkg.DimensionMismatch, match="periodic"):
        extras.diffusion_terms((5, 4), np.ones(20), periodic=(True,))
    # periodic=None and no periodic axis are the open terms
    c = vc.coeff((6, 5, 4))
    for per in (False, (False, False, False)):
        for a, b in zip(extras.diffusion_terms((6, 5, 4), c, 0.7, periodic=per), extras.diffusion_terms((6, 5, 4), c, 0.7)):
            assert np.array_equal(_bits(a), _bits(b))


def test_constant_coefficient_with_bloch_phases_has_the_analytic_spectrum():
    """sum_a (c / h_a^2) (2 - 2 cos((2 pi j_a + theta_a) / m_a)), to the tolerance tests/test_grid_periodic_cpu.py uses for its cosine
    spectrum; the diagonal does not depend on theta."""
    shape, h, theta, cval = (6, 5, 4), (1.0, 1.25, 2.0), (0.7, 1.1, 1.9), 0.5      # (spectral radius below 4, as there)
    c = np.full(gc.size(shape), cval)
    taps, diag = extras.diffusion_terms(shape, c, spacing=h, periodic=True)
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True, wrap=extras.bloch_wrap(taps, theta))
    assert A.dtype == np.complex128 and (A - A.conj().T).nnz == 0
    got = np.linalg.eigvalsh(A.toarray())
    parts = [cval / (ha * ha) * (2.0 - 2.0 * np.cos((2.0 * np.pi * np.arange(m) + th) / m)) for m, ha, th in zip(shape, h, theta)]
    want = np.sort((parts[0][None, None, :] + parts[1][None, :, None] + parts[2][:, None, None]).ravel())
    assert want.max() < 4.0 and np.abs(got - want).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ the solve cases of the GPU test
def test_spectra_of_the_two_solve_cases_are_well_separated():
    """12 x 10 x 9 (n = 1080), the matrices tests/test_gpu_grid_var_periodic.py solves: the diffusion operator on the torus plus the
    harmonic potential, real and with Bloch phases; the criterion of test_diffusion_spectrum_of_the_solve_case_is_well_separated."""
    shape = vp.SOLVE_SHAPE
    c = vc.coeff(shape)
    taps, diag = extras.diffusion_terms(shape, c, potential=vp.solve_potential(), periodic=True)
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True)
    B = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True, wrap=extras.bloch_wrap(taps, vp.SOLVE_THETA))
    assert A.shape == (1080, 1080) and (A - A.T).nnz == 0 and (B - B.conj().T).nnz == 0
    for M in (A, B):
        w = np.linalg.eigvalsh(M.toarray())[:5]
        print("lowest five:", w)
        assert np.diff(w).min() > 0.03, w
