"""No GPU: the matrix that DEFINES the box-stencil grid operator with periodic axes (`ks_host_grid_box_matrix_periodic`,
include/kschur.h (xii-b)) against an assembly that shares no code with the library (tests/grid_box_periodic_cases.py), its row order
against the nested-offset definition, its reductions (no periodic axis: `host_grid_box_matrix`; 1-D: `host_grid_matrix` with wrap
values; star taps: `host_grid_matrix(periodic=True)`), `extras.box_bloch_links`, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import grid_box_cases as bc
import grid_box_periodic_cases as pc
import grid_cases as gc
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
TENSOR = np.array([[1.0, 0.3, 0.2], [0.3, 1.5, 0.25], [0.2, 0.25, 2.0]])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(A, B):
    A.sort_indices(), B.sort_indices()
    assert A.shape == B.shape and A.dtype == B.dtype
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    assert np.array_equal(_bits(A.data), _bits(B.data))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_host_matrix_is_the_independent_assembly(case, dtype):
    shape, flags = case
    t, w = pc.taps(len(shape), dtype), pc.links(len(shape), dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_box_matrix(shape, t, v, periodic=flags, links=w)
        assert A.has_sorted_indices and A.nnz == pc.nnz(shape, flags) and A.dtype == np.dtype(dtype)
        B = A.copy()
        B.has_sorted_indices = False
        B.sort_indices()
        assert np.array_equal(A.indices, B.indices)   # the columns as the library wrote them ascend
        _same(A, pc.assemble(shape, flags, t, w, v))
    # links=None: every crossing link carries the tap of its slot
    _same(pkg.host_grid_box_matrix(shape, t, periodic=flags), pc.assemble(shape, flags, t))


@pytest.mark.parametrize("case", [((3, 3, 3), pc.ALL3), ((4, 3, 5), (True, False, True)), ((5, 4, 3), (False, True, False)), ((4, 3), pc.ALL2),
                                  ((5,), (True,))], ids=pc.case_id)
def test_row_order_is_the_nested_offset_definition(case):
    shape, flags = case
    ndim = len(shape)
    t, w = pc.taps(ndim, np.float64), pc.links(ndim, np.float64)
    A = pkg.host_grid_box_matrix(shape, t, periodic=flags, links=w)
    flat = {e: k for k, e in enumerate(pc.classes(ndim))}
    for r in range(A.shape[0]):
        want = pc.row_by_definition(shape, flags, r)
        cols = [c for c, _ in want]
        vals = [w[flat[e]] if any(c in (0, 4) for c in e) else t[pc.slot_of(e, ndim)] for _, e in want]
        assert cols == sorted(cols) and len(set(cols)) == len(cols)
        assert list(A.indices[A.indptr[r]:A.indptr[r + 1]]) == cols
        assert np.array_equal(A.data[A.indptr[r]:A.indptr[r + 1]], np.array(vals))


def test_nnz_formula_and_cap_too_small_still_reports_nnz():
    lib = pkg._lib.load()
    for shape, flags in [((3, 3, 3), pc.ALL3), ((7, 1, 4), (True, False, True)), ((5, 4), (False, True)), ((9,), (True,)), ((6, 5, 4), (False, False, False))]:
        ndim = len(shape)
        t = pc.taps(ndim, np.float64)
        want = int(np.prod([3 * m if f else 3 * m - 2 for m, f in zip(shape, flags)]))
        assert pkg.host_grid_box_matrix(shape, t, periodic=flags).nnz == want
        dims, fl, got = np.array(shape, dtype=np.int64), np.array(flags, dtype=np.int32), C.c_int64(-1)
        rowptr = np.zeros(gc.size(shape) + 1, dtype=np.int64)
        rc = lib.ks_host_grid_box_matrix_periodic(ndim, dims.ctypes.data, pkg._lib.KS_F64, t.ctypes.data, None, fl.ctypes.data, None,
                                                  rowptr.ctypes.data, None, None, 0, C.byref(got))
        assert rc != 0 and got.value == want
        assert "too small" in lib.ks_last_error_string().decode()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_periodic_axis_is_the_open_matrix(dtype):
    for shape in [(5, 4, 3), (33, 2), (7,), (2, 1, 2)]:
        ndim = len(shape)
        t, w, v = pc.taps(ndim, dtype), pc.links(ndim, dtype), gc.potential(shape, dtype)
        for flags in (False, (False,) * ndim, None):
            _same(pkg.host_grid_box_matrix(shape, t, v, periodic=flags, links=w), pkg.host_grid_box_matrix(shape, t, v))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_dimension_is_the_periodic_three_point_matrix(dtype):
    for m in (3, 4, 65):
        t, w, v = pc.taps(1, dtype), pc.links(1, dtype), gc.potential((m,), dtype)
        _same(pkg.host_grid_box_matrix((m,), t, v, periodic=True, links=w),
              pkg.host_grid_matrix((m,), t, v, periodic=True, wrap=np.array([w[0], w[4]])))


@pytest.mark.parametrize("shape", [(5,), (4, 3), (3, 4, 5)], ids=["1d", "2d", "3d"])
def test_star_taps_without_links_are_the_periodic_star_matrix(shape):
    ndim = len(shape)
    t7 = gc.taps(ndim, np.float64)
    A = pkg.host_grid_box_matrix(shape, bc.embed_star(t7, ndim), periodic=True)
    A.eliminate_zeros()
    _same(A, pkg.host_grid_matrix(shape, t7, periodic=True))


def test_bloch_links_are_exactly_hermitian_and_match_bloch_wrap():
    for ndim, shape, theta in ((3, (5, 4, 3), (0.7, 1.1, 1.9)), (2, (4, 3), (0.3, -2.2)), (1, (6,), (1.3,))):
        t = extras.tensor_laplacian_taps(TENSOR[:ndim, :ndim])
        w = extras.box_bloch_links(t, theta)
        assert w.shape == (5 ** ndim,) and w.dtype == np.complex128
        assert np.array_equal(w.reshape((5,) * ndim)[(slice(None, None, -1),) * ndim].ravel(), np.conj(w))   # mirror: e_a -> 4 - e_a
        A = pkg.host_grid_box_matrix(shape, t, gc.harmonic(shape), periodic=True, links=w)
        assert A.dtype == np.complex128 and (A - A.conj().T).nnz == 0
        inner = w.reshape((5,) * ndim)[(slice(1, 4),) * ndim].ravel()
        assert np.array_equal(inner, t.astype(np.complex128))
    # complex taps with taps[-k] = conj(taps[k])
    rng = np.random.default_rng(3)
    h = rng.random(27) - 0.5 + 1j * (rng.random(27) - 0.5)
    t = h + np.conj(h[::-1])
    w = extras.box_bloch_links(t, (0.7, 1.1, 1.9))
    assert np.array_equal(w.reshape(5, 5, 5)[::-1, ::-1, ::-1].ravel(), np.conj(w))
    assert (lambda A: (A - A.conj().T).nnz)(pkg.host_grid_box_matrix((3, 4, 5), t, periodic=True, links=w)) == 0
    # 1-D: bloch_wrap bit for bit
    t3 = np.array([-1.25, 2.5, -0.75])
    w = extras.box_bloch_links(t3, 1.3)
    assert np.array_equal(_bits(np.array([w[0], w[4]])), _bits(extras.bloch_wrap(t3, 1.3)))
    # antiperiodic
    anti = -extras.box_bloch_links(t3, np.zeros(1)).real
    assert np.array_equal(anti, [1.25, 1.25, -2.5, 0.75, 0.75])
    with pytest.raises(pkg.DimensionMismatch, match="theta"):
        extras.box_bloch_links(t3, (1.0, 2.0))
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        extras.box_bloch_links(np.ones(7), (1.0, 2.0, 3.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ignored_link_entries_may_be_nan(dtype):
    for shape, flags in [((4, 3, 5), (True, False, True)), ((4, 3), (False, True)), ((5, 4, 3), pc.ALL3)]:
        ndim = len(shape)
        t, w = pc.taps(ndim, dtype), pc.links(ndim, dtype)
        bad = w.copy()
        bad[~pc.read_mask(ndim, flags)] = np.nan
        _same(pkg.host_grid_box_matrix(shape, t, periodic=flags, links=bad), pkg.host_grid_box_matrix(shape, t, periodic=flags, links=w))
        # every read entry is checked
        for k in np.flatnonzero(pc.read_mask(ndim, flags))[:: 7]:
            bad = w.copy()
            bad[k] = np.inf
            with pytest.raises(pkg.ArgumentError, match=f"link value {k} is not finite"):
                pkg.host_grid_box_matrix(shape, t, periodic=flags, links=bad)


def test_every_refusal_names_its_cause():
    t, w = pc.taps(3, np.float64), pc.links(3, np.float64)
    with pytest.raises(pkg.ArgumentError, match=r"periodic axis 1 \(y\) has extent 2"):
        pkg.host_grid_box_matrix((4, 2, 3), t, periodic=True)
    with pytest.raises(pkg.ArgumentError, match=r"periodic axis 2 \(z\) has extent 1"):
        pkg.host_grid_box_matrix((4, 3, 1), t, periodic=(False, False, True))
    with pytest.raises(pkg.DimensionMismatch, match="125 link values"):
        pkg.host_grid_box_matrix((4, 3, 3), t, periodic=True, links=w[:25])
    with pytest.raises(pkg.DimensionMismatch, match="link values"):
        pkg.host_grid_box_matrix((4, 3, 3), t, periodic=True, links=w.reshape(25, 5))
    with pytest.raises(pkg.DimensionMismatch, match="one bool per axis"):
        pkg.host_grid_box_matrix((4, 3, 3), t, periodic=(True, True))
    with pytest.raises(pkg.ArgumentError, match="imaginary part"):
        pkg.host_grid_box_matrix((4, 3, 3), t, dtype=np.float64, periodic=True, links=w + 1j)
    with pytest.raises(pkg.ArgumentError, match="tap 20 is not finite"):
        bad = t.copy()
        bad[20] = np.nan
        pkg.host_grid_box_matrix((4, 3, 3), bad, periodic=True, links=w)
    with pytest.raises(pkg.ArgumentError, match="potential entry 5 is not finite"):
        v = np.zeros(36)
        v[5] = np.inf
        pkg.host_grid_box_matrix((4, 3, 3), t, v, periodic=True, links=w)
    # a complex table promotes; a pinned Float64 takes one whose read entries are real; the (5,) * ndim shape is [e_z, e_y, e_x]
    assert pkg.host_grid_box_matrix((4, 3, 3), t, periodic=True, links=w + 1j).dtype == np.complex128
    A = pkg.host_grid_box_matrix((4, 3, 3), t, dtype=np.float64, periodic=True, links=(w + 0j).reshape(5, 5, 5))
    _same(A, pkg.host_grid_box_matrix((4, 3, 3), t, periodic=True, links=w))


def test_the_solve_cases_have_separated_lowest_eigenvalues():
    """What tests/test_gpu_grid_box_periodic.py solves for (nev = 4, :SR): the five lowest eigenvalues of the real torus and of the
    Bloch operator are at least 0.1 apart, so the solves converge to single eigenvalues and their counts are reproducible."""
    t, V = extras.tensor_laplacian_taps(pc.SOLVE_TENSOR), pc.solve_potential()
    for w in (None, extras.box_bloch_links(t, pc.SOLVE_THETA)):
        A = pkg.host_grid_box_matrix(pc.SOLVE_SHAPE, t, V, periodic=True, links=w)
        assert (A - A.conj().T).nnz == 0
        lam = np.linalg.eigvalsh(A.toarray())[:5]
        assert np.diff(lam).min() >= 0.1, lam
