"""`-m gpu`: star stencils of radius 2, 3, 4 for the matrix-free grid operator (`ks_operator_grid_star`, k_grid_star of
csrc/ks_grid.hpp) -- mul!(y, A, x), src/expansion.jl:121, for central differences of order 4, 6, 8 plus a per-point diagonal with
nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_matrix(..., radius=R)` returns (tests/test_grid_star_cpu.py pins that matrix to an
independent assembly), so a plain product must carry the bits of `seq_matvec` on that matrix and of `csr_operator` applied to it;
the Newton step is held to the bound of its operation sequence, (L + 3) eps w with L the row length.  Conventions of
tests/test_gpu_grid_operator.py: NaN-poisoned destination, KS_GUARD=1 and `guard_intact()` after every product, x unchanged.

Shapes (tests/grid_star_cases.py): with t the tile extent (32; 1024 where ny == 1; 16 and 512 for the half tiles of ComplexF64 at
R >= 3) and zc = 8 R the shortest z-range, every axis in turn at 1, 2, R, R + 1, 2 R, 2 R + 1, t - 1, t, t + 1, t + R, 2 t + 1 and
z at 1, 2, R, R + 1, zc - 1, zc, zc + 1, 2 zc + 1, plus the shapes where every axis has all its taps."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_star_cases as sc
import spmv_reference as ref
from __graft_entry__ import import_package
from test_gpu_grid_operator import Checked
from test_gpu_shifted_product import PAIRS, _assert_bound, _assert_plain_bits, _bits

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
ENV = ("KS_SHIFT_FUSED", "KS_SHIFT_PLAIN", "KS_SPMV_FORMAT", "KS_SSTEP")


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _check_plain(shape, R, dtype, ctx, x=None):
    """With and without a potential: bits of seq_matvec on the host matrix, and of csr_operator of that matrix on the same x."""
    t = sc.taps(len(shape), R, dtype)
    x = sc.vector(shape, dtype) if x is None else x
    for v in (None, sc.potential(shape, dtype)):
        A = pkg.host_grid_matrix(shape, t, v, radius=R)
        want = ref.seq_matvec(A, x)
        op = pkg.grid_operator(shape, t, v, ctx=ctx, radius=R)
        what = "star %s R=%d %s potential=%s" % (shape, R, np.dtype(dtype).name, v is not None)
        assert op.shape == A.shape and op.dtype == np.dtype(dtype)
        assert op.grid_info["shape"] == tuple(shape) and op.grid_info["radius"] == R and op.grid_info["has_potential"] == (v is not None)
        assert op.grid_info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
        y = Checked(op, x).plain()
        _assert_plain_bits(y, want, what)
        stored = Checked(pkg.csr_operator(A, ctx), x).plain()
        _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
        assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shapes", [sc.shapes_1d, sc.shapes_2d, sc.shapes_3d], ids=["1d", "2d", "3d"])
@pytest.mark.parametrize("R", sc.RADII)
def test_plain_product_bit_for_bit(R, shapes, dtype, ctx):
    for shape in shapes(R):
        _check_plain(shape, R, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
@pytest.mark.parametrize("R", sc.RADII)
def test_non_finite_x_reaches_exactly_the_in_grid_neighbours(R, shape, dtype, ctx):
    """NaN at the last point of an x-line, Inf at a corner: a kernel that wraps around the end of a line, or multiplies a tap it
    should skip (outside the grid, or beyond the radius), puts a non-finite value into a row that is no neighbour."""
    ext = list(shape) + [1] * (3 - len(shape))
    nx, ny, nz = ext
    x = sc.vector(shape, dtype)
    p_nan = (nx - 1) + nx * ((1 if ny > 1 else 0) + ny * (1 if nz > 1 else 0))
    p_inf = 0
    x[p_nan], x[p_inf] = np.nan, np.inf
    want = _check_plain(shape, R, dtype, ctx, x)
    hit = np.zeros(sc.size(shape), dtype=bool)
    hit[list(sc.neighbours(shape, p_nan, R) | sc.neighbours(shape, p_inf, R))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself: the host matrix has no wrap-around entries)
    if ny > 1:
        assert np.all(np.isfinite(want[p_nan + 1 + R : p_nan + nx - R]))   # the next line: only its ends can be neighbours (of p_nan's column)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
@pytest.mark.parametrize("R", sc.RADII)
def test_newton_step_within_its_forward_error_bound(R, shape, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid_star) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both
    (theta, sigma) pairs, both stores, with and without a potential; the two stores of the fused form carry the same values."""
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t = sc.taps(len(shape), R, dtype)
    x = sc.vector(shape, dtype)
    for v in (None, sc.potential(shape, dtype)):
        A = pkg.host_grid_matrix(shape, t, v, radius=R)
        P = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, radius=R), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.array_equal(hp[2], np.diff(A.indptr)) and hp[2].max() == 2 * len(shape) * R + 1   # the bound follows the row length
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "star %s R=%d %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, R, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        # the plain product after shifted ones is still the plain product
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ whole solves
SOLVE_SHAPE = (12, 10, 9)
COUNTS = ("mvproducts", "nconverged", "converged", "nev", "restarts", "reorth", "breakdowns", "explicit_steps")


def _pair(R, ctx):
    v = gc.harmonic(SOLVE_SHAPE)
    t = extras.fd_laplacian_taps(3, 2 * R)
    A = pkg.host_grid_matrix(SOLVE_SHAPE, t, v, radius=R)
    return A, pkg.grid_operator(SOLVE_SHAPE, t, v.reshape(SOLVE_SHAPE[::-1]), ctx=ctx, radius=R), pkg.csr_operator(A, ctx)


def _solve(op, sstep):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, np.float64, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


@pytest.mark.parametrize("R", [2, 4])
def test_whole_solve_step_by_step_is_interchangeable_with_the_stored_matrix(R, ctx):
    """Central differences of order 2 R + harmonic potential on 12 x 10 x 9, :SR, nev = 4, set_sstep(0): the products are
    bit-identical, so eigenvalues, R and the History counts must be."""
    A, grid, stored = _pair(R, ctx)
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, c) for c in COUNTS] == [getattr(hs, c) for c in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    import scipy.sparse.linalg as spla

    exact = np.sort(spla.eigsh(A.tocsc(), k=4, sigma=0.0, which="LM", return_eigenvectors=False))
    assert np.abs(np.sort(dg.eigenvalues.real)[:4] - exact).max() <= 1e-8


@pytest.mark.parametrize("R", [2, 4])
def test_whole_solve_default_block_expansion(R, ctx):
    """The default (s-step) expansion takes the fused Newton step of k_grid_star: same mvproducts, restart count and nconverged as
    the stored operator, eigenvalues within 1e-10."""
    _A, grid, stored = _pair(R, ctx)
    (dg, hg, wg), (ds, hs, _) = _solve(grid, None), _solve(stored, None)
    assert (hg.mvproducts, hg.restarts, hg.nconverged) == (hs.mvproducts, hs.restarts, hs.nconverged), (hg, hs)
    assert np.abs(np.sort_complex(dg.eigenvalues) - np.sort_complex(ds.eigenvalues)).max() <= 1e-10
    assert wg.sstep_info["blocks"] > 0, wg.sstep_info      # (otherwise this test ran the step-by-step path)


# ------------------------------------------------------------------------------------------------ composition, size, radius 1
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composes_with_device_vectors_residuals_and_products(dtype, ctx):
    shape, R = (33, 7, 9), 3
    t = sc.taps(3, R, dtype, symmetric=True)
    v = gc.harmonic(shape).astype(dtype)
    A = pkg.host_grid_matrix(shape, t, v, radius=R)
    op = pkg.grid_operator(shape, t, v, ctx=ctx, radius=R)
    x = sc.vector(shape, dtype)
    y1 = Checked(op, x).plain()
    y2 = Checked(op, y1).plain()
    prod = pkg.product_operator(op, op, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two star operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(A, ref.seq_matvec(A, x))))
    dec, hist = pkg.partialschur(op, v1=sc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    AQ = Q.apply(op)
    assert np.abs(AQ.download() - A @ Q.download()).max() <= 1e-12 * abs(A).sum(axis=1).max()
    resid, qn = pkg.residuals(op, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)


@pytest.mark.parametrize("R", sc.RADII)
def test_size_reports_the_formula(R, ctx):
    for shape in [(5, 4, 3), (9, 2, 11), (7,), (3, 12)]:
        op = pkg.grid_operator(shape, sc.taps(len(shape), R, np.float64), ctx=ctx, radius=R)
        n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
        pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
        assert (n.value, nnz.value, dt.value) == (sc.size(shape), sc.nnz(shape, R), pkg._lib.KS_F64)
        assert nnz.value == pkg.host_grid_matrix(shape, sc.taps(len(shape), R, np.float64), radius=R).nnz


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radius_one_through_the_new_entry_point_is_the_existing_operator(dtype, ctx):
    """ks_operator_grid_star with radius 1 (called directly: the Python layer takes today's path for radius=1) gives the bits of
    ks_operator_grid, plain and shifted; so does grid_operator(..., radius=1)."""
    L = pkg._lib.load()
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    for shape in [(33, 34, 9), (1025, 1, 9), (65, 33), (2049,)]:
        t, v, x = gc.taps(len(shape), dtype), gc.potential(shape, dtype), gc.vector(shape, dtype)
        dims = np.asarray(shape, dtype=np.int64)
        h = C.c_void_p()
        pkg._lib.check(L.ks_operator_grid_star(ctx._h, len(shape), dims.ctypes.data, 1, pkg._lib.KS_F64 if kind == "f" else pkg._lib.KS_C64,
                                               t.ctypes.data, v.ctypes.data, C.byref(h)))
        n = sc.size(shape)
        star = pkg.api.Operator(ctx, h, (n, n), np.dtype(dtype))
        old = Checked(pkg.grid_operator(shape, t, v, ctx=ctx), x)
        kw = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, radius=1), x)
        new = Checked(star, x)
        want = old.plain()
        assert np.array_equal(_bits(new.plain()), _bits(want)) and np.array_equal(_bits(kw.plain()), _bits(want))
        assert np.array_equal(_bits(want), _bits(ref.seq_matvec(pkg.host_grid_matrix(shape, t, v), x)))
        th, sg = PAIRS[kind][0]
        assert np.array_equal(_bits(new.shifted(th, sg, False)), _bits(old.shifted(th, sg, False)))
        nn, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
        pkg._lib.check(L.ks_operator_size(h, C.byref(nn), C.byref(nnz), C.byref(dt)))
        assert (nn.value, nnz.value) == (n, pkg.host_grid_matrix(shape, t, v).nnz)


def test_wrong_use_is_refused(ctx):
    t = sc.taps(3, 2, np.float64)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_operator((4, 3, 2), t, ctx=dctx, radius=2)
    for radius in (0, 5):
        with pytest.raises(pkg.ArgumentError, match="radius"):
            pkg.grid_operator((4, 3, 2), t, ctx=ctx, radius=radius)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.grid_operator((4, 3, 2), t, ctx=ctx)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.grid_operator((4, 3, 2), t, ctx=ctx, radius=3)
    bad = t.copy()
    bad[12] = np.inf
    with pytest.raises(pkg.ArgumentError, match="tap 12"):
        pkg.grid_operator((4, 3, 2), bad, ctx=ctx, radius=2)
    for kw in (dict(periodic=True), dict(wrap=np.ones(6))):
        with pytest.raises(pkg.ArgumentError, match="(?s)(periodic.*radius)|(radius.*periodic)"):
            pkg.grid_operator((4, 4, 4), t, ctx=ctx, radius=2, **kw)
    op = pkg.grid_operator((4, 3, 2), t, ctx=ctx, radius=2)
    ws = pkg.ArnoldiWorkspace(24, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(op, 1, 1)
