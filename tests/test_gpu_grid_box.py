"""`-m gpu`: the matrix-free box-stencil grid operator (`ks_operator_grid_box`, k_grid_box of csrc/ks_grid_box.hpp) -- mul!(y, A, x),
src/expansion.jl:121, for the 3-, 9- or 27-point stencil with the diagonal neighbours and nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_box_matrix` returns (tests/test_grid_box_cpu.py pins that matrix to an independent
assembly), so a plain product must carry the bits of `seq_matvec` on that matrix and of `csr_operator` applied to it -- a kernel
that feeds a term to the accumulator of the wrong plane, adds the terms of a row out of slot order, reads a corner halo cell one
buffer late or exchanges two taps fails there, because all 27 taps are distinct with full mantissas; the Newton step is held to the
bound of its operation sequence, (L + 3) eps w.  Conventions of tests/test_gpu_grid_var.py: NaN-poisoned destination, KS_GUARD=1
and `guard_intact()` after every product, x unchanged.

Shapes: those of tests/grid_cases.py (every axis at the edges of the 32 x 32 / 1024 x 1 tiles, which both element types take, and
of the 8-plane z-range; (35, 34, 17) crosses tiles in x and y -- the corner halo cell at a tile junction -- and three z-ranges)."""
import ctypes as C

import numpy as np
import pytest

import grid_box_cases as bc
import grid_cases as gc
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
TENSOR = np.array([[1.0, 0.3, 0.2], [0.3, 1.5, 0.25], [0.2, 0.25, 2.0]])


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _check_plain(shape, dtype, ctx, x=None):
    """With and without a potential: bits of seq_matvec on the host matrix, and of csr_operator of that matrix on the same x."""
    t = bc.taps(len(shape), dtype)
    x = gc.vector(shape, dtype) if x is None else x
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_box_matrix(shape, t, v)
        want = ref.seq_matvec(A, x)
        op = pkg.grid_box_operator(shape, t, v, ctx=ctx)
        what = "box grid %s %s potential=%s" % (shape, np.dtype(dtype).name, v is not None)
        assert op.shape == A.shape and op.dtype == np.dtype(dtype)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
        y = Checked(op, x).plain()
        _assert_plain_bits(y, want, what)
        stored = Checked(pkg.csr_operator(A, ctx), x).plain()
        _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
        assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shapes", [bc.SHAPES_1D, bc.SHAPES_2D, bc.SHAPES_3D], ids=["1d", "2d", "3d"])
def test_plain_product_bit_for_bit(shapes, dtype, ctx):
    for shape in shapes:
        _check_plain(shape, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", bc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_non_finite_x_reaches_exactly_the_in_grid_neighbours(shape, dtype, ctx):
    """NaN at the last point of an x-line, Inf at corner 0: a kernel that wraps around the end of a line, or multiplies a slot it
    should skip (a corner beyond an edge of the grid), puts a non-finite value into a row that is no neighbour."""
    nx, ny, nz = list(shape) + [1] * (3 - len(shape))
    x = gc.vector(shape, dtype)
    p_nan = (nx - 1) + nx * ((1 if ny > 1 else 0) + ny * (1 if nz > 1 else 0))
    p_inf = 0
    x[p_nan], x[p_inf] = np.nan, np.inf
    want = _check_plain(shape, dtype, ctx, x)
    hit = np.zeros(gc.size(shape), dtype=bool)
    hit[list(bc.neighbours(shape, p_nan) | bc.neighbours(shape, p_inf))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself: the host matrix has no wrap-around entries)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", bc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_newton_step_within_its_forward_error_bound(shape, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid_box) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both
    (theta, sigma) pairs, both stores, with and without a potential; the two stores of the fused form carry the same values."""
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t = bc.taps(len(shape), dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_box_matrix(shape, t, v)
        P = Checked(pkg.grid_box_operator(shape, t, v, ctx=ctx), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.array_equal(hp[2], np.diff(A.indptr)) and hp[2].max() == 3 ** len(shape)   # the bound follows the row length
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "box grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        # the plain product after shifted ones is still the plain product
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ whole solves
SOLVE_SHAPE = (12, 10, 9)
COUNTS = ("mvproducts", "nconverged", "converged", "nev", "restarts", "reorth", "breakdowns", "explicit_steps")


@pytest.fixture(scope="module")
def pair(ctx):
    """-div(D grad) + harmonic potential on 12 x 10 x 9 with a full tensor D: (matrix, matrix-free, stored)."""
    taps = extras.tensor_laplacian_taps(TENSOR)
    V = gc.harmonic(SOLVE_SHAPE)
    A = pkg.host_grid_box_matrix(SOLVE_SHAPE, taps, V)
    op = pkg.grid_box_operator(SOLVE_SHAPE, taps.reshape(3, 3, 3), potential=V.reshape(SOLVE_SHAPE[::-1]), ctx=ctx)
    return A, op, pkg.csr_operator(A, ctx)


def _solve(op, sstep):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, np.float64, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


def test_whole_solve_step_by_step_is_interchangeable_with_the_stored_matrix(pair):
    """:SR, nev = 4, set_sstep(0): the products are bit-identical, so eigenvalues, R and the History counts must be."""
    A, grid, stored = pair
    assert (A - A.T).nnz == 0
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, c) for c in COUNTS] == [getattr(hs, c) for c in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    import scipy.sparse.linalg as spla

    exact = np.sort(spla.eigsh(A.tocsc(), k=4, sigma=0.0, which="LM", return_eigenvectors=False))
    assert np.abs(np.sort(dg.eigenvalues.real)[:4] - exact).max() <= 1e-8


def test_whole_solve_default_block_expansion(pair):
    """The default (s-step) expansion takes the fused Newton step of k_grid_box: same mvproducts, restart count and nconverged as
    the stored operator, eigenvalues within 1e-10."""
    _A, grid, stored = pair
    (dg, hg, wg), (ds, hs, _) = _solve(grid, None), _solve(stored, None)
    assert (hg.mvproducts, hg.restarts, hg.nconverged) == (hs.mvproducts, hs.restarts, hs.nconverged), (hg, hs)
    assert np.abs(np.sort_complex(dg.eigenvalues) - np.sort_complex(ds.eigenvalues)).max() <= 1e-10
    assert wg.sstep_info["blocks"] > 0, wg.sstep_info      # (otherwise this test ran the step-by-step path)


# ------------------------------------------------------------------------------------------------ composition, size, refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composes_with_device_vectors_residuals_and_products(dtype, ctx):
    """The Q1 stiffness matrix (plus a harmonic term that separates its lowest eigenvalues) as A, the Q1 mass matrix as B."""
    shape = (33, 7, 9)
    kt, mt = extras.q1_fem_taps(3)
    kt, mt, V = kt.astype(dtype), mt.astype(dtype), gc.harmonic(shape).astype(dtype)
    K, M = pkg.host_grid_box_matrix(shape, kt, V), pkg.host_grid_box_matrix(shape, mt)
    opK, opM = pkg.grid_box_operator(shape, kt, V, ctx=ctx), pkg.grid_box_operator(shape, mt, ctx=ctx)
    assert K.dtype == opK.dtype == opM.dtype == np.dtype(dtype)
    x = gc.vector(shape, dtype)
    y1 = Checked(opK, x).plain()
    y2 = Checked(opK, y1).plain()
    prod = pkg.product_operator(opK, opK, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two box operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(K, ref.seq_matvec(K, x))))
    dec, hist = pkg.partialschur(opK, v1=gc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    KQ = Q.apply(opK)
    Qh = Q.download()
    assert np.abs(KQ.download() - K @ Qh).max() <= 1e-12 * abs(K).sum(axis=1).max()
    resid, qn = pkg.residuals(opK, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)
    # ||K x - lambda M x|| against the two ORIGINAL operators, and the same quantity from the two host matrices and the downloaded X
    lam = np.asarray(dec.eigenvalues)[: Qh.shape[1]]
    lam = lam.astype(dtype) if np.dtype(dtype).kind == "c" else np.ascontiguousarray(lam.real)
    resid, bn = pkg.residuals(opK, Q, lam, opM)
    MQ = M @ Qh
    want = np.linalg.norm(K @ Qh - MQ * lam[None, :], axis=0)
    tol = 1e-12 * (abs(K).sum(axis=1).max() + np.abs(lam).max() * abs(M).sum(axis=1).max())
    print("generalized residuals on the device:", resid, "on the host:", want, "tolerance", tol)
    assert np.abs(resid - want).max() <= tol and np.abs(bn - np.linalg.norm(MQ, axis=0)).max() <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_size_and_grid_info(dtype, ctx):
    code = pkg._lib.KS_F64 if np.dtype(dtype).kind == "f" else pkg._lib.KS_C64
    for shape in [(5, 4, 3), (9, 2, 11), (7,), (3, 12)]:
        t = bc.taps(len(shape), dtype)
        for v in (None, gc.potential(shape, dtype)):
            op = pkg.grid_box_operator(shape, t.reshape((3,) * len(shape)), v, ctx=ctx)
            n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
            pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
            assert (n.value, nnz.value, dt.value) == (gc.size(shape), bc.nnz(shape), code)
            assert nnz.value == pkg.host_grid_box_matrix(shape, t, v).nnz
            assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
            info = op.grid_info
            assert info["shape"] == tuple(shape) and info["box"] is True and info["has_potential"] == (v is not None)
            assert info["taps"].shape == (3 ** len(shape),) and np.array_equal(info["taps"], t)
            assert info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2)


def test_wrong_use_is_refused(ctx):
    t = bc.taps(3, np.float64)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_box_operator((4, 3, 2), t, ctx=dctx)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.grid_box_operator((4, 3, 2), gc.taps(3, np.float64), ctx=ctx)     # a star stencil's seven
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.grid_box_operator((4, 3), t, ctx=ctx)
    bad = t.copy()
    bad[20] = np.inf
    with pytest.raises(pkg.ArgumentError, match="tap 20 is not finite"):
        pkg.grid_box_operator((4, 3, 2), bad, ctx=ctx)
    op = pkg.grid_box_operator((4, 3, 2), t, ctx=ctx)
    ws = pkg.ArnoldiWorkspace(24, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(op, 1, 1)                                   # x and y of a product are distinct
    for n, dt in ((25, np.float64), (24, np.complex128)):   # a workspace of another size or element type
        with pytest.raises(pkg.DimensionMismatch):
            pkg.ArnoldiWorkspace(n, 2, dt, ctx=ctx).apply(op, 0, 1)
