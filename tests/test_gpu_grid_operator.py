"""`-m gpu`: the matrix-free grid operator (`ks_operator_grid`, csrc/ks_grid.hpp: one kernel family, k_grid) -- mul!(y, A, x),
src/expansion.jl:121, for a constant-coefficient stencil plus a per-point diagonal with nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_matrix` returns (tests/test_grid_operator_cpu.py pins that matrix to an independent
assembly), so a plain product must carry the bits of `seq_matvec` on that matrix (tests/spmv_reference.py) and of `csr_operator`
applied to it; the Newton step is held to the bound of its operation sequence, (L + 3) eps w (x 4 in modulus for complex), never
to a measured number.  Conventions of every product test (helpers of tests/test_gpu_shifted_product.py): the destination column is
poisoned with NaN, KS_GUARD=1 puts canary zones around the basis and `guard_intact()` is asserted after every product, and x is
asserted unchanged.

Shapes (tests/grid_cases.py) are the smallest at which k_grid can go wrong: with t the tile extent along an axis (32 along x and
y, 1024 along x where ny == 1, z-ranges of at least 8 planes) every axis at 1, 2, t - 1, t, t + 1, 2 t + 1."""
import numpy as np
import pytest

import grid_cases as gc
import spmv_reference as ref
from __graft_entry__ import import_package
from test_gpu_shifted_product import PAIRS, Product, _assert_bound, _assert_plain_bits, _bits

pytestmark = pytest.mark.gpu
pkg = import_package()
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


class Checked(Product):
    """Product (column 0 = x, column 1 = the poisoned destination) that checks the guard zones and x after every product."""

    def __init__(self, op, x):
        super().__init__(op, x, ncols=1)

    def _after(self, y):
        assert self.ws.guard_intact()
        assert np.array_equal(_bits(self.ws.col(0)), _bits(self.x)), "x was written"
        return y

    def plain(self):
        return self._after(super().plain())

    def shifted(self, theta, sigma, cacheable):
        return self._after(super().shifted(theta, sigma, cacheable))


def _check_plain(shape, dtype, ctx, x=None):
    """With and without a potential: bits of seq_matvec on the host matrix, and of csr_operator of that matrix on the same x."""
    t = gc.taps(len(shape), dtype)
    x = gc.vector(shape, dtype) if x is None else x
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_matrix(shape, t, v)
        want = ref.seq_matvec(A, x)
        op = pkg.grid_operator(shape, t, v, ctx=ctx)
        what = "grid %s %s potential=%s" % (shape, np.dtype(dtype).name, v is not None)
        assert op.shape == A.shape and op.dtype == np.dtype(dtype)
        assert op.grid_info["shape"] == tuple(shape) and op.grid_info["has_potential"] == (v is not None)
        assert op.grid_info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
        y = Checked(op, x).plain()
        _assert_plain_bits(y, want, what)
        stored = Checked(pkg.csr_operator(A, ctx), x).plain()
        _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
        assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shapes", [gc.SHAPES_1D, gc.SHAPES_2D, gc.SHAPES_3D], ids=["1d", "2d", "3d"])
def test_plain_product_bit_for_bit(shapes, dtype, ctx):
    for shape in shapes:
        _check_plain(shape, dtype, ctx)


def test_size_reports_the_in_grid_taps(ctx):
    import ctypes as C

    shape = (5, 4, 3)
    op = pkg.grid_operator(shape, gc.taps(3, np.float64), ctx=ctx)
    n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
    pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
    assert (n.value, nnz.value, dt.value) == (60, pkg.host_grid_matrix(shape, gc.taps(3, np.float64)).nnz, pkg._lib.KS_F64)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_non_finite_x_reaches_exactly_the_in_grid_neighbours(shape, dtype, ctx):
    """NaN at the last point of an x-line, Inf at a corner: a kernel that wraps around the end of a line, or multiplies a tap it
    should skip, puts a non-finite value into a row that is no neighbour."""
    ext = list(shape) + [1] * (3 - len(shape))
    nx, ny, nz = ext
    x = gc.vector(shape, dtype)
    p_nan = (nx - 1) + nx * ((1 if ny > 1 else 0) + ny * (1 if nz > 1 else 0))
    p_inf = 0 if p_nan != 0 else gc.size(shape) - 1
    x[p_nan], x[p_inf] = np.nan, np.inf
    want = _check_plain(shape, dtype, ctx, x)
    hit = np.zeros(gc.size(shape), dtype=bool)
    hit[list(gc.neighbours(shape, p_nan) | gc.neighbours(shape, p_inf))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself: the host matrix has no wrap-around entries)
    if nx > 1 and p_nan + 1 < gc.size(shape) and ny > 1:
        assert np.isfinite(want[p_nan + 1])            # the first point of the next line is no neighbour


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_newton_step_within_its_forward_error_bound(shape, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both (theta,
    sigma) pairs, both stores, with and without a potential; the two stores of the fused form carry the same values."""
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t = gc.taps(len(shape), dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_matrix(shape, t, v)
        P = Checked(pkg.grid_operator(shape, t, v, ctx=ctx), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        # the plain product after shifted ones is still the plain product
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ whole solves
SOLVE_SHAPE = (12, 10, 9)
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
COUNTS = ("mvproducts", "nconverged", "converged", "nev", "restarts", "reorth", "breakdowns", "explicit_steps")


def _pair(ctx):
    v = gc.harmonic(SOLVE_SHAPE)
    A = pkg.host_grid_matrix(SOLVE_SHAPE, LAPLACE, v)
    return A, pkg.grid_operator(SOLVE_SHAPE, LAPLACE, v.reshape(SOLVE_SHAPE[::-1]), ctx=ctx), pkg.csr_operator(A, ctx)


def _solve(op, sstep):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, np.float64, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


def test_whole_solve_step_by_step_is_interchangeable_with_the_stored_matrix(ctx):
    """-Laplacian + harmonic potential on 12 x 10 x 9, :SR, nev = 4, set_sstep(0): the products are bit-identical, so eigenvalues, R
    and the History counts must be."""
    A, grid, stored = _pair(ctx)
    assert stored.format["layout"] != "stencil"     # the varying diagonal is what the stencil layout cannot hold
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, c) for c in COUNTS] == [getattr(hs, c) for c in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    import scipy.sparse.linalg as spla

    exact = np.sort(spla.eigsh(A.tocsc(), k=4, sigma=0.0, which="LM", return_eigenvectors=False))
    assert np.abs(np.sort(dg.eigenvalues.real)[:4] - exact).max() <= 1e-8


def test_whole_solve_default_block_expansion(ctx):
    """The default (s-step) expansion takes the fused Newton step of k_grid: same mvproducts and restart count as the stored
    operator, eigenvalues within 1e-10, and -- after four restart cycles driven by hand -- an Arnoldi relation at the level the
    stored operator reaches on this problem (<= 10 x its value, measured here)."""
    _A, grid, stored = _pair(ctx)
    (dg, hg, wg), (ds, hs, _) = _solve(grid, None), _solve(stored, None)
    assert (hg.mvproducts, hg.restarts, hg.nconverged) == (hs.mvproducts, hs.restarts, hs.nconverged), (hg, hs)
    assert np.abs(np.sort_complex(dg.eigenvalues) - np.sort_complex(ds.eigenvalues)).max() <= 1e-10
    assert wg.sstep_info["blocks"] > 0, wg.sstep_info      # (otherwise this test ran the step-by-step path)
    rel = []
    for op in (grid, stored):
        n = op.shape[0]
        ws = pkg.ArnoldiWorkspace(n, 20, np.float64, ctx=ctx)
        ws.reinitialize(0, pkg.matrices.start_vector(n))
        ws.iterate_arnoldi(op, 1, 10)
        k, active, trail = 10, 0, []
        for _ in range(4):
            r = ws.expand_restart(op, k, active, 4, "SR", 1e-10, 10, 20)
            k, active = r["k"], min(r["nlock"], 3)
            trail.append((k, active))
        rel.append((ws.arnoldi_relation(op, k), trail, ws.sstep_info["blocks"]))
        assert ws.guard_intact()
    (rg, og), tg, bg = rel[0]
    (rs, os_), ts, bs = rel[1]
    print("arnoldi relation: grid %.3e stored %.3e, orthogonality %.3e / %.3e, blocks %d / %d" % (rg, rs, og, os_, bg, bs))
    assert tg == ts and bg == bs and bg > 0
    assert rg <= 10 * rs and og <= 10 * os_


# ------------------------------------------------------------------------------------------------ composition and refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composes_with_device_vectors_residuals_and_products(dtype, ctx):
    shape = (33, 7, 9)
    t = gc.taps(3, dtype, symmetric=True)
    v = gc.harmonic(shape).astype(dtype)
    A = pkg.host_grid_matrix(shape, t, v)
    op = pkg.grid_operator(shape, t, v, ctx=ctx)
    # a two-factor product equals two plain products bit for bit
    x = gc.vector(shape, dtype)
    y1 = Checked(op, x).plain()
    y2 = Checked(op, y1).plain()
    prod = pkg.product_operator(op, op, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two grid operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(A, ref.seq_matvec(A, x))))
    # partialschur on the operator, then the checks against the ORIGINAL operator on the device
    dec, hist = pkg.partialschur(op, v1=gc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    AQ = Q.apply(op)
    assert np.abs(AQ.download() - A @ Q.download()).max() <= 1e-12 * abs(A).sum(axis=1).max()
    resid, qn = pkg.residuals(op, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)


def test_wrong_use_is_refused(ctx):
    t = gc.taps(3, np.float64)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_operator((4, 3, 2), t, ctx=dctx)
    # the refusals of the host function, from the operator's entry point
    with pytest.raises(pkg.ArgumentError, match="extent"):
        pkg.grid_operator((4, 0, 2), t, ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="32-bit"):
        pkg.grid_operator((2 ** 16, 2 ** 16), gc.taps(2, np.float64), ctx=ctx)
    bad = t.copy()
    bad[0] = np.inf
    with pytest.raises(pkg.ArgumentError, match="tap 0"):
        pkg.grid_operator((4, 3, 2), bad, ctx=ctx)
    v = np.zeros(24)
    v[7] = np.nan
    with pytest.raises(pkg.ArgumentError, match="potential entry 7"):
        pkg.grid_operator((4, 3, 2), t, v, ctx=ctx)
    with pytest.raises(pkg.DimensionMismatch, match="potential"):
        pkg.grid_operator((4, 3, 2), t, np.zeros(25), ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.grid_operator((4, 3, 2), gc.taps(3, np.complex128), dtype=np.float64, ctx=ctx)
    # x and y of a product must be distinct
    op = pkg.grid_operator((4, 3, 2), t, ctx=ctx)
    ws = pkg.ArnoldiWorkspace(24, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(op, 1, 1)
