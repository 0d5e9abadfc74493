"""`-m gpu`: the matrix-free variable-coefficient grid operator (`ks_operator_grid_var`, k_grid_var of csrc/ks_grid_var.hpp) --
mul!(y, A, x), src/expansion.jl:121, for A = -div(c(x) grad) + V(x) with a cell-centred coefficient and nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_variable_matrix` returns (tests/test_grid_var_cpu.py pins that matrix to an
independent assembly), so a plain product must carry the bits of `seq_matvec` on that matrix and of `csr_operator` applied to it --
a kernel that pairs the c of the wrong plane or neighbour with an x, or reads the c halo one buffer late, fails there, because the
random coefficient makes every link's entry its own; the Newton step is held to the bound of its operation sequence, (L + 3) eps w.
Conventions of tests/test_gpu_grid_star.py: NaN-poisoned destination, KS_GUARD=1 and `guard_intact()` after every product, x
unchanged.

Shapes: those of tests/grid_cases.py (every axis at the edges of the 32 x 32 / 1024 x 1 tiles and of the 8-plane z-range; (35, 34, 17)
crosses tiles in x and y and three z-ranges, (33, 5, 9) has odd nx), plus the edges of the 32 x 16 / 512 x 1 tiles ComplexF64 takes."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_var_cases as vc
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


def _check_plain(shape, dtype, ctx, x=None):
    """With and without a potential: bits of seq_matvec on the host matrix, and of csr_operator of that matrix on the same x."""
    t = gc.taps(len(shape), dtype)
    c = vc.random_coeff(shape)
    x = gc.vector(shape, dtype) if x is None else x
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_variable_matrix(shape, t, c, v)
        want = ref.seq_matvec(A, x)
        op = pkg.grid_variable_operator(shape, t, c, v, ctx=ctx)
        what = "variable grid %s %s potential=%s" % (shape, np.dtype(dtype).name, v is not None)
        assert op.shape == A.shape and op.dtype == np.dtype(dtype)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
        y = Checked(op, x).plain()
        _assert_plain_bits(y, want, what)
        stored = Checked(pkg.csr_operator(A, ctx), x).plain()
        _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
        assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shapes", [gc.SHAPES_1D, gc.SHAPES_2D, gc.SHAPES_3D, vc.SHAPES_C64_TILE], ids=["1d", "2d", "3d", "c64tile"])
def test_plain_product_bit_for_bit(shapes, dtype, ctx):
    for shape in shapes:
        _check_plain(shape, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_non_finite_x_reaches_exactly_the_in_grid_neighbours(shape, dtype, ctx):
    """NaN at the last point of an x-line, Inf at a corner: a kernel that wraps around the end of a line, or multiplies a link it
    should skip, puts a non-finite value into a row that is no neighbour."""
    nx, ny, nz = list(shape) + [1] * (3 - len(shape))
    x = gc.vector(shape, dtype)
    p_nan = (nx - 1) + nx * ((1 if ny > 1 else 0) + ny * (1 if nz > 1 else 0))
    p_inf = 0
    x[p_nan], x[p_inf] = np.nan, np.inf
    want = _check_plain(shape, dtype, ctx, x)
    hit = np.zeros(gc.size(shape), dtype=bool)
    hit[list(gc.neighbours(shape, p_nan) | gc.neighbours(shape, p_inf))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself: the host matrix has no wrap-around entries)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_newton_step_within_its_forward_error_bound(shape, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid_var) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both
    (theta, sigma) pairs, both stores, with and without a potential; the two stores of the fused form carry the same values."""
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t = gc.taps(len(shape), dtype)
    c = vc.random_coeff(shape)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_variable_matrix(shape, t, c, v)
        P = Checked(pkg.grid_variable_operator(shape, t, c, v, ctx=ctx), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.array_equal(hp[2], np.diff(A.indptr)) and hp[2].max() == 2 * len(shape) + 1   # the bound follows the row length
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "variable grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
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
    """-div(c grad) + harmonic potential on 12 x 10 x 9, Dirichlet, the smooth coefficient with a jump: (matrix, matrix-free, stored)."""
    c = vc.coeff(SOLVE_SHAPE)
    taps, diag = extras.diffusion_terms(SOLVE_SHAPE, c, potential=gc.harmonic(SOLVE_SHAPE), boundary="dirichlet")
    A = pkg.host_grid_variable_matrix(SOLVE_SHAPE, taps, c, diag)
    op = pkg.grid_variable_operator(SOLVE_SHAPE, taps, c.reshape(SOLVE_SHAPE[::-1]), potential=diag.reshape(SOLVE_SHAPE[::-1]), ctx=ctx)
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
    """The default (s-step) expansion takes the fused Newton step of k_grid_var: same mvproducts, restart count and nconverged as
    the stored operator, eigenvalues within 1e-10."""
    _A, grid, stored = pair
    (dg, hg, wg), (ds, hs, _) = _solve(grid, None), _solve(stored, None)
    assert (hg.mvproducts, hg.restarts, hg.nconverged) == (hs.mvproducts, hs.restarts, hs.nconverged), (hg, hs)
    assert np.abs(np.sort_complex(dg.eigenvalues) - np.sort_complex(ds.eigenvalues)).max() <= 1e-10
    assert wg.sstep_info["blocks"] > 0, wg.sstep_info      # (otherwise this test ran the step-by-step path)


# ------------------------------------------------------------------------------------------------ composition, size, refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composes_with_device_vectors_residuals_and_products(dtype, ctx):
    shape = (33, 7, 9)
    c = vc.coeff(shape)
    taps, diag = extras.diffusion_terms(shape, c, potential=gc.harmonic(shape))
    taps, diag = taps.astype(dtype), diag.astype(dtype)
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag)
    op = pkg.grid_variable_operator(shape, taps, c, diag, ctx=ctx)
    assert A.dtype == op.dtype == np.dtype(dtype)
    x = gc.vector(shape, dtype)
    y1 = Checked(op, x).plain()
    y2 = Checked(op, y1).plain()
    prod = pkg.product_operator(op, op, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two variable-coefficient operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(A, ref.seq_matvec(A, x))))
    dec, hist = pkg.partialschur(op, v1=gc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    AQ = Q.apply(op)
    assert np.abs(AQ.download() - A @ Q.download()).max() <= 1e-12 * abs(A).sum(axis=1).max()
    resid, qn = pkg.residuals(op, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_size_and_grid_info(dtype, ctx):
    code = pkg._lib.KS_F64 if np.dtype(dtype).kind == "f" else pkg._lib.KS_C64
    for shape in [(5, 4, 3), (9, 2, 11), (7,), (3, 12)]:
        t, c = gc.taps(len(shape), dtype), vc.coeff(shape)
        for v in (None, gc.potential(shape, dtype)):
            op = pkg.grid_variable_operator(shape, t, c, v, ctx=ctx)
            n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
            pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
            assert (n.value, nnz.value, dt.value) == (gc.size(shape), vc.nnz(shape), code)
            assert nnz.value == pkg.host_grid_variable_matrix(shape, t, c, v).nnz
            info = op.grid_info
            assert info["shape"] == tuple(shape) and info["variable"] is True and info["has_potential"] == (v is not None)
            assert np.array_equal(info["taps"], t)
            assert info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2) + 8


def test_wrong_use_is_refused(ctx):
    t, c = gc.taps(3, np.float64), np.ones(24)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_variable_operator((4, 3, 2), t, c, ctx=dctx)
    with pytest.raises(pkg.DimensionMismatch, match="coeff"):
        pkg.grid_variable_operator((4, 3, 2), t, np.ones(23), ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        pkg.grid_variable_operator((4, 3, 2), t, c + 0j, ctx=ctx)
    bad = c.copy()
    bad[13] = np.nan
    with pytest.raises(pkg.ArgumentError, match="coefficient entry 13"):
        pkg.grid_variable_operator((4, 3, 2), t, bad, ctx=ctx)
    with pytest.raises(pkg.DimensionMismatch, match="taps"):
        pkg.grid_variable_operator((4, 3), t, np.ones(12), ctx=ctx)
    op = pkg.grid_variable_operator((4, 3, 2), t, c, ctx=ctx)
    ws = pkg.ArnoldiWorkspace(24, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(op, 1, 1)                                   # x and y of a product are distinct
    for n, dt in ((25, np.float64), (24, np.complex128)):   # a workspace of another size or element type
        with pytest.raises(pkg.DimensionMismatch):
            pkg.ArnoldiWorkspace(n, 2, dt, ctx=ctx).apply(op, 0, 1)
