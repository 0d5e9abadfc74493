"""`-m gpu`: the device layouts of a stored matrix (mul!(y, A, x), src/expansion.jl:121) -- CSR row blocks
(skewed rows, rows longer than a block, 64-bit offsets), sliced ELLPACK (padding, sigma-window sorting), the
delta-value-indexed kernel's rows-per-thread variants -- against scipy and against each other BIT for bit
(every layout rounds each product on its own and adds in CSR order).  All through the C ABI."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import layout_cases as lc
from __graft_entry__ import import_package
from layout_cases import rnd
from oracle import arnoldi as oa
from oracle.matrices import laplace3d

pytestmark = pytest.mark.gpu
pkg = import_package()
DTYPES = [np.float64, np.complex128]


def _apply(A, x, dtype, ctx=None):
    op = pkg.csr_operator(A, ctx)
    ws = pkg.ArnoldiWorkspace(A.shape[0], 2, dtype, ctx=op.ctx)
    ws.set_col(0, x)
    ws.apply(op, 0, 1)
    return ws.col(1), op.format, op


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ptr64", ["0", "1"])
def test_csr_row_blocks_long_rows_and_64bit_offsets(dtype, ptr64, monkeypatch):
    """k_spmv_csr on a skewed matrix: blocks closed by the non-zero budget, rows with more entries than a block holds
    (all-threads path), empty rows -- vs scipy to 1e-13 relative; the int64-offset instantiation (what a matrix with
    nnz >= 2^31 gets, forced by KS_SPMV_PTR64=1) must be BIT-identical to the int32 one; and the same matrix handed
    over as CSC / Int64 / 1-based (Julia's SparseMatrixCSC) builds the same operator."""
    A, x = lc.skewed_case(dtype)
    n = A.shape[0]
    monkeypatch.setenv("KS_SPMV_PTR64", ptr64)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    y, fmt, op = _apply(A, x, dtype)
    assert fmt["layout"] == "csr"
    ref = A @ x
    scale = np.abs(A) @ np.abs(x)
    assert np.all(np.abs(y - ref) <= 1e-13 * (scale + 1e-300))
    assert np.all(y[10:30] == 0)
    monkeypatch.setenv("KS_SPMV_PTR64", "0")
    y0, _, _ = _apply(A, x, dtype, op.ctx)
    assert np.array_equal(y0, y)
    Ac = A.tocsc()
    L = pkg._lib.load()
    h = C.c_void_p()
    ptr, idx, val = (Ac.indptr.astype(np.int64) + 1), (Ac.indices.astype(np.int64) + 1), np.ascontiguousarray(Ac.data)
    pkg._lib.check(L.ks_operator_csr(op.ctx._h, n, n, Ac.nnz, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, pkg._lib.KS_CSC, 1,
                                     pkg._lib.KS_I64, pkg._lib.KS_C64 if np.dtype(dtype).kind == "c" else pkg._lib.KS_F64, C.byref(h)))
    opj = pkg.Operator(op.ctx, h, (n, n), dtype)
    ws = pkg.ArnoldiWorkspace(n, 2, dtype, ctx=op.ctx)
    ws.set_col(0, x)
    ws.apply(opj, 0, 1)
    assert np.array_equal(ws.col(1), y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sliced_ellpack_is_bit_identical_and_chosen_for_uniform_rows(dtype, monkeypatch):
    """A 7-point stencil with VARIABLE coefficients (no dictionary layout applies) is stored as sliced ELLPACK by
    default; y must equal the CSR-block kernel's bit for bit.  Forced on a ragged matrix (heavy padding, empty rows,
    Inf in x next to padding) with and without sigma-window sorting it must still agree; a value-indexed SELL too."""
    A, x, R, xr = lc.varcoef_and_ragged(dtype)
    y, fmt, op = _apply(A, x, dtype)
    assert fmt["layout"] == "sell" and fmt["ndict"] == 0 and fmt["bytes_per_nnz"] < 1.15 * (4 + np.dtype(dtype).itemsize)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    y_csr, f_csr, _ = _apply(A, x, dtype, op.ctx)
    assert f_csr["layout"] == "csr" and np.array_equal(y.view(np.uint64), y_csr.view(np.uint64))
    np.testing.assert_allclose(y, A @ x, rtol=1e-13, atol=1e-13)
    # ragged: rows of 0..40 entries, a few distinct values; Inf in xr (a padding entry must never be multiplied)
    ref, _, op2 = _apply(R, xr, dtype)
    assert _["layout"] == "csr"
    for fmt_name, sigma in (("sell", "1"), ("sell", "256"), ("sellvi", "1"), ("sellvi", "640")):
        monkeypatch.setenv("KS_SPMV_FORMAT", fmt_name)
        monkeypatch.setenv("KS_SELL_SIGMA", sigma)
        got, f, _o = _apply(R, xr, dtype, op2.ctx)
        assert f["layout"] == ("sell-vi" if fmt_name == "sellvi" else "sell"), f
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (fmt_name, sigma)
    monkeypatch.setenv("KS_SPMV_PTR64", "1")
    got, f, _o = _apply(R, xr, dtype, op2.ctx)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("rpt", ["1", "2", "4"])
@pytest.mark.parametrize("shape", [(37, 41, 43), (5, 3, 2), (300, 7, 1)])
def test_dvi_rows_per_thread_variants_bit_identical(rpt, shape, monkeypatch):
    """k_spmv_dvi with 1 / 2 / 4 rows per thread (LDS-staged codes) vs the CSR blocks and sliced ELLPACK: bit-identical
    y, including grids whose row count is not a multiple of the tile and tiles with ragged rows (stencil boundaries)."""
    A = laplace3d(*shape)
    n = A.shape[0]
    x = oa.uniform_hash(9, np.arange(n)) - 0.5
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    y0, f0, op0 = _apply(A, x, np.float64)
    assert f0["bytes_per_nnz"] == 12.0
    monkeypatch.setenv("KS_SPMV_FORMAT", "dvi")
    monkeypatch.setenv("KS_DVI_RPT", rpt)
    y1, f1, _ = _apply(A, x, np.float64, op0.ctx)
    assert f1["layout"] == "csr-dvi" and f1["bytes_per_nnz"] == 1.0
    assert np.array_equal(y1, y0)
    monkeypatch.setenv("KS_SPMV_FORMAT", "sellvi")
    y2, f2, _ = _apply(A, x, np.float64, op0.ctx)
    assert f2["layout"] == "sell-vi" and np.array_equal(y2, y0)
    monkeypatch.setenv("KS_SPMV_FORMAT", "stencil")
    y3, f3, _ = _apply(A, x, np.float64, op0.ctx)
    assert f3["layout"] == "stencil" and f3["ndict"] <= 7 and np.array_equal(y3, y0)
    np.testing.assert_allclose(y0, A @ x, rtol=0, atol=1e-14 * 12)


def test_solver_end_to_end_on_each_layout(monkeypatch):
    """The layout must not change what the solver does: same mat-vec count and Ritz values on every layout."""
    A = laplace3d(14, 15, 16)
    n = A.shape[0]
    v1 = oa.uniform_hash(oa.DEFAULT_SEED, np.arange(n))
    out = {}
    for f in ("stencil", "dvi", "vi", "csr", "sell", "sellvi"):
        monkeypatch.setenv("KS_SPMV_FORMAT", f)
        dec, hist = pkg.partialschur(A, v1=v1, nev=5, which="SR", tol=1e-10, maxdim=25)
        out[f] = (hist.mvproducts, np.sort(dec.eigenvalues.real))
        assert hist.converged
    for f in out:
        assert out[f][0] == out["csr"][0] and np.array_equal(out[f][1], out["csr"][1]), f


@pytest.mark.parametrize("dtype", DTYPES)
def test_stencil_mask_layout(dtype, monkeypatch):
    """One bit per dictionary slot and row.  (i) 27-point-like stencil with 19 slots (32-bit masks), complex values,
    boundary rows = sub-sequences: bit-identical to the CSR blocks.  (ii) x containing Inf next to ABSENT slots: a
    skipped slot must never be multiplied.  (iii) a matrix whose rows cannot be embedded in one entry order (two rows
    using the same two dictionary entries in opposite orders) falls back to the delta-value-indexed layout;
    KS_SPMV_FORMAT=stencil then refuses.  (iv) 33 dictionary entries: too many slots -> DVI."""
    cplx = np.dtype(dtype).kind == "c"
    A, xv, rng = lc.stencil19(dtype)
    y, f, op = _apply(A, xv, dtype)
    assert f["layout"] == "stencil" and f["ndict"] == 19
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    y0, f0, _ = _apply(A, xv, dtype, op.ctx)
    assert f0["layout"] == "csr" and np.array_equal(y.view(np.uint64), y0.view(np.uint64))
    # (ii)
    monkeypatch.delenv("KS_SPMV_FORMAT")
    L = laplace3d(6, 5, 4).astype(dtype)
    m = L.shape[0]
    xi = rnd(rng, dtype, m)
    xi[5] = np.inf                      # x index 5 = right neighbour of row 4... and NOT a neighbour of row 6 (x = 0 of the next line)
    yi, fi, opi = _apply(L, xi, dtype)
    assert fi["layout"] == "stencil"
    ref = L @ xi
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(yi), fin) and np.allclose(yi[fin], ref[fin], rtol=1e-13, atol=1e-13)
    # (iii)
    # A conflict needs the SAME two entries in both orders, which sorted columns forbid (same deltas, same order); unsorted CSR
    # input can do it: row 0: (d1,5),(d2,7); row 2: (d2,7),(d1,5)  -> cycle
    ptr, idx, val = lc.opposite_orders(dtype)
    import ctypes as C

    Lh = pkg._lib.load()
    h = C.c_void_p()
    code = pkg._lib.KS_C64 if cplx else pkg._lib.KS_F64
    pkg._lib.check(Lh.ks_operator_csr(op.ctx._h, 6, 6, 4, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, pkg._lib.KS_CSR, 0, pkg._lib.KS_I64, code, C.byref(h)))
    opc = pkg.Operator(op.ctx, h, (6, 6), dtype)
    assert opc.format["layout"] == "csr-dvi"
    ws6 = pkg.ArnoldiWorkspace(6, 2, dtype, ctx=op.ctx)
    x6 = rnd(rng, dtype, 6)
    ws6.set_col(0, x6)
    ws6.apply(opc, 0, 1)
    want = np.zeros(6, dtype=dtype)
    want[0] = 5.0 * x6[1] + 7.0 * x6[2]
    want[2] = 7.0 * x6[4] + 5.0 * x6[3]
    np.testing.assert_allclose(ws6.col(1), want, rtol=1e-14)
    monkeypatch.setenv("KS_SPMV_FORMAT", "stencil")
    h2 = C.c_void_p()
    rc = Lh.ks_operator_csr(op.ctx._h, 6, 6, 4, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, pkg._lib.KS_CSR, 0, pkg._lib.KS_I64, code, C.byref(h2))
    assert rc == pkg._lib.KS_ERR_ARGUMENT
    monkeypatch.delenv("KS_SPMV_FORMAT")
    # (iv) a banded matrix with 33 distinct diagonals
    G = lc.banded33(dtype)
    n4 = G.shape[0]
    y4, f4, _ = _apply(G, rnd(rng, dtype, n4), dtype, op.ctx)
    assert f4["layout"] == "csr-dvi" and f4["ndict"] == 33


def test_malformed_pointer_arrays_are_rejected():
    """a non-monotone or out-of-range pointer array must be refused at upload (it would index host arrays
    during the CSC conversion, or device arrays in the SpMV, out of bounds)."""
    L = pkg._lib.load()
    ctx = pkg.default_context()
    val = np.ones(4)
    idx = np.array([0, 1, 2, 3], dtype=np.int64)
    for layout in (pkg._lib.KS_CSR, pkg._lib.KS_CSC):
        for ptr in ([0, 3, 2, 4, 4], [0, 1, 5, 3, 4], [1, 1, 2, 3, 4], [0, 1, 2, 3, 3]):
            p = np.array(ptr, dtype=np.int64)
            h = C.c_void_p()
            rc = L.ks_operator_csr(ctx._h, 4, 4, 4, p.ctypes.data, idx.ctypes.data, val.ctypes.data, layout, 0, pkg._lib.KS_I64, pkg._lib.KS_F64, C.byref(h))
            assert rc == pkg._lib.KS_ERR_ARGUMENT, (layout, ptr)
    bad_col = np.array([0, 1, 2, 7], dtype=np.int64)
    p = np.array([0, 1, 2, 3, 4], dtype=np.int64)
    h = C.c_void_p()
    assert L.ks_operator_csr(ctx._h, 4, 4, 4, p.ctypes.data, bad_col.ctypes.data, val.ctypes.data, pkg._lib.KS_CSR, 0, pkg._lib.KS_I64, pkg._lib.KS_F64, C.byref(h)) == pkg._lib.KS_ERR_ARGUMENT


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_blocked_csr_is_bit_identical(dtype, monkeypatch):
    """KS_LAYOUT_CSR_CB: the matrix split into column blocks, one launch each, the row sums continued from launch to launch
    in CSR order -- y must equal the plain CSR row-block layout BIT for bit, for 2, 3 and 5 blocks, with empty rows, rows
    confined to one block and rows that span all of them; the auto rule picks it for config 3's matrix (n = 1e6: x = 8 MB,
    scattered columns) and leaves a banded matrix alone."""
    A, x, rng = lc.colblock_matrix(dtype)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    monkeypatch.setenv("KS_SPMV_COLBLOCKS", "0")
    y0, f0, _ = _apply(A, x, dtype)
    assert f0["layout"] == "csr"
    for nb in ("2", "3", "5"):
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", nb)
        y, f, _ = _apply(A, x, dtype)
        assert f["layout"] == "csr-cb", f
        assert np.array_equal(y, y0), nb
    # the SINGLE-LAUNCH form (k_spmv_csr_cb: a workgroup keeps its rows' sums in registers while it walks the column blocks;
    # automatic from 5 blocks on): every rows-per-workgroup variant, 2 / 5 / 8 blocks, against one launch per block
    for nb in ("2", "5", "8"):
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", nb)
        for rpt in ("1", "2", "4", "8", "16"):
            monkeypatch.setenv("KS_SPMV_CB_RPT", rpt)
            y, f, _ = _apply(A, x, dtype)
            assert f["layout"] == "csr-cb" and np.array_equal(y, y0), (nb, rpt)
        monkeypatch.delenv("KS_SPMV_CB_RPT")
        monkeypatch.setenv("KS_SPMV_CB_SINGLE", "0")
        y, f, _ = _apply(A, x, dtype)
        assert np.array_equal(y, y0), nb
        monkeypatch.delenv("KS_SPMV_CB_SINGLE")
    # unsorted rows: the order of the additions would change -> the layout must refuse
    monkeypatch.setenv("KS_SPMV_COLBLOCKS", "2")
    U = lc.reversed_row(A, 5000)
    assert U is not None
    yu, fu, _ = _apply(U, x, dtype)
    assert fu["layout"] == "csr"
    monkeypatch.delenv("KS_SPMV_FORMAT")
    monkeypatch.delenv("KS_SPMV_COLBLOCKS")
    if np.dtype(dtype).kind == "f":
        H, xh, Bd = lc.colblock_big(rng, pkg, dtype)
        yh, fh, _ = _apply(H, xh, dtype)
        assert fh["layout"] == "csr-cb", fh
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", "0")
        yp, fp, _ = _apply(H, xh, dtype)
        assert fp["layout"] == "csr" and np.array_equal(yh, yp)
        monkeypatch.delenv("KS_SPMV_COLBLOCKS")
        _, fb, _ = _apply(Bd, xh, dtype)
        assert fb["layout"] != "csr-cb", fb


@pytest.mark.parametrize("grid", [(182, 182, 9), (181, 182, 10), (256, 128, 8), (64, 64, 70)])
def test_marching_forms_of_the_stencil_product_are_bit_identical(grid, monkeypatch):
    """Float64 stencil-mask products on one GPU go through the persistent kernels of csrc/ks_spmv_march.hpp: the z-marching form
    where a plane has >= 64 tiles of 512 rows and there are >= 8 planes (the first three grids: nx even, nx odd -- the near taps
    +-nx then sit at odd offsets --, a power-of-two plane), the window form for smaller planes (the last grid), the register form
    behind them.  Every form, k_spmv_stencil2 and the CSR row blocks must give the SAME bits (products rounded separately, added in
    slot order under the row's mask), for the plain product and -- through two block cycles of the expansion, whose Newton steps
    y = sigma (A x - theta x) are fused into these kernels -- for the shifted one: identical Hessenberg matrices, bit for bit."""
    from test_gpu_sstep import _lockstep

    mx, my, mz = grid
    A = laplace3d(mx, my, mz)
    n = A.shape[0]
    rng = np.random.default_rng(5)
    xv = rnd(rng, np.float64, n)
    forms = {"default": {}, "window": {"KS_MARCH_Z": "0"}, "registers": {"KS_MARCH_Z": "0", "KS_MARCH_WINDOW": "0"}, "stencil2": {"KS_STENCIL_MARCH": "0"},
             "z-ranges 5": {"KS_MARCH_ZR": "5"}}
    ys, Hs = {}, {}
    ctx = None
    for name, env in forms.items():
        for k_ in ("KS_MARCH_Z", "KS_MARCH_WINDOW", "KS_STENCIL_MARCH", "KS_MARCH_ZR"):
            monkeypatch.delenv(k_, raising=False)
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        y, f, op = _apply(A, xv, np.float64, ctx)
        ctx = op.ctx
        assert f["layout"] == "stencil"
        ys[name] = y
        for cyc, _Hs, Hb, _Vs, _Vb, rel, orth, info in _lockstep(A, np.float64, 8, 6, 8, 16, "SR", 2):
            if cyc == 1:
                assert info["blocks"] > 0 and info["abandoned"] == 0, (name, info)
                Hs[name] = Hb
    ref = A @ xv
    np.testing.assert_allclose(ys["default"], ref, rtol=0, atol=1e-13 * np.abs(ref).max())
    for name in forms:
        assert np.array_equal(ys[name].view(np.uint64), ys["default"].view(np.uint64)), name
        assert np.array_equal(Hs[name].view(np.uint64), Hs["default"].view(np.uint64)), name
    monkeypatch.delenv("KS_MARCH_ZR", raising=False)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    y0, f0, _ = _apply(A, xv, np.float64, ctx)
    assert f0["layout"] == "csr" and np.array_equal(y0.view(np.uint64), ys["default"].view(np.uint64))
