"""`-m "not gpu"`: which device layout a stored matrix gets (csrc/ks_csr_layout.hpp) through ks_host_csr_plan -- the plan make_csr
uploads, made without a device.  Every LAYOUT assertion of tests/test_gpu_spmv_layouts.py on the same matrices
(tests/layout_cases.py), the record of what uploaded operators reported before the planning was split from the upload
(tests/golden/csr_layout_plans.json: exact, floats included), and what only a plan can show: the stencil slot order, where the
column blocks are cut, how the row blocks tile the matrix."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import layout_cases as lc
from __graft_entry__ import ROOT, import_package
from oracle.matrices import laplace3d

pkg = import_package()
_lib = pkg._lib
DTYPES = [np.float64, np.complex128]
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "csr_layout_plans.json")))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in lc.LAYOUT_ENV:
        monkeypatch.delenv(k, raising=False)


def plan(M, dtype, arrays=False, rc_only=False):
    """ks_host_csr_plan on a scipy matrix or on the dict of layout_cases.matrix()."""
    if sp.issparse(M):
        M = lc._csr(M)
    L = _lib.load()
    dtype = np.dtype(dtype)
    val = np.ascontiguousarray(M["val"], dtype=dtype)
    n, nghost = M["n"], M["nghost"]
    lay, nd, bpn, aux = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    facts = np.zeros(len(_lib.PLAN_FACTS), dtype=np.int64)
    sdelta = np.zeros(32, dtype=np.int32)
    cap = n + 2 + len(val) // 1024 if arrays else 0   # (every block but a chunk of a long row holds a whole row)
    blkrow, blkptr, cbb = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64), np.zeros(9, dtype=np.int64)
    rc = L.ks_host_csr_plan(n, n + max(nghost, 0), len(val), M["ptr"].ctypes.data, M["idx"].ctypes.data, val.ctypes.data, _lib.KS_CSR, 0,
                            _lib.KS_I64, _lib.KS_C64 if dtype.kind == "c" else _lib.KS_F64, lc.NUM_CU, nghost, M["nlow"], C.byref(lay),
                            C.byref(nd), C.byref(bpn), C.byref(aux), facts.ctypes.data, sdelta.ctypes.data, blkrow.ctypes.data,
                            blkptr.ctypes.data, cap, cbb.ctypes.data, len(cbb))
    if rc_only or rc != 0:
        return rc
    out = dict(zip(_lib.PLAN_FACTS, (int(v) for v in facts)), layout=_lib.LAYOUTS[lay.value], ndict=nd.value, bytes_per_nnz=bpn.value,
               aux_bytes=aux.value, stencil_delta=sdelta[:int(facts[_lib.PLAN_FACTS.index("nstencil")])].tolist())
    if arrays:
        nb = out["nblk"]
        assert nb + 1 <= cap
        out.update(blkrow=blkrow[:nb + 1].copy(), blkptr=blkptr[:nb + 1].copy())
    out["cb_bounds"] = cbb[:out["ncolblocks"] + 1].tolist() if out["ncolblocks"] else []
    return out


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_plan_equals_the_record_of_uploaded_operators(case, monkeypatch):
    """layout, ndict and bytes_per_nnz of every recorded case: exactly what ks_operator_format reported for the uploaded operator
    on the MI355X before planning and upload were split (refused uploads: the same error code)."""
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    want = GOLDEN[lc.case_id(case)]
    got = plan(lc.matrix(case["matrix"], case["dtype"]), case["dtype"])
    if "error" in want:
        assert got == want["error"]
    else:
        assert {k: got[k] for k in ("layout", "ndict", "bytes_per_nnz")} == want


def test_record_covers_every_case():
    assert set(GOLDEN) == {lc.case_id(c) for c in lc.CASES}


@pytest.mark.parametrize("shape", [(37, 41, 43), (5, 3, 2), (300, 7, 1)])
def test_constant_coefficient_stencil_default_and_forced_formats(shape, monkeypatch):
    A = laplace3d(*shape)
    assert plan(A, np.float64)["layout"] == "stencil"
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    f0 = plan(A, np.float64)
    assert f0["layout"] == "csr" and f0["bytes_per_nnz"] == 12.0
    monkeypatch.setenv("KS_SPMV_FORMAT", "dvi")
    for rpt in ("1", "2", "4"):
        monkeypatch.setenv("KS_DVI_RPT", rpt)
        f1 = plan(A, np.float64)
        assert f1["layout"] == "csr-dvi" and f1["bytes_per_nnz"] == 1.0
    monkeypatch.setenv("KS_SPMV_FORMAT", "sellvi")
    assert plan(A, np.float64)["layout"] == "sell-vi"
    monkeypatch.setenv("KS_SPMV_FORMAT", "stencil")
    f3 = plan(A, np.float64)
    assert f3["layout"] == "stencil" and f3["ndict"] <= 7
    want = {"stencil": "stencil", "dvi": "csr-dvi", "vi": "csr-vi", "csr": "csr", "sell": "sell", "sellvi": "sell-vi"}
    for f, name in want.items():
        monkeypatch.setenv("KS_SPMV_FORMAT", f)
        assert plan(laplace3d(14, 15, 16), np.float64)["layout"] == name


@pytest.mark.parametrize("dtype", DTYPES)
def test_variable_coefficients_get_sliced_ellpack(dtype, monkeypatch):
    A, _x, R, _xr = lc.varcoef_and_ragged(dtype)
    f = plan(A, dtype)
    assert f["layout"] == "sell" and f["ndict"] == 0 and f["bytes_per_nnz"] < 1.15 * (4 + np.dtype(dtype).itemsize)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    assert plan(A, dtype)["layout"] == "csr"
    assert plan(R, dtype)["layout"] == "csr"
    for fmt_name, sigma in (("sell", "1"), ("sell", "256"), ("sellvi", "1"), ("sellvi", "640")):
        monkeypatch.setenv("KS_SPMV_FORMAT", fmt_name)
        monkeypatch.setenv("KS_SELL_SIGMA", sigma)
        f = plan(R, dtype)
        assert f["layout"] == ("sell-vi" if fmt_name == "sellvi" else "sell"), f


@pytest.mark.parametrize("dtype", DTYPES)
def test_stencil_mask_cases(dtype, monkeypatch):
    A, _x, _rng = lc.stencil19(dtype)
    f = plan(A, dtype)
    assert f["layout"] == "stencil" and f["ndict"] == 19 and f["stencil_mask_bytes"] == 4
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    assert plan(A, dtype)["layout"] == "csr"
    monkeypatch.delenv("KS_SPMV_FORMAT")
    assert plan(laplace3d(6, 5, 4).astype(dtype), dtype)["layout"] == "stencil"
    opp = lc.matrix("opposite", np.dtype(dtype).name)
    assert plan(opp, dtype)["layout"] == "csr-dvi"
    monkeypatch.setenv("KS_SPMV_FORMAT", "stencil")
    assert plan(opp, dtype, rc_only=True) == _lib.KS_ERR_ARGUMENT
    assert b"not sub-sequences of one entry order" in _lib.load().ks_last_error_string()
    monkeypatch.delenv("KS_SPMV_FORMAT")
    f4 = plan(lc.banded33(dtype), dtype)
    assert f4["layout"] == "csr-dvi" and f4["ndict"] == 33


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_blocks(dtype, monkeypatch):
    A, _x, rng = lc.colblock_matrix(dtype)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    monkeypatch.setenv("KS_SPMV_COLBLOCKS", "0")
    assert plan(A, dtype)["layout"] == "csr"
    for nb in ("2", "3", "5"):
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", nb)
        f = plan(A, dtype)
        assert f["layout"] == "csr-cb" and f["ncolblocks"] == int(nb), f
        assert (f["cb_rpt"] > 0) == (nb == "5")                  # the single launch from 5 blocks on
    for nb in ("2", "5", "8"):
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", nb)
        for rpt in ("1", "2", "4", "8", "16"):
            monkeypatch.setenv("KS_SPMV_CB_RPT", rpt)
            f = plan(A, dtype)
            assert f["layout"] == "csr-cb" and f["cb_rpt"] > 0, (nb, rpt)
        monkeypatch.delenv("KS_SPMV_CB_RPT")
        monkeypatch.setenv("KS_SPMV_CB_SINGLE", "0")
        f = plan(A, dtype)
        assert f["layout"] == "csr-cb" and f["cb_rpt"] == 0
        monkeypatch.delenv("KS_SPMV_CB_SINGLE")
    # unsorted rows: the order of the additions would change -> the layout must refuse
    monkeypatch.setenv("KS_SPMV_COLBLOCKS", "2")
    U = lc.reversed_row(A)
    assert U is not None
    assert plan(U, dtype)["layout"] == "csr"
    monkeypatch.delenv("KS_SPMV_FORMAT")
    monkeypatch.delenv("KS_SPMV_COLBLOCKS")
    if np.dtype(dtype).kind == "f":
        H, _xh, Bd = lc.colblock_big(rng, pkg, dtype)
        fh = plan(H, dtype)
        assert fh["layout"] == "csr-cb", fh
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", "0")
        assert plan(H, dtype)["layout"] == "csr"
        monkeypatch.delenv("KS_SPMV_COLBLOCKS")
        assert plan(Bd, dtype)["layout"] != "csr-cb"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ptr64", ["0", "1"])
def test_skewed_rows_long_rows_and_64bit_offsets(dtype, ptr64, monkeypatch):
    """KS_SPMV_PTR64=1 sets ptr64; rows longer than ni * 256 entries are cut into chunk blocks; the row blocks tile [0, nrows) and
    [0, nnz) exactly and none holds more than ni * 256 entries."""
    A, _x = lc.skewed_case(dtype)
    monkeypatch.setenv("KS_SPMV_PTR64", ptr64)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    f = plan(A, dtype, arrays=True)
    assert f["layout"] == "csr" and f["ptr64"] == int(ptr64)
    assert f["ni"] * 256 * np.dtype(dtype).itemsize <= 32768
    cap = f["ni"] * 256
    rowlen = np.diff(A.indptr)
    assert f["nlong"] == int((rowlen > cap).sum()) > 0
    br, bp = f["blkrow"], f["blkptr"]
    assert br[0] == 0 and br[-1] == A.shape[0] and bp[0] == 0 and bp[-1] == A.nnz
    assert np.all(np.diff(br) >= 0) and np.all(np.diff(br) <= 256) and np.all(np.diff(bp) >= 0) and np.all(np.diff(bp) <= cap)
    # a block is whole rows [br[b], br[b+1]) with exactly their entries -- or a chunk of one long row
    chunk = np.diff(br) == 0
    whole = ~chunk & ~np.isin(br[:-1], br[1:][chunk])
    assert np.array_equal(bp[:-1][whole], A.indptr[br[:-1][whole]]) and np.array_equal(bp[1:][whole], A.indptr[br[1:][whole]])
    assert np.all(rowlen[br[:-1][chunk]] > cap)


def test_stencil_slot_order_is_deterministic():
    """Two plans of one matrix: the same slots in the same order; the 7-point Laplacian in ascending column offset (the shape the
    marching kernels are selected by), its trailing slots on a slab naming ghost columns only."""
    A = laplace3d(9, 8, 7)
    a, b = plan(A, np.float64), plan(A, np.float64)
    assert a == b and a["stencil_delta"] == [-72, -9, -1, 0, 1, 9, 72]
    S, _x, _rng = lc.stencil19(np.complex128)
    a, b = plan(S, np.complex128), plan(S, np.complex128)
    assert a == b and len(set(a["stencil_delta"])) == 19
    M = lc.matrix("slab:24x24x24/3/1", "float64")
    a, b = plan(M, np.float64), plan(M, np.float64)
    assert a == b and a["layout"] == "stencil" and a["nstencil_local"] < a["nstencil"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rank", [0, 1, 2])
def test_column_blocks_of_a_distributed_row_block_respect_the_segments(rank, dtype, monkeypatch):
    """Ghosts above (rank 0), on both sides (rank 1), below (rank 2): in key space the columns are [ghosts of lower ranks | local
    columns | ghosts of higher ranks] and no column block straddles a segment boundary."""
    M = lc.matrix("slab:24x24x24/3/%d" % rank, np.dtype(dtype).name)
    monkeypatch.setenv("KS_SPMV_FORMAT", "csr")
    for nb in ("2", "4", "8"):
        monkeypatch.setenv("KS_SPMV_COLBLOCKS", nb)
        f = plan(M, dtype)
        assert f["layout"] == "csr-cb" and f["cb_rpt"] > 0, f     # (a distributed operator always takes the single launch)
        b = f["cb_bounds"]
        n, nlow, nghost = M["n"], M["nlow"], M["nghost"]
        assert b[0] == 0 and b[-1] == n + nghost and all(x < y for x, y in zip(b, b[1:])) and 2 <= len(b) - 1 <= 8
        for edge in (nlow, nlow + n):
            assert edge in b, (edge, b)
