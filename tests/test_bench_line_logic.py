"""`-m "not gpu"`: the part of bench.py that turns measured passes into the ONE JSON line, on synthetic passes -- a
failing transport must not take the line down, a deviating peer-to-peer pass is dropped, the roofline block carries the
moved-bytes figure next to the algorithmic one and marks committed PMC traffic as not measured in the run."""
import argparse
import importlib.util
import json
import os

import numpy as np

from __graft_entry__ import ROOT

spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

ARGS = argparse.Namespace(steps=10, warmup=2, no_cpu_baseline=True)
WL = dict(m=216, n=216 ** 3, nev=20, mindim=20, maxdim=40, which="SR")


def _pass(elapsed, ritz_shift=0.0, steps=200):
    prof = {k: dict(ms=100.0, bytes=5e11, count=200) for k in ("spmv", "dots", "axpy", "fused")}
    prof["fused"]["ms"] = 120.0
    prof.update(scale=dict(ms=0.0, bytes=0.0, count=0), rotate=dict(ms=9.0, bytes=4.8e10, count=10), fin=dict(ms=2.0, bytes=0.0, count=400))
    state = dict(steps=steps, bytes=3.0e12, moved=2.4e12, t_expand=0.9 * elapsed, t_restart=0.1 * elapsed, reorth=steps,
                 trail=[(20, 0)] * 10, ritz=np.sort_complex(np.arange(20.0) + ritz_shift + 0j))
    return dict(elapsed=elapsed, state=state, prof=prof, nnz_global=70263936, A_host=None,
                fmt=dict(bytes_per_nnz=0.1434, ndict=7, layout="stencil"), placement=dict(candidates=0),
                validation=dict(arnoldi_rel=3e-14, orth=9e-15, k=20, locked=0, ok=True),
                spmv_csr=dict(layout="csr", bytes_per_nnz=12.0, launches=20, avg_launch_ms=0.2, bytes_per_launch=1.04e9, GBps=5200.0, frac=0.65,
                              measured_in_run=True))


def test_single_gpu_line_has_contract_fields_and_honest_roofline():
    out = bench.make_line(ARGS, None, {"single": _pass(0.3)}, ["single"], 1, 0, False, WL, False)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["value"] == 200 / 0.3 and out["dtype"] == "f64" and out["vs_baseline"] is None and "workload" in out["config"]
    r = out["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and r["kernel"].startswith("k_axpy_dots_cs")
    fs = r["fused_step"]
    assert fs["moved_frac"] < fs["algorithmic_frac"] and "moved_bytes" in fs and "quote this one" in fs["what"]
    assert r["spmv"]["layout"] == "stencil" and r["spmv"]["frac"] == r["spmv"]["GBps"] / 8000.0
    if r["traffic"] is not None:
        assert r["traffic"]["measured_in_run"] is False
    json.dumps(out)


def test_line_comes_from_the_survivor_when_a_transport_failed():
    passes = {"p2p": _pass(0.25), "rccl": {"error": "RuntimeError: ncclAllReduce failed"}}
    out = bench.make_line(ARGS, None, passes, ["p2p", "rccl"], 8, 0, False, WL, False)
    assert out["value"] == 200 / 0.25 and out["config"]["transport"] == "p2p" and out["n_gpus"] == 8
    assert out["transports"]["rccl"] == {"error": "RuntimeError: ncclAllReduce failed"} and "value" in out["transports"]["p2p"]
    passes = {"p2p": {"error": "pass did not finish within 300 s (hung exchange?)"}, "rccl": _pass(0.31)}
    out = bench.make_line(ARGS, None, passes, ["p2p", "rccl"], 8, 0, False, WL, False)
    assert out["config"]["transport"] == "rccl" and out["value"] == 200 / 0.31


def test_line_appears_with_null_value_when_nothing_survived():
    passes = {"p2p": {"error": "x"}, "rccl": {"error": "y"}}
    out = bench.make_line(ARGS, None, passes, ["p2p", "rccl"], 8, 0, False, WL, False)
    assert out["value"] is None and out["metric"] == "arnoldi_iters_per_sec" and set(out["transports"]) == {"p2p", "rccl"}
    json.dumps(out)


def test_deviating_peer_to_peer_pass_is_dropped_and_faster_valid_pass_wins():
    passes = {"p2p": _pass(0.2, ritz_shift=1e-3), "rccl": _pass(0.3)}
    out = bench.make_line(ARGS, None, passes, ["p2p", "rccl"], 8, 0, False, WL, False)
    assert out["config"]["transport"] == "rccl" and "differ" in out["transports"]["p2p"]["error"]
    passes = {"p2p": _pass(0.2), "rccl": _pass(0.3)}
    out = bench.make_line(ARGS, None, passes, ["p2p", "rccl"], 8, 0, False, WL, False)
    assert out["config"]["transport"] == "p2p" and out["value"] == 200 / 0.2


def test_cpu_budget_respects_cgroup_quota():
    assert 1 <= bench.CPU_BUDGET <= (os.cpu_count() or 1)


def test_line_carries_validation_of_the_benched_state_and_the_plain_csr_spmv():
    """the line validates itself (test/expansion.jl:29-30 on the benched workspace) and reports the
    SpMV BASELINE.json's metric names -- plain CSR through k_spmv_csr -- measured in the run, next to the layout in use."""
    out = bench.make_line(ARGS, None, {"single": _pass(0.3)}, ["single"], 1, 0, False, WL, False)
    assert out["validation"]["ok"] is True and out["validation"]["arnoldi_rel"] < 1e-11 and out["validation"]["orth"] < 1.5e-10
    pc = out["roofline"]["spmv_plain_csr"]
    assert pc["layout"] == "csr" and pc["measured_in_run"] is True and pc["frac"] == 0.65 and "traffic" in pc
    assert out["roofline"]["spmv"]["layout"] == "stencil"  # what the solver ran is still reported as such
    json.dumps(out)


def test_rccl_runs_first_and_alone_by_default():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'os.environ.get("KS_BENCH_TRANSPORTS", "rccl,p2p")' in src
    assert 'init_process_group("nccl"' not in src  # control plane over gloo: the library's communicator is the only RCCL user


def test_spmv_bytes_follow_the_layout_and_a_block_cycle_moves_1156_n():
    """DESIGN 3S "Bytes": a headline block cycle (20 steps from k = 21, one block of 20) moves 20 * 17 n + 8 n * 41 + 8 n * 61
    = 1 156 n bytes -- the stencil-mask layout has no row pointers (17 B per row: one mask byte + x + y); VERDICT r4 found
    4 (n + 1) booked per product on top.  Layouts with row pointers keep them."""
    n, nnz = 216 ** 3, 70263936
    st = dict(bytes_per_nnz=n / nnz, ndict=7, layout="stencil")     # one mask byte per row
    assert abs(bench.spmv_bytes(st, nnz, n) - 17.0 * n) < 1.0
    cycle = 20 * bench.spmv_bytes(st, nnz, n) + 8.0 * n * (21 + 20) + 8.0 * n * (21 + 40)
    assert abs(cycle - 1156.0 * n) < 100.0
    assert bench.spmv_bytes(dict(bytes_per_nnz=12.0, ndict=0, layout="csr"), nnz, n) == 12.0 * nnz + 4.0 * (n + 1) + 16.0 * n
    assert bench.spmv_bytes(dict(bytes_per_nnz=12.0, ndict=0, layout="sell"), nnz, n) == 12.0 * nnz + 4.0 * (n / 64.0 + 1) + 16.0 * n


def test_block_cycles_report_no_dgks_passes_and_the_spread_of_the_timed_cycles():
    p = _pass(0.3)
    p["state"].update(blk_cycles=10, blk_blocks=10, cycle_s=[0.004, 0.0038, 0.0041, 0.0039, 0.0040, 0.0038, 0.0039, 0.0042, 0.0038, 0.0039])
    p["sstep"] = 20
    out = bench.make_line(ARGS, None, {"single": p}, ["single"], 1, 0, False, WL, False)
    assert out["config"]["dgks_second_passes"] is None and out["config"]["steps_in_blocks_with_second_stage"] == 200
    c = out["cycle_ms"]
    assert c["n"] == 10 and c["min"] == 3.8 and c["max"] == 4.2 and c["min"] <= c["median"] <= c["max"]
    assert out["roofline"]["kernel"].startswith("k_bupdate_mfma")
    p0 = _pass(0.3)
    out0 = bench.make_line(ARGS, None, {"single": p0}, ["single"], 1, 0, False, WL, False)
    assert out0["config"]["dgks_second_passes"] == 200 and out0["config"]["steps_in_blocks_with_second_stage"] is None


def test_traffic_fractions_book_speculative_products_to_the_interval_they_ran_in():
    """Round 5's line divided every byte of a cycle by the expansion interval although 10 of its 20 products had run during the
    previous restart interval (0.652 against a true 0.545).  The quoted figure is bytes over the WHOLE cycle time; the
    expansion-interval figure takes the speculative bytes out of its numerator."""
    n = 216 ** 3
    spmv_b = 17.0 * n
    moved = 20 * (20 * spmv_b + 6.611e9 + 4.918e9)          # 20 block cycles of the headline
    spec_bytes = 20 * bench.spec_chain_products(20) * spmv_b  # 10 products per cycle ran speculatively
    assert bench.spec_chain_products(20) == 10 and bench.spec_chain_products(5) == 4 and bench.spec_chain_products(1) == 0
    tf = bench.traffic_fractions(moved, spec_bytes, 20 * 2.869e-3, 20 * 0.558e-3, 1, 8000.0)
    assert abs(tf["cycle_frac"] - moved / (20 * 3.427e-3) / 1e9 / 8000.0) < 1e-12
    assert 0.53 < tf["cycle_frac"] < 0.56                                   # the reviewer's recomputation: 0.545
    assert abs(tf["expand_frac"] - (moved - spec_bytes) / (20 * 2.869e-3) / 1e9 / 8000.0) < 1e-12
    assert 0.56 < tf["expand_frac"] < 0.59 and tf["expand_frac"] < moved / (20 * 2.869e-3) / 1e9 / 8000.0   # 0.577, not 0.652
    # the line: a state with adopted chains
    p = _pass(0.3)
    p["state"].update(spec_products=100, spec_bytes=100 * spmv_b)
    fs = bench.make_line(ARGS, None, {"single": p}, ["single"], 1, 0, False, WL, False)["roofline"]["fused_step"]
    st = p["state"]
    assert fs["moved_frac"] == fs["cycle_frac"] == st["moved"] / (st["t_expand"] + st["t_restart"]) / 1e9 / 8000.0
    assert fs["expand_interval_frac"] == (st["moved"] - 100 * spmv_b) / st["t_expand"] / 1e9 / 8000.0
    assert fs["spec_products"] == 100 and "WHOLE cycle time" in fs["what"]


def test_dump_outputs_hold_the_last_cycle_in_float64_within_the_limit(tmp_path):
    """--dump-outputs: the last timed cycle's return values, H[0:k+1, 0:k] and the basis columns 0..k at a fixed, seeded
    sample of rows (the same rows every run), float64, at most 64 MB in all -- also at the headline size with k = maxdim - 1."""
    n, maxdim, k = 216 ** 3, 40, 39

    class _Ws:
        H = np.arange((maxdim + 1) * maxdim, dtype=np.float64).reshape(maxdim + 1, maxdim)

        def col(self, j):     # row-dependent: the sample must come from the rows it lists
            return np.arange(n, dtype=np.float64) + 1e7 * j

    lams = np.arange(maxdim) + 0.5j
    state = dict(k=k, last=dict(k=k, nlock=3, purge=0, eigenvalues=lams, residuals=np.ones(maxdim)))
    out = bench.last_cycle_outputs(_Ws(), state, n)
    assert out["H"].shape == (k + 1, k) and (out["H"] == _Ws.H[: k + 1, :k]).all()
    assert (out["eigenvalues_re"] == lams.real).all() and (out["eigenvalues_im"] == 0.5).all() and list(out["restart"]) == [k, 3, 0]
    assert out["V_rows"].shape == (bench.DUMP_SAMPLE_ROWS, k + 1)
    rows = out["V_row_index"]
    assert len(np.unique(rows)) == len(rows) and rows.max() < n and (np.diff(rows) > 0).all()
    for j in range(k + 1):
        assert (out["V_rows"][:, j] == rows + 1e7 * j).all(), j
    small = bench.last_cycle_outputs(_Ws(), dict(state, k=k), 1000)   # n below the sample size: every row, in order
    assert (small["V_row_index"] == np.arange(1000)).all() and (small["V_rows"][:, 3] == np.arange(1000) + 3e7).all()
    assert (bench.last_cycle_outputs(_Ws(), state, n)["V_row_index"] == rows).all()
    assert "V_rows" not in bench.last_cycle_outputs(_Ws(), state, n, sample_rows=False)
    bench.write_outputs(str(tmp_path / "d"), out)
    files = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert files == sorted(name + ".npy" for name in out)
    assert sum((tmp_path / "d" / f).stat().st_size for f in files) <= 64 << 20
    assert all(np.load(tmp_path / "d" / f).dtype == np.float64 for f in files)


def test_exit_status_fails_only_a_validated_state_that_violates_the_invariants():
    """A plain run carries no `validation`; a config-5 record (--config5 without --full included) carries its own.  Only
    a validation that failed -- of the headline or of config 5 -- makes the run exit 4; a record without one, or with an
    error instead of a measurement, does not."""
    ok, bad = dict(ok=True), dict(ok=False)
    assert bench.exit_status(dict(value=None)) == 3
    assert bench.exit_status(dict(value=1.0)) == 0
    assert bench.exit_status(dict(value=1.0, validation=ok, config5=dict(validation=ok))) == 0
    assert bench.exit_status(dict(value=1.0, config5=dict(value=2.0, validation=ok))) == 0
    assert bench.exit_status(dict(value=1.0, config5=dict(value=2.0, validation=None))) == 0
    assert bench.exit_status(dict(value=1.0, config5=dict(error="CommTimeout", transport="p2p"))) == 0
    assert bench.exit_status(dict(value=1.0, config5=None)) == 0
    assert bench.exit_status(dict(value=1.0, validation=bad)) == 4
    assert bench.exit_status(dict(value=1.0, config5=dict(value=2.0, validation=bad))) == 4
