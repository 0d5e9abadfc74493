#!/usr/bin/env python3
"""Per-product time of the tridiagonal shift-invert operator (ks_operator_tridiag_solve) from the library's own HIP-event profile
(ks_profile_get class 0), with its algorithmic bytes against 8 TB/s:

    python tools/tridiag_bench.py [--n N] [--real] [--block-rows M] [--reps R]

Default: BASELINE config 4's matrix (laplace1d + i diag(0.3 rand), sigma = 1.7 + 0.1i, ComplexF64) at n = 5e5; --real: laplace1d +
diag(0.3 rand), sigma = 1.7, Float64.  Prints ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from __graft_entry__ import import_package  # noqa: E402

ks = import_package()
PEAK = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--real", action="store_true")
    ap.add_argument("--block-rows", type=int, default=0)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(0)
    r = 0.3 * rng.random(n)
    d = 2.0 + (r if args.real else 1j * r)
    off = -np.ones(n - 1)
    sigma = 1.7 if args.real else 1.7 + 0.1j
    ctx = ks.Context(0)
    t0 = time.perf_counter()
    op = ks.tridiagonal_solve_operator(off, d, off, sigma, ctx, block_rows=args.block_rows)
    t_upload = time.perf_counter() - t0
    ws = ks.ArnoldiWorkspace(n, 2, op.dtype, ctx=ctx)
    ws.fill_uniform(0, 1)
    for _ in range(5):
        ws.apply(op, 0, 1)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(args.reps):
        ws.apply(op, 0, 1)
    ctx.synchronize()
    p = ctx.profile_get()["spmv"]
    ctx.profile_enable(False)
    us = 1e3 * p["ms"] / p["count"]
    gbs = p["bytes"] / (p["ms"] * 1e-3) / 1e9
    print(json.dumps({"n": n, "dtype": "f64" if args.real else "c128", "info": op.tridiag_info, "upload_seconds": t_upload, "products": p["count"],
                      "us_per_product": us, "bytes_per_product": p["bytes"] / p["count"], "GBps": gbs, "frac_of_8TBps": gbs / PEAK}), flush=True)


if __name__ == "__main__":
    main()
