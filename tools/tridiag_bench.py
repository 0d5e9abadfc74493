#!/usr/bin/env python3
"""Per-product time of the tridiagonal shift-invert operator (ks_operator_tridiag_solve) from the library's own HIP-event profile
(ks_profile_get class 0), with its algorithmic bytes against 8 TB/s:

    python tools/tridiag_bench.py [--n N] [--real] [--block-rows M] [--reps R] [--pencil [--rounds K]]

Default: BASELINE config 4's matrix (laplace1d + i diag(0.3 rand), sigma = 1.7 + 0.1i, ComplexF64) at n = 5e5; --real: laplace1d +
diag(0.3 rand), sigma = 1.7, Float64.  Prints ONE JSON line.

--pencil: that matrix as K of the pencil (K, M) with the consistent FEM mass M (1/6, 4/6, 1/6), T = K - sigma M.  Times, in ONE
process and alternating over K rounds of R products each, the fused operator y = T^-1 M x (ks_operator_tridiag_pencil), the same
product composed from two operators (product_operator(tridiagonal_solve_operator(T), csr_operator(M))) and the plain solve with T
alone (the floor): per-product time of every round, median, spread, and the algorithmic bytes the operators book."""
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
    ap.add_argument("--pencil", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    n = args.n
    rng = np.random.default_rng(0)
    r = 0.3 * rng.random(n)
    d = 2.0 + (r if args.real else 1j * r)
    off = -np.ones(n - 1)
    sigma = 1.7 if args.real else 1.7 + 0.1j
    ctx = ks.Context(0)
    if args.pencil:
        return pencil(args, ctx, off, d, sigma)
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


def pencil(args, ctx, off, d, sigma):
    import scipy.sparse as sp

    n = args.n
    mo, md = np.full(n - 1, 1.0 / 6.0), np.full(n, 4.0 / 6.0)
    fused = ks.tridiagonal_pencil_operator(off, d, off, mo, md, mo, sigma, ctx, block_rows=args.block_rows)
    T = (off - sigma * mo, d - sigma * md, off - sigma * mo)
    plain = ks.tridiagonal_solve_operator(*T, 0.0, ctx, block_rows=args.block_rows)
    M = sp.diags([mo, md, mo], [-1, 0, 1], format="csr").astype(fused.dtype)
    mul = ks.csr_operator(M, ctx)
    composed = ks.product_operator(plain, mul, ctx=ctx)
    forms = (("fused", fused), ("composed", composed), ("plain_solve", plain))
    ws = ks.ArnoldiWorkspace(n, 2, fused.dtype, ctx=ctx)
    ws.fill_uniform(0, 1)
    for _, op in forms:
        for _ in range(5):
            ws.apply(op, 0, 1)
    us = {name: [] for name, _ in forms}
    by = {}
    ctx.profile_enable(True)
    for _ in range(args.rounds):
        for name, op in forms:
            ctx.profile_reset()
            for _ in range(args.reps):
                ws.apply(op, 0, 1)
            ctx.synchronize()
            p = ctx.profile_get()["spmv"]
            us[name].append(1e3 * p["ms"] / args.reps)
            by[name] = p["bytes"] / args.reps
    ctx.profile_enable(False)
    out = {"n": n, "dtype": "f64" if args.real else "c128", "info": fused.tridiag_info, "layout_of_M": mul.format["layout"], "reps": args.reps,
           "rounds": args.rounds}
    for name, _ in forms:
        v = np.array(us[name])
        out[name] = {"us_per_product": [round(float(x), 3) for x in v], "median_us": float(np.median(v)), "min_us": float(v.min()),
                     "max_us": float(v.max()), "bytes_per_product": by[name], "GBps_at_median": by[name] / (np.median(v) * 1e-6) / 1e9}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
