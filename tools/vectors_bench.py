#!/usr/bin/env python3
"""Eigenvectors and their residuals against the ORIGINAL matrix after a converged solve, two ways, in ONE process:

    python tools/vectors_bench.py [--grid 216] [--nev 20] [--tol 1e-6] [--rounds 5] [--trace-only]

  host    what the library offered before `ks_vectors`: partialeigen(P) -- the product V Y on the device and then a copy of all of
          it to the host -- followed by scipy `A @ X` and numpy column norms of A X - X diag(lambda)
  device  partialeigen(P, device=True) + api.residuals(A, X, lambda): the vectors stay in HBM, 2 r numbers come back

on the headline problem (7-point Laplacian on grid^3 points, nev = 20, which = SR, 20/40) after `partialschur` has converged.  Both
paths are warmed up once and then alternate over the rounds; every round's wall time (both end in a stream synchronisation) is
printed, the spread before the medians.  The two residual vectors are compared with the bound of tests/test_device_vectors_cpu.py
(`resid_bound`).  Prints ONE JSON line.

--trace-only runs the device path alone (three times), for `rocprofv3 --kernel-trace --stats -- python tools/vectors_bench.py
--trace-only`: the time of k_resid_cols alone; with 2 n r 8 bytes per call it is a bandwidth (the kernel is memory-bound: r
multiply-adds per 16 bytes read)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import import_package  # noqa: E402

ks = import_package()
M = ks.matrices
PEAK = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--nev", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    m, nev = args.grid, args.nev
    n = m ** 3
    A = M.to_scipy(*M.laplace3d_csr(m, m, m), n)
    ctx = ks.Context(0)
    op = ks.csr_operator(A, ctx)
    ws = ks.ArnoldiWorkspace(M.start_vector(n), max(20, 2 * nev), ctx=ctx)
    t0 = time.perf_counter()
    dec, hist = ks.partialschur_(op, ws, nev=nev, which="SR", tol=args.tol, restarts=2000)
    t_solve = time.perf_counter() - t0
    assert hist.converged, hist

    def host():
        lam, X = ks.partialeigen(dec)
        lam = lam.real
        AX = A @ X
        return lam, np.linalg.norm(AX - X * lam, axis=0), AX, X

    def device():
        lam, X = ks.partialeigen(dec, device=True)
        lam = lam.real
        res, bn = ks.residuals(op, X, lam)
        X.close()
        return lam, res, bn

    if args.trace_only:
        for _ in range(3):
            lam, res, _ = device()
        r = len(lam)
        print(json.dumps({"n": n, "r": r, "resid_max": float(res.max()), "bytes_per_k_resid_cols": 2.0 * n * r * 8}), flush=True)
        return
    from test_device_vectors_cpu import resid_bound

    lam, res_h, AX, X = host()
    _, res_d, bn = device()
    r = len(lam)
    bound = resid_bound(AX, X, np.diag(lam), res_h)
    ratio = np.abs(res_d - res_h) / bound
    del AX, X
    t = {"host": [], "device": []}
    for _ in range(args.rounds):
        for name, fn in (("host", host), ("device", device)):
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t[name].append(time.perf_counter() - t0)
    out = {"n": n, "r": r, "tol": args.tol, "solve_seconds": t_solve, "mvproducts": hist.mvproducts, "rounds": args.rounds,
           "bytes_copied_to_host": {"host": 8.0 * n * r, "device": 16.0 * r}}
    for name in ("host", "device"):
        v = np.array(t[name])
        out[name] = {"seconds": [round(float(x), 4) for x in v], "min_s": float(v.min()), "max_s": float(v.max()), "median_s": float(np.median(v))}
    out["speedup_at_median"] = out["host"]["median_s"] / out["device"]["median_s"]
    out["residuals"] = {"host_max": float(res_h.max()), "device_max": float(res_d.max()), "largest_abs_difference": float(np.abs(res_d - res_h).max()),
                        "largest_difference_over_bound": float(ratio.max()), "bnorm_minus_one_max": float(np.abs(bn - 1.0).max())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
