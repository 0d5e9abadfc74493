"""The conjugate-gradient solve operator (ks_operator_cg, csrc/ks_cg.hpp) at a size a user would run: what one iteration costs and
where, against the same recurrence composed from torch operations -- what a user could do before the operator existed.

    python tools/cg_bench.py [--size 216] [--rounds 5] [--tol 1e-12] [--out profiles/cg_operator.txt]

Operators (Float64, m^3 grid): (mass) the Q1 mass matrix as a 27-point box operator, (lap7) the 7-point -Laplacian + V, V ~ U(0, 1).
Per operator:
  split    one solve under the library's HIP-event profile: us per launch of the product (class spmv) and of k_cg_pq (dots),
           k_cg_resid (axpy), k_cg_dir (fused), k_cg_init + k_cg_start (scale); each kernel's algorithmic bytes (16 / 24 / 40 per
           row) over its time as a fraction of the 8 TB/s HBM rate.  Events slow the enqueue down: a pass of its own.
  solve    ms per solve (host clock around a synchronised apply), `rounds` alternating rounds of: the operator at check_every =
           8 (the default), 4, 16, 32, and the torch yardstick -- the identical recurrence as torch.dot / add_ calls (96 bytes per row
           and iteration) around ks_operator_apply_raw, inside a device_operator, both scalars read back every iteration.
Next to them the rates of the Arnoldi kernels of the same job (classes dots / axpy / fused of ks_orthogonalize on 8 columns).
Prints one JSON line per operator and writes the table to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from __graft_entry__ import import_package  # noqa: E402

ks = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

PEAK = 8.0e12
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
EVERY = (8, 4, 16, 32)
KERNELS = (("product", "spmv"), ("k_cg_pq", "dots"), ("k_cg_resid", "axpy"), ("k_cg_dir", "fused"), ("k_cg_init+start", "scale"))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), std=float(v.std(ddof=1)) if v.size > 1 else 0.0, min=float(v.min()), max=float(v.max()),
                rounds=[round(float(x), 3) for x in v])


def torch_cg_operator(A, tol, maxit, ctx):
    """The recurrence of csrc/ks_cg.hpp in torch operations on the library's stream, the product through ks_operator_apply_raw."""
    import torch

    n = A.shape[0]
    ld = (n + 63) // 64 * 64
    dev = torch.device("cuda", ctx.device)
    lib = ks._lib.load()
    state = {"iterations": 0, "buf": None}

    def fn(y, x):
        if state["buf"] is None:      # (padded like a basis column: stored-matrix kernels may read the pad rows of p)
            state["buf"] = [torch.zeros(ld, dtype=torch.float64, device=dev) for _ in range(3)]
        rb, pb, qb = state["buf"]
        r, p, q = rb[:n], pb[:n], qb[:n]
        y.zero_()
        r.copy_(x)
        p.copy_(x)
        rho = rho0 = float(torch.dot(r, r).item())
        k = 0
        while k < maxit and rho0 > 0.0:
            k += 1
            ks._lib.check(lib.ks_operator_apply_raw(A._h, pb.data_ptr(), qb.data_ptr()))
            pq = float(torch.dot(p, q).item())
            if not (np.isfinite(pq) and pq > 0.0):
                raise RuntimeError("not positive definite")
            alpha = rho / pq
            r.add_(q, alpha=-alpha)
            rho_new = float(torch.dot(r, r).item())
            y.add_(p, alpha=alpha)
            if rho_new <= tol * tol * rho0:
                break
            torch.add(r, p, alpha=rho_new / rho, out=p)
            rho = rho_new
        state["iterations"] = k

    op = ks.device_operator(fn, n, np.float64, ctx=ctx)
    op.state = state
    return op


def timed_solve(ctx, ws, op):
    ctx.synchronize()
    t0 = time.perf_counter()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def bench_operator(ctx, name, A, n, args, lines):
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    solvers = {"cg/%d" % e: ks.cg_operator(A, tol=args.tol, maxit=args.maxit, check_every=e) for e in EVERY}
    solvers["torch"] = torch_cg_operator(A, args.tol, args.maxit, ctx)
    its = {}
    for key, op in solvers.items():      # warm-up: every solver once; the results must agree
        timed_solve(ctx, ws, op)
        its[key] = op.state["iterations"] if key == "torch" else op.cg_info["last_iterations"]
    ref = ws.col(1)
    ws.apply(solvers["cg/8"], 0, 1)
    y8 = ws.col(1)
    agree = float(np.linalg.norm(y8 - ref) / np.linalg.norm(ref))      # (ref: the torch solve, the last of the warm-up)
    ms = {key: [] for key in solvers}
    for _ in range(args.rounds):
        for key, op in solvers.items():
            ms[key].append(timed_solve(ctx, ws, op))
    # the split: one solve under the event profile
    cg = solvers["cg/8"]
    ctx.profile_enable(True)
    ctx.profile_reset()
    ws.apply(cg, 0, 1)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    split = {}
    for label, cls in KERNELS:
        p = prof[cls]
        us = 1e3 * p["ms"] / max(p["count"], 1)
        split[label] = dict(launches=p["count"], us=us, bytes_per_row=p["bytes"] / max(p["count"], 1) / n,
                            hbm_fraction=(p["bytes"] / (1e-3 * p["ms"]) / PEAK) if p["ms"] > 0 else 0.0)
    it8 = its["cg/8"]
    out = dict(operator=name, n=n, tol=args.tol, iterations=its, agreement_with_torch=agree, ms_per_solve={k: stats(v) for k, v in ms.items()},
               split=split, us_per_iteration={k: 1e3 * float(np.mean(v)) / max(its[k], 1) for k, v in ms.items()})
    print(json.dumps(out), flush=True)
    fused, torch_ms = out["ms_per_solve"]["cg/8"], out["ms_per_solve"]["torch"]
    lines.append("%s, n = %d, tol = %g: %d iterations (torch recurrence: %d), ||y - y_torch|| / ||y_torch|| = %.2e" % (name, n, args.tol, it8, its["torch"], agree))
    lines.append("  kernel            launches   us/launch   bytes/row   of 8 TB/s")
    for label, _ in KERNELS:
        s = split[label]
        lines.append("  %-16s %9d %11.2f %11.1f %10.1f %%" % (label, s["launches"], s["us"], s["bytes_per_row"], 100 * s["hbm_fraction"]))
    lines.append("  (launches beyond the %d iterations belong to the last chunk, which is enqueued whole: their kernels return at entry)" % it8)
    per_it = sum(split[label]["us"] for label, _ in KERNELS[:4])
    lines.append("  one iteration by events: %.1f us (product %.1f + vector work %.1f); by the host clock: %.1f us" %
                 (per_it, split["product"]["us"], per_it - split["product"]["us"], out["us_per_iteration"]["cg/8"]))
    lines.append("  ms per solve, %d alternating rounds (mean +- std [min, max]):" % args.rounds)
    for key in solvers:
        s = out["ms_per_solve"][key]
        lines.append("    %-8s %9.2f +- %6.2f  [%9.2f, %9.2f]   %d iterations" % (key, s["mean"], s["std"], s["min"], s["max"], its[key]))
    lines.append("  torch recurrence / fused operator: %.2fx per solve (%.2f ms against %.2f ms)" % (torch_ms["mean"] / fused["mean"], torch_ms["mean"], fused["mean"]))
    # which check_every beat the default by more than the spread (max - min) of the rounds, here; main() holds the operators together
    alt = {e: out["ms_per_solve"]["cg/%d" % e] for e in EVERY[1:]}
    out["better_than_default"] = [e for e, s in alt.items() if s["mean"] + max(fused["max"] - fused["min"], s["max"] - s["min"]) < fused["mean"]]
    lines.append("  check_every faster than the default 8 by more than the spread of the rounds, on this operator: %s" % (out["better_than_default"] or "none"))
    lines.append("")
    for op in solvers.values():
        op.close()
    ws.close()
    return out


def bench_arnoldi_kernels(ctx, A, n, lines):
    """k_dots / k_axpy and their fused kin in the same job: ks_orthogonalize of column 8 against 8 columns, event profile."""
    ws = ks.ArnoldiWorkspace(n, 9, np.float64, ctx=ctx)
    ws.reinitialize(0, ks.matrices.start_vector(n))
    ws.iterate_arnoldi(A, 1, 8)
    for _ in range(3):
        ws.fill_uniform(8, 3)
        ws.orthogonalize(8)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(10):
        ws.fill_uniform(8, 3)
        ws.orthogonalize(8)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    lines.append("Arnoldi kernels of the same job (ks_orthogonalize of one column against 8, n = %d):" % n)
    out = {}
    for cls in ("dots", "axpy", "fused"):
        p = prof[cls]
        if p["count"] == 0:
            lines.append("  class %-6s not run on this path" % cls)
            continue
        frac = p["bytes"] / (1e-3 * p["ms"]) / PEAK
        out[cls] = dict(launches=p["count"], us=1e3 * p["ms"] / p["count"], hbm_fraction=frac)
        lines.append("  class %-6s %4d launches %9.2f us/launch %6.1f %% of 8 TB/s" % (cls, p["count"], out[cls]["us"], 100 * frac))
    lines.append("")
    ws.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_operator.txt"))
    args = ap.parse_args()
    import torch      # (before the library's first device call, as in bench.py: the yardstick runs torch kernels on the library's stream)

    if not torch.cuda.is_available():
        raise SystemExit("cg_bench.py needs a GPU (the product path has no CPU fallback)")
    m = args.size
    shape, n = (m, m, m), m ** 3
    ctx = ks.Context(0)
    V = np.random.default_rng(5).random(n)
    ops = {"mass (27-point box, Q1)": ks.grid_box_operator(shape, extras.q1_fem_taps(3)[1], ctx=ctx),
           "lap7 (7-point -Laplacian + V)": ks.grid_operator(shape, LAPLACE, V, ctx=ctx)}
    lines = ["conjugate-gradient solve operator (tools/cg_bench.py --size %d --rounds %d --tol %g), Float64" % (m, args.rounds, args.tol), ""]
    results = [bench_operator(ctx, name, A, n, args, lines) for name, A in ops.items()]
    everywhere = sorted(set.intersection(*[set(r["better_than_default"]) for r in results]))
    lines.append("default check_every: %s" % ("no value is faster than 8 by more than the spread on every operator: it stays 8" if not everywhere
                                              else "faster than 8 by more than the spread on every operator: %s" % everywhere))
    lines.append("")
    bench_arnoldi_kernels(ctx, ops["lap7 (7-point -Laplacian + V)"], n, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
