"""The preconditioned conjugate-gradient solve operator (ks_operator_pcg, csrc/ks_pcg.hpp) at a size a user would run, next to
ks_operator_cg measured the same way in the same job: what the new kernels cost per launch, and what a preconditioner buys per solve.

    python tools/pcg_bench.py [--size 216] [--rounds 3] [--tol 1e-12] [--out profiles/pcg_operator.txt]

Operators (Float64, m^3 grid):
  jump   -div(c grad), Dirichlet, c = 1 for x < m / 2 and 100 beyond, times exp(0.3 N(0, 1)) per cell (extras.diffusion_terms,
         grid_variable_operator); solvers: cg_operator, pcg_operator with extras.jacobi_preconditioner on the fused path and, under
         KS_PCG_FUSED=0, on the generic one.
  aniso  the 7-point stencil with taps (z, y, x) = (1e-2, 1e-2, 1) (-1, 2, -1) plus a potential 0.05 U(0, 1) (grid_operator);
         solvers: cg_operator and pcg_operator with extras.line_preconditioner.
Per solver:
  split  `rounds` solves, each under the library's HIP-event profile (means; the spread of a share is its max - min over them): us per launch by class -- spmv: the product (generic path: and M), dots:
         k_*_pq (generic path: and k_pcg_rz, 16 bytes per row each), axpy: k_*_resid, fused: k_*_dir, scale: the start -- and each
         class's algorithmic bytes over its time as a fraction of the 8 TB/s HBM rate.  Events slow the enqueue down: a pass of its own.
  solve  ms per solve (host clock around a synchronised apply), `rounds` alternating rounds of all solvers of the operator.
Then the diagonal operator alone, and the three expectations of the feature with the measured values next to them.
Prints one JSON line per operator and writes the table to --out."""
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
from arnoldimethod_jl_amd import extras  # noqa: E402

PEAK = 8.0e12
CLASSES = ("spmv", "dots", "axpy", "fused", "scale")
VECTOR = ("dots", "axpy", "fused")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), std=float(v.std(ddof=1)) if v.size > 1 else 0.0, min=float(v.min()), max=float(v.max()),
                rounds=[round(float(x), 3) for x in v])


def info_of(op):
    return op.pcg_info if hasattr(op, "preconditioner") else op.cg_info


def timed_solve(ctx, ws, op):
    ctx.synchronize()
    t0 = time.perf_counter()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def split_of(ctx, ws, op, n):
    ctx.profile_enable(True)
    ctx.profile_reset()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    out = {}
    for cls in CLASSES:
        p = prof[cls]
        out[cls] = dict(launches=p["count"], us=1e3 * p["ms"] / max(p["count"], 1), bytes_per_row=p["bytes"] / max(p["count"], 1) / n,
                        hbm_fraction=(p["bytes"] / (1e-3 * p["ms"]) / PEAK) if p["ms"] > 0 else 0.0)
    return out


def split_rounds(ctx, ws, op, n, rounds):
    """split_of `rounds` times: the means, and per class the spread (max - min) of the HBM share over the rounds."""
    runs = [split_of(ctx, ws, op, n) for _ in range(rounds)]
    out = {}
    for cls in CLASSES:
        fr = [r[cls]["hbm_fraction"] for r in runs]
        out[cls] = dict(launches=runs[0][cls]["launches"], us=float(np.mean([r[cls]["us"] for r in runs])), bytes_per_row=runs[0][cls]["bytes_per_row"],
                        hbm_fraction=float(np.mean(fr)), hbm_spread=float(max(fr) - min(fr)))
    return out


def bench_operator(ctx, name, n, solvers, args, lines):
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    its, ys = {}, {}
    for key, op in solvers.items():      # warm-up: every solver once; the results must agree
        timed_solve(ctx, ws, op)
        its[key] = info_of(op)["last_iterations"]
        ys[key] = ws.col(1)
    first = next(iter(solvers))
    agree = {key: float(np.linalg.norm(ys[key] - ys[first]) / np.linalg.norm(ys[first])) for key in solvers}
    same_bits = {key: bool(np.array_equal(ys[key], ys["pcg-jacobi"])) for key in solvers if key == "pcg-generic"}
    ms = {key: [] for key in solvers}
    for _ in range(args.rounds):
        for key, op in solvers.items():
            ms[key].append(timed_solve(ctx, ws, op))
    split = {key: split_rounds(ctx, ws, op, n, args.rounds) for key, op in solvers.items()}
    vector = {key: sum(split[key][c]["us"] * split[key][c]["launches"] for c in VECTOR) / max(split[key]["fused"]["launches"], 1) for key in solvers}
    out = dict(operator=name, n=n, tol=args.tol, iterations=its, agreement=agree, same_bits=same_bits,
               ms_per_solve={k: stats(v) for k, v in ms.items()}, split=split, vector_us_per_iteration=vector,
               us_per_iteration={k: 1e3 * float(np.mean(v)) / max(its[k], 1) for k, v in ms.items()})
    print(json.dumps(out), flush=True)
    lines.append("%s, n = %d, tol = %g" % (name, n, args.tol))
    for key in solvers:
        lines.append("  %s: %d iterations, ||y - y_%s|| / ||y_%s|| = %.2e" % (key, its[key], first, first, agree[key]))
        lines.append("    class   launches   us/launch   bytes/row   of 8 TB/s   (mean of %d profiled solves; +- spread of the share)" % args.rounds)
        for cls in CLASSES:
            s = split[key][cls]
            lines.append("    %-6s %9d %11.2f %11.1f %10.1f %%   +- %.1f" % (cls, s["launches"], s["us"], s["bytes_per_row"], 100 * s["hbm_fraction"], 100 * s["hbm_spread"]))
        lines.append("    vector work of one iteration by events: %.1f us; one iteration by the host clock: %.1f us" % (vector[key], out["us_per_iteration"][key]))
    if same_bits:
        lines.append("  pcg-generic and pcg-jacobi give the same bits: %s" % same_bits["pcg-generic"])
    lines.append("  ms per solve, %d alternating rounds (mean +- std [min, max]):" % args.rounds)
    for key in solvers:
        s = out["ms_per_solve"][key]
        lines.append("    %-12s %10.2f +- %7.2f  [%10.2f, %10.2f]   %d iterations" % (key, s["mean"], s["std"], s["min"], s["max"], its[key]))
    lines.append("")
    ws.close()
    return out


def bench_diagonal(ctx, n, lines):
    D = ks.diagonal_operator(0.5 + np.random.default_rng(3).random(n), ctx=ctx)
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    for _ in range(3):
        ws.apply(D, 0, 1)
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(20):
        ws.apply(D, 0, 1)
    ctx.synchronize()
    p = ctx.profile_get()["spmv"]
    ctx.profile_enable(False)
    out = dict(launches=p["count"], us=1e3 * p["ms"] / p["count"], hbm_fraction=p["bytes"] / (1e-3 * p["ms"]) / PEAK)
    lines.append("diagonal operator alone (k_diag_apply, 24 bytes per row, n = %d): %d launches %9.2f us/launch %6.1f %% of 8 TB/s"
                 % (n, out["launches"], out["us"], 100 * out["hbm_fraction"]))
    lines.append("")
    ws.close()
    D.close()
    return out


def expectations(jump, aniso, lines):
    """The three expectations of the feature against what this job measured; a miss is said so ("about" the iteration ratio: at
    least 80 % of it)."""
    cg, pj, pg = jump["split"]["cg"], jump["split"]["pcg-jacobi"], jump["split"]["pcg-generic"]
    lines.append("expectations (jump):")
    shares = [cg[c]["hbm_fraction"] for c in VECTOR]
    lo, hi = min(shares), max(shares)
    tol = max(max(s[c]["hbm_spread"] for c in VECTOR) for s in (cg, pj, pg))      # run to run: the largest max - min of any kernel's share
    lines.append("  1. the new streaming kernels reach the HBM-rate share of the CG kernels of this job (%.2f - %.2f) within the spread of "
                 "the shares over the profiled solves (%.3f):" % (lo, hi, tol))
    for label, s, c in (("k_pcg_resid<jacobi> (32 B/row)", pj, "axpy"), ("k_pcg_dir<jacobi> (48 B/row)", pj, "fused"), ("k_pcg_pq (16 B/row)", pj, "dots"),
                        ("k_pcg_resid (24 B/row)", pg, "axpy"), ("k_pcg_dir (40 B/row)", pg, "fused"), ("k_pcg_pq + k_pcg_rz (16 B/row)", pg, "dots")):
        f, ref = s[c]["hbm_fraction"], cg[c]["hbm_fraction"]
        lines.append("     %-34s %.3f against %.3f of its CG counterpart: %s" % (label, f, ref, "met" if f >= ref - tol else "MISSED"))
    vcg, vpj = jump["vector_us_per_iteration"]["cg"], jump["vector_us_per_iteration"]["pcg-jacobi"]
    spread = max((s["max"] - s["min"]) / s["mean"] for s in jump["ms_per_solve"].values())
    lines.append("  2. a fused Jacobi iteration costs at most 96/80 = 1.20 of a CG iteration's vector time (plus the spread of the rounds, %.3f): "
                 "%.1f us against %.1f us, ratio %.3f: %s" % (spread, vpj, vcg, vpj / vcg, "met" if vpj / vcg <= 1.2 + spread else "MISSED"))
    for tag, res, a, b in (("jump, fused Jacobi", jump, "cg", "pcg-jacobi"), ("jump, generic Jacobi", jump, "cg", "pcg-generic"), ("aniso, line solve", aniso, "cg", "pcg-line")):
        ri = res["iterations"][a] / max(res["iterations"][b], 1)
        rt = res["ms_per_solve"][a]["mean"] / res["ms_per_solve"][b]["mean"]
        lines.append("  3. time per solve falls by about the iteration ratio (%s): iterations %d -> %d (%.2fx), ms %.2f -> %.2f (%.2fx), "
                     "%.0f %% of the iteration ratio: %s" % (tag, res["iterations"][a], res["iterations"][b], ri, res["ms_per_solve"][a]["mean"],
                                                             res["ms_per_solve"][b]["mean"], rt, 100 * rt / ri, "met" if rt >= 0.8 * ri else "MISSED"))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxit", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_operator.txt"))
    args = ap.parse_args()
    import torch      # (as in bench.py: the device is looked for before the library's first call)

    if not torch.cuda.is_available():
        raise SystemExit("pcg_bench.py needs a GPU (the product path has no CPU fallback)")
    m = args.size
    shape, n = (m, m, m), m ** 3
    ctx = ks.Context(0)
    kw = dict(tol=args.tol, maxit=args.maxit)
    lines = ["preconditioned conjugate-gradient solve operator (tools/pcg_bench.py --size %d --rounds %d --tol %g), Float64" % (m, args.rounds, args.tol), ""]
    # jump
    rng = np.random.default_rng(29)
    c = np.where(np.arange(n) % m < m // 2, 1.0, 100.0) * np.exp(0.3 * rng.standard_normal(n))
    taps, d = extras.diffusion_terms(shape, c, 1.0, None)
    A = ks.grid_variable_operator(shape, taps, c, d, ctx=ctx)
    M = extras.jacobi_preconditioner(d, ctx=ctx)
    solvers = {"cg": ks.cg_operator(A, **kw), "pcg-jacobi": ks.pcg_operator(A, M, **kw)}
    os.environ["KS_PCG_FUSED"] = "0"
    solvers["pcg-generic"] = ks.pcg_operator(A, M, **kw)
    del os.environ["KS_PCG_FUSED"]
    assert solvers["pcg-jacobi"].pcg_info["path"] == "jacobi" and solvers["pcg-generic"].pcg_info["path"] == "generic"
    jump = bench_operator(ctx, "jump (-div(c grad), jump of 100 in c)", n, solvers, args, lines)
    for op in list(solvers.values()) + [M, A]:
        op.close()
    # aniso
    t = np.array([-1e-2, -1e-2, -1.0, 2.0 * 1.02, -1.0, -1e-2, -1e-2])
    v = 0.05 * np.random.default_rng(31).random(n)
    A = ks.grid_operator(shape, t, v, ctx=ctx)
    t0 = time.perf_counter()
    M = extras.line_preconditioner(shape, t, v, ctx=ctx)
    lines.append("line_preconditioner: factored on the host in %.2f s, %s" % (time.perf_counter() - t0, M.tridiag_info))
    solvers = {"cg": ks.cg_operator(A, **kw), "pcg-line": ks.pcg_operator(A, M, **kw)}
    aniso = bench_operator(ctx, "aniso (7-point, taps (1e-2, 1e-2, 1) (-1, 2, -1) + 0.05 U)", n, solvers, args, lines)
    for op in list(solvers.values()) + [M, A]:
        op.close()
    bench_diagonal(ctx, n, lines)
    expectations(jump, aniso, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
