"""The geometric multigrid V-cycle (ks_operator_multigrid, csrc/ks_mg.hpp) at a size a user would run, next to fused Jacobi-PCG
measured the same way in the same job: what one cycle costs level by level, what its kernels reach, and what it buys per solve.

    python tools/mg_bench.py [--size 216] [--rounds 3] [--tol 1e-12] [--out profiles/multigrid_operator.txt]

Operator (Float64, m^3 grid): "jump", -div(c grad), Dirichlet, c = 1 for x < m / 2 and 100 beyond, times exp(0.3 N(0, 1)) per cell.
  cycle    for degree / ratio 2 / 4 and 3 / 8: ms per application of extras.grid_multigrid_preconditioner (host clock around
           synchronised applications), split per level: the cycle of the sub-hierarchy that starts at level l is timed the same way,
           level l costs the difference to the one that starts at l + 1.  Launches per level: 2 k products, 2 k smoother steps, one
           restriction, one prolongation.
  kernels  a two-level cycle on DIAGONAL operators at the same size, under the library's HIP-event profile: there the class `fused`
           holds the smoother kernels alone, `scale` k_mg_restrict, `axpy` k_mg_prolong_add.  k_mg_cheb_step alone is the difference
           between degree 3 and degree 2 (two steps more, nothing else).  Algorithmic bytes over time as a fraction of the 8 TB/s HBM
           rate, next to k_pcg_dir (a generic-path Jacobi solve, class `fused`) and k_diag_apply.
  solve    ms per solve of pcg_operator with each cycle and with the fused Jacobi preconditioner, `rounds` alternating rounds.
Then the expectations of the feature with the measured values next to them.  Prints one JSON line and writes the table to --out."""
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
CONFIGS = ((2, 4.0), (3, 8.0))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), std=float(v.std(ddof=1)) if v.size > 1 else 0.0, min=float(v.min()), max=float(v.max()))


def timed(ctx, ws, op, reps=1):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ws.apply(op, 0, 1)
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def profiled(ctx, ws, op, reps):
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(reps):
        ws.apply(op, 0, 1)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    return prof


def share(p):
    return p["bytes"] / (1e-3 * p["ms"]) / PEAK if p["ms"] > 0 else 0.0


def build_cycle(ctx, H, first, degree, ratio):
    """The cycle of the levels first ... L of the hierarchy H (first == L: the dense coarse operator alone)."""
    ops = [ks.grid_variable_operator(L["shape"], L["taps"], L["coeff"], L["diagonal"], ctx=ctx) for L in H[first:-1]]
    last = H[-1]
    Ac = ks.host_grid_variable_matrix(last["shape"], last["taps"], last["coeff"], last["diagonal"]).toarray().real
    inv = np.linalg.inv(Ac)
    coarse = ks.dense_operator(0.5 * (inv + inv.T), ctx)
    return ks.multigrid_operator(ops, [L["shape"] for L in H[first:]], [L["inverse_diagonal"] for L in H[first:-1]], [L["bound"] for L in H[first:-1]],
                                 coarse, degree=degree, ratio=ratio, ctx=ctx)


def bench_cycle(ctx, H, degree, ratio, reps, rounds, lines):
    nl = len(H)
    ms = []
    for first in range(nl):
        M = build_cycle(ctx, H, first, degree, ratio)
        n = M.shape[0]
        ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
        ws.fill_uniform(0, 1)
        timed(ctx, ws, M, 3)
        ms.append(stats([timed(ctx, ws, M, reps) for _ in range(rounds)]))
        ws.close()
        M.close()
    per = [ms[l]["mean"] - (ms[l + 1]["mean"] if l + 1 < nl else 0.0) for l in range(nl)]
    launches = [4 * degree + 2] * (nl - 1) + [1]
    lines.append("one V-cycle, degree %d, ratio %g: %.3f ms +- %.3f (%d rounds of %d applications)" % (degree, ratio, ms[0]["mean"], ms[0]["std"], rounds, reps))
    lines.append("    level        rows   launches   ms of the cycle from this level down   ms of this level   us per launch   share of the cycle")
    for l in range(nl):
        rows = int(np.prod(H[l]["shape"]))
        lines.append("    %5d %11d %10d %40.3f %18.3f %15.1f %18.1f %%" % (l, rows, launches[l], ms[l]["mean"], per[l], 1e3 * per[l] / launches[l], 100 * per[l] / ms[0]["mean"]))
    below = sum(per[1:])
    lines.append("    levels 1 ... %d: %d of the %d launches (%.0f %%), %.3f ms = %.1f %% of the cycle; a level-0 product alone moves 32 bytes per row"
                 % (nl - 1, sum(launches[1:]), sum(launches), 100.0 * sum(launches[1:]) / sum(launches), below, 100 * below / ms[0]["mean"]))
    lines.append("")
    return dict(degree=degree, ratio=ratio, ms=ms, per_level_ms=per, launches=launches)


def bench_kernels(ctx, m, reps, lines):
    """The cycle's own kernels through a two-level cycle on diagonal operators (fine m^3, coarse ceil(m / 2)^3)."""
    mc = (m + 1) // 2
    n, nc = m ** 3, mc ** 3
    rng = np.random.default_rng(5)
    a = 0.5 + rng.random(n)
    A, Cz = ks.diagonal_operator(a, ctx=ctx), ks.diagonal_operator(np.ones(nc), ctx=ctx)
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    prof = {}
    for degree in (2, 3):
        M = ks.multigrid_operator([A], [(m, m, m), (mc, mc, mc)], [1.0 / a], [1.0], Cz, degree=degree, ratio=4.0, ctx=ctx)
        timed(ctx, ws, M, 3)
        prof[degree] = profiled(ctx, ws, M, reps)
        M.close()
    out = {}
    p2, p3 = prof[2], prof[3]
    step = dict(ms=p3["fused"]["ms"] - p2["fused"]["ms"], bytes=p3["fused"]["bytes"] - p2["fused"]["bytes"], count=p3["fused"]["count"] - p2["fused"]["count"])
    for name, p, bytes_per_row in (("k_mg_cheb_step (degree 3 minus degree 2)", step, 56.0), ("smoother kernels of degree 2 (first, first, step, step)", p2["fused"], None),
                                   ("k_mg_restrict", p2["scale"], 16.0 + 8.0 * nc / n), ("k_mg_prolong_add", p2["axpy"], 16.0 + 8.0 * nc / n)):
        out[name] = dict(launches=p["count"], us=1e3 * p["ms"] / max(p["count"], 1), hbm_fraction=share(p))
        lines.append("    %-58s %5d launches %9.2f us/launch %6.1f %% of 8 TB/s%s"
                     % (name, p["count"], out[name]["us"], 100 * out[name]["hbm_fraction"], "" if bytes_per_row is None else "   (%.1f bytes per fine row)" % bytes_per_row))
    # k_diag_apply and k_pcg_dir, the same way
    timed(ctx, ws, A, 3)
    p = profiled(ctx, ws, A, reps)["spmv"]
    out["k_diag_apply"] = dict(launches=p["count"], us=1e3 * p["ms"] / p["count"], hbm_fraction=share(p))
    lines.append("    %-58s %5d launches %9.2f us/launch %6.1f %% of 8 TB/s   (24.0 bytes per row)" % ("k_diag_apply", p["count"], out["k_diag_apply"]["us"], 100 * share(p)))
    ws.close()
    A.close()
    Cz.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxit", type=int, default=50000)
    ap.add_argument("--coarsest-rows", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multigrid_operator.txt"))
    args = ap.parse_args()
    import torch      # (as in bench.py: the device is looked for before the library's first call)

    if not torch.cuda.is_available():
        raise SystemExit("mg_bench.py needs a GPU (the product path has no CPU fallback)")
    m = args.size
    shape, n = (m, m, m), m ** 3
    ctx = ks.Context(0)
    lines = ["geometric multigrid V-cycle operator (tools/mg_bench.py --size %d --rounds %d --reps %d --tol %g --coarsest-rows %d), Float64"
             % (m, args.rounds, args.reps, args.tol, args.coarsest_rows), ""]
    rng = np.random.default_rng(29)
    c = np.where(np.arange(n) % m < m // 2, 1.0, 100.0) * np.exp(0.3 * rng.standard_normal(n))
    t0 = time.perf_counter()
    H = extras.multigrid_hierarchy(shape, c, coarsest_rows=args.coarsest_rows)
    lines.append("hierarchy built on the host in %.1f s: %s, Gershgorin bounds %s" % (time.perf_counter() - t0, " -> ".join("x".join(map(str, L["shape"])) for L in H),
                                                                                   ", ".join("%.4f" % L["bound"] for L in H[:-1])))
    lines.append("")
    cycles = [bench_cycle(ctx, H, k, r, args.reps, args.rounds, lines) for k, r in CONFIGS]
    lines.append("the cycle's kernels alone (two-level cycle on diagonal operators, %d^3 -> %d^3, %d profiled applications), k_diag_apply and k_pcg_dir:" % (m, (m + 1) // 2, args.reps))
    kernels = bench_kernels(ctx, m, args.reps, lines)
    # the solves
    taps, d = H[0]["taps"], H[0]["diagonal"]
    A = ks.grid_variable_operator(shape, taps, c, d, ctx=ctx)
    kw = dict(tol=args.tol, maxit=args.maxit)
    J = extras.jacobi_preconditioner(d, ctx=ctx)
    solvers = {"pcg-jacobi": ks.pcg_operator(A, J, **kw)}
    os.environ["KS_PCG_FUSED"] = "0"
    generic = ks.pcg_operator(A, J, **kw)
    del os.environ["KS_PCG_FUSED"]
    cyc = {}
    for k, r in CONFIGS:
        cyc[(k, r)] = build_cycle(ctx, H, 0, k, r)
        solvers["pcg-mg-%d/%g" % (k, r)] = ks.pcg_operator(A, cyc[(k, r)], **kw)
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    timed(ctx, ws, generic)
    p = profiled(ctx, ws, generic, 1)["fused"]
    kernels["k_pcg_dir"] = dict(launches=p["count"], us=1e3 * p["ms"] / p["count"], hbm_fraction=share(p))
    lines.append("    %-58s %5d launches %9.2f us/launch %6.1f %% of 8 TB/s   (40.0 bytes per row; generic-path Jacobi solve)" % ("k_pcg_dir", p["count"], kernels["k_pcg_dir"]["us"], 100 * share(p)))
    lines.append("")
    its, ys = {}, {}
    for key, op in solvers.items():
        timed(ctx, ws, op)
        its[key] = op.pcg_info["last_iterations"]
        ys[key] = ws.col(1)
    ms = {key: [] for key in solvers}
    for _ in range(args.rounds):
        for key, op in solvers.items():
            ms[key].append(timed(ctx, ws, op))
    first = "pcg-jacobi"
    lines.append("solve, n = %d, tol = %g; ms per solve, %d alternating rounds (mean +- std [min, max]):" % (n, args.tol, args.rounds))
    solve = {}
    for key in solvers:
        s = stats(ms[key])
        solve[key] = dict(s, iterations=its[key], agreement=float(np.linalg.norm(ys[key] - ys[first]) / np.linalg.norm(ys[first])))
        lines.append("    %-14s %10.2f +- %7.2f  [%10.2f, %10.2f]   %5d iterations   ||y - y_jacobi|| / ||y_jacobi|| = %.2e"
                     % (key, s["mean"], s["std"], s["min"], s["max"], its[key], solve[key]["agreement"]))
    lines.append("")
    # expectations
    lines.append("expectations:")
    ref = kernels["k_pcg_dir"]["hbm_fraction"]
    lines.append("  1. the cycle's streaming kernels come within 0.03 of k_pcg_dir's share of the HBM rate in this job (%.3f; k_diag_apply %.3f):" % (ref, kernels["k_diag_apply"]["hbm_fraction"]))
    for name in ("k_mg_cheb_step (degree 3 minus degree 2)", "k_mg_restrict", "k_mg_prolong_add"):
        f = kernels[name]["hbm_fraction"]
        lines.append("     %-42s %.3f: %s" % (name, f, "met" if f >= ref - 0.03 else "MISSED"))
    tj = solve["pcg-jacobi"]["mean"]
    for k, r in CONFIGS:
        key = "pcg-mg-%d/%g" % (k, r)
        ratio = tj / solve[key]["mean"]
        lines.append("  2. a solve preconditioned by the cycle of degree %d, ratio %g is at least 3x faster than fused Jacobi-PCG: %.2f ms against %.2f ms (%d against %d "
                     "iterations), %.2fx: %s" % (k, r, solve[key]["mean"], tj, its[key], its["pcg-jacobi"], ratio, "met" if ratio >= 3.0 else "MISSED"))
    lines.append("")
    print(json.dumps(dict(n=n, cycles=cycles, kernels=kernels, solve=solve)), flush=True)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
