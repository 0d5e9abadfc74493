"""The MINRES solve operator (ks_operator_minres, csrc/ks_minres.hpp) at a size a user would run: what one iteration costs and
where, against the same recurrence composed from torch operations -- what a user could do before the operator existed -- and against
the conjugate-gradient operator's iteration on a positive definite system of the same job (112 against 80 bytes per row).

    python tools/minres_bench.py [--size 216] [--rounds 5] [--tol 1e-12] [--out profiles/minres_operator.txt]

Operator (Float64, m^3 grid): the 7-point -Laplacian + V with V = 8 + U(0, 1) and six isolated wells V = -12, -11, ..., -7 (defect
states): the band lies above 8, each well binds one state below 0, so the shift sigma = 6 has exactly six eigenvalues below it and
a gap of about 2 to the band -- a shift INSIDE the spectrum at which a solve still ends in a few dozen iterations at any grid
size (a shift inside the band of a 10^7-point grid is 10^-6 from an eigenvalue).
  split    one solve under the library's HIP-event profile: us per launch of the product (class spmv) and of k_mr_alpha (dots),
           k_mr_resid (axpy), k_mr_step (fused), k_mr_init + k_mr_start (scale); each kernel's algorithmic bytes (16 / 32 / 64 per
           row; less in the first two iterations and the finishing step, counted here) over its time as a fraction of the 8 TB/s
           HBM rate.  The solver of this pass has maxit = the known iteration count, so no chunk is enqueued past the end and
           every launch in the averages is a working one.  Events slow the enqueue down: a pass of its own.
  solve    ms per solve (host clock around a synchronised apply), `rounds` alternating rounds of: the operator at check_every = 8
           (the default), 4, 16, the torch yardstick -- the identical recurrence as torch.dot / add_ calls around
           ks_operator_apply_raw inside a device_operator, alpha and beta' read back every iteration -- and cg_operator on
           A + 7 I (positive definite) for the per-iteration comparison.
Prints one JSON line and writes the table to --out."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from __graft_entry__ import import_package  # noqa: E402

ks = import_package()

PEAK = 8.0e12
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
EVERY = (8, 4, 16)
SIGMA = 6.0
CG_SHIFT = -7.0
WELLS = (-12.0, -11.0, -10.0, -9.0, -8.0, -7.0)
KERNELS = (("product", "spmv"), ("k_mr_alpha", "dots"), ("k_mr_resid", "axpy"), ("k_mr_step", "fused"), ("k_mr_init+start", "scale"))
CG_KERNELS = (("product", "spmv"), ("k_cg_pq", "dots"), ("k_cg_resid", "axpy"), ("k_cg_dir", "fused"))


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), std=float(v.std(ddof=1)) if v.size > 1 else 0.0, min=float(v.min()), max=float(v.max()),
                rounds=[round(float(x), 3) for x in v])


def potential(m):
    """V = 8 + U(0, 1) with six wells on the diagonal of the cube, at least m / 8 points apart (never neighbours)."""
    V = 8.0 + np.random.default_rng(5).random(m ** 3)
    for j, depth in enumerate(WELLS):
        i = (j + 1) * m // 8
        V[i + m * (i + m * i)] = depth
    return V


def torch_minres(product, x, y, bufs, shift, tol, maxit):
    """The recurrence of csrc/ks_minres.hpp in torch operations: y ~ (A - shift)^-1 x with `product(v_padded, q_padded)` filling
    q = A v; `bufs`: five padded vectors (v, v_, q, w_, w__).  Returns the iteration count."""
    import torch

    n = x.shape[0]
    vb, vmb, qb, wmb, wmmb = bufs
    y.zero_()
    beta1 = float(torch.linalg.vector_norm(x).item())
    if not beta1 > 0.0:
        return 0
    torch.div(x, beta1, out=vb[:n])
    for t in (vmb, wmb, wmmb):
        t.zero_()
    wm, wmm, q = wmb[:n], wmmb[:n], qb[:n]
    beta, c, s, c_, s_, phibar = 0.0, 1.0, 0.0, 1.0, 0.0, beta1
    for k in range(1, maxit + 1):
        v, vm = vb[:n], vmb[:n]
        product(vb, qb)
        if shift != 0.0:
            q.add_(v, alpha=-shift)
        alpha = float(torch.dot(v, q).item())
        q.add_(vm, alpha=-beta).add_(v, alpha=-alpha)
        beta_new = float(torch.linalg.vector_norm(q).item())
        eps, dbar = s_ * beta, c_ * beta
        delta, gbar = c * dbar + s * alpha, -s * dbar + c * alpha
        gamma = math.hypot(gbar, beta_new)
        if not (gamma > 0.0 and math.isfinite(gamma)):
            raise RuntimeError("singular")
        cn, sn = gbar / gamma, beta_new / gamma
        phi, phibar = cn * phibar, -sn * phibar
        wmm.mul_(-eps).add_(wm, alpha=-delta).add_(v).div_(gamma)      # the new w, over w__
        y.add_(wmm, alpha=phi)
        if abs(phibar) <= tol * beta1:
            return k
        torch.div(q, beta_new, out=vm)                                  # v+ over v_
        vb, vmb = vmb, vb
        wm, wmm = wmm, wm
        beta, c_, s_, c, s = beta_new, c, s, cn, sn
    return maxit


def torch_minres_operator(A, shift, tol, maxit, ctx):
    """`torch_minres` on the library's stream, the product through ks_operator_apply_raw, inside a device_operator."""
    import torch

    n = A.shape[0]
    ld = (n + 63) // 64 * 64
    dev = torch.device("cuda", ctx.device)
    lib = ks._lib.load()
    state = {"iterations": 0, "buf": None}

    def product(vb, qb):
        ks._lib.check(lib.ks_operator_apply_raw(A._h, vb.data_ptr(), qb.data_ptr()))

    def fn(y, x):
        if state["buf"] is None:      # (padded like a basis column: stored-matrix kernels may read the pad rows of v)
            state["buf"] = [torch.zeros(ld, dtype=torch.float64, device=dev) for _ in range(5)]
        state["iterations"] = torch_minres(product, x, y, state["buf"], shift, tol, maxit)

    op = ks.device_operator(fn, n, np.float64, ctx=ctx)
    op.state = state
    return op


def timed_solve(ctx, ws, op):
    ctx.synchronize()
    t0 = time.perf_counter()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def minres_bytes_per_row(its):
    """Bytes per row that the three MINRES kernels move over a whole solve of `its` iterations (Float64): the first iteration reads
    neither v_ nor a direction, the second no w__, and the finishing step neither reads r nor writes w and v+."""
    step = 0
    for k in range(1, its + 1):
        reads = 16 + (8 if k >= 2 else 0) + (8 if k >= 3 else 0)      # v, y, w_, w__
        step += reads + (8 if k == its else 8 + 24)                      # done: y; else r read, w, y, v+ written
    return {"k_mr_alpha": 16 * its, "k_mr_resid": 24 + 32 * (its - 1), "k_mr_step": step}


def cg_bytes_per_row(its):
    """... and the three conjugate-gradient kernels (the finishing k_cg_dir moves 24 instead of 40)."""
    return {"k_cg_pq": 16 * its, "k_cg_resid": 24 * its, "k_cg_dir": 40 * (its - 1) + 24}


def event_split(ctx, ws, op, kernels, n, its, total_bytes_per_row):
    """One solve under the HIP-event profile.  `op` has maxit = its, the known iteration count, so that every launch is a working
    one (a chunk enqueued past `done` would add kernels that return at entry to the averages); the streaming kernels are priced
    with the bytes counted by the functions above, the product with the library's own figure."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    split = {}
    for label, cls in kernels:
        p = prof[cls]
        if cls != "scale" and p["count"] != its:
            raise SystemExit("%s: %d launches in a solve of %d iterations: the split would average over idle launches" % (label, p["count"], its))
        total = total_bytes_per_row.get(label, p["bytes"] / n) * n
        split[label] = dict(launches=p["count"], us=1e3 * p["ms"] / max(p["count"], 1), bytes_per_row=total / max(p["count"], 1) / n,
                            hbm_fraction=(total / (1e-3 * p["ms"]) / PEAK) if p["ms"] > 0 else 0.0)
    return split


def split_lines(split, kernels, lines):
    lines.append("  kernel            launches   us/launch   bytes/row   of 8 TB/s")
    for label, _ in kernels:
        s = split[label]
        lines.append("  %-16s %9d %11.2f %11.1f %10.1f %%" % (label, s["launches"], s["us"], s["bytes_per_row"], 100 * s["hbm_fraction"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minres_operator.txt"))
    args = ap.parse_args()
    import torch      # (before the library's first device call, as in bench.py: the yardstick runs torch kernels on the library's stream)

    if not torch.cuda.is_available():
        raise SystemExit("minres_bench.py needs a GPU (the product path has no CPU fallback)")
    m = args.size
    shape, n = (m, m, m), m ** 3
    ctx = ks.Context(0)
    A = ks.grid_operator(shape, LAPLACE, potential(m), ctx=ctx)
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    solvers = {"minres/%d" % e: ks.minres_operator(A, shift=SIGMA, tol=args.tol, maxit=args.maxit, check_every=e) for e in EVERY}
    solvers["torch"] = torch_minres_operator(A, SIGMA, args.tol, args.maxit, ctx)
    solvers["cg/8"] = ks.cg_operator(A, shift=CG_SHIFT, tol=args.tol, maxit=args.maxit)

    def count(key):
        op = solvers[key]
        return op.state["iterations"] if key == "torch" else (op.cg_info if key.startswith("cg") else op.minres_info)["last_iterations"]

    its, ys = {}, {}
    for key, op in solvers.items():      # warm-up: every solver once; the two MINRES forms must agree
        timed_solve(ctx, ws, op)
        its[key] = count(key)
        ys[key] = ws.col(1)
    agree = float(np.linalg.norm(ys["minres/8"] - ys["torch"]) / np.linalg.norm(ys["torch"]))
    # the true residual of the fused solve, on the device: (A - sigma) y against b
    b = ws.col(0)
    wr = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    wr.set_col(0, ys["minres/8"])
    wr.apply(A, 0, 1)
    true_res = float(np.linalg.norm(wr.col(1) - SIGMA * ys["minres/8"] - b) / np.linalg.norm(b))
    wr.close()
    ms = {key: [] for key in solvers}
    for _ in range(args.rounds):
        for key, op in solvers.items():
            ms[key].append(timed_solve(ctx, ws, op))
    # the split: solvers that stop enqueueing at the known count (same bits, same count, no idle launches behind `done`)
    exact = ks.minres_operator(A, shift=SIGMA, tol=args.tol, maxit=its["minres/8"])
    cg_exact = ks.cg_operator(A, shift=CG_SHIFT, tol=args.tol, maxit=its["cg/8"])
    split = event_split(ctx, ws, exact, KERNELS, n, its["minres/8"], minres_bytes_per_row(its["minres/8"]))
    cg_split = event_split(ctx, ws, cg_exact, CG_KERNELS, n, its["cg/8"], cg_bytes_per_row(its["cg/8"]))
    assert exact.minres_info["last_iterations"] == its["minres/8"] and cg_exact.cg_info["last_iterations"] == its["cg/8"]
    per_it = sum(split[label]["us"] for label, _ in KERNELS[:4])
    cg_per_it = sum(cg_split[label]["us"] for label, _ in CG_KERNELS)
    out = dict(n=n, tol=args.tol, sigma=SIGMA, iterations=its, agreement_with_torch=agree, true_relres=true_res,
               ms_per_solve={k: stats(v) for k, v in ms.items()}, split=split, cg_split=cg_split,
               us_per_iteration={k: 1e3 * float(np.mean(v)) / max(its[k], 1) for k, v in ms.items()})
    print(json.dumps(out), flush=True)
    fused, torch_ms = out["ms_per_solve"]["minres/8"], out["ms_per_solve"]["torch"]
    lines = ["MINRES solve operator (tools/minres_bench.py --size %d --rounds %d --tol %g), Float64" % (m, args.rounds, args.tol), "",
             "7-point -Laplacian + V (V = 8 + U(0, 1), six wells -12 ... -7), n = %d, shift %g (six eigenvalues below it), tol = %g:" % (n, SIGMA, args.tol),
             "  %d iterations (torch recurrence: %d), ||y - y_torch|| / ||y_torch|| = %.2e, true residual ||(A - sigma) y - b|| / ||b|| = %.2e"
             % (its["minres/8"], its["torch"], agree, true_res)]
    split_lines(split, KERNELS, lines)
    lines.append("  (a solve with maxit = %d: every launch is a working one; bytes/row is the mean over the solve -- the first two iterations and the finishing step move less)" % its["minres/8"])
    tail8 = -its["minres/8"] % 8
    lines.append("  one iteration by events: %.1f us (product %.1f + vector work %.1f); the timed solve / %d iterations by the host clock: %.1f us"
                 " (it also holds k_mr_init + k_mr_start and the %d products the last chunk of 8 runs past the end)" %
                 (per_it, split["product"]["us"], per_it - split["product"]["us"], its["minres/8"], out["us_per_iteration"]["minres/8"], tail8))
    lines.append("  ms per solve, %d alternating rounds (mean +- std [min, max]):" % args.rounds)
    for key in solvers:
        s = out["ms_per_solve"][key]
        lines.append("    %-10s %9.2f +- %6.2f  [%9.2f, %9.2f]   %d iterations" % (key, s["mean"], s["std"], s["min"], s["max"], its[key]))
    lines.append("  torch recurrence / fused operator: %.2fx per solve (%.2f ms against %.2f ms)" % (torch_ms["mean"] / fused["mean"], torch_ms["mean"], fused["mean"]))
    lines.append("")
    lines.append("conjugate gradients on A + %g I (positive definite) in the same job, %d iterations:" % (-CG_SHIFT, its["cg/8"]))
    split_lines(cg_split, CG_KERNELS, lines)
    lines.append("  one iteration by events: %.1f us (vector work %.1f for 80 B/row); the timed solve / %d iterations by the host clock: %.1f us (with k_cg_init + k_cg_start and %d products past the end)" %
                 (cg_per_it, cg_per_it - cg_split["product"]["us"], its["cg/8"], out["us_per_iteration"]["cg/8"], -its["cg/8"] % 8))
    lines.append("  MINRES / CG per iteration: %.2fx by events, %.2fx by the host clock; vector work %.2fx for 112 / 80 = 1.40x the bytes" %
                 (per_it / cg_per_it, out["us_per_iteration"]["minres/8"] / out["us_per_iteration"]["cg/8"],
                  (per_it - split["product"]["us"]) / (cg_per_it - cg_split["product"]["us"])))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
