"""The BiCGStab(2) solve operator (ks_operator_bicgstab, csrc/ks_bicgstab.hpp) at a size a user would run: what one iteration costs
and where, against the same recurrence composed from torch operations -- what a user could do before the operator existed -- and
against the conjugate-gradient operator's kernels on a symmetric system of the same job (88 against 80 bytes per row and product).

    python tools/bicgstab_bench.py [--size 216] [--rounds 5] [--tol 1e-12] [--out profiles/bicgstab_operator.txt]

Operator (Float64, m^3 grid): the 7-point convection-diffusion stencil [-1 - cz, -1 - cy, -1 - cx, 6, -1 + cx, -1 + cy, -1 + cz] with
c = (0.4, 0.3, 0.2) plus a potential V = U(0, 1): not symmetric; its spectrum lies right of 0 and the shift theta = -1 left of it.
  split    one solve under the library's HIP-event profile: us per launch of the product (class spmv) and of the streaming kernels
           by their profile classes -- k_bs_dot x 3 (dots), k_bs_u0 (axpy), k_bs_step1 and k_bs_dir2 (rotate: both read four
           vectors and write two), k_bs_step2 (fin), k_bs_mr_sums (scale), k_bs_mr with the one-workgroup k_bs_close (fused) --
           each priced with the bytes its WORKING launches move (counted here: the first k_bs_u0 reads no u0; the launches of the
           last iteration behind the stage that ended the solve return at entry and move nothing) as a fraction of the 8 TB/s HBM
           rate.  The solver of this pass has maxit = the known iteration count, so no chunk is enqueued past the end.  Events slow
           the enqueue down: a pass of its own.
  solve    ms per solve (host clock around a synchronised apply), `rounds` alternating rounds of: the operator at check_every = 8
           (the default), 4, 16, the torch yardstick -- the identical recurrence as torch.vdot / add_ calls around
           ks_operator_apply_raw inside a device_operator, every scalar read back -- and cg_operator on the symmetric part's
           -Laplacian + V + I for the per-kernel comparison.
Prints one JSON line and writes the table to --out."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minres_bench as mb  # noqa: E402  (stats, timed_solve, the CG split)

ks = mb.ks
PEAK = mb.PEAK
EVERY = (8, 4, 16)
THETA = -1.0
CG_SHIFT = -1.0
CONVECTION = (0.4, 0.3, 0.2)
# label, profile class, launches per full iteration
KERNELS = (("product", "spmv", 4), ("k_bs_dot", "dots", 3), ("k_bs_u0", "axpy", 1), ("k_bs_step1+dir2", "rotate", 2), ("k_bs_step2", "fin", 1),
           ("k_bs_mr_sums", "scale", 1), ("k_bs_mr+close", "fused", 1))


def taps():
    cx, cy, cz = CONVECTION
    return np.array([-1 - cz, -1 - cy, -1 - cx, 6.0, -1 + cx, -1 + cy, -1 + cz])


def working(its, stage):
    """label -> (working launches, bytes per row they move in all) of a solve that ended at `stage` of iteration `its`."""
    full = its - 1                       # iterations run in full; the last one runs as far as its stage
    s2, s3 = int(stage >= 2), int(stage >= 3)
    return {
        "product": (4 * full + 1 + s2 + s2 + s3, None),      # u1 always; r1, u2 behind stage 1; r2 behind stage 2 (the idle ones still run, too)
        "k_bs_dot": (3 * full + 1 + 2 * s2, 16 * (3 * full + 1 + 2 * s2)),
        "k_bs_u0": (its, 24 * its - 8),
        "k_bs_step1+dir2": (2 * full + 1 + s2, 48 * (2 * full + 1 + s2)),
        "k_bs_step2": (full + s2, 72 * (full + s2)),
        "k_bs_mr_sums": (full + s3, 24 * (full + s3)),
        "k_bs_mr+close": (full + s3, 88 * (full + s3)),
    }


def torch_bicgstab(product, x, y, bufs, shift, tol, maxit):
    """The recurrence of csrc/ks_bicgstab.hpp in torch operations: y ~ (A - shift)^-1 x with `product(v_padded, q_padded)` filling
    q = A v; `bufs`: six padded vectors (r0, r1, r2, u0, u1, u2).  Returns (iterations, stage)."""
    import torch

    n = x.shape[0]
    r0b, r1b, r2b, u0b, u1b, u2b = bufs
    r0, r1, r2, u0, u1, u2 = (t[:n] for t in bufs)
    dot = lambda a, c: float(torch.dot(a, c).item())
    y.zero_()
    beta1 = float(torch.linalg.vector_norm(x).item())
    if not beta1 > 0.0:
        return 0, 0
    stop = tol * beta1

    def mul(src_b, dst_b, src, dst):
        product(src_b, dst_b)
        if shift != 0.0:
            dst.add_(src, alpha=-shift)

    r0.copy_(x)
    rho0, alpha, omega = 1.0, 0.0, 1.0
    rho1 = dot(x, r0)
    for k in range(1, maxit + 1):
        rho0 = -omega * rho0
        beta = alpha * rho1 / rho0
        rho0 = rho1
        if k == 1:
            u0.copy_(r0)
        else:
            u0.mul_(-beta).add_(r0)
        mul(u0b, u1b, u0, u1)
        alpha = rho0 / dot(x, u1)
        r0.add_(u1, alpha=-alpha)
        y.add_(u0, alpha=alpha)
        if float(torch.linalg.vector_norm(r0).item()) <= stop:
            return k, 1
        mul(r0b, r1b, r0, r1)
        rho1 = dot(x, r1)
        beta = alpha * rho1 / rho0
        rho0 = rho1
        u0.mul_(-beta).add_(r0)
        u1.mul_(-beta).add_(r1)
        mul(u1b, u2b, u1, u2)
        alpha = rho0 / dot(x, u2)
        r0.add_(u1, alpha=-alpha)
        r1.add_(u2, alpha=-alpha)
        y.add_(u0, alpha=alpha)
        if float(torch.linalg.vector_norm(r0).item()) <= stop:
            return k, 2
        mul(r1b, r2b, r1, r2)
        g = torch.stack([torch.dot(r1, r1), torch.dot(r2, r2), torch.dot(r1, r2), torch.dot(r1, r0), torch.dot(r2, r0)]).tolist()
        det = g[0] * g[1] - g[2] * g[2]
        g1, g2 = (g[1] * g[3] - g[2] * g[4]) / det, (g[0] * g[4] - g[2] * g[3]) / det
        y.add_(r0, alpha=g1).add_(r1, alpha=g2)
        r0.add_(r1, alpha=-g1).add_(r2, alpha=-g2)
        u0.add_(u1, alpha=-g1).add_(u2, alpha=-g2)
        omega = g2
        rho1 = dot(x, r0)
        if not math.isfinite(rho1):
            raise RuntimeError("breakdown")
        if float(torch.linalg.vector_norm(r0).item()) <= stop:
            return k, 3
    return maxit, 3


def torch_bicgstab_operator(A, shift, tol, maxit, ctx):
    """`torch_bicgstab` on the library's stream, the product through ks_operator_apply_raw, inside a device_operator."""
    import torch

    n = A.shape[0]
    ld = (n + 63) // 64 * 64
    dev = torch.device("cuda", ctx.device)
    lib = ks._lib.load()
    state = {"iterations": 0, "stage": 0, "buf": None}

    def product(vb, qb):
        ks._lib.check(lib.ks_operator_apply_raw(A._h, vb.data_ptr(), qb.data_ptr()))

    def fn(y, x):
        if state["buf"] is None:      # (padded like a basis column: stored-matrix kernels may read the pad rows)
            state["buf"] = [torch.zeros(ld, dtype=torch.float64, device=dev) for _ in range(6)]
        state["iterations"], state["stage"] = torch_bicgstab(product, x, y, state["buf"], shift, tol, maxit)

    op = ks.device_operator(fn, n, np.float64, ctx=ctx)
    op.state = state
    return op


def event_split(ctx, ws, op, n, its, stage):
    """One solve under the HIP-event profile; `op` has maxit = its.  us per WORKING launch (the few launches of the last iteration
    behind its stage return at entry; their microseconds stay in the class total, which reads the average slightly high)."""
    ctx.profile_enable(True)
    ctx.profile_reset()
    ws.apply(op, 0, 1)
    ctx.synchronize()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    work = working(its, stage)
    split = {}
    for label, cls, per_it in KERNELS:
        p = prof[cls]
        if p["count"] != per_it * its:
            raise SystemExit("%s: %d launches in a solve of %d iterations (expected %d)" % (label, p["count"], its, per_it * its))
        launches, rows = work[label]
        if label == "product":
            launches, total = p["count"], p["bytes"]
        else:
            total = float(rows) * n
        split[label] = dict(launches=launches, us=1e3 * p["ms"] / max(launches, 1), bytes_per_row=total / max(launches, 1) / n,
                            hbm_fraction=(total / (1e-3 * p["ms"]) / PEAK) if p["ms"] > 0 else 0.0, ms=p["ms"])
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=216)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-12)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab_operator.txt"))
    args = ap.parse_args()
    import torch      # (before the library's first device call, as in bench.py: the yardstick runs torch kernels on the library's stream)

    if not torch.cuda.is_available():
        raise SystemExit("bicgstab_bench.py needs a GPU (the product path has no CPU fallback)")
    m = args.size
    shape, n = (m, m, m), m ** 3
    ctx = ks.Context(0)
    V = np.random.default_rng(5).random(n)
    A = ks.grid_operator(shape, taps(), V, ctx=ctx)
    Asym = ks.grid_operator(shape, mb.LAPLACE, V, ctx=ctx)
    ws = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.fill_uniform(0, 1)
    solvers = {"bicgstab/%d" % e: ks.bicgstab_operator(A, shift=THETA, tol=args.tol, maxit=args.maxit, check_every=e) for e in EVERY}
    solvers["torch"] = torch_bicgstab_operator(A, THETA, args.tol, args.maxit, ctx)
    solvers["cg/8"] = ks.cg_operator(Asym, shift=CG_SHIFT, tol=args.tol, maxit=args.maxit)

    def count(key):
        op = solvers[key]
        return op.state["iterations"] if key == "torch" else (op.cg_info if key.startswith("cg") else op.bicgstab_info)["last_iterations"]

    its, ys = {}, {}
    for key, op in solvers.items():      # warm-up: every solver once; the two BiCGStab(2) forms must agree
        mb.timed_solve(ctx, ws, op)
        its[key] = count(key)
        ys[key] = ws.col(1)
    stage = solvers["torch"].state["stage"]
    agree = float(np.linalg.norm(ys["bicgstab/8"] - ys["torch"]) / np.linalg.norm(ys["torch"]))
    # the true residual of the fused solve, on the device: (A - theta) y against b
    b = ws.col(0)
    wr = ks.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    wr.set_col(0, ys["bicgstab/8"])
    wr.apply(A, 0, 1)
    true_res = float(np.linalg.norm(wr.col(1) - THETA * ys["bicgstab/8"] - b) / np.linalg.norm(b))
    wr.close()
    ms = {key: [] for key in solvers}
    for _ in range(args.rounds):
        for key, op in solvers.items():
            ms[key].append(mb.timed_solve(ctx, ws, op))
    same_end = its["torch"] == its["bicgstab/8"]      # (the stage is the torch form's: the counters of the operator do not hold it)
    exact = ks.bicgstab_operator(A, shift=THETA, tol=args.tol, maxit=its["bicgstab/8"])
    cg_exact = ks.cg_operator(Asym, shift=CG_SHIFT, tol=args.tol, maxit=its["cg/8"])
    split = event_split(ctx, ws, exact, n, its["bicgstab/8"], stage if same_end else 3)
    cg_split = mb.event_split(ctx, ws, cg_exact, mb.CG_KERNELS, n, its["cg/8"], mb.cg_bytes_per_row(its["cg/8"]))
    assert exact.bicgstab_info["last_iterations"] == its["bicgstab/8"] and cg_exact.cg_info["last_iterations"] == its["cg/8"]
    k = its["bicgstab/8"]
    per_it = sum(split[label]["ms"] for label, _, _ in KERNELS) * 1e3 / k
    vec_it = per_it - split["product"]["ms"] * 1e3 / k
    cg_per_it = sum(cg_split[label]["us"] for label, _ in mb.CG_KERNELS)
    out = dict(n=n, tol=args.tol, theta=THETA, iterations=its, stage=stage, agreement_with_torch=agree, true_relres=true_res,
               ms_per_solve={key: mb.stats(v) for key, v in ms.items()}, split=split, cg_split=cg_split,
               us_per_iteration={key: 1e3 * float(np.mean(v)) / max(its[key], 1) for key, v in ms.items()})
    print(json.dumps(out), flush=True)
    fused, torch_ms = out["ms_per_solve"]["bicgstab/8"], out["ms_per_solve"]["torch"]
    lines = ["BiCGStab(2) solve operator (tools/bicgstab_bench.py --size %d --rounds %d --tol %g), Float64" % (m, args.rounds, args.tol), "",
             "7-point convection-diffusion, c = %s, V = U(0, 1), n = %d, shift %g (left of the spectrum), tol = %g:" % (CONVECTION, n, THETA, args.tol),
             "  %d iterations of four products (torch recurrence: %d, ending at stage %d), ||y - y_torch|| / ||y_torch|| = %.2e, true residual ||(A - theta) y - b|| / ||b|| = %.2e"
             % (k, its["torch"], stage, agree, true_res),
             "  kernel            launches   us/launch   bytes/row   of 8 TB/s"]
    for label, _, _ in KERNELS:
        s = split[label]
        lines.append("  %-16s %9d %11.2f %11.1f %10.1f %%" % (label, s["launches"], s["us"], s["bytes_per_row"], 100 * s["hbm_fraction"]))
    lines.append("  (a solve with maxit = %d: no chunk is enqueued past the end; launches = working launches, the ones of the last iteration behind stage %d return at entry)" % (k, stage))
    lines.append("  one iteration by events: %.1f us (four products %.1f + vector work %.1f for 352 B/row); the timed solve / %d iterations by the host clock: %.1f us"
                 " (it also holds k_bs_init + k_bs_start and the %d iterations' products the last chunk of 8 runs past the end)" %
                 (per_it, per_it - vec_it, vec_it, k, out["us_per_iteration"]["bicgstab/8"], -k % 8))
    lines.append("  ms per solve, %d alternating rounds (mean +- std [min, max]):" % args.rounds)
    for key in solvers:
        s = out["ms_per_solve"][key]
        lines.append("    %-12s %9.2f +- %6.2f  [%9.2f, %9.2f]   %d iterations" % (key, s["mean"], s["std"], s["min"], s["max"], its[key]))
    lines.append("  torch recurrence / fused operator: %.2fx per solve (%.2f ms against %.2f ms)" % (torch_ms["mean"] / fused["mean"], torch_ms["mean"], fused["mean"]))
    lines.append("")
    lines.append("conjugate gradients on -Laplacian + V + %g I (symmetric positive definite) in the same job, %d iterations:" % (-CG_SHIFT, its["cg/8"]))
    mb.split_lines(cg_split, mb.CG_KERNELS, lines)
    cg_vec = cg_per_it - cg_split["product"]["us"]
    lines.append("  one CG iteration by events: %.1f us (vector work %.1f for 80 B/row); BiCGStab(2) vector work per product: %.1f us for 88 B/row (%.2fx for 1.10x the bytes)" %
                 (cg_per_it, cg_vec, vec_it / 4, vec_it / 4 / cg_vec))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
