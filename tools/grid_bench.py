#!/usr/bin/env python3
"""The matrix-free grid operator (ks_operator_grid) against the stored layouts, in the solver's own access pattern:

    python tools/grid_bench.py [--sizes 216,100] [--rounds 7] [--chains 5] [--cycles 20] [--no-solve] [--periodic] [--radius R] [--variable] [--box]
                               [--complex [--wide]] [--chebyshev M]

Float64, 7-point -Laplacian (+ a harmonic potential) on m x m x m grids.  Per size, in ONE process:

  products   the chain column i -> column i + 1 over the 41 columns of a 20/40 workspace (a basis that does not fit the caches),
             `chains` chains per round, every timed region closed by a device synchronisation; the operators alternate inside
             every round, so a difference is seen against the spread of the same session (a host clock: at 100^3 it measures the
             enqueue, not the kernel -- the HIP-event time of the kernels alone is printed next to it):
               (a) grid_operator with a potential              24 n bytes
               (b) csr_operator(host_grid_matrix(...))         the same matrix stored: the only way to run it without (a)
               (c) grid_operator without a potential           16 n bytes
               (d) csr_operator of the plain Laplacian         the stencil layout (marching kernel)
             --periodic adds, on the torus (ks_operator_grid_periodic):
               (e) grid_operator(..., periodic=True) with the potential     24 n bytes, as (a)
               (f) csr_operator(host_grid_matrix(..., periodic=True))       the same matrix stored
             --radius R (2, 3, 4; ks_operator_grid_star) runs (a), (b) and (c) with the star stencil of central differences of
             order 2 R, extras.fd_laplacian_taps(3, 2 R), instead of the 7-point one: (a) and (c) still move 24 n / 16 n bytes,
             (b) streams the 6 R + 1 entries of a row.  (d) belongs to the 7-point stencil and is left out.  With --periodic as
             well (ks_operator_grid_star_periodic), on the torus:
               (a) the open star operator with the potential                                     24 n bytes
               (e) grid_star_operator(..., periodic=True) with the potential                     24 n bytes, as (a)
               (f) csr_operator(host_grid_star_matrix(..., periodic=True))                       the same matrix stored
             in the same rounds, and the solve on (e) and (f).
             --variable (ks_operator_grid_var) runs the variable-coefficient operator -div(c grad) + V, c a smooth field with a jump
             (extras.diffusion_terms, Dirichlet), in the same rounds as today's constant-coefficient operator, the floor:
               (a) grid_variable_operator with the diagonal        32 n bytes
               (b) csr_operator(host_grid_variable_matrix(...))    the same matrix stored: the only way to run it without (a)
               (c) grid_variable_operator without a diagonal       24 n bytes
               (d) grid_operator with a potential                  24 n bytes: (a) of the plain run, the constant-coefficient floor
             and the solve on (a) and (b).  With --periodic as well (ks_operator_grid_var_periodic), on the torus:
               (e) grid_variable_operator(..., periodic=True) with the diagonal of the torus     32 n bytes, as (a)
               (f) csr_operator(host_grid_variable_matrix(..., periodic=True))                   the same matrix stored
             in the same rounds, and the solve on (e) and (f) too.
             --box (ks_operator_grid_box) runs the 27-point box stencil of -div(D grad) + V with a full constant tensor D
             (extras.tensor_laplacian_taps; 19 of the 27 taps are non-zero, all 27 are stored and multiplied) in the same rounds as
             the 7-point operator, the floor:
               (a) grid_box_operator with the potential            24 n bytes
               (b) csr_operator(host_grid_box_matrix(...))         the same matrix stored: the only way to run it without (a)
               (c) grid_box_operator without a potential           16 n bytes
               (d) grid_operator with a potential                  24 n bytes: (a) of the plain run, the 7-point floor
             and the solve on (a) and (b).  With --periodic as well (ks_operator_grid_box_periodic), on the torus:
               (e) grid_box_operator(..., periodic=True) with the potential                      24 n bytes, as (a)
               (f) csr_operator(host_grid_box_matrix(..., periodic=True))                        the same matrix stored
             in the same rounds as the open box operator (a), and the solve on (e) and (f) too.
             --complex runs the grid operators of the run that the other switches select -- (a) and (c); --periodic: (e) alone
             (--radius R --periodic: (e) of the star stencil with Bloch wrap values at theta = (0.7, 1.1, 1.9));
             --variable: (a), (c), (d); --variable --periodic: (e) alone, at the k-point theta = (0.7, 1.1, 1.9) (Bloch wrap values) -- in the same rounds with ComplexF64 taps, potential and vectors (twice the bytes; c stays
             Float64): products only, no stored matrix and no solve.  --wide puts them on the m^2 x 1 x m grid, which takes the
             one-row tiles.
             The HIP-event time is taken per round as well (`event_rounds`): its mean and max - min are what two builds are
             compared by.
  solve      iterations/s of nev = 20, mindim / maxdim = 20 / 40, :SR on (a) and (b): `cycles` timed restart cycles after 3 warm-up
             cycles (what bench.py times), alternating (a) and (b) -- and (e) and (f) with --periodic -- per round.

  --chebyshev M   the Chebyshev filter (ks_operator_chebyshev) of degree M on the grid operator the other switches select: the
             Clenshaw step fused into the product against product + streaming pass, cacheable against streaming intermediate stores,
             and a filtered solve against the plain :SR solve (main_chebyshev).

Prints one JSON line per size and a short table; fractions are of the 8 TB/s HBM rate."""
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
PEAK = 8.0e12
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])
MAXDIM, MINDIM, NEV = 40, 20, 20


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), std=float(v.std(ddof=1)) if v.size > 1 else 0.0, min=float(v.min()), max=float(v.max()),
                rounds=[round(float(x), 3) for x in v])


def bench_products(ctx, ops, n, rounds, chains, dtype=np.float64):
    ws = ks.ArnoldiWorkspace(n, MAXDIM, dtype, ctx=ctx)
    ws.fill_uniform(0, 1)
    us = {name: [] for name in ops}
    for name, op in ops.items():      # warm-up: every operator over every column
        for i in range(MAXDIM):
            ws.apply(op, i, i + 1)
    ctx.synchronize()
    for _ in range(rounds):
        for name, op in ops.items():
            ws.fill_uniform(0, 1)     # (keeps the chain's values in range; untimed)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _c in range(chains):
                for i in range(MAXDIM):
                    ws.apply(op, i, i + 1)
            ctx.synchronize()
            us[name].append(1e6 * (time.perf_counter() - t0) / (chains * MAXDIM))
    out = {name: stats(v) for name, v in us.items()}
    # the kernels alone: the library's HIP-event profile (class "spmv"), in a pass of its own -- the events slow the enqueue down
    ctx.profile_enable(True)
    ev = {name: [] for name in ops}
    for _ in range(rounds):
        for name, op in ops.items():
            ctx.profile_reset()
            for _c in range(chains):
                for i in range(MAXDIM):
                    ws.apply(op, i, i + 1)
            ctx.synchronize()
            p = ctx.profile_get()["spmv"]
            ev[name].append(1e3 * p["ms"] / max(p["count"], 1))
            out[name]["event_launches_per_product"] = p["count"] / (chains * MAXDIM)
    for name, v in ev.items():
        out[name]["event_rounds"] = stats(v)
        out[name]["event_us"] = out[name]["event_rounds"]["mean"]
    ctx.profile_enable(False)
    ws.close()
    return out


class Solve:
    """bench.py's cycle: expand_restart from the basis size the previous restart left, synchronised."""

    def __init__(self, ctx, op, n):
        self.ctx, self.op = ctx, op
        self.ws = ks.ArnoldiWorkspace(n, MAXDIM, np.float64, ctx=ctx)
        self.ws.reinitialize(0, ks.matrices.start_vector(n))
        self.ws.iterate_arnoldi(op, 1, MINDIM)
        self.k, self.active, self.trail = MINDIM, 0, []

    def cycles(self, count):
        tol = float(np.sqrt(np.finfo(np.float64).eps))
        self.ctx.synchronize()
        steps, t0 = 0, time.perf_counter()
        for _ in range(count):
            r = self.ws.expand_restart(self.op, self.k, self.active, NEV, "SR", tol, MINDIM, MAXDIM)
            self.ctx.synchronize()
            steps += MAXDIM - self.k
            self.k, self.active = r["k"], r["nlock"]
            self.trail.append((self.k, self.active))
        return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="216,100")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--chains", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--periodic", action="store_true", help="add (e) the periodic grid operator and (f) its stored matrix")
    ap.add_argument("--radius", type=int, default=None, help="2, 3 or 4: (a), (b), (c) with the star stencil of order 2 R")
    ap.add_argument("--variable", action="store_true", help="the variable-coefficient operator against its stored matrix and the constant-coefficient floor")
    ap.add_argument("--box", action="store_true", help="the 27-point box operator against its stored matrix and the 7-point floor")
    ap.add_argument("--complex", action="store_true", help="the selected grid operators alone, in ComplexF64: products only")
    ap.add_argument("--wide", action="store_true", help="with --complex: the m^2 x 1 x m grid (one-row tiles)")
    ap.add_argument("--chebyshev", type=int, default=None, metavar="M", help="the Chebyshev filter of degree M on the selected grid operator: fused against generic steps, and a filtered solve")
    args = ap.parse_args()
    if args.chebyshev is not None:
        if args.complex:
            raise SystemExit("--chebyshev takes no --complex")
        main_chebyshev(args)
        return
    if args.complex:
        main_complex(args)
        return
    if args.wide:
        raise SystemExit("--wide belongs to --complex")
    if args.box:
        main_box(args)
        return
    if args.variable:
        main_variable(args)
        return
    if args.radius is not None:
        main_star(args)
        return
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = (m, m, m), m ** 3
        V = ks.matrices.harmonic_potential(shape)
        t0 = time.perf_counter()
        A = ks.host_grid_matrix(shape, LAPLACE, V)
        ip, ix, dv = ks.matrices.laplace3d_csr(m, m, m)
        ops = {
            "a_grid_potential": ks.grid_operator(shape, LAPLACE, V, ctx=ctx),
            "b_stored_potential": ks.csr_operator(A, ctx),
            "c_grid_plain": ks.grid_operator(shape, LAPLACE, ctx=ctx),
            "d_stored_laplacian": ks.csr_operator(ks.matrices.to_scipy(ip, ix, dv, n), ctx),
        }
        nnz = {"b_stored_potential": A.nnz, "d_stored_laplacian": A.nnz}
        if args.periodic:
            Ap = ks.host_grid_matrix(shape, LAPLACE, V, periodic=True)
            ops["e_grid_periodic"] = ks.grid_operator(shape, LAPLACE, V, ctx=ctx, periodic=True)
            ops["f_stored_periodic"] = ks.csr_operator(Ap, ctx)
            nnz["f_stored_periodic"] = Ap.nnz
            del Ap
        setup_s = time.perf_counter() - t0
        del A, ip, ix, dv
        fmt = {k: ops[k].format for k in nnz}
        by = {"a_grid_potential": 24.0 * n, "c_grid_plain": 16.0 * n, "e_grid_periodic": 24.0 * n}
        by.update({k: fmt[k]["bytes_per_nnz"] * nnz[k] + 16.0 * n for k in nnz})
        nnz = nnz["b_stored_potential"]
        out = dict(m=m, n=n, nnz=nnz, setup_seconds=round(setup_s, 2), formats=fmt, chains=args.chains, products_per_round=args.chains * MAXDIM)
        prod = bench_products(ctx, ops, n, args.rounds, args.chains)
        for name, s in prod.items():
            s["bytes_per_product"] = by[name]
            s["hbm_fraction_at_mean"] = by[name] / (s["mean"] * 1e-6) / PEAK
            s["hbm_fraction_of_kernels"] = by[name] / (s["event_us"] * 1e-6) / PEAK
        out["us_per_product"] = prod
        if not args.no_solve:
            names = ("a_grid_potential", "b_stored_potential") + (("e_grid_periodic", "f_stored_periodic") if args.periodic else ())
            runs = {name: Solve(ctx, ops[name], n) for name in names}
            for s in runs.values():
                s.cycles(3)
            rate = {name: [] for name in runs}
            for _ in range(max(3, args.rounds // 2)):
                for name, s in runs.items():
                    rate[name].append(s.cycles(args.cycles))
            out["iterations_per_s"] = {name: stats(v) for name, v in rate.items()}
            out["same_restart_trail"] = runs["a_grid_potential"].trail == runs["b_stored_potential"].trail
            if args.periodic:
                out["same_restart_trail_periodic"] = runs["e_grid_periodic"].trail == runs["f_stored_periodic"].trail
            out["blocks"] = {name: s.ws.sstep_info["blocks"] for name, s in runs.items()}
            for s in runs.values():
                s.ws.close()
        report(out, prod, m, n, args)
        for op in ops.values():
            op.close()


def report(out, prod, m, n, args):
    print(json.dumps(out), flush=True)
    print("m = %d (n = %d): us per product, mean +- std [min, max] over %d rounds of %d products; fraction of 8 TB/s" % (m, n, args.rounds, args.chains * MAXDIM))
    for name, s in prod.items():
        e = s["event_rounds"]
        print("  %-20s %8.2f +- %5.2f  [%7.2f, %7.2f]   %5.1f B/row  %5.1f %%   kernels alone (HIP events) %7.2f us  [%7.2f, %7.2f]  %5.1f %%" % (
            name, s["mean"], s["std"], s["min"], s["max"], s["bytes_per_product"] / n, 100 * s["hbm_fraction_at_mean"], e["mean"], e["min"], e["max"],
            100 * s["hbm_fraction_of_kernels"]))
    if not args.no_solve:
        for name, s in out["iterations_per_s"].items():
            print("  %-20s %8.0f +- %5.0f iterations/s  [%7.0f, %7.0f]" % (name, s["mean"], s["std"], s["min"], s["max"]))
    sys.stdout.flush()


def main_star(args):
    """--radius R: (a), (b), (c) with the star stencil of central differences of order 2 R; with --periodic (a), the operator on
    the torus (e) and its stored matrix (f), and the solve on (e) and (f)."""
    from arnoldimethod_jl_amd import extras

    R = args.radius
    if R not in (2, 3, 4):
        raise SystemExit("--radius takes 2, 3 or 4")
    taps = extras.fd_laplacian_taps(3, 2 * R)
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = (m, m, m), m ** 3
        V = ks.matrices.harmonic_potential(shape)
        t0 = time.perf_counter()
        if args.periodic:
            A = ks.host_grid_star_matrix(shape, taps, R, V, periodic=True)
            stored, solve = "f_stored_star_periodic", ("e_star_periodic", "f_stored_star_periodic")
            ops = {
                "a_grid_potential": ks.grid_operator(shape, taps, V, ctx=ctx, radius=R),
                "e_star_periodic": ks.grid_star_operator(shape, taps, R, V, ctx=ctx, periodic=True),
                stored: ks.csr_operator(A, ctx),
            }
        else:
            A = ks.host_grid_matrix(shape, taps, V, radius=R)
            stored, solve = "b_stored_potential", ("a_grid_potential", "b_stored_potential")
            ops = {
                "a_grid_potential": ks.grid_operator(shape, taps, V, ctx=ctx, radius=R),
                stored: ks.csr_operator(A, ctx),
                "c_grid_plain": ks.grid_operator(shape, taps, ctx=ctx, radius=R),
            }
        nnz = A.nnz
        setup_s = time.perf_counter() - t0
        del A
        fmt = {stored: ops[stored].format}
        by = {"a_grid_potential": 24.0 * n, "c_grid_plain": 16.0 * n, "e_star_periodic": 24.0 * n, stored: fmt[stored]["bytes_per_nnz"] * nnz + 16.0 * n}
        out = dict(m=m, n=n, radius=R, periodic=args.periodic, nnz=nnz, setup_seconds=round(setup_s, 2), formats=fmt, chains=args.chains, products_per_round=args.chains * MAXDIM)
        prod = bench_products(ctx, ops, n, args.rounds, args.chains)
        for name, s in prod.items():
            s["bytes_per_product"] = by[name]
            s["hbm_fraction_at_mean"] = by[name] / (s["mean"] * 1e-6) / PEAK
            s["hbm_fraction_of_kernels"] = by[name] / (s["event_us"] * 1e-6) / PEAK
        out["us_per_product"] = prod
        if not args.no_solve:
            runs = {name: Solve(ctx, ops[name], n) for name in solve}
            for s in runs.values():
                s.cycles(3)
            rate = {name: [] for name in runs}
            for _ in range(max(3, args.rounds // 2)):
                for name, s in runs.items():
                    rate[name].append(s.cycles(args.cycles))
            out["iterations_per_s"] = {name: stats(v) for name, v in rate.items()}
            out["same_restart_trail"] = runs[solve[0]].trail == runs[solve[1]].trail
            out["blocks"] = {name: s.ws.sstep_info["blocks"] for name, s in runs.items()}
            for s in runs.values():
                s.ws.close()
        report(out, prod, m, n, args)
        for op in ops.values():
            op.close()


def jump_coefficient(shape):
    """1 + 0.5 sin(0.7 x + 0.3 y) cos(0.5 z) + 1.5 [x > nx // 2] on the point indices, flat in row order: smooth, with a jump."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij", sparse=True)
    return (1.0 + 0.5 * np.sin(0.7 * x + 0.3 * y) * np.cos(0.5 * z) + 1.5 * (x > nx // 2)).ravel()


def main_variable(args):
    """--variable: the variable-coefficient operator with (a) and without (c) its diagonal, its stored matrix (b), and the
    constant-coefficient operator with a potential (d) as the floor, in the same rounds; the solve on (a) and (b)."""
    from arnoldimethod_jl_amd import extras

    if args.radius is not None:
        raise SystemExit("--variable takes no --radius")
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = (m, m, m), m ** 3
        V = ks.matrices.harmonic_potential(shape)
        c = jump_coefficient(shape)
        t0 = time.perf_counter()
        taps, diag = extras.diffusion_terms(shape, c, potential=V)
        A = ks.host_grid_variable_matrix(shape, taps, c, diag)
        ops = {
            "a_var_diagonal": ks.grid_variable_operator(shape, taps, c, diag, ctx=ctx),
            "b_stored_variable": ks.csr_operator(A, ctx),
            "c_var_plain": ks.grid_variable_operator(shape, LAPLACE, c, ctx=ctx),
            "d_grid_potential": ks.grid_operator(shape, LAPLACE, V, ctx=ctx),
        }
        nnz = A.nnz
        stored = {"b_stored_variable": nnz}
        if args.periodic:
            tp, dp = extras.diffusion_terms(shape, c, potential=V, periodic=True)
            Ap = ks.host_grid_variable_matrix(shape, tp, c, dp, periodic=True)
            ops["e_var_periodic"] = ks.grid_variable_operator(shape, tp, c, dp, ctx=ctx, periodic=True)
            ops["f_stored_var_periodic"] = ks.csr_operator(Ap, ctx)
            stored["f_stored_var_periodic"] = Ap.nnz
            del Ap
        setup_s = time.perf_counter() - t0
        del A
        fmt = {k: ops[k].format for k in stored}
        by = {"a_var_diagonal": 32.0 * n, "c_var_plain": 24.0 * n, "d_grid_potential": 24.0 * n, "e_var_periodic": 32.0 * n}
        by.update({k: fmt[k]["bytes_per_nnz"] * stored[k] + 16.0 * n for k in stored})
        out = dict(m=m, n=n, variable=True, nnz=nnz, setup_seconds=round(setup_s, 2), formats=fmt, chains=args.chains, products_per_round=args.chains * MAXDIM)
        prod = bench_products(ctx, ops, n, args.rounds, args.chains)
        for name, s in prod.items():
            s["bytes_per_product"] = by[name]
            s["hbm_fraction_at_mean"] = by[name] / (s["mean"] * 1e-6) / PEAK
            s["hbm_fraction_of_kernels"] = by[name] / (s["event_us"] * 1e-6) / PEAK
        out["us_per_product"] = prod
        if not args.no_solve:
            names = ("a_var_diagonal", "b_stored_variable") + (("e_var_periodic", "f_stored_var_periodic") if args.periodic else ())
            runs = {name: Solve(ctx, ops[name], n) for name in names}
            for s in runs.values():
                s.cycles(3)
            rate = {name: [] for name in runs}
            for _ in range(max(3, args.rounds // 2)):
                for name, s in runs.items():
                    rate[name].append(s.cycles(args.cycles))
            out["iterations_per_s"] = {name: stats(v) for name, v in rate.items()}
            out["same_restart_trail"] = runs["a_var_diagonal"].trail == runs["b_stored_variable"].trail
            if args.periodic:
                out["same_restart_trail_periodic"] = runs["e_var_periodic"].trail == runs["f_stored_var_periodic"].trail
            out["blocks"] = {name: s.ws.sstep_info["blocks"] for name, s in runs.items()}
            for s in runs.values():
                s.ws.close()
        report(out, prod, m, n, args)
        for op in ops.values():
            op.close()


TENSOR = np.array([[1.0, 0.3, 0.2], [0.3, 1.5, 0.25], [0.2, 0.25, 2.0]])


def main_box(args):
    """--box: the 27-point box operator of -div(D grad) + V with (a) and without (c) the potential, its stored matrix (b), and the
    7-point operator with a potential (d) as the floor, in the same rounds; the solve on (a) and (b).  --periodic adds the operator
    on the torus (e) and its stored matrix (f) to the rounds and to the solves."""
    from arnoldimethod_jl_amd import extras

    if args.radius is not None or args.variable or args.complex:
        raise SystemExit("--box takes no --radius, --variable or --complex")
    taps = extras.tensor_laplacian_taps(TENSOR)
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = (m, m, m), m ** 3
        V = ks.matrices.harmonic_potential(shape)
        t0 = time.perf_counter()
        A = ks.host_grid_box_matrix(shape, taps, V)
        ops = {
            "a_box_potential": ks.grid_box_operator(shape, taps, V, ctx=ctx),
            "b_stored_box": ks.csr_operator(A, ctx),
            "c_box_plain": ks.grid_box_operator(shape, taps, ctx=ctx),
            "d_grid_potential": ks.grid_operator(shape, LAPLACE, V, ctx=ctx),
        }
        nnz = A.nnz
        stored = {"b_stored_box": nnz}
        if args.periodic:
            Ap = ks.host_grid_box_matrix(shape, taps, V, periodic=True)
            ops["e_box_periodic"] = ks.grid_box_operator(shape, taps, V, ctx=ctx, periodic=True)
            ops["f_stored_box_periodic"] = ks.csr_operator(Ap, ctx)
            stored["f_stored_box_periodic"] = Ap.nnz
            del Ap
        setup_s = time.perf_counter() - t0
        del A
        fmt = {k: ops[k].format for k in stored}
        by = {"a_box_potential": 24.0 * n, "c_box_plain": 16.0 * n, "d_grid_potential": 24.0 * n, "e_box_periodic": 24.0 * n}
        by.update({k: fmt[k]["bytes_per_nnz"] * stored[k] + 16.0 * n for k in stored})
        out = dict(m=m, n=n, box=True, nnz=nnz, setup_seconds=round(setup_s, 2), formats=fmt, chains=args.chains, products_per_round=args.chains * MAXDIM)
        prod = bench_products(ctx, ops, n, args.rounds, args.chains)
        for name, s in prod.items():
            s["bytes_per_product"] = by[name]
            s["hbm_fraction_at_mean"] = by[name] / (s["mean"] * 1e-6) / PEAK
            s["hbm_fraction_of_kernels"] = by[name] / (s["event_us"] * 1e-6) / PEAK
        out["us_per_product"] = prod
        if not args.no_solve:
            names = ("a_box_potential", "b_stored_box") + (("e_box_periodic", "f_stored_box_periodic") if args.periodic else ())
            runs = {name: Solve(ctx, ops[name], n) for name in names}
            for s in runs.values():
                s.cycles(3)
            rate = {name: [] for name in runs}
            for _ in range(max(3, args.rounds // 2)):
                for name, s in runs.items():
                    rate[name].append(s.cycles(args.cycles))
            out["iterations_per_s"] = {name: stats(v) for name, v in rate.items()}
            out["same_restart_trail"] = runs["a_box_potential"].trail == runs["b_stored_box"].trail
            if args.periodic:
                out["same_restart_trail_periodic"] = runs["e_box_periodic"].trail == runs["f_stored_box_periodic"].trail
            out["blocks"] = {name: s.ws.sstep_info["blocks"] for name, s in runs.items()}
            for s in runs.values():
                s.ws.close()
        report(out, prod, m, n, args)
        for op in ops.values():
            op.close()


def main_complex(args):
    """--complex: the grid operators of the selected run alone, every tap and the potential times 1 + 0.25i."""
    from arnoldimethod_jl_amd import extras

    R = 1 if args.radius is None else args.radius
    if R not in (1, 2, 3, 4) or (R > 1 and args.variable):
        raise SystemExit("--complex takes one of --periodic, --radius 2 / 3 / 4 (or --radius R --periodic) and --variable (or --variable --periodic)")
    phase = 1.0 + 0.25j
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = ((m * m, 1, m) if args.wide else (m, m, m)), m ** 3
        V = phase * ks.matrices.harmonic_potential(shape)
        t0 = time.perf_counter()
        if args.variable and args.periodic:      # a Bloch operator, theta != 0: Hermitian, every wrap value complex
            c = jump_coefficient(shape)
            per = tuple(e >= 3 for e in shape)
            taps, diag = extras.diffusion_terms(shape, c, potential=V.real, periodic=per)
            ops = {"e_var_periodic": ks.grid_variable_operator(shape, taps, c, diag, ctx=ctx, periodic=per,
                                                               wrap=extras.bloch_wrap(taps, (0.7, 1.1, 1.9)))}
            by = {"e_var_periodic": 56.0 * n}
        elif args.variable:
            c = jump_coefficient(shape)
            taps, diag = extras.diffusion_terms(shape, c, potential=V.real)
            ops = {
                "a_var_diagonal": ks.grid_variable_operator(shape, phase * taps, c, phase * diag, ctx=ctx),
                "c_var_plain": ks.grid_variable_operator(shape, phase * LAPLACE, c, ctx=ctx),
                "d_grid_potential": ks.grid_operator(shape, phase * LAPLACE, V, ctx=ctx),
            }
            by = {"a_var_diagonal": 56.0 * n, "c_var_plain": 40.0 * n, "d_grid_potential": 48.0 * n}
        elif args.periodic and R > 1:            # the star stencil at a k-point: Hermitian, every wrap value complex
            taps = extras.fd_laplacian_taps(3, 2 * R)
            per = tuple(e >= 2 * R + 1 for e in shape)
            ops = {"e_star_periodic": ks.grid_star_operator(shape, taps, R, V.real, ctx=ctx, periodic=per,
                                                            wrap=extras.bloch_wrap(taps, (0.7, 1.1, 1.9), radius=R))}
            by = {"e_star_periodic": 48.0 * n}
        elif args.periodic:
            ops = {"e_grid_periodic": ks.grid_operator(shape, phase * LAPLACE, V, ctx=ctx, periodic=tuple(e >= 3 for e in shape))}
            by = {"e_grid_periodic": 48.0 * n}
        else:
            taps = phase * (LAPLACE if R == 1 else extras.fd_laplacian_taps(3, 2 * R))
            ops = {
                "a_grid_potential": ks.grid_operator(shape, taps, V, ctx=ctx, radius=R),
                "c_grid_plain": ks.grid_operator(shape, taps, ctx=ctx, radius=R),
            }
            by = {"a_grid_potential": 48.0 * n, "c_grid_plain": 32.0 * n}
        setup_s = time.perf_counter() - t0
        out = dict(m=m, n=n, shape=list(shape), dtype="complex128", radius=R, variable=args.variable, periodic=args.periodic,
                   setup_seconds=round(setup_s, 2), chains=args.chains, products_per_round=args.chains * MAXDIM)
        prod = bench_products(ctx, ops, n, args.rounds, args.chains, np.complex128)
        for name, s in prod.items():
            s["bytes_per_product"] = by[name]
            s["hbm_fraction_at_mean"] = by[name] / (s["mean"] * 1e-6) / PEAK
            s["hbm_fraction_of_kernels"] = by[name] / (s["event_us"] * 1e-6) / PEAK
        out["us_per_product"] = prod
        args.no_solve = True
        report(out, prod, m, n, args)
        for op in ops.values():
            op.close()


CHEB_VARIANTS = {   # name -> environment of the run (read per step / per product by the library)
    "fused": {"KS_CHEB_FUSED": "1"},                               # the step in the product's launch, intermediates cacheable
    "generic": {"KS_CHEB_FUSED": "0"},                             # product + streaming pass
    "fused_streaming": {"KS_CHEB_FUSED": "1", "KS_CHEB_PLAIN": "0"},   # ... with streaming stores for the intermediate steps
    "generic_streaming": {"KS_CHEB_FUSED": "0", "KS_CHEB_PLAIN": "0"},
}


def _cheb_env(env):
    for k in ("KS_CHEB_FUSED", "KS_CHEB_PLAIN"):
        os.environ.pop(k, None)
    os.environ.update(env)


def _cheb_family(args, shape, V, ctx):
    """(name, operator with the potential, safe spectrum bounds) of the family the switches select."""
    from arnoldimethod_jl_amd import extras

    if args.box:
        taps = extras.tensor_laplacian_taps(TENSOR)
        s = float(np.abs(taps).sum() - abs(taps[taps.size // 2]))
        return "box", ks.grid_box_operator(shape, taps, V, ctx=ctx, periodic=args.periodic or None), (taps[taps.size // 2] + V.min() - s, taps[taps.size // 2] + V.max() + s)
    if args.variable:
        c = jump_coefficient(shape)
        taps, diag = extras.diffusion_terms(shape, c, potential=V, periodic=True if args.periodic else None)
        B = float(np.abs(diag).max() + 2.0 * c.max() * (np.abs(taps).sum() - abs(taps[3])))   # a crude Gershgorin radius: timing only
        return "variable", ks.grid_variable_operator(shape, taps, c, diag, ctx=ctx, periodic=True if args.periodic else None), (-B, B)
    R = 1 if args.radius is None else args.radius
    taps = LAPLACE if R == 1 else extras.fd_laplacian_taps(3, 2 * R)
    if args.periodic:
        op = ks.grid_star_operator(shape, taps, R, V, ctx=ctx, periodic=True)
    else:
        op = ks.grid_operator(shape, taps, V, ctx=ctx, radius=R)
    return ("7-point" if R == 1 else "star%d" % R), op, extras.grid_spectrum_bounds(taps, V, radius=R)


def main_chebyshev(args):
    """--chebyshev M: the Chebyshev filter of degree M (ks_operator_chebyshev) on the grid operator the other switches select
    (--radius R, --variable, --box, each with --periodic; with the potential), per size in ONE process:

      steps    the filter applied column i -> i + 1 over four columns, `chains` chains per round, the variants of CHEB_VARIANTS and
               the plain product of the same operator alternating inside every round: host clock per STEP (one product and what
               the variant adds), and in a pass of its own the HIP-event time of the kernels alone (classes spmv + scale);
      solve    nev = 20, 20 / 40, tol = sqrt(eps), at most 200 restarts: the plain :SR solve of the operator against which = LR on
               the damping polynomial of degree M that is 1 at the lower spectrum bound and damps everything above the wanted
               eigenvalues (the cut is taken from the plain solve's own result), fused and generic: restarts, products of A,
               seconds, converged pairs, and the residuals ||A x - theta x|| of the filtered solve's vectors (on the device)."""
    from arnoldimethod_jl_amd import extras

    M = args.chebyshev
    ctx = ks.Context(0)
    for m in (int(s) for s in args.sizes.split(",")):
        shape, n = (m, m, m), m ** 3
        V = ks.matrices.harmonic_potential(shape)
        family, A, bounds = _cheb_family(args, shape, V, ctx)
        a, b = bounds
        F = ks.chebyshev_operator(A, *extras.chebyshev_window(a + 0.05 * (b - a), a + 0.10 * (b - a), bounds, M))
        ws = ks.ArnoldiWorkspace(n, 4, np.float64, ctx=ctx)
        names = list(CHEB_VARIANTS) + ["plain_product"]

        def run(name):
            _cheb_env(CHEB_VARIANTS.get(name, {}))
            for _c in range(args.chains):
                for i in range(4):
                    ws.apply(A if name == "plain_product" else F, i, i + 1)
            return args.chains * 4 * (1 if name == "plain_product" else M)

        ws.fill_uniform(0, 1)
        for name in names:
            run(name)
        ctx.synchronize()
        us = {name: [] for name in names}
        for _ in range(args.rounds):
            for name in names:
                ws.fill_uniform(0, 1)
                ctx.synchronize()
                t0 = time.perf_counter()
                steps = run(name)
                ctx.synchronize()
                us[name].append(1e6 * (time.perf_counter() - t0) / steps)
        ctx.profile_enable(True)
        ev = {name: [] for name in names}
        for _ in range(args.rounds):
            for name in names:
                ws.fill_uniform(0, 1)
                ctx.synchronize()
                ctx.profile_reset()
                steps = run(name)
                ctx.synchronize()
                p = ctx.profile_get()
                ev[name].append(1e3 * (p["spmv"]["ms"] + p["scale"]["ms"]) / steps)
        ctx.profile_enable(False)
        _cheb_env({})
        elem = 8.0
        by = {"fused": 5 * elem, "fused_streaming": 5 * elem, "generic": 8 * elem, "generic_streaming": 8 * elem, "plain_product": 3 * elem}
        if args.variable:
            by = {k: v + elem for k, v in by.items()}
        out = dict(m=m, n=n, family=family, periodic=args.periodic, degree=M, chains=args.chains, steps_per_round=args.chains * 4 * M,
                   info=F.chebyshev_info, us_per_step={k: stats(v) for k, v in us.items()}, event_us_per_step={k: stats(v) for k, v in ev.items()},
                   bytes_per_row=by)
        if not args.no_solve:
            tol = float(np.sqrt(np.finfo(np.float64).eps))
            v1 = ks.matrices.start_vector(n)
            solves = {}
            t0 = time.perf_counter()
            dec, hist = ks.partialschur(A, v1=v1, nev=NEV, which="SR", tol=tol, mindim=MINDIM, maxdim=MAXDIM, ctx=ctx)
            ctx.synchronize()
            solves["plain_SR"] = dict(seconds=time.perf_counter() - t0, restarts=hist.restarts, products_of_A=hist.mvproducts, nconverged=hist.nconverged,
                                      converged=hist.converged)
            low = np.sort(dec.eigenvalues.real)
            cut = low[-1] + 0.5 * (low[-1] - low[0]) if low.size > 1 else a + 0.05 * (b - a)
            c, e, g = extras.chebyshev_damping((cut, b), below=a, degree=M)
            Fd = ks.chebyshev_operator(A, c, e, g)
            for name in ("fused", "generic"):
                _cheb_env(CHEB_VARIANTS[name])
                t0 = time.perf_counter()
                dec_f, hist_f = ks.partialschur(Fd, v1=v1, nev=NEV, which="LR", tol=tol, mindim=MINDIM, maxdim=MAXDIM, ctx=ctx)
                ctx.synchronize()
                sec = time.perf_counter() - t0
                rec = dict(seconds=sec, restarts=hist_f.restarts, products_of_A=hist_f.mvproducts * M, nconverged=hist_f.nconverged, converged=hist_f.converged, cut=float(cut))
                if dec_f.nconverged:
                    X = ks.schur_vectors(dec_f)
                    theta = np.real(np.diag(ks.gram(X, X.apply(A))))
                    r, _qn = ks.residuals(A, X, theta)
                    rec.update(theta_min=float(theta.min()), theta_max=float(theta.max()), max_residual=float(r.max()),
                               lowest_of_plain=float(low[0]) if low.size else None)
                    X.close()
                solves[name] = rec
            _cheb_env({})
            Fd.close()
            out["solve"] = solves
        print(json.dumps(out), flush=True)
        print("m = %d (n = %d), %s%s, degree %d: us per Clenshaw step, mean +- std [min, max] over %d rounds of %d steps; B/row; fraction of 8 TB/s" % (
            m, n, family, " periodic" if args.periodic else "", M, args.rounds, args.chains * 4 * M))
        for name in names:
            s, e_ = out["us_per_step"][name], out["event_us_per_step"][name]
            print("  %-18s %8.2f +- %5.2f  [%7.2f, %7.2f]   %4.0f B/row  %5.1f %%   kernels alone (HIP events) %7.2f us  [%7.2f, %7.2f]  %5.1f %%" % (
                name, s["mean"], s["std"], s["min"], s["max"], by[name], 100 * by[name] * n / (s["mean"] * 1e-6) / PEAK, e_["mean"], e_["min"], e_["max"],
                100 * by[name] * n / (e_["mean"] * 1e-6) / PEAK))
        for name, rec in out.get("solve", {}).items():
            print("  solve %-10s %s" % (name, rec))
        sys.stdout.flush()
        ws.close()
        F.close()
        A.close()


if __name__ == "__main__":
    main()
