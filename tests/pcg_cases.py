"""Operators, preconditioners and recorded iteration counts of the preconditioned conjugate-gradient tests
(tests/test_pcg_model_cpu.py, tests/test_gpu_pcg_operator.py).  Plain numpy / scipy: no device, no library; the matrices of
tests/cg_cases.py are reused by import.

  "jump"   -div(c grad) with Dirichlet boundaries on 12 x 10 x 8, unit spacing: c = 1 for x < 6 and JUMP = 100 for x >= 6, times
           exp(0.3 N(0, 1)) per cell (`jump_coeff`), assembled by extras.diffusion_terms / grid_variable_operator.  cond 3.2e3.
  "aniso"  the 7-point stencil with taps (z, y, x) = (1e-2, 1e-2, 1) (-1, 2, -1) plus a potential 0.05 U(0, 1) on 12 x 10 x 8
           (`aniso_terms`): the x links dominate, so the x-lines carry the ill-conditioning and the diagonal says nothing.

ITERATION BANDS, as in tests/bicgstab_cases.py: the device and the numpy model (tests/pcg_model.py) differ in the order of their
sums; what summation order alone does to the MODEL is measured by summing every inner product of a solve in a permuted row order
(`PERMUTATION_SEEDS`: numpy's own order and five random ones).  `SPREAD[case]` is max - min of those six counts as recorded on a
CPU; tests/test_pcg_model_cpu.py recomputes and prints every one of them and holds each permuted count to the band.  The device's
count must lie within `band(case)` = max(2 SPREAD, 1) of `MODEL_ITS[case]`, the model's count in numpy's order.  `CG_ITS[case]` is
the count of the model of plain conjugate gradients (tests/cg_model.py) on the same matrix and right-hand side: the preconditioned
count must be at most a third of it."""
import numpy as np

import cg_cases as cc

TOL = 1e-13
SHAPE = cc.GRID_SHAPE
JUMP = 100.0
PERMUTATION_SEEDS = (None, 101, 102, 103, 104, 105)


def diag3_entries(n):
    """The diagonal of cg_cases.diag3(n)."""
    return np.array([1.0, 2.0, 4.0])[np.arange(n) % 3]


def two_cluster_diagonal(n):
    """M = diag(1, 1, 1/2, ...): M diag3 has the eigenvalues 1, 2, 2 -- two distinct ones, exactly two iterations, where plain
    conjugate gradients need three and a wrong beta (or z and r mixed up) dozens."""
    return np.array([1.0, 1.0, 0.5])[np.arange(n) % 3]


def jump_coeff(shape=SHAPE, jump=JUMP, seed=29):
    """The cell-centred coefficient of "jump", flat in row order (x fastest)."""
    nx = shape[0]
    n = cc.size(shape)
    ix = np.arange(n) % nx
    noise = np.exp(0.3 * np.random.default_rng(seed + n).standard_normal(n))
    return np.where(ix < nx // 2, 1.0, float(jump)) * noise


def aniso_terms(shape=SHAPE, seed=31):
    """(taps, potential) of "aniso"."""
    ez, ey, ex = 1e-2, 1e-2, 1.0
    taps = np.array([-ez, -ey, -ex, 2.0 * (ex + ey + ez), -ex, -ey, -ez])
    return taps, 0.05 * np.random.default_rng(seed + cc.size(shape)).random(cc.size(shape))


def order(n, seed):
    """The row order in which pcg_model.solve sums its inner products: None for seed None, else a permutation."""
    return None if seed is None else np.random.default_rng(seed).permutation(n)


# the model's counts at TOL = 1e-13 with cg_cases.rhs(960, Float64) as recorded on a CPU (numpy 2.x; recomputed and printed by
# test_pcg_model_cpu.py::test_recorded_counts_and_spread)
MODEL_ITS = {"jump": 72, "aniso": 16}
PERMUTED_ITS = {"jump": (72, 72, 72, 72, 72, 72), "aniso": (16, 16, 16, 16, 16, 16)}   # measured spread: 0 and 0
CG_ITS = {"jump": 519, "aniso": 94}   # (cond 3.2e3 and 49; Jacobi on "aniso": 94, the diagonal is almost constant)
# "jump" with a jump of 1e4 in c (`jump_coeff(jump=JUMP_HARD)`, cond 3.2e5): the preconditioned count stays where plain conjugate
# gradients take almost three times as long; recomputed by test_pcg_model_cpu.py::test_a_larger_jump_moves_only_the_plain_count
JUMP_HARD = 1e4
HARD_ITS = {"pcg": 74, "cg": 1381}
SPREAD = {case: max(v) - min(v) for case, v in PERMUTED_ITS.items()}


def band(case):
    """How far the device's iteration count may lie from MODEL_ITS[case]: twice what summation order alone did to the model, at
    least 1."""
    return max(2 * SPREAD[case], 1)
