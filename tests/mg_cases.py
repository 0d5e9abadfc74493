"""Grids, hierarchies and recorded figures of the multigrid tests (tests/test_mg_model_cpu.py, tests/test_gpu_multigrid_operator.py).
The operator is "jump" of tests/pcg_cases.py, -div(c grad) with Dirichlet boundaries and a jump of 100 in c, on the grids below;
the hierarchy is `extras.multigrid_hierarchy`'s, the level matrices are `host_grid_variable_matrix`'s, the coarsest level is the
symmetrised dense inverse -- what `extras.grid_multigrid_preconditioner` puts on the device.

CASES: each grid is the smallest at which its kernel can still go wrong.
  "three-level"  12 x 10 x 8, coarsest_rows = 64: 960 -> 120 -> 18 rows
  "two-level"    12 x 10 x 8: 960 -> 120
  "odd"          13 x 11 x 7: odd extents, single-cell tails on every axis
  "long-x"       129 x 3 x 2: more than two waves along x, fine lines that start at odd elements (unaligned pairs), a z axis that
                 ends at extent 1
  "2d", "1d"     16 x 12 and 37 (three levels: 37 -> 19 -> 10): unused axes stay 1
  "flat-y"       6 x 1 x 4: an extent-1 axis in the middle that is never halved
  "wide"         40 x 18 x 6, coarsest_rows = 128: 4 320 -> 540 -> 100 rows: a whole cycle whose transfers take more than one workgroup
                 of 256 threads (restrictions: 3 with a last one of 28 threads, and 1; prolongations: 9 and 2)

TRANSFER_PAIRS: the (fine, coarse) pairs on which the transfers are held bit for bit, on the host against the definition
(tests/test_mg_model_cpu.py) and on the device against the host (tests/test_gpu_multigrid_operator.py): the first two levels of every
case, and for each branch of k_mg_restrict / k_mg_prolong_add (csrc/ks_mg.hpp) the smallest pair that reaches it -- see the comments
in the list.  test_mg_model_cpu.py::test_transfer_pairs_meet_the_coverage_condition computes from the shapes alone that they do.

ITERATION BAND, as in tests/pcg_cases.py: `MODEL_ITS[case]` is the count of tests/pcg_model.py with the numpy cycle (tests/mg_model.py)
as M at TOL with cg_cases.rhs, `PERMUTED_ITS` the counts with every inner product summed in a permuted row order, `SPREAD` their
max - min; the device's count must lie within max(2 SPREAD, 1) of the model's.  tests/test_mg_model_cpu.py recomputes and prints all
of them.

ERR[case]: the relative max-norm difference between the Float64 model's M b and the same model evaluated in np.longdouble (x86
extended precision), b = cg_cases.rhs: the reference's own rounding error.  The device is allowed 4 ERR against the np.longdouble
result: the factor covers the fused multiply-adds of its smoother and the summation order of its products.  Recorded on a CPU with
numpy 2.x; tests/test_mg_model_cpu.py recomputes and prints them and holds each recomputed value to within a factor of two of the
recorded one (the dense product of the coarsest level is summed in the order of the BLAS at hand)."""
import numpy as np

import cg_cases as cc
import mg_model
import pcg_cases as pc

TOL = pc.TOL
JUMP, JUMP_HARD = pc.JUMP, pc.JUMP_HARD
DEGREE, RATIO = 2, 4.0
CASES = {   # case -> (shape, coarsest_rows)
    "three-level": ((12, 10, 8), 64),
    "two-level": ((12, 10, 8), 512),
    "odd": ((13, 11, 7), 512),
    "long-x": ((129, 3, 2), 512),
    "2d": ((16, 12), 64),
    "1d": ((37,), 16),
    "flat-y": ((6, 1, 4), 8),
    "wide": ((40, 18, 6), 128),
}
LEVEL_SHAPES = {
    "three-level": [(12, 10, 8), (6, 5, 4), (3, 3, 2)],
    "two-level": [(12, 10, 8), (6, 5, 4)],
    "odd": [(13, 11, 7), (7, 6, 4)],
    "long-x": [(129, 3, 2), (65, 2, 1)],
    "2d": [(16, 12), (8, 6)],
    "1d": [(37,), (19,), (10,)],
    "flat-y": [(6, 1, 4), (3, 1, 2)],
    "wide": [(40, 18, 6), (20, 9, 3), (10, 5, 2)],
}
KBLOCK = 256   # threads per workgroup of the transfer kernels: one per coarse cell (restriction), one per coarse x-cell of a fine line
# the first two levels of every case (under the case's name: "wide" is (40, 18, 6) -> (20, 9, 3), 540 coarse rows: 3 restriction
# workgroups, the last one of 28 threads, and 9 prolongation workgroups), then one pair per branch
_BRANCH_PAIRS = [
    ((45, 19, 7), (23, 10, 4)),     # 920 coarse rows; odd tails on all axes; fine lines that start at odd elements, across workgroups
    ((70001,), (35001,)),           # 137 workgroups in 1-D, an odd tail
    ((4096,), (2048,)),             # 8 full workgroups, aligned pairs only
    ((12, 10, 8), (12, 5, 4)),      # x kept with extent > 1: the scalar-load branch of both kernels, `two` false on every thread
    ((12, 10, 8), (6, 10, 4)),      # y kept
    ((12, 10, 8), (6, 5, 8)),       # z kept
    ((13, 6, 5), (13, 3, 5)),       # one halved axis only (s = 1/2); x kept and odd
    ((5, 4), (5, 2)),
    ((2, 9, 5), (1, 5, 3)),         # nxc = 1 from a halved x
    ((1, 64, 3), (1, 32, 2)),       # x of extent 1 next to halved y and z
    ((31, 12, 7), (16, 6, 4)),      # mixed parity
    ((6, 5, 4), (3, 3, 2)),         # the second-level pairs of "three-level" and "1d"
    ((19,), (10,)),
]
TRANSFER_PAIRS = [(s[0], s[1]) for s in LEVEL_SHAPES.values()] + _BRANCH_PAIRS
TRANSFER_IDS = list(LEVEL_SHAPES) + ["x".join(map(str, f)) + "-" + "x".join(map(str, c)) for f, c in _BRANCH_PAIRS]
PERMUTATION_SEEDS = pc.PERMUTATION_SEEDS

# recorded on a CPU (numpy 2.x); recomputed and printed by tests/test_mg_model_cpu.py
# (Jacobi: pcg_cases.MODEL_ITS["jump"] = 72 on 12 x 10 x 8; on the grid of "wide" the model of Jacobi takes 99, and 91 at shift = -1)
MODEL_ITS = {"two-level": 16, "three-level": 16, "wide": 19}
PERMUTED_ITS = {"two-level": (16,) * 6, "three-level": (16,) * 6, "wide": (19,) * 6}   # measured spread: 0, 0 and 0
HARD_ITS = {"two-level": 16, "three-level": 17, "wide": 20}           # the same with a jump of 1e4 in c
SHIFTED_ITS = {"two-level": 14, "three-level": 15, "wide": 16}        # shift = -1
SPREAD = {case: max(v) - min(v) for case, v in PERMUTED_ITS.items()}
# the larger of the Float64 and the ComplexF64 figure
ERR = {"three-level": 2.43e-16, "two-level": 2.39e-16, "odd": 2.61e-16, "long-x": 2.38e-16, "2d": 1.72e-16, "1d": 1.88e-16, "flat-y": 1.63e-16,
       "wide": 2.53e-16}


def band(case):
    return max(2 * SPREAD[case], 1)


def setup(pkg, extras, case, jump=JUMP, shift=0.0):
    """(hierarchy, level matrices, coarse): the levels of `case` from extras.multigrid_hierarchy, their host matrices (all levels),
    and the symmetrised dense inverse of the last one minus the shift."""
    shape, rows = CASES[case]
    H = extras.multigrid_hierarchy(shape, pc.jump_coeff(shape, jump), shift=shift, coarsest_rows=rows)
    mats = [pkg.host_grid_variable_matrix(L["shape"], L["taps"], L["coeff"], L["diagonal"]) for L in H]
    last = mats[-1].toarray().real
    inv = np.linalg.inv(last - float(shift) * np.eye(last.shape[0]))
    return H, mats, 0.5 * (inv + inv.T)


def model(H, mats, coarse, shift=0.0, degree=DEGREE, ratio=RATIO, real=np.float64):
    return mg_model.Cycle(mats[:-1], [L["shape"] for L in H], [L["inverse_diagonal"] for L in H[:-1]], [L["bound"] for L in H[:-1]], coarse,
                          shift=shift, degree=degree, ratio=ratio, real=real)


def rel_err(got, want):
    """The relative max-norm difference, evaluated in the precision of `want`."""
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got).astype(want.dtype) - want)) / np.max(np.abs(want)))


def rhs(case, dtype):
    return cc.rhs(cc.size(CASES[case][0]), dtype)
