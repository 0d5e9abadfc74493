"""Matrices, shifts and recorded figures of the MINRES tests (tests/test_minres_model_cpu.py, tests/test_gpu_minres_operator.py).
Plain numpy / scipy: no device, no library.  Every matrix is Hermitian; most are indefinite after their shift.

ITERATION BANDS.  The device and the numpy model (tests/minres_model.py) differ in the order of their sums only, but an indefinite
MINRES solve of several hundred iterations is sensitive to that: the Lanczos vectors lose orthogonality along the way and the
count moves by per cents, not by one.  What summation order alone does to the MODEL is measured by solving each case under
symmetric row permutations (`PERMUTATION_SEEDS`: the identity and five random ones) -- the same problem, the same right-hand side,
other sums.  `SPREAD[case]` is max - min of those six counts as recorded on a CPU (6 at shift 1.2: 4 %; 8 at shift 3.0: 1 %);
tests/test_minres_model_cpu.py recomputes and prints every one of them and holds each permuted count to the band (not to the
recorded figure itself: numpy's and the BLAS's sums depend on the CPU's vector width).  The device's count must lie within
`band(case)` = max(2 SPREAD, 2) of `MODEL_ITS`, the model's count in the natural ordering."""
import numpy as np
import scipy.sparse as sp

import cg_cases

TOL = cg_cases.TOL
DIAG_SIZES = cg_cases.DIAG_SIZES      # 37, 4096, 70001
PM_SIZES = (38, 4096, 70002)          # even: b = ones has as much weight on +1 as on -1
PERMUTATION_SEEDS = (None, 1, 2, 3, 4, 5)   # None: the identity

# the periodic Bloch operator of test_gpu_cg_operator._bloch (12 x 10 x 8, ComplexF64) has its six lowest eigenvalues 1.4894, 1.6972,
# 1.8093, 1.8179, 1.8762, 1.9208 below 2.0 and the next one, 2.0257, above: 6 eigenvalues below the shift, the nearest 0.0257 away;
# the model needs 167 iterations at tol 1e-12.
BLOCH_SHIFT = 2.0
BLOCH_BELOW = 6

# case -> (shift, eigenvalues below the shift)
SOLVES = {
    "laplace-v-1.2": (1.2, 6),
    "laplace-v-3.0": (3.0, 71),
    "random-csr": (0.797, 10),
    "bloch-c64": (BLOCH_SHIFT, BLOCH_BELOW),
    "mass-box": (0.0, 0),
}
# the model's count in the natural ordering, and the counts under PERMUTATION_SEEDS (numpy 2.x with its pairwise sums and an
# OpenBLAS dot product; recomputed by test_permutations_record_the_spread)
MODEL_ITS = {"laplace-v-1.2": 153, "laplace-v-3.0": 794, "random-csr": 260, "bloch-c64": 167, "mass-box": 61}
PERMUTED_ITS = {
    "laplace-v-1.2": (153, 154, 153, 154, 154, 148),
    "laplace-v-3.0": (794, 795, 802, 802, 799, 796),
    "random-csr": (260, 266, 267, 266, 262, 262),
    "bloch-c64": (167, 167, 167, 162, 167, 163),
    "mass-box": (61, 61, 61, 61, 61, 61),
}
SPREAD = {case: max(v) - min(v) for case, v in PERMUTED_ITS.items()}


def band(case):
    """How far the device's iteration count may lie from MODEL_ITS[case]: twice what summation order alone did to the model."""
    return max(2 * SPREAD[case], 2)


def cyclic_diag(values, n, dtype=np.float64):
    """diag(values[0], values[1], ..., values[0], ...): len(values) distinct eigenvalues, so MINRES ends after exactly that many
    iterations."""
    d = np.asarray(values, dtype=np.float64)[np.arange(n) % len(values)]
    return sp.diags(d.astype(dtype)).tocsr()


THREE = (1.0, -2.0, 4.0)               # indefinite, three eigenvalues: the third iteration is the first to use eps and w__
FIVE = (-3.0, -1.0, 1.0, 2.0, 4.0)
PLUS_MINUS = (1.0, -1.0)               # with b = ones: alpha_1 = 0, the first step makes no progress (c' = 0, phi = 0)


def permuted(A, b, seed):
    """(P A P^T, P b) for the row permutation of default_rng(seed); seed None: A and b themselves."""
    if seed is None:
        return A, b
    p = np.random.default_rng(seed).permutation(A.shape[0])
    return sp.csr_matrix(A)[p][:, p].tocsr(), b[p]


def bounds(A, y, ystar, b, tol, shift=0.0):
    """(true residual, its bound, error, its bound): ||(A - shift) y - b|| <= 2 tol ||b|| and, from ||e|| <= ||(A - shift)^-1|| ||r||,
    ||y - y*|| <= 2 tol ||b|| / min |lambda - shift|.  Also returns the number of eigenvalues below the shift."""
    M = np.asarray(A.todense()) - shift * np.eye(A.shape[0])
    ev = np.linalg.eigvalsh(M)
    nb = float(np.linalg.norm(b))
    return (float(np.linalg.norm(M @ y - b)), 2.0 * tol * nb, float(np.linalg.norm(y - ystar)), 2.0 * tol * nb / float(np.abs(ev).min()),
            int((ev < 0).sum()))
