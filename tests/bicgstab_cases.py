"""Matrices, shifts and recorded figures of the BiCGStab(2) tests (tests/test_bicgstab_model_cpu.py,
tests/test_gpu_bicgstab_operator.py).  Plain numpy / scipy: no device, no library.  No matrix here is Hermitian.

The grid problems are 7-point convection-diffusion operators on 12 x 10 x 8 with open boundaries: taps
[-1 - cz, -1 - cy, -1 - cx, 6, -1 + cx, -1 + cy, -1 + cz] plus a potential V ~ U(0, 1) on the diagonal.
  "convdiff"  c = (0.4, 0.3, 0.2): |c| < 1, similar to a symmetric matrix by a diagonal scaling -- a real spectrum (1.0436 ... 11.99),
              but non-normal.
  "swirl"     c = (1.6, 0.3, 0.2): the x links have opposite signs, so the spectrum has complex pairs (|Im| up to 2.42, smallest real
              part 2.81).

ITERATION BANDS, as in tests/minres_cases.py: the device and the numpy model (tests/bicgstab_model.py) differ in the order of their
sums; what summation order alone does to the MODEL is measured by solving each case under symmetric row permutations
(`PERMUTATION_SEEDS`: the identity and five random ones).  `SPREAD[case]` is max - min of those six counts as recorded on a CPU;
tests/test_bicgstab_model_cpu.py recomputes and prints every one of them and holds each permuted count to the band.  The device's
count must lie within `band(case)` = max(2 SPREAD, 2) of `MODEL_ITS`, the model's count in the natural ordering."""
import functools

import numpy as np
import scipy.sparse as sp

import grid_cases

TOL = 1e-12
SHAPE = (12, 10, 8)
N = 960
DIAG_SIZES = (37, 4096, 70001)   # below one wave; whole packs and workgroups; odd, a ragged last workgroup, several partial sums
PERMUTATION_SEEDS = (None, 1, 2, 3, 4, 5)   # None: the identity
CONVECTION = {"convdiff": (0.4, 0.3, 0.2), "swirl": (1.6, 0.3, 0.2)}

_rng = np.random.default_rng(0)
V = _rng.random(N)
B = _rng.standard_normal(N)
B_IMAG = np.random.default_rng(1).standard_normal(N)   # the imaginary part of the ComplexF64 right-hand side


def taps(kind, dtype=np.float64):
    cx, cy, cz = CONVECTION[kind]
    return np.array([-1 - cz, -1 - cy, -1 - cx, 6.0, -1 + cx, -1 + cy, -1 + cz]).astype(dtype)


def grid_matrix(kind, dtype=np.float64):
    """The host matrix of a grid case, assembled without the library (what host_grid_matrix(SHAPE, taps, V) gives)."""
    return sp.csr_matrix(grid_cases.kron_matrix(SHAPE, taps(kind, dtype), V.astype(dtype)))


@functools.lru_cache(maxsize=None)
def random_nonsymmetric(n=1500, seed=3):
    """A random sparse NON-symmetric matrix, strictly diagonally dominant by rows: ragged rows with random values and random
    columns, so no dictionary, stencil or sliced layout fits.  Its diagonal is 0.5 + U(0, 1) above the absolute row sum."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n, 6 * n)
    cols = rng.integers(0, n, 6 * n)
    keep = rows != cols
    S = sp.coo_matrix((rng.random(int(keep.sum())) - 0.5, (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 0.5 + rng.random(n)
    A = sp.csr_matrix(S + sp.diags(d))
    A.sort_indices()
    return A


def rhs(n, dtype):
    if n == N:
        b = B if np.dtype(dtype).kind != "c" else B + 1j * B_IMAG
    else:
        rng = np.random.default_rng(7 + n)
        b = rng.standard_normal(n)
        if np.dtype(dtype).kind == "c":
            b = b + 1j * rng.standard_normal(n)
    return np.asarray(b).astype(dtype)


# case -> (matrix kind, dtype, shift)
SOLVES = {
    "convdiff-0": ("convdiff", np.float64, 0.0),
    "convdiff-0.9936": ("convdiff", np.float64, 0.9936),
    "swirl-0": ("swirl", np.float64, 0.0),
    "swirl-2.0": ("swirl", np.float64, 2.0),
    "swirl-c64": ("swirl", np.complex128, 2.0 + 0.5j),
    "convdiff-c64": ("convdiff", np.complex128, 2.0 + 0.5j),
    "random-csr": ("random", np.float64, 0.4),
}


def host_case(case):
    """(A, b, shift) of a case of SOLVES on the host."""
    kind, dtype, shift = SOLVES[case]
    A = random_nonsymmetric() if kind == "random" else grid_matrix(kind, dtype)
    return A, rhs(A.shape[0], dtype), shift


# the model's count in the natural ordering, and the counts under PERMUTATION_SEEDS (numpy 2.x with its pairwise sums and an
# OpenBLAS dot product; recomputed by test_model_holds_the_bounds_and_permutations_record_the_spread)
MODEL_ITS = {"convdiff-0": 14, "convdiff-0.9936": 33, "swirl-0": 16, "swirl-2.0": 52, "swirl-c64": 46, "convdiff-c64": 56, "random-csr": 17}
PERMUTED_ITS = {
    "convdiff-0": (14, 14, 14, 14, 14, 14),
    "convdiff-0.9936": (33, 33, 33, 33, 33, 33),
    "swirl-0": (16, 16, 16, 16, 16, 16),
    "swirl-2.0": (52, 51, 51, 50, 51, 51),
    "swirl-c64": (46, 46, 46, 46, 46, 46),
    "convdiff-c64": (56, 57, 59, 54, 56, 55),
    "random-csr": (17, 17, 17, 17, 17, 17),
}
SPREAD = {case: max(v) - min(v) for case, v in PERMUTED_ITS.items()}


def band(case):
    """How far the device's iteration count may lie from MODEL_ITS[case]: twice what summation order alone did to the model."""
    return max(2 * SPREAD[case], 2)


def cyclic_diag(values, n, dtype=np.float64):
    """diag(values[0], values[1], ..., values[0], ...): len(values) distinct eigenvalues."""
    d = np.asarray(values)[np.arange(n) % len(values)]
    return sp.diags(d.astype(dtype)).tocsr()


THREE = (1.0, -2.0, 4.0)
THREE_C = (1.0 + 1.0j, 2.0 - 1.0j, -1.0 + 0.5j)
DIAG_MAX_ITS = 8      # BiCGStab(2) ends a problem of three eigenvalues after two iterations in exact arithmetic; in floating point
                      # the finite termination is approximate and a few more follow (the model: see the CPU test's output)


def permuted(A, b, seed):
    """(P A P^T, P b) for the row permutation of default_rng(seed); seed None: A and b themselves."""
    if seed is None:
        return A, b
    p = np.random.default_rng(seed).permutation(A.shape[0])
    return sp.csr_matrix(A)[p][:, p].tocsr(), b[p]


def true_residual(A, y, b, shift=0.0):
    return float(np.linalg.norm(A @ y - shift * y - b))
