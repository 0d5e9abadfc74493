"""Matrices and right-hand sides of the conjugate-gradient tests (tests/test_cg_model_cpu.py, tests/test_gpu_cg_operator.py).  Plain
numpy / scipy: no device, no library.  Every case is Hermitian positive definite (after its shift)."""
import functools

import numpy as np
import scipy.sparse as sp

TOL = 1e-12
DIAG_SIZES = (37, 4096, 70001)   # below one wave; whole packs and workgroups; odd, a ragged last workgroup, several partial sums
MASS_SHAPE = (33, 7, 9)
GRID_SHAPE = (12, 10, 8)
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])


def size(shape):
    return int(np.prod(shape))


def rhs(n, dtype, seed=7):
    """b ~ U(0.5, 1.5) (both parts for ComplexF64)."""
    rng = np.random.default_rng(seed + n)
    b = rng.random(n) + 0.5
    if np.dtype(dtype).kind == "c":
        b = b + 1j * (rng.random(n) + 0.5)
    return b.astype(dtype)


def diag3(n, dtype=np.float64):
    """diag(1, 2, 4, 1, 2, 4, ...): three distinct eigenvalues, so conjugate gradients end after exactly three iterations -- with a
    wrong beta they degrade to steepest descent and need dozens."""
    d = np.array([1.0, 2.0, 4.0])[np.arange(n) % 3]
    return sp.diags(d.astype(dtype)).tocsr()


def indefinite(n, dtype=np.float64):
    """(A, b): diag3 with entry 5 replaced by -3, and a right-hand side that weighs that entry 100 times: the first curvature
    p^H A p = b^H A b = -3e4 + O(n) is negative (n below twelve thousand), so the failure is certain at iteration 1.  (With a
    generic b conjugate gradients may well solve an indefinite diagonal system without ever meeting a negative curvature.)"""
    A = diag3(n, dtype).tolil()
    A[5, 5] = -3.0
    b = np.ones(n, dtype=dtype)
    b[5] = 100.0
    return A.tocsr(), b


def _kron3(parts):
    """Kronecker product with axis 0 (x) fastest: row r = ix + nx (iy + ny iz)."""
    out = parts[-1]
    for m in parts[-2::-1]:
        out = sp.kron(out, m, format="csr")
    return sp.csr_matrix(out)


def mass(shape=MASS_SHAPE):
    """The truncated Q1 mass matrix with unit spacing: the Kronecker product of tridiag(1/6, 4/6, 1/6), cond = 22.8 on 33 x 7 x 9
    (what host_grid_box_matrix(shape, q1_fem_taps(3)[1]) assembles)."""
    return _kron3([sp.diags([np.full(m - 1, 1.0 / 6.0), np.full(m, 4.0 / 6.0), np.full(m - 1, 1.0 / 6.0)], [-1, 0, 1]) for m in shape])


def potential(shape=GRID_SHAPE, lo=0.0, seed=13):
    """V ~ U(lo, lo + 1), flat in row order."""
    return np.random.default_rng(seed + size(shape)).random(size(shape)) + lo


def laplace_v(shape=GRID_SHAPE, v=None):
    """7-point -Laplacian + diag(V) with open boundaries."""
    v = potential(shape) if v is None else v
    one = [sp.diags([np.full(m - 1, -1.0), np.full(m, 2.0), np.full(m - 1, -1.0)], [-1, 0, 1]) for m in shape]
    eye = [sp.identity(m) for m in shape]
    A = sum(_kron3([one[b] if b == a else eye[b] for b in range(len(shape))]) for a in range(len(shape)))
    return sp.csr_matrix(A + sp.diags(v))


@functools.lru_cache(maxsize=None)
def random_spd(n=1500, seed=3):
    """A random sparse symmetric matrix made strictly diagonally dominant: ragged rows (0 to about a dozen off-diagonal entries)
    with random values and random columns, so no dictionary, stencil or sliced layout fits: CSR row blocks."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n, 3 * n)
    cols = rng.integers(0, n, 3 * n)
    keep = rows != cols
    S = sp.coo_matrix((rng.random(int(keep.sum())) - 0.5, (rows[keep], cols[keep])), shape=(n, n)).tocsr()
    S = S + S.T
    d = np.asarray(abs(S).sum(axis=1)).ravel() + 0.5 + rng.random(n)
    A = sp.csr_matrix(S + sp.diags(d))
    A.sort_indices()
    return A


def bounds(A, y, ystar, b, tol, shift=0.0):
    """(true residual, its bound, error, its bound): ||(A - shift) y - b|| <= 2 tol ||b|| and, from ||e|| <= ||A^-1|| ||r||,
    ||y - y*|| <= 2 tol ||b|| / lambda_min."""
    M = np.asarray(A.todense()) - shift * np.eye(A.shape[0])
    lam_min = float(np.linalg.eigvalsh(M)[0])
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(M @ y - b)), 2.0 * tol * nb, float(np.linalg.norm(y - ystar)), 2.0 * tol * nb / lam_min
