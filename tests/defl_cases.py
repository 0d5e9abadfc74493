"""Shared cases of the IN-CHAIN DEFLATION tests (csrc/ks_block_kernels.hpp: k_defl_dots / k_defl_reduce / k_defl_apply, the
c_i / sigma_i term of k_fin_blk; csrc/ks_defl_plan.hpp): matrices, solver parameters and -- recorded from the numpy model
(tests/sstep_model.py) -- what each case does cycle by cycle.  tests/test_defl_cases_cpu.py re-derives every recorded constant from
the model and holds the conditions the cases were chosen by; tests/test_gpu_defl_chain.py runs the cases on the device against the
recorded constants (no model run on the GPU machine).

All cases: :LM, tol = 1e-10, five restarts = expansions ("cycles") 0..5.  Cycle 0 runs step by step (no Ritz values yet); the
first restart already locks the outliers, so cycles 1..5 run in blocks with a deflated chain.  Cycle 1 starts from bit-identical
data in a per-step and a block run; the invariants (and COLRES) cover cycles 2..5.

Rows (workgroups of 256 rows; the deflation kernels launch min(1024, 4 x CUs, ceil(n / 256)) of them):
  255 -> one workgroup;  257 -> two;  16 385 -> 65 partial sums, the second trip of the 64-lane loops over the partials in
  k_defl_apply / k_defl_reduce;  262 401 -> 1 025 row tiles on at most 1 024 workgroups, the grid-stride wrap of k_defl_dots /
  k_defl_apply.
Columns: 1 (`disc`), 3 with a locked 2 x 2 block (`pair`), 2 complex (`cplx`: the conjugation of k_defl_dots), 16 = kDeflMax
(`cap16`, two and three blocks per batch)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import arnoldi as oa

CYCLES = 6            # expansions 0..5: five restarts in between
TOL = 1e-10


def outlier_matrix(N, dtype, planted, seed, dense_vectors=True):
    """Planted dominant eigenvalues coupled to a sparse random bulk, order N (tests/test_gpu_random_stress.py::_outlier_case with
    explicit parameters): B a sparse random bulk of spectral radius ~1 (6 entries per row, variance 1/6), D the planted blocks -- a
    scalar is a 1 x 1 block, a pair (a, b) the 2 x 2 block [[a, b], [-b, a]] with eigenvalues a +- b i.  The planted values are
    exact eigenvalues of the whole; their Schur vectors are not orthogonal to the invariant subspace of the rest, which is what
    makes a Newton chain grow along them.  ComplexF64: a complex diagonal (0.1 i x normal) on the bulk.

    dense_vectors=False: the block UPPER triangular [[D, C], [0, B]] of _outlier_case, C an O(1) coupling of ~20 entries per row.
    Its planted Schur vectors are e_1 .. e_k exactly: the deflation kernels' dot products live in the first row tile, every other
    partial sum is zero, the update touches k rows -- a wrong sum over the partials cannot be seen (tried: with the loops over the
    partials cut at 64 the n = 16 385 case passed with every digit unchanged).
    dense_vectors=True (the cases of this file): the planted block LAST, [[B, L], [0, D]], with a DENSE coupling L (every bulk
    row, variance 20 / n: ||L x|| ~ 4.5 ||x||): the Schur vectors [(lambda - B)^-1 L x; x] carry ~1 % of their weight spread evenly
    over all rows -- every row tile contributes to every dot product, every row is updated -- and the rest in the LAST rows: the
    last partial sum (n = 16 385: the 65th, one row) and the wrapped tile (n = 262 401: the 1 025th) carry what the deflation is
    about.  (A chain deflated with a slightly wrong c_i is still an exact chain -- the H recovery adds whatever c_i was used -- so a
    small error in the sums only costs conditioning; losing a planted row's share of them loses the deflation.)"""
    rng = np.random.default_rng(seed)
    blocks = []
    for p in planted:
        if isinstance(p, tuple):
            a, b = p
            blocks.append(np.array([[a, b], [-b, a]]))
        else:
            blocks.append(np.array([[p]]))
    D = sp.block_diag(blocks, format="csr")
    k = D.shape[0]
    n = N - k
    B = sp.random(n, n, density=6.0 / n, random_state=rng, format="csr", data_rvs=lambda m: rng.standard_normal(m) / np.sqrt(6.0))
    if dense_vectors:
        L = sp.csr_matrix(rng.standard_normal((n, k)) * np.sqrt(20.0 / n))
        A = sp.bmat([[B, L], [None, D]], format="csr")
    else:
        C = sp.csr_matrix(rng.standard_normal((k, n)) * (rng.random((k, n)) < 20.0 / n))
        A = sp.bmat([[D, C], [None, B]], format="csr")
    if np.dtype(dtype).kind == "c":
        bulk = 0.1 * rng.standard_normal(n)
        A = (A + 1j * sp.diags(np.concatenate([bulk, np.zeros(k)] if dense_vectors else [np.zeros(k), bulk]))).tocsr()
    A = A.astype(dtype)
    A.sort_indices()
    return A


def start_vector(N, dtype, seed=3):
    v = oa.uniform_hash(seed, np.arange(N))
    if np.dtype(dtype).kind == "c":
        v = v + 1j * oa.uniform_hash(seed + 1, np.arange(N))
    return v.astype(dtype)


def _disc():
    """the dense operator of tests/test_gpu_sstep.py::test_in_chain_deflation_keeps_the_blocks_on_dominant_outliers (test/partial_schur.jl:122-138)"""
    rng = np.random.default_rng(5)
    A = rng.standard_normal((400, 400)) / 20.0
    A[0, 0] = 50.0
    return A


def _pair(N):
    return lambda: outlier_matrix(N, np.float64, [50.0, (30.0 * np.cos(0.4), 30.0 * np.sin(0.4))], seed=7100)


def _cplx(N):
    return lambda: outlier_matrix(N, np.complex128, [40.0 + 5.0j, -35.0j], seed=7200)


def _cap16():
    from oracle.matrices import hashed_nonsymmetric
    return hashed_nonsymmetric(2000, seed=11, planted=[(60.0 - 2.0 * i, 0.0) for i in range(16)])


_SMALL = dict(nev=5, mindim=10, maxdim=30)

# id -> (matrix builder, dtype, block size, solver parameters)
CASES = {
    "disc-s5": (_disc, np.float64, 5, _SMALL),
    "disc-s10": (_disc, np.float64, 10, _SMALL),
    "disc-s20": (_disc, np.float64, 20, _SMALL),
    "pair": (_pair(1500), np.float64, 10, _SMALL),
    "cplx": (_cplx(1500), np.complex128, 10, _SMALL),
    "cap16": (_cap16, np.float64, 10, dict(nev=19, mindim=24, maxdim=50)),
    "pair-255": (_pair(255), np.float64, 10, _SMALL),
    "pair-257": (_pair(257), np.float64, 10, _SMALL),
    "pair-16385": (_pair(16385), np.float64, 10, _SMALL),
    "pair-262401": (_pair(262401), np.float64, 10, _SMALL),
    "cplx-255": (_cplx(255), np.complex128, 10, _SMALL),
    "cplx-257": (_cplx(257), np.complex128, 10, _SMALL),
    "cplx-16385": (_cplx(16385), np.complex128, 10, _SMALL),
}

# ---- recorded from the model (tests/test_defl_cases_cpu.py re-derives all of it) ----
# (k, nlock) the restart behind cycles 0..4 leaves (block run of the model)
TRAIL = {
    "disc-s5": [(11, 1), (11, 1), (11, 1), (11, 1), (11, 1)],
    "disc-s10": [(11, 1), (11, 1), (11, 1), (11, 1), (11, 1)],
    "disc-s20": [(11, 1), (11, 1), (11, 1), (11, 1), (11, 1)],
    "pair": [(13, 3), (13, 3), (13, 3), (13, 3), (13, 3)],
    "cplx": [(12, 2), (12, 2), (12, 2), (12, 2), (12, 2)],
    "cap16": [(37, 16), (38, 17), (37, 17), (37, 17), (37, 17)],
    "pair-255": [(13, 3), (13, 3), (14, 3), (13, 3), (13, 3)],
    "pair-257": [(13, 3), (14, 3), (13, 3), (13, 3), (13, 3)],
    "pair-16385": [(13, 3), (13, 3), (14, 3), (14, 3), (14, 3)],
    "pair-262401": [(13, 3), (14, 3), (13, 3), (13, 3), (13, 3)],
    "cplx-255": [(12, 2), (12, 2), (12, 2), (12, 2), (12, 2)],
    "cplx-257": [(12, 2), (12, 2), (12, 2), (12, 2), (12, 2)],
    "cplx-16385": [(12, 2), (12, 2), (12, 2), (12, 2), (12, 2)],
}
# columns the chain of each cycle 0..5 is deflated against
NDEFL = {
    "disc-s5": [0, 1, 1, 1, 1, 1],
    "disc-s10": [0, 1, 1, 1, 1, 1],
    "disc-s20": [0, 1, 1, 1, 1, 1],
    "pair": [0, 3, 3, 3, 3, 3],
    "cplx": [0, 2, 2, 2, 2, 2],
    "cap16": [0, 16, 16, 16, 16, 16],
    "pair-255": [0, 3, 3, 3, 3, 3],
    "pair-257": [0, 3, 3, 3, 3, 3],
    "pair-16385": [0, 3, 3, 3, 3, 3],
    "pair-262401": [0, 3, 3, 3, 3, 3],
    "cplx-255": [0, 2, 2, 2, 2, 2],
    "cplx-257": [0, 2, 2, 2, 2, 2],
    "cplx-16385": [0, 2, 2, 2, 2, 2],
}
# deflated cycles on which the model's per-step and block runs agree to 1e-13 max|H| in H and 1e-11 in V (100 x inside the device
# bounds) once the kept active columns carry the same signs (lockstep_diff): the cycles compared in lockstep on the device.
LOCKSTEP = {
    "disc-s5": [1, 2, 3, 4, 5],
    "disc-s10": [1, 2, 3, 4, 5],
    "disc-s20": [1, 2, 3, 4, 5],
    "pair": [1, 2, 3, 4, 5],
    "cplx": [1, 2, 3, 4, 5],
    "cap16": [1, 2, 3, 4, 5],
    "pair-255": [1, 2, 3, 4],
    "pair-257": [1, 2, 3, 4, 5],
    "pair-16385": [1, 2, 3, 4, 5],
    "pair-262401": [1, 2, 3, 4, 5],
    "cplx-255": [1, 2, 3, 4, 5],
    "cplx-257": [1, 2, 3],
    "cplx-16385": [1, 2, 3, 4, 5],
}
# worst column residual ||A v_j - V_{m+1} H[:, j]||_2 of the model's block run over the columns written in cycles 2..5, times 1.4
# (test_defl_cases_cpu.py: at least the model's value, at most twice it)
COLRES = {
    "disc-s5": 3.94e-15,
    "disc-s10": 1.24e-14,
    "disc-s20": 3.06e-13,
    "pair": 4.18e-15,
    "cplx": 3.15e-15,
    "cap16": 2.06e-12,
    "pair-255": 2.49e-14,
    "pair-257": 1.32e-14,
    "pair-16385": 2.72e-15,
    "pair-262401": 1.9e-15,
    "cplx-255": 8.33e-15,
    "cplx-257": 1.39e-14,
    "cplx-16385": 1.36e-15,
}

# the control (KS_CHAIN_DEFLATE=0, model: deflate=False): blocks are abandoned, the block size goes down to single steps, and the
# small blocks on the way carry the growth of the chain along the locked outliers (x 50 per step) into H -- the same quantity,
# ~90 x the deflated run's; same rule
COLRES_NO_DEFLATION = {
    "pair": 3.63e-13,
}


def build(case):
    mk, dtype, s, kw = CASES[case]
    A = mk()
    return A, np.dtype(dtype), s, dict(kw, which="LM", tol=TOL)


# ---- lockstep comparison of two runs of the same solve ----
def lockstep_diff(Hs, Vs, Hb, Vb, nlock, k):
    """(max |H_s - H_b| / max |H_s|, max |V_s - V_b|) of two factorisations of the same cycle, the second one brought to the first
    one's SIGN CONVENTION on the kept active columns nlock..k-1 first (real arithmetic only).

    Why: the restart's Schur vectors are unique up to a sign each (a rotation by pi for the two columns of a 2 x 2 block of the real
    Schur form), and which sign the QR iteration lands on is a function of the last bits of its input.  Two runs whose H differ by
    1e-15 therefore come out of a restart with V_b = V_s D, H_b = D H_s D for a diagonal D = diag(+-1) on the kept active columns --
    the same factorisation -- about every other cycle (model: every real case of this file; the locked columns and every column
    the expansion writes agree as they stand, ComplexF64 runs have no such freedom and are compared as they stand).  D is read off
    the basis (sign of <v_s, v_b>), applied to rows and columns of H, and everything is then held to the full bounds: a column
    that differs by anything but its sign fails the V bound by nine orders of magnitude."""
    d = np.ones(Vs.shape[1])
    if Vs.dtype.kind == "f":
        for j in range(nlock, k):
            if np.dot(Vs[:, j], Vb[:, j]) < 0:
                d[j] = -1.0
    m = Hs.shape[1]
    Hg = d[: m + 1, None] * Hb * d[None, :m]
    return float(np.abs(Hs - Hg).max() / np.abs(Hs).max()), float(np.abs(Vs - Vb * d[None, :]).max()), int((d < 0).sum())


# ---- the reference evaluation of a column residual: extended precision on the host ----
def _ld(dtype):
    return np.clongdouble if np.dtype(dtype).kind == "c" else np.longdouble


class Residual:
    """||A v_j - V H[:, j]||_2 per column in np.longdouble (64-bit significand: unit roundoff u = 2^-64): the dense operator by
    matmul, the CSR product as np.add.reduceat over the longdouble products of each row.  `noise(j)` bounds the evaluation's own
    rounding a priori: (terms per row + 2) u || |A| |v_j| + |V| |H[:, j]| ||_2."""

    def __init__(self, A):
        self.A = A
        self.ld = _ld(A.dtype)
        if sp.issparse(A):
            A = A.tocsr()
            self.data = A.data.astype(self.ld)
            self.indices, ptr = A.indices, A.indptr
            self.nonempty = ptr[1:] > ptr[:-1]
            self.starts = ptr[:-1][self.nonempty]
            self.absA = abs(A)
            self.terms = int((ptr[1:] - ptr[:-1]).max())
        else:
            self.dense = np.asarray(A).astype(self.ld)
            self.absA = np.abs(np.asarray(A))
            self.terms = A.shape[1]

    def matvec(self, x):
        if not sp.issparse(self.A):
            return self.dense @ x
        out = np.zeros(self.A.shape[0], dtype=self.ld)
        out[self.nonempty] = np.add.reduceat(self.data * x[self.indices], self.starts)
        return out

    def columns(self, V, H, cols):
        """(residual norms of the columns `cols`, the largest a-priori rounding bound of their evaluation)"""
        cols = list(cols)
        Vl = np.asfortranarray(V).astype(self.ld)
        m1 = V.shape[1]
        res, noise = [], 0.0
        u = float(np.finfo(np.longdouble).eps) / 2
        VH = Vl @ H[:m1, cols].astype(self.ld)
        for i, j in enumerate(cols):
            r = self.matvec(Vl[:, j]) - VH[:, i]
            res.append(float(np.sqrt(np.sum(np.abs(r) ** 2))))
            mag = self.absA @ np.abs(V[:, j]) + np.abs(V) @ np.abs(H[:m1, j])
            noise = max(noise, (self.terms + m1 + 2) * u * float(np.linalg.norm(mag)))
        return np.asarray(res), noise


# ---- the model's run of a case (CPU tests only) ----
def model_run(case, s=None, keep=(), on_cycle=None, deflate=True):
    """sm.solve on the case with block size `s` (default: the case's; 1 = step by step).  Returns dict(trail, ndefl[cycle],
    bails[cycle], blocks[cycle], snap[cycle] = (H, V) for the cycles in `keep`); `deflate=False`: the model of KS_CHAIN_DEFLATE=0; `on_cycle(cycle, k, H, V, stats)` sees every
    cycle's factorisation while it stands."""
    import sstep_model as sm

    A, dtype, s_case, kw = build(case)
    s = s_case if s is None else s
    out = dict(ndefl=[], bails=[], blocks=[], defl_blocks=[], k=[], snap={})
    maxdim = kw["maxdim"]

    def trace(cyc, k, st, stats):
        out["ndefl"].append(stats.get("defl_last", 0))
        out["bails"].append(stats.get("bails", 0))
        out["blocks"].append(stats.get("blocks", 0))
        out["defl_blocks"].append(stats.get("defl_blocks", 0))
        out["k"].append(k)
        if cyc in keep or on_cycle is not None:
            H, V = st.H.copy(), st.true_basis(maxdim + 1)
            if cyc in keep:
                out["snap"][cyc] = (H, V)
            if on_cycle is not None:
                on_cycle(cyc, k, H, V, stats)

    r = sm.solve(A, start_vector(A.shape[0], dtype), restarts=CYCLES, dtype=dtype, s=s, check=False, trace=trace, deflate=deflate, **kw)
    out["trail"] = [tuple(int(x) for x in t) for t in r["trail"]]
    out["A"] = A
    return out
