"""`-m "not gpu"`: the cases of tests/defl_cases.py on the numpy model (tests/sstep_model.py) -- every constant the device tests
(tests/test_gpu_defl_chain.py) lean on is re-derived here, and the conditions the cases were chosen by are held:

  * six cycles run, the per-step (s = 1) and the block run of the model leave the same restart trail, and it is the recorded one;
  * the recorded deflated column count per cycle (`cap16`: exactly 16 = kDeflMax); no block abandoned; at least three deflated
    cycles among 2..5, where the device's invariants are checked;
  * on the recorded lockstep cycles (and possibly more) the two model runs agree to 1e-13 max|H| and 1e-11 in V -- 100 x inside the device bounds
    (1e-11, 1e-9) -- modulo the signs of the kept active columns (defl_cases.lockstep_diff says why); at least two such cycles per
    case (`cap16`: one).  A case that misses this gets another seed or size, never a looser bound;
  * COLRES is at least the model's worst column residual over cycles 2..5 and at most twice it: it cannot be padded;
  * the extended-precision evaluation of those residuals rounds at least 10 x below the device bound 10 COLRES.

Measured: 33 s for the file, 17 s of it the n = 262 401 case (mostly its extended-precision residuals)."""
import numpy as np
import pytest

import defl_cases as dc


@pytest.mark.parametrize("case", list(dc.CASES))
def test_recorded_constants_are_the_models(case):
    A, dtype, s, kw = dc.build(case)
    maxdim = kw["maxdim"]
    step = dc.model_run(case, s=1, keep=range(1, dc.CYCLES))
    R = dc.Residual(A)
    diff, colres, noise = {}, {}, {}

    def on_cycle(cyc, k, H, V, stats):
        if cyc >= 1:
            Hs, Vs = step["snap"].pop(cyc)
            kk, nlock = step["trail"][cyc - 1]
            diff[cyc] = dc.lockstep_diff(Hs, Vs, H, V, nlock, kk)
        if cyc >= 2:
            res, nz = R.columns(V, H, range(k, maxdim))
            colres[cyc], noise[cyc] = float(res.max()), nz

    blk = dc.model_run(case, on_cycle=on_cycle)
    assert len(blk["ndefl"]) == dc.CYCLES and len(step["ndefl"]) == dc.CYCLES          # (neither run converged early)
    assert blk["trail"][:5] == dc.TRAIL[case] and step["trail"] == blk["trail"], (blk["trail"], step["trail"])
    assert blk["ndefl"] == dc.NDEFL[case], blk["ndefl"]
    assert blk["bails"][-1] == 0 and blk["blocks"][0] == 0
    deflated = [c for c in range(2, dc.CYCLES) if blk["ndefl"][c] > 0]
    assert len(deflated) >= 3
    for c in range(1, dc.CYCLES):                                                       # every deflated cycle ran its blocks deflated
        assert blk["defl_blocks"][c] == blk["defl_blocks"][c - 1] + (1 if blk["ndefl"][c] > 0 else 0), blk["defl_blocks"]
        assert blk["blocks"][c] > blk["blocks"][c - 1]
    if case == "cap16":
        assert all(blk["ndefl"][c] == 16 for c in deflated)
        assert blk["blocks"][2] - blk["blocks"][1] >= 2                                 # (more than one block per batch)
    lock = [c for c in range(1, dc.CYCLES) if blk["ndefl"][c] > 0 and diff[c][0] <= 1e-13 and diff[c][1] <= 1e-11]
    assert set(dc.LOCKSTEP[case]) <= set(lock), (lock, diff)            # (a cycle at the edge of 1e-13 may join on another BLAS; none may leave)
    assert len(dc.LOCKSTEP[case]) >= (1 if case == "cap16" else 2)
    worst = max(colres[c] for c in range(2, dc.CYCLES))
    assert worst <= dc.COLRES[case] <= 2.0 * worst, (worst, dc.COLRES[case])
    assert max(noise.values()) <= dc.COLRES[case], (noise, dc.COLRES[case])


def test_the_control_without_deflation():
    """`pair` with deflate=False (the model of KS_CHAIN_DEFLATE=0): nothing is deflated, blocks are abandoned, the restart trail is
    the same, and the blocks on the way down are more than 50 x less accurate than the deflated ones -- COLRES_NO_DEFLATION is this run's worst
    column residual (same rule: at least the model's, at most twice it)."""
    case = "pair"
    A, dtype, s, kw = dc.build(case)
    R = dc.Residual(A)
    colres = {}

    def on_cycle(cyc, k, H, V, stats):
        if cyc >= 2:
            colres[cyc] = float(R.columns(V, H, range(k, kw["maxdim"]))[0].max())

    off = dc.model_run(case, on_cycle=on_cycle, deflate=False)
    assert off["trail"][:5] == dc.TRAIL[case] and off["defl_blocks"][-1] == 0 and off["bails"][-1] >= 1, off
    worst = max(colres.values())
    assert worst <= dc.COLRES_NO_DEFLATION[case] <= 2.0 * worst, (worst, dc.COLRES_NO_DEFLATION[case])
    assert worst >= 50.0 * dc.COLRES[case]


def test_locked_schur_vectors_reach_every_row_tile():
    """What lets the row cases see a wrong sum over the partials: the dominant eigenvector of `pair` carries weight in EVERY tile
    of 256 rows (dense_vectors=True), while the block upper triangular form of _outlier_case keeps it in the first rows alone."""
    for dense in (True, False):
        A = dc.outlier_matrix(1500, np.float64, [50.0, (30.0 * np.cos(0.4), 30.0 * np.sin(0.4))], seed=7100, dense_vectors=dense)
        lam, X = np.linalg.eig(A.toarray())
        u = X[:, np.argmin(np.abs(lam - 50.0))].real
        u /= np.linalg.norm(u)
        assert abs(lam[np.argmin(np.abs(lam - 50.0))] - 50.0) < 1e-10                       # an exact eigenvalue either way
        tiles = [np.linalg.norm(u[r:r + 256]) for r in range(256, 1500, 256)]
        assert (min(tiles) > 1e-2) if dense else (max(tiles) < 1e-12), (dense, tiles)


def test_lockstep_gauge_only_forgives_signs():
    """lockstep_diff: a flipped kept column (with its row and column of H) compares equal; a flipped LOCKED column, a flipped
    WRITTEN column, a perturbed kept column and any change of a ComplexF64 run do not."""
    rng = np.random.default_rng(1)
    V, _ = np.linalg.qr(rng.standard_normal((50, 9)))
    H = np.triu(rng.standard_normal((9, 8)), -1)
    d = np.ones(9)
    d[3] = d[4] = -1.0
    Vb, Hb = V * d[None, :], d[:, None] * H * d[None, :8]
    assert dc.lockstep_diff(H, V, Hb, Vb, 2, 6) == (0.0, 0.0, 2)
    assert dc.lockstep_diff(H, V, Hb, Vb, 4, 6)[1] > 0.1          # column 3 counts as locked: as it stands
    assert dc.lockstep_diff(H, V, Hb, Vb, 2, 4)[1] > 0.1          # column 4 counts as written: as it stands
    Vp = Vb.copy()
    Vp[:, 3] += 1e-8
    assert 0.9e-8 < dc.lockstep_diff(H, V, Hb, Vp, 2, 6)[1] < 1.1e-8
    Vc, Hc = V.astype(np.complex128), H.astype(np.complex128)
    assert dc.lockstep_diff(Hc, Vc, Hc * d[:, None] * d[None, :8], Vc * d[None, :], 2, 6)[1] > 0.1


def test_extended_precision_residual_against_exact_arithmetic():
    """Residual.columns on integers small enough for exact float64 arithmetic: zero where A v = V h exactly, the planted defect
    otherwise; an empty row of the CSR matrix contributes nothing."""
    import scipy.sparse as sp

    A = sp.csr_matrix(np.array([[2.0, 0, 1, 0], [0, 0, 0, 0], [0, 3, 0, 1], [1, 0, 0, 4]]))
    V = np.array([[1.0, 0, 0, 0], [2, 1, 0, 0], [3, 0, 1, 0], [1, 1, 6, 1]])      # unit triangular: an integer inverse
    Vinv = np.round(np.linalg.inv(V))
    assert np.array_equal(Vinv @ V, np.eye(4))
    H = np.zeros((4, 3))
    H[:, 0] = Vinv @ (A @ V[:, 0])
    H[:, 1] = Vinv @ (A @ V[:, 1]) - np.array([0, 0, 0.5, 0])                      # defect V[:, 2] / 2, norm sqrt(37) / 2
    res, noise = dc.Residual(A).columns(V, H, [0, 1])
    assert res[0] == 0.0 and abs(res[1] - np.sqrt(37.0) / 2) <= 1e-15 and noise < 1e-16
    res_d, _ = dc.Residual(A.toarray()).columns(V, H, [0, 1])
    assert np.abs(res - res_d).max() <= 1e-15
