"""`-m "not gpu"`: the host plan of the multigrid V-cycle (csrc/ks_mg_plan.hpp through ks_host_multigrid_plan / _restrict /
_prolong_add) against closed forms, a plain loop written from the definition and every refusal; the numpy model of the cycle
(tests/mg_model.py) on the very cases tests/test_gpu_multigrid_operator.py runs on the device -- so the counts and bounds asserted
there are known to hold for the reference alone; and `extras.multigrid_hierarchy`."""
from fractions import Fraction

import numpy as np
import pytest

import cg_cases as cc
import mg_cases as cases
import mg_model as model
import pcg_cases as pc
import pcg_model
from __graft_entry__ import import_package

pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

EPS = np.finfo(np.float64).eps
PAIRS = [(s[0], s[1]) for s in cases.LEVEL_SHAPES.values()] + [((37,), (19,)), ((19,), (10,)), ((6, 5, 4), (3, 3, 2)), ((5, 4), (5, 2))]
PAIRS += [p for p in cases.TRANSFER_PAIRS if p not in PAIRS]     # every pair the device is held to the host functions on
DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the plan
def _cheb(j, s):
    """T_j(s) in exact arithmetic."""
    t0, t1 = Fraction(1), s
    for _ in range(j):
        t0, t1 = t1, 2 * s * t1 - t0
    return t0


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("lam,ratio", [(2.0, 4.0), (1.9337, 8.0), (1.0, 30.0), (3.75, 1.5)])
def test_smoother_coefficients_against_closed_forms(degree, lam, ratio):
    """rho_j = T_j(sig) / T_{j+1}(sig), so a_j = T_{j-1} / T_{j+1} and b_j = 2 T_j / (del T_{j+1}) in exact rational arithmetic.  The
    plan rounds three times per rho_j and inherits the error of rho_{j-1} damped by rho_j^2 < 1: 4 (j + 1) eps covers it."""
    p = pkg.host_multigrid_plan([(8,), (4,)], [lam], degree=degree, ratio=ratio)
    L, Rt = Fraction(lam), Fraction(ratio)
    thc, dl = (L + L / Rt) / 2, (L - L / Rt) / 2
    sig = thc / dl
    assert p["a"].shape == p["b"].shape == (1, degree) and p["rows"] == (8, 4) and p["scale"][0] == 0.5
    assert p["a"][0, 0] == 0.0 and p["b"][0, 0] == 1.0 / ((lam + lam / ratio) / 2.0)
    assert abs(Fraction(p["b"][0, 0]) - 1 / thc) <= 2 * EPS / thc
    for j in range(1, degree):
        a, b = _cheb(j - 1, sig) / _cheb(j + 1, sig), 2 * _cheb(j, sig) / (dl * _cheb(j + 1, sig))
        assert abs(Fraction(p["a"][0, j]) - a) <= 4 * (j + 1) * EPS * a, (j, p["a"][0, j], float(a))
        assert abs(Fraction(p["b"][0, j]) - b) <= 4 * (j + 1) * EPS * b, (j, p["b"][0, j], float(b))
    # ... and bit for bit what the numpy model computes in the same order
    ma, mb = model.coefficients(lam, ratio, degree)
    assert np.array_equal(_bits(p["a"][0]), _bits(np.array(ma))) and np.array_equal(_bits(p["b"][0]), _bits(np.array(mb)))


def test_plan_rows_scales_and_levels():
    p = pkg.host_multigrid_plan([(12, 10, 8), (6, 5, 4), (3, 3, 2)], [2.0, 1.9], degree=2, ratio=4.0)
    assert p["rows"] == (960, 120, 18) and list(p["scale"]) == [0.125, 0.125]
    p = pkg.host_multigrid_plan([(129, 3, 2), (65, 2, 1), (65, 1, 1), (33,)], [2.0, 2.0, 2.0])
    assert p["rows"] == (774, 130, 65, 33) and list(p["scale"]) == [0.125, 0.5, 0.5]
    p = pkg.host_multigrid_plan([(6, 1, 4), (3, 1, 2)], [1.5])
    assert p["rows"] == (24, 6) and list(p["scale"]) == [0.25]
    assert pkg.host_multigrid_plan([(7, 3)], [])["rows"] == (21,)       # no smoothed level
    chain = [(2 ** 15,)]
    while len(chain) < 16:
        chain.append(((chain[-1][0] + 1) // 2,))
    assert len(pkg.host_multigrid_plan(chain, [2.0] * 15)["rows"]) == 16


def test_plan_refusals_name_the_level_and_the_entry():
    ok = [(12, 10, 8), (6, 5, 4), (3, 3, 2)]
    plan = pkg.host_multigrid_plan
    with pytest.raises(pkg.ArgumentError, match=r"level 1 has the extents 6 x 5 x 4, level 2 the extents 3 x 2 x 2: axis 1 must keep its extent 5 or halve it to 3"):
        plan([(12, 10, 8), (6, 5, 4), (3, 2, 2)], [2.0, 2.0])
    with pytest.raises(pkg.ArgumentError, match=r"level 0 .* axis 0 must keep its extent 12 or halve it to 6"):
        plan([(12, 10, 8), (4, 5, 4)], [2.0])
    with pytest.raises(pkg.ArgumentError, match=r"level 0 .* axis 0"):
        plan([(6, 5, 4), (12, 5, 4)], [2.0])                             # growing
    with pytest.raises(pkg.ArgumentError, match=r"level 1 and level 2 have the same extents 6 x 5 x 4 \(at least one axis must be halved per level\)"):
        plan([(12, 10, 8), (6, 5, 4), (6, 5, 4)], [2.0, 2.0])
    with pytest.raises(pkg.ArgumentError, match=r"same extents 1 x 1 x 1"):
        plan([(1,), (1,)], [2.0])                                        # ceil(1 / 2) = 1: nothing left to halve
    with pytest.raises(pkg.ArgumentError, match=r"level 1 has the extents 6 x 0 x 4"):
        plan([(12, 1, 8), (6, 0, 4)], [2.0])
    chain = [(2 ** 17,)]
    while len(chain) < 17:
        chain.append(((chain[-1][0] + 1) // 2,))
    with pytest.raises(pkg.ArgumentError, match=r"17 levels \(at most 16 are supported\)"):
        plan(chain, [2.0] * 16)
    with pytest.raises(pkg.ArgumentError, match=r"fewer than 2\^31 rows"):
        plan([(2 ** 11, 2 ** 10, 2 ** 10), (2 ** 10, 2 ** 9, 2 ** 9)], [2.0])
    for degree in (0, -1):
        with pytest.raises(pkg.ArgumentError, match=r"degree = %d \(must be at least 1\)" % degree):
            plan(ok, [2.0, 2.0], degree=degree)
    for ratio in (1.0, 0.5, 0.0, -4.0, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match=r"ratio = .* \(must be finite and above 1\)"):
            plan(ok, [2.0, 2.0], ratio=ratio)
    for lam in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match=r"level 1: lambda_max = .* \(must be positive and finite\)"):
            plan(ok, [2.0, lam])
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = [np.ones(960), np.ones(120)]
        d[1][77] = bad
        with pytest.raises(pkg.ArgumentError, match=r"level 1: inv_diag entry 77 = .* \(must be positive and finite\)"):
            plan(ok, [2.0, 2.0], inverse_diagonals=d)
    assert plan(ok, [2.0, 2.0], inverse_diagonals=[np.ones(960), np.full(120, 1e-300)])["rows"] == (960, 120, 18)
    # the Python layer: counts and shapes that do not fit
    with pytest.raises(pkg.DimensionMismatch, match="2 smoothed levels take 2 bounds, got 1"):
        plan(ok, [2.0])
    with pytest.raises(pkg.DimensionMismatch, match="inverse diagonal of level 1 has 119 entries"):
        plan(ok, [2.0, 2.0], inverse_diagonals=[np.ones(960), np.ones(119)])
    with pytest.raises(pkg.ArgumentError, match="1 to 3 integer extents"):
        plan([(2, 2, 2, 2), (1, 1, 1, 1)], [2.0])


# ------------------------------------------------------------------------------------------------ the transfers
def _restrict_loop(fine, coarse, b, t):
    """The definition, cell by cell: per coarse cell the terms fl(b[i] - t[i]) added to +0.0 in ascending fine row order."""
    f, c, h = model.dims3(fine), model.dims3(coarse), model.halved(fine, coarse)
    s = 2.0 ** -sum(h)
    out = np.zeros(int(np.prod(c)), dtype=b.dtype)
    for K in range(c[2]):
        for J in range(c[1]):
            for I in range(c[0]):
                acc = b.dtype.type(0.0)
                for k in range(K << h[2], min((K << h[2]) + h[2] + 1, f[2])):
                    for j in range(J << h[1], min((J << h[1]) + h[1] + 1, f[1])):
                        for i in range(I << h[0], min((I << h[0]) + h[0] + 1, f[0])):
                            r = i + f[0] * (j + f[1] * k)
                            acc = acc + (b[r] - t[r])
                out[I + c[0] * (J + c[1] * K)] = s * acc
    return out


def _prolong_add_loop(fine, coarse, e, x):
    f, c, h = model.dims3(fine), model.dims3(coarse), model.halved(fine, coarse)
    out = x.copy()
    for k in range(f[2]):
        for j in range(f[1]):
            for i in range(f[0]):
                out[i + f[0] * (j + f[1] * k)] += e[(i >> h[0]) + c[0] * ((j >> h[1]) + c[1] * (k >> h[2]))]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fine,coarse", PAIRS, ids=["x".join(map(str, p[0])) + "-" + "x".join(map(str, p[1])) for p in PAIRS])
def test_host_transfers_bit_for_bit_against_the_definition(fine, coarse, dtype):
    nf, nc = cc.size(fine), cc.size(coarse)
    b, t, e = cc.rhs(nf, dtype), cc.rhs(nf, dtype, seed=9) * 1e-3, cc.rhs(nc, dtype, seed=11)
    got = pkg.host_multigrid_restrict(fine, coarse, b, t)
    assert got.dtype == np.dtype(dtype) and got.shape == (nc,)
    assert np.array_equal(_bits(got), _bits(_restrict_loop(fine, coarse, b, t)))
    assert np.array_equal(_bits(got), _bits(model.restrict(fine, coarse, b, t)))
    x = pkg.host_multigrid_prolong_add(fine, coarse, e, b)
    assert x.dtype == np.dtype(dtype) and x.shape == (nf,)
    assert np.array_equal(_bits(x), _bits(_prolong_add_loop(fine, coarse, e, b)))
    assert np.array_equal(_bits(x), _bits(b + model.prolong(fine, coarse, e)))


@pytest.mark.parametrize("fine,coarse", PAIRS, ids=["x".join(map(str, p[0])) + "-" + "x".join(map(str, p[1])) for p in PAIRS])
def test_restriction_is_the_scaled_adjoint_of_the_prolongation(fine, coarse):
    """<R v, w> = s <v, P w> exactly on integer-valued data (every sum is exact)."""
    nf, nc = cc.size(fine), cc.size(coarse)
    rng = np.random.default_rng(nf)
    v, w = rng.integers(-50, 50, nf).astype(np.float64), rng.integers(-50, 50, nc).astype(np.float64)
    s = 2.0 ** -sum(model.halved(fine, coarse))
    Rv = pkg.host_multigrid_restrict(fine, coarse, v, np.zeros(nf))
    Pw = pkg.host_multigrid_prolong_add(fine, coarse, w, np.zeros(nf))
    assert np.dot(Rv, w) == s * np.dot(v, Pw)


def test_transfer_pairs_meet_the_coverage_condition():
    """TRANSFER_PAIRS reaches every branch of k_mg_restrict (one thread per coarse cell) and k_mg_prolong_add (one thread per coarse
    x-cell of a fine line), 256 threads per workgroup -- computed from the shapes, so that a change of shapes cannot lose a branch
    silently: workgroups past the first two with a partial last one, each axis kept with an extent above 1 (x kept: the scalar
    accesses with a single cell per thread), a single coarse x-cell, fine lines that start at odd elements (odd nxf, more than one
    line), and a scale of 1/2."""
    assert cases.KBLOCK == 256 and len(cases.TRANSFER_IDS) == len(cases.TRANSFER_PAIRS) == len(set(cases.TRANSFER_IDS))
    assert cases.TRANSFER_PAIRS[:len(cases.LEVEL_SHAPES)] == [(s[0], s[1]) for s in cases.LEVEL_SHAPES.values()]
    for p in [((6, 5, 4), (3, 3, 2)), ((19,), (10,))]:                # the second-level pairs of the hierarchies
        assert p in cases.TRANSFER_PAIRS and p in [(s[1], s[2]) for s in cases.LEVEL_SHAPES.values() if len(s) > 2]
    geo = [(model.dims3(f), model.dims3(c), model.halved(f, c)) for f, c in cases.TRANSFER_PAIRS]

    def blocks(threads):
        return -(-threads // cases.KBLOCK)

    assert any(blocks(c[0] * c[1] * c[2]) >= 3 and (c[0] * c[1] * c[2]) % cases.KBLOCK != 0 for f, c, h in geo)
    assert any(blocks(c[0] * f[1] * f[2]) >= 3 for f, c, h in geo)
    for axis in range(3):
        assert any(not h[axis] and f[axis] > 1 for f, c, h in geo), axis
    assert any(c[0] == 1 and h[0] for f, c, h in geo) and any(c[0] == 1 and not h[0] for f, c, h in geo)
    assert any(f[0] % 2 == 1 and f[1] * f[2] > 1 and h[0] for f, c, h in geo)
    assert any(sum(h) == 1 for f, c, h in geo)
    assert any(len({e % 2 for e in f}) == 2 and all(h) for f, c, h in geo)      # mixed parity with every axis halved
    print("restriction workgroups %s, prolongation workgroups %s"
          % ([blocks(c[0] * c[1] * c[2]) for f, c, h in geo], [blocks(c[0] * f[1] * f[2]) for f, c, h in geo]))


def test_transfers_refuse_grids_that_are_not_consecutive():
    with pytest.raises(pkg.ArgumentError, match="ks_host_multigrid_restrict.*axis 0"):
        pkg.host_multigrid_restrict((12,), (5,), np.ones(12), np.ones(12))
    with pytest.raises(pkg.ArgumentError, match="ks_host_multigrid_prolong_add.*same extents"):
        pkg.host_multigrid_prolong_add((12,), (12,), np.ones(12), np.ones(12))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.host_multigrid_restrict((12,), (6,), np.ones(11), np.ones(12))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.host_multigrid_prolong_add((12,), (6,), np.ones(7), np.ones(12))


# ------------------------------------------------------------------------------------------------ the hierarchy
@pytest.mark.parametrize("case", list(cases.CASES))
def test_hierarchy_shapes_means_and_bounds(case):
    shape, rows = cases.CASES[case]
    c = pc.jump_coeff(shape)
    v = cc.potential(shape)
    H = extras.multigrid_hierarchy(shape, c, potential=v, coarsest_rows=rows)
    assert [L["shape"] for L in H] == cases.LEVEL_SHAPES[case]
    assert cc.size(H[-1]["shape"]) <= rows < cc.size(H[-2]["shape"])
    for l, L in enumerate(H):
        n = cc.size(L["shape"])
        assert np.array_equal(L["spacing"], np.where(np.array(L["shape"]) != np.array(H[l - 1]["shape"] if l else L["shape"]), 2.0, 1.0) *
                              (H[l - 1]["spacing"] if l else 1.0))
        taps, d = extras.diffusion_terms(L["shape"], L["coeff"], L["spacing"], L["potential"])
        assert np.array_equal(L["taps"], taps) and np.array_equal(L["diagonal"], d) and np.array_equal(L["inverse_diagonal"], 1.0 / d)
        # the bound is Gershgorin's for D^-1 A: at least the true largest eigenvalue, at most 2 for a diagonally dominant matrix
        A = pkg.host_grid_variable_matrix(L["shape"], taps, L["coeff"], d).toarray().real
        off = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
        assert L["bound"] == pytest.approx(np.max((d + off) / d), rel=1e-14)
        lam = np.linalg.eigvals(A / d[:, None]).real.max()
        assert lam <= L["bound"] * (1 + 1e-12) <= 2.0 * (1 + 1e-12), (lam, L["bound"])
        if l:
            F = H[l - 1]
            f, h = model.dims3(F["shape"]), model.halved(F["shape"], L["shape"])
            cd = model.dims3(L["shape"])
            for name in ("coeff", "potential"):
                fine = F[name].reshape(f[2], f[1], f[0])
                for I in {0, cd[0] - 1}:
                    for J in {0, cd[1] - 1}:
                        for K in {0, cd[2] - 1}:
                            cell = fine[K << h[2]:(K << h[2]) + h[2] + 1, J << h[1]:(J << h[1]) + h[1] + 1, I << h[0]:(I << h[0]) + h[0] + 1]
                            assert L[name][I + cd[0] * (J + cd[1] * K)] == pytest.approx(cell.mean(), rel=4 * EPS)
        assert L["coeff"].shape == (n,)


def test_hierarchy_of_the_laplacian_is_the_laplacian_scaled_by_a_quarter_per_level():
    shape = (12, 10, 8)
    H = extras.multigrid_hierarchy(shape, np.ones(960), coarsest_rows=16)
    assert [L["shape"] for L in H] == [(12, 10, 8), (6, 5, 4), (3, 3, 2), (2, 2, 1)]
    lap = extras.fd_laplacian_taps(3, 2)
    for l, L in enumerate(H[:3]):
        assert np.all(L["coeff"] == 1.0) and L["potential"] is None
        want = lap * 0.25 ** l
        off = np.delete(want, 3)
        assert np.array_equal(np.delete(L["taps"], 3), off) and L["taps"][3] == 0.0
        assert np.all(L["diagonal"] == want[3])
        A = pkg.host_grid_variable_matrix(L["shape"], L["taps"], L["coeff"], L["diagonal"])
        B = pkg.host_grid_matrix(L["shape"], want)
        assert (A != B).nnz == 0
    assert H[3]["spacing"].tolist() == [8.0, 8.0, 8.0]
    # an axis that has reached extent 1 is halved no more and keeps its spacing
    G = extras.multigrid_hierarchy((8, 2), np.ones(16), spacing=(1.0, 3.0), coarsest_rows=1)
    assert [L["shape"] for L in G] == [(8, 2), (4, 1), (2, 1), (1, 1)] and [L["spacing"].tolist() for L in G] == [[1, 3], [2, 6], [4, 6], [8, 6]]


def test_hierarchy_refusals():
    c = np.ones(24)
    with pytest.raises(pkg.ArgumentError, match=r"level 0: diagonal - shift must be positive"):
        extras.multigrid_hierarchy((6, 4), c, shift=4.0)
    with pytest.raises(pkg.ArgumentError, match="shift is not finite"):
        extras.multigrid_hierarchy((6, 4), c, shift=np.nan)
    with pytest.raises(pkg.ArgumentError, match="coarsest_rows"):
        extras.multigrid_hierarchy((6, 4), c, coarsest_rows=0)
    with pytest.raises(pkg.DimensionMismatch):
        extras.multigrid_hierarchy((6, 4), np.ones(23))
    with pytest.raises(pkg.DimensionMismatch):
        extras.multigrid_hierarchy((6, 4), c, potential=np.ones(5))
    assert len(extras.multigrid_hierarchy((6, 4), c, coarsest_rows=24)) == 1
    assert [L["shape"] for L in extras.multigrid_hierarchy((3,), np.ones(3), coarsest_rows=1)] == [(3,), (2,), (1,)]


# ------------------------------------------------------------------------------------------------ the model of the cycle
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_model_cycle_is_symmetric_positive_definite_and_its_own_error_is_recorded(case, dtype):
    """<u, M v> - <M u, v> at rounding level and u^H M u > 0 on eight random columns; ERR[case] recomputed."""
    H, mats, coarse = cases.setup(pkg, extras, case)
    M = cases.model(H, mats, coarse)
    n = mats[0].shape[0]
    rng = np.random.default_rng(n)
    U = rng.standard_normal((n, 8)) + (1j * rng.standard_normal((n, 8)) if np.dtype(dtype).kind == "c" else 0.0)
    MU = np.stack([M(U[:, j]) for j in range(8)], axis=1)
    G = U.conj().T @ MU
    asym = np.abs(G - G.conj().T).max() / np.abs(G).max()
    print("%s %s: asymmetry %.3g, min u^H M u %.3g" % (case, np.dtype(dtype).name, asym, np.diag(G).real.min()))
    # (a Gram entry is a sum of n products of M's entries, each carrying the cycle's rounding error of a few eps)
    assert asym <= 64 * EPS
    assert np.all(np.diag(G).real > 0) and np.all(np.linalg.eigvalsh(0.5 * (G + G.conj().T)) > 0)
    assert M.products == [8 * 2 * cases.DEGREE] * (len(H) - 1)
    b = cases.rhs(case, dtype)
    err = cases.rel_err(M(b), cases.model(H, mats, coarse, real=np.longdouble)(b))
    print("%s %s: ERR %.3g (recorded %.3g)" % (case, np.dtype(dtype).name, err, cases.ERR[case]))
    assert 0.5 * cases.ERR[case] <= err <= 2 * cases.ERR[case]


@pytest.mark.parametrize("case", list(cases.MODEL_ITS))
def test_recorded_counts_and_spread(case):
    """The counts of mg_cases recomputed: at most a third of Jacobi's 72, a jump of 1e4 within 3 of a jump of 100, and what the
    order of the sums does to the count."""
    H, mats, coarse = cases.setup(pkg, extras, case)
    M = cases.model(H, mats, coarse)
    A = mats[0]
    n = A.shape[0]
    b = cc.rhs(n, np.float64)
    counts = []
    for seed in cases.PERMUTATION_SEEDS:
        y, its, relres = pcg_model.solve(A, M, b, tol=cases.TOL, order=pc.order(n, seed))
        counts.append(its)
        assert np.linalg.norm(A @ y - b) <= 10 * cases.TOL * np.linalg.norm(b)
    Hh, mh, ch = cases.setup(pkg, extras, case, jump=cases.JUMP_HARD)
    hard = pcg_model.solve(mh[0], cases.model(Hh, mh, ch), b, tol=cases.TOL)[1]
    Hs, ms, cs = cases.setup(pkg, extras, case, shift=-1.0)
    shifted = pcg_model.solve(ms[0], cases.model(Hs, ms, cs, shift=-1.0), b, shift=-1.0, tol=cases.TOL)[1]
    cplx = pcg_model.solve(A, M, cc.rhs(n, np.complex128), tol=cases.TOL)[1]
    print("%s: counts %s (recorded %s), jump 1e4: %d (recorded %d), shift -1: %d (recorded %d), ComplexF64: %d; Jacobi %d"
          % (case, counts, cases.PERMUTED_ITS[case], hard, cases.HARD_ITS[case], shifted, cases.SHIFTED_ITS[case], cplx, pc.MODEL_ITS["jump"]))
    assert counts[0] == cases.MODEL_ITS[case] and tuple(counts) == cases.PERMUTED_ITS[case]
    assert 3 * counts[0] <= pc.MODEL_ITS["jump"]
    assert hard == cases.HARD_ITS[case] and abs(hard - counts[0]) <= 3
    assert shifted == cases.SHIFTED_ITS[case]
    assert abs(cplx - counts[0]) <= cases.band(case)
    for c in counts:
        assert abs(c - cases.MODEL_ITS[case]) <= cases.band(case)


def test_new_symbols_are_exported():
    import ctypes as C

    L = C.CDLL(pkg._lib.LIB_PATH)
    for sym, nargs in (("ks_operator_multigrid", 11), ("ks_operator_multigrid_info", 5), ("ks_host_multigrid_plan", 10),
                       ("ks_host_multigrid_restrict", 6), ("ks_host_multigrid_prolong_add", 5)):
        assert hasattr(L, sym) and len(pkg._lib.PROTOTYPES[sym]) == nargs
    for name in ("multigrid_operator", "host_multigrid_plan", "host_multigrid_restrict", "host_multigrid_prolong_add"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
