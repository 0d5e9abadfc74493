"""`-m gpu`: the geometric multigrid V-cycle operator (`ks_operator_multigrid`, csrc/ks_mg.hpp), from its transfer and smoother
kernels up to a shift-invert eigenproblem preconditioned by it.

References: the host transfers (`host_multigrid_restrict` / `_prolong_add`, held to the definition by tests/test_mg_model_cpu.py),
closed forms of the Chebyshev polynomial, the numpy model of the cycle (tests/mg_model.py) and of preconditioned conjugate
gradients (tests/pcg_model.py).  Bounds: equal BITS where the device runs only individually rounded operations (degree 1 on diagonal
level operators), 4 ERR of tests/mg_cases.py for the whole cycle, the iteration bands of mg_cases.  Conventions of every product
test here: the destination is poisoned with NaN, KS_GUARD=1 puts canaries around the basis."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import cg_cases as cc
import mg_cases as cases
import mg_model
import pcg_cases as pc
import pcg_model
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
EPS = np.finfo(np.float64).eps
ENV = ("KS_SHIFT_FUSED", "KS_SHIFT_PLAIN", "KS_SPMV_FORMAT", "KS_SSTEP", "KS_PCG_FUSED")


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Solver:
    """One operator on one workspace: column 0 = b, column 1 = the (poisoned) destination."""

    def __init__(self, op):
        self.op = op
        self.ws = pkg.ArnoldiWorkspace(op.shape[0], 1, op.dtype, ctx=op.ctx)
        self.poison = np.full(op.shape[0], np.nan, dtype=op.dtype)

    def __call__(self, b):
        b = np.asarray(b, dtype=self.op.dtype)
        self.ws.set_col(0, b)
        self.ws.set_col(1, self.poison)
        self.ws.apply(self.op, 0, 1)
        assert self.ws.guard_intact()
        assert np.array_equal(_bits(self.ws.col(0)), _bits(b)), "the right-hand side was written"
        return self.ws.col(1)


def _scale(d, v):
    """d o v with a real d, part by part: one rounded product per part, as the diagonal operator and the smoother form it."""
    v = np.asarray(v)
    if v.dtype.kind == "c":
        return (d * v.real) + 1j * (d * v.imag)
    return d * v


# ------------------------------------------------------------------------------------------------ 1. the transfers alone
@pytest.mark.parametrize("variant", ["restriction-alone", "whole-cycle"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fine,coarse", cases.TRANSFER_PAIRS, ids=cases.TRANSFER_IDS)
def test_transfers_carry_the_bits_of_the_host_functions(fine, coarse, dtype, variant, ctx):
    """Two levels, degree 1, diagonal operators on both: every step of the cycle is one individually rounded operation per entry, so
    numpy and the host transfers reproduce the device bit for bit --
        x1 = b0 (dinv o b);  r_c = R(b - a o x1);  x2 = x1 + P (e o r_c);  y = x2 + b0 (dinv o (b - a o x2)).
    "restriction-alone": dinv = 2^-200 and e = 1 make x1 and the post-smoothing step vanish against P r_c: y holds the very bits of
    the coarse right-hand side, prolonged -- every coarse cell of every workgroup of the restriction is seen on its fine rows.
    On mg_cases.TRANSFER_PAIRS: the first two levels of every case and one pair per branch of the two kernels (workgroups past the
    first, kept axes, a single coarse x-cell, unaligned lines), as tests/test_mg_model_cpu.py computes from the shapes."""
    nf, nc = cc.size(fine), cc.size(coarse)
    rng = np.random.default_rng(nf)
    a = 0.5 + rng.random(nf)
    if variant == "restriction-alone":
        dinv, e = np.full(nf, 2.0 ** -200), np.ones(nc)
    else:
        dinv, e = (0.5 + rng.random(nf)) / a, 0.5 + rng.random(nc)
    lam, ratio = 1.0, 4.0
    b0 = pkg.host_multigrid_plan([fine, coarse], [lam], degree=1, ratio=ratio)["b"][0, 0]
    M = pkg.multigrid_operator([pkg.diagonal_operator(a, dtype, ctx)], [fine, coarse], [dinv], [lam], pkg.diagonal_operator(e, dtype, ctx),
                               degree=1, ratio=ratio)
    assert M.shape == (nf, nf) and M.dtype == np.dtype(dtype)
    b = cc.rhs(nf, dtype)
    y = Solver(M)(b)
    x1 = b0 * _scale(dinv, b)
    rc = pkg.host_multigrid_restrict(fine, coarse, b, _scale(a, x1))
    x2 = pkg.host_multigrid_prolong_add(fine, coarse, _scale(e, rc), x1)
    want = x2 + b0 * _scale(dinv, b - _scale(a, x2))
    assert np.array_equal(_bits(y), _bits(want.astype(dtype))), np.abs(y - want).max()
    if variant == "restriction-alone":
        assert np.array_equal(_bits(y), _bits(pkg.host_multigrid_prolong_add(fine, coarse, rc, np.zeros(nf, dtype=dtype))))
    info = M.multigrid_info
    assert info == dict(levels=2, rows=(nf, nc), applications=1, level_products=(2,), coarse_applications=1), info


def _diagonal_chain(shapes, a, dinv, b0, e, b, l=0):
    """cycle_l(b) of a chain of diagonal levels at degree 1, every operation rounded once in the order of the device:
        l == L: e o b;  x1 = b0_l (dinv_l o b);  r_c = R(b - a_l o x1);  x2 = x1 + P cycle_{l+1}(r_c);  x2 + b0_l (dinv_l o (b - a_l o x2))."""
    if l == len(shapes) - 1:
        return _scale(e, b)
    x1 = b0[l] * _scale(dinv[l], b)
    rc = pkg.host_multigrid_restrict(shapes[l], shapes[l + 1], b, _scale(a[l], x1))
    x2 = pkg.host_multigrid_prolong_add(shapes[l], shapes[l + 1], _diagonal_chain(shapes, a, dinv, b0, e, rc, l + 1), x1)
    return x2 + b0[l] * _scale(dinv[l], b - _scale(a[l], x2))


_HALVINGS = [(2 ** k + 1,) for k in range(15, 0, -1)] + [(2,)]     # 32769 -> 16385 -> ... -> 3 -> 2: the 16 levels the plan accepts
CHAINS = {
    # 2 604 and 384 coarse rows: 11 and 2 restriction workgroups, each with a partial last one, on levels of mixed parity
    "three-3d": [(61, 23, 13), (31, 12, 7), (16, 6, 4)],
    # y kept, then z kept: the kept and the halved axes change from level to level
    "kept-then-halved": [(45, 19, 7), (23, 19, 4), (12, 10, 4)],
    "sixteen-1d": _HALVINGS,
}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_a_chain_of_diagonal_levels_carries_the_bits_of_the_recursion(chain, dtype, ctx):
    """The two-level closed form of test_transfers_carry_the_bits_of_the_host_functions, recursively: degree 1 and a diagonal operator
    on every level, so numpy and the host transfers reproduce the device bit for bit at any depth.  Unlike the whole-cycle tests
    this holds the right-hand sides and solutions of the levels l >= 1 (rhs[l + 1], sol[l + 1] of csrc/ks_mg.hpp) to the bit: a
    wrong value in any of them reaches y through the prolongations.  Each level has a bound of its own, so a coefficient taken from
    another level shows.  The second application runs on temporaries the first one has written."""
    shapes = CHAINS[chain]
    rows = [cc.size(s) for s in shapes]
    L = len(shapes) - 1
    rng = np.random.default_rng(rows[0])
    a = [0.5 + rng.random(n) for n in rows[:-1]]
    dinv = [(0.5 + rng.random(n)) / a[l] for l, n in enumerate(rows[:-1])]
    e = 0.5 + rng.random(rows[-1])
    bounds = [1.0 + 0.125 * l for l in range(L)]
    b0 = pkg.host_multigrid_plan(shapes, bounds, degree=1, ratio=4.0)["b"][:, 0]
    assert len(set(b0)) == L
    M = pkg.multigrid_operator([pkg.diagonal_operator(v, dtype, ctx) for v in a], shapes, dinv, bounds, pkg.diagonal_operator(e, dtype, ctx),
                               degree=1, ratio=4.0)
    b = cc.rhs(rows[0], dtype)
    want = _diagonal_chain(shapes, a, dinv, b0, e, b).astype(dtype)
    assert np.all(np.isfinite(want.view(np.float64))) and np.all(want.view(np.float64) != 0.0)
    solve = Solver(M)
    y = solve(b)
    assert np.array_equal(_bits(y), _bits(want)), np.abs(y - want).max()
    assert M.multigrid_info == dict(levels=L + 1, rows=tuple(rows), applications=1, level_products=(2,) * L, coarse_applications=1)
    assert np.array_equal(_bits(solve(b)), _bits(want))
    assert M.multigrid_info == dict(levels=L + 1, rows=tuple(rows), applications=2, level_products=(4,) * L, coarse_applications=2)


# ------------------------------------------------------------------------------------------------ 2. the smoother in closed form
def _cheb(k, s):
    t0, t1 = 1.0, s
    for _ in range(k):
        t0, t1 = t1, 2.0 * s * t1 - t0
    return t0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [37, 4096, 70001])
def test_exact_smoother_gives_the_closed_form_polynomial(n, degree, dtype, ctx):
    """A = D, dinv = 1 / d, lambda = 1: B = I, every Chebyshev step scales the error by a number.  With a coarse operator of zeros the
    cycle is post- after pre-smoothing: y = (1 - q^2) b / d with q = T_k((thc - 1) / del) / T_k(thc / del) the residual polynomial
    at 1; degree 1: q = 1 - 1 / thc.  The bound: an error in x is carried on by 1 - b_j, below 1 in magnitude, so only the roundings of
    a step count, in units of eps |b / d| with |x|, |t| <= 1.6, |rhs - t| <= 0.6, b_j <= 2: t 0.8 b_j, rhs - t and dinv o 0.3 b_j each,
    the products by b_j and the fma 0.5 each, x + d 0.8 -- at most 4.6 per step, 9.2 k for the 2 k steps, over a result of at least
    (1 - 0.36) |b / d|: 16 k eps.  n = 37 (below one wave), 4096 and 70001 (odd: a half-filled pack in Float64, a ragged last
    workgroup) on (n,) -> (ceil(n / 2),)."""
    rng = np.random.default_rng(n)
    d = 0.5 + rng.random(n)
    nc = (n + 1) // 2
    ratio = 4.0
    thc, dl = (1.0 + 1.0 / ratio) / 2.0, (1.0 - 1.0 / ratio) / 2.0
    q = _cheb(degree, (thc - 1.0) / dl) / _cheb(degree, thc / dl)
    if degree == 1:
        assert q == pytest.approx(1.0 - 1.0 / thc, rel=4 * EPS)
    M = pkg.multigrid_operator([pkg.diagonal_operator(d, dtype, ctx)], [(n,), (nc,)], [1.0 / d], [1.0], pkg.diagonal_operator(np.zeros(nc), dtype, ctx),
                               degree=degree, ratio=ratio)
    b = cc.rhs(n, dtype)
    y = Solver(M)(b)
    want = (1.0 - q * q) * b / d
    err = np.abs(y - want).max() / np.abs(want).max()
    print("n = %d, degree %d: |y - (1 - q^2) b / d| = %.3g of max" % (n, degree, err))
    assert np.all(np.abs(y - want) <= 16 * degree * EPS * np.abs(want)), err
    info = M.multigrid_info
    assert info["level_products"] == ((2 * degree - 1) + 1,) and info["applications"] == 1 and info["coarse_applications"] == 1, info
    Solver(M)(b)
    assert M.multigrid_info["level_products"] == (4 * degree,)


# ------------------------------------------------------------------------------------------------ 3. no smoothed level
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_without_smoothed_levels_the_cycle_is_the_coarse_operator(dtype, ctx):
    n = 37
    rng = np.random.default_rng(n)
    C = rng.standard_normal((n, n)).astype(dtype)
    b = cc.rhs(n, dtype)
    for coarse in (pkg.dense_operator(C, ctx), pkg.diagonal_operator(rng.standard_normal(n), dtype, ctx)):
        M = pkg.multigrid_operator([], [(n,)], [], [], coarse)
        assert np.array_equal(_bits(Solver(M)(b)), _bits(Solver(coarse)(b)))
        assert M.multigrid_info == dict(levels=1, rows=(n,), applications=1, level_products=(), coarse_applications=1)


# ------------------------------------------------------------------------------------------------ 4. the whole cycle
@functools.lru_cache(maxsize=None)
def _case(case, shift=0.0, jump=cases.JUMP):
    return cases.setup(pkg, extras, case, jump=jump, shift=shift)


def _device_cycle(case, dtype, ctx, shift=0.0, degree=cases.DEGREE, ratio=cases.RATIO, bound_factor=1.0, jump=cases.JUMP, stored=False):
    """`stored`: the level operators are the stored matrices `csr_operator(mats[l])` instead of the matrix-free grid operators."""
    H, mats, coarse = _case(case, shift, jump)
    if stored:
        ops = [pkg.csr_operator(m.astype(dtype), ctx) for m in mats[:-1]]
    else:
        ops = [pkg.grid_variable_operator(L["shape"], L["taps"], L["coeff"], L["diagonal"], dtype=dtype, ctx=ctx) for L in H[:-1]]
    M = pkg.multigrid_operator(ops, [L["shape"] for L in H], [L["inverse_diagonal"] for L in H[:-1]], [bound_factor * L["bound"] for L in H[:-1]],
                               pkg.dense_operator(coarse.astype(dtype), ctx), shift=shift, degree=degree, ratio=ratio)
    assert M.levels == tuple(ops) and M.dtype == np.dtype(dtype)
    return M, ops[0]


@functools.lru_cache(maxsize=None)
def _exact_cycle(case, dtype):
    """(b, M b of the numpy model in np.longdouble, M b of the Float64 model): computed once, read only."""
    H, mats, coarse = _case(case)
    b = cases.rhs(case, dtype)
    out = b, cases.model(H, mats, coarse, real=np.longdouble)(b), cases.model(H, mats, coarse)(b)
    for v in out:
        v.setflags(write=False)
    return out


def _check_whole_cycle(case, dtype, ctx, stored):
    M, _ = _device_cycle(case, dtype, ctx, stored=stored)
    b, exact, model = _exact_cycle(case, dtype)
    y = Solver(M)(b)
    err, err_model = cases.rel_err(y, exact), cases.rel_err(model, exact)
    print("%s %s%s: device %.3g, Float64 model %.3g, ERR %.3g, allowed %.3g"
          % (case, np.dtype(dtype).name, ", stored matrices" if stored else "", err, err_model, cases.ERR[case], 4 * cases.ERR[case]))
    assert np.all(np.isfinite(y))
    assert err <= 4 * cases.ERR[case], (err, cases.ERR[case])
    info = M.multigrid_info
    assert info["rows"] == tuple(cc.size(s) for s in cases.LEVEL_SHAPES[case])
    assert info["level_products"] == (2 * cases.DEGREE,) * (len(cases.LEVEL_SHAPES[case]) - 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_whole_cycle_against_the_model(case, dtype, ctx):
    """M b against the numpy model evaluated in np.longdouble: the Float64 model lies ERR[case] from it (mg_cases), the device may
    lie 4 ERR from it."""
    _check_whole_cycle(case, dtype, ctx, stored=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["three-level", "wide"])
def test_whole_cycle_with_stored_matrices_as_level_operators(case, dtype, ctx):
    """The cycle is generic in its level operators: the same matrices as `csr_operator`s give the same map with another order of the
    sums inside a product, so the same bound of 4 ERR holds."""
    _check_whole_cycle(case, dtype, ctx, stored=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["three-level", "odd", "long-x"])
def test_cycle_is_symmetric_positive_and_reproducible(case, dtype, ctx):
    """<u, M v> = <M u, v> through `gram` on eight random columns, to the bound the model is held to (64 eps of the largest entry);
    u^H M u > 0; equal bits on a second application and after an unrelated operator ran in between."""
    M, A = _device_cycle(case, dtype, ctx)
    n = M.shape[0]
    rng = np.random.default_rng(n)
    U = rng.standard_normal((n, 8)) + (1j * rng.standard_normal((n, 8)) if np.dtype(dtype).kind == "c" else 0.0)
    X = pkg.DeviceVectors.from_host(np.asfortranarray(U.astype(dtype)), ctx)
    MX = X.apply(M)
    G = pkg.gram(X, MX)
    asym = np.abs(G - G.conj().T).max() / np.abs(G).max()
    print("%s %s: asymmetry %.3g, min u^H M u %.3g" % (case, np.dtype(dtype).name, asym, np.diag(G).real.min()))
    assert asym <= 64 * EPS
    assert np.all(np.diag(G).real > 0) and np.all(np.linalg.eigvalsh(0.5 * (G + G.conj().T)) > 0)
    first = MX.download()
    assert np.array_equal(_bits(X.apply(M).download()), _bits(first))
    solve = Solver(M)
    y = solve(U[:, 3])
    assert np.array_equal(_bits(y), _bits(first[:, 3]))
    other = pkg.multigrid_operator([A], cases.LEVEL_SHAPES[case][:2], [np.ones(n)], [9.0],
                                   pkg.diagonal_operator(np.ones(cc.size(cases.LEVEL_SHAPES[case][1])), dtype, ctx), degree=3, ratio=2.0)
    Solver(other)(U[:, 5])
    Solver(A)(U[:, 6])
    assert np.array_equal(_bits(solve(U[:, 3])), _bits(y))


# ------------------------------------------------------------------------------------------------ 5. as the preconditioner of pcg_operator
def _assert_solution(A, y, b, shift, tol):
    res = np.linalg.norm(A @ y - shift * y - b)
    assert np.all(np.isfinite(y)) and res <= 10 * tol * np.linalg.norm(b), (res, tol * np.linalg.norm(b))
    return res


@pytest.mark.parametrize("shift", [0.0, -1.0], ids=["shift0", "shift-1"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", list(cases.MODEL_ITS))
def test_pcg_with_the_cycle_on_the_coefficient_jump(case, dtype, shift, ctx):
    """pcg_operator(A, M) on "jump": the count within max(2 SPREAD, 1) of the model's and at most a third of Jacobi's, measured on
    the device in this test; ||(A - shift) y - b|| <= 10 tol ||b||; the generic path; one application of the cycle per application of
    the preconditioner."""
    H, mats, coarse = _case(case, shift)
    M, A = _device_cycle(case, dtype, ctx, shift=shift)
    b = cases.rhs(case, dtype)
    _, its_model, _ = pcg_model.solve(mats[0], cases.model(H, mats, coarse, shift=shift), b, shift=shift, tol=cases.TOL)
    recorded = cases.MODEL_ITS[case] if shift == 0.0 else cases.SHIFTED_ITS[case]
    pcg = pkg.pcg_operator(A, M, shift=shift, tol=cases.TOL)
    y = Solver(pcg)(b)
    info = pcg.pcg_info
    jac = pkg.pcg_operator(A, extras.jacobi_preconditioner(H[0]["diagonal"], shift=shift, dtype=dtype, ctx=ctx), shift=shift, tol=cases.TOL)
    yj = Solver(jac)(b)
    its, its_jacobi = info["last_iterations"], jac.pcg_info["last_iterations"]
    res = _assert_solution(mats[0], y, b, shift, cases.TOL)
    print("%s %s shift %g: %d iterations (model %d, recorded %d), Jacobi on the device %d; residual %.3g; %s; %s"
          % (case, np.dtype(dtype).name, shift, its, its_model, recorded, its_jacobi, res, info, M.multigrid_info))
    assert abs(its_model - recorded) <= cases.band(case)
    assert abs(its - its_model) <= cases.band(case), (its, its_model)
    assert 3 * its <= its_jacobi, (its, its_jacobi)
    assert info["path"] == "generic" and info["last_relres"] <= cases.TOL * (1.0 + 8 * EPS)
    assert info["preconditioner_applications"] == M.multigrid_info["applications"] >= its + 1
    _assert_solution(mats[0], yj, b, shift, cases.TOL)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_larger_jump_moves_the_count_by_at_most_three(dtype, ctx):
    H, mats, coarse = _case("three-level", 0.0, cases.JUMP_HARD)
    M, A = _device_cycle("three-level", dtype, ctx, jump=cases.JUMP_HARD)
    b = cases.rhs("three-level", dtype)
    pcg = pkg.pcg_operator(A, M, tol=cases.TOL)
    y = Solver(pcg)(b)
    its = pcg.pcg_info["last_iterations"]
    print("jump 1e4: %d iterations (recorded for the model: %d; jump 100: %d)" % (its, cases.HARD_ITS["three-level"], cases.MODEL_ITS["three-level"]))
    _assert_solution(mats[0], y, b, 0.0, cases.TOL)
    assert abs(its - cases.HARD_ITS["three-level"]) <= cases.band("three-level") and abs(its - cases.MODEL_ITS["three-level"]) <= 3 + cases.band("three-level")


def test_the_recipe_builds_the_same_cycle(ctx):
    """extras.grid_multigrid_preconditioner against the cycle assembled by hand from the same hierarchy: equal bits."""
    shape, rows = cases.CASES["three-level"]
    M = extras.grid_multigrid_preconditioner(shape, pc.jump_coeff(shape), coarsest_rows=rows, ctx=ctx)
    hand, _ = _device_cycle("three-level", np.float64, ctx)
    b = cases.rhs("three-level", np.float64)
    assert [L["shape"] for L in M.hierarchy] == cases.LEVEL_SHAPES["three-level"] and M.multigrid_info["rows"] == (960, 120, 18)
    assert np.array_equal(_bits(Solver(M)(b)), _bits(Solver(hand)(b)))
    Mc = extras.grid_multigrid_preconditioner(shape, pc.jump_coeff(shape), coarsest_rows=rows, dtype=np.complex128, ctx=ctx)
    handc, _ = _device_cycle("three-level", np.complex128, ctx)
    bc = cases.rhs("three-level", np.complex128)
    assert Mc.dtype == np.dtype(np.complex128) and np.array_equal(_bits(Solver(Mc)(bc)), _bits(Solver(handc)(bc)))


# ------------------------------------------------------------------------------------------------ 6. refusals and failures
def test_wrong_use_is_refused(ctx):
    fine, coarse = (6, 4), (3, 2)
    A, Cz = pkg.diagonal_operator(np.ones(24), ctx=ctx), pkg.diagonal_operator(np.ones(6), ctx=ctx)
    good = dict(operators=[A], shapes=[fine, coarse], inverse_diagonals=[np.ones(24)], bounds=[1.0], coarse=Cz)

    def make(**kw):
        return pkg.multigrid_operator(**{**good, **kw})

    assert make().multigrid_info["rows"] == (24, 6)
    with pytest.raises(pkg.ArgumentError, match=r"the operator of level 0 has 24 rows, the extents 6 x 5 x 1 of level 0 give 30"):
        make(shapes=[(6, 5), (3, 3)], inverse_diagonals=[np.ones(30)], coarse=pkg.diagonal_operator(np.ones(9), ctx=ctx))
    with pytest.raises(pkg.ArgumentError, match=r"the coarse operator has 6 rows, the extents 3 x 4 x 1 of level 1 give 12"):
        make(shapes=[fine, (3, 4)])
    with pytest.raises(pkg.ArgumentError, match=r"axis 1 must keep its extent 4 or halve it to 2"):
        make(shapes=[fine, (3, 3)])
    with pytest.raises(pkg.ArgumentError, match="the same extents"):
        make(shapes=[fine, fine], coarse=pkg.diagonal_operator(np.ones(24), ctx=ctx))
    with pytest.raises(pkg.ArgumentError, match="the operator of level 0 does not have the element type of the coarse operator"):
        make(coarse=pkg.diagonal_operator(np.ones(6), np.complex128, ctx=ctx))
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="the operator of level 0 lives on another context"):
        make(operators=[pkg.diagonal_operator(np.ones(24), ctx=other)])
    with pytest.raises(pkg.ArgumentError, match="the coarse operator lives on another context"):
        make(coarse=pkg.diagonal_operator(np.ones(6), ctx=other), ctx=ctx)
    host = pkg.host_operator(lambda y, x: np.copyto(y, x), 24, ctx=ctx)
    inner = pkg.cg_operator(A, tol=1e-10)
    for bad in (host, inner):
        with pytest.raises(pkg.ArgumentError, match="the operator of level 0 cannot be enqueued ahead"):
            make(operators=[bad])
    with pytest.raises(pkg.ArgumentError, match="the coarse operator cannot be enqueued ahead"):
        make(coarse=pkg.cg_operator(Cz, tol=1e-10))
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.multigrid_operator([pkg.diagonal_operator(np.ones(24), ctx=dctx)], [fine, coarse], [np.ones(24)], [1.0],
                               pkg.diagonal_operator(np.ones(6), ctx=dctx))
    chain = [(2 ** 17,)]
    while len(chain) < 17:
        chain.append(((chain[-1][0] + 1) // 2,))
    with pytest.raises(pkg.ArgumentError, match="17 levels"):
        pkg.multigrid_operator([A] * 16, chain, [np.ones(cc.size(s)) for s in chain[:-1]], [1.0] * 16, Cz)
    for degree in (0, -2):
        with pytest.raises(pkg.ArgumentError, match="degree = %d" % degree):
            make(degree=degree)
    for ratio in (1.0, 0.25, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="ratio = "):
            make(ratio=ratio)
    for lam in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="level 0: lambda_max = "):
            make(bounds=[lam])
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = np.ones(24)
        d[13] = bad
        with pytest.raises(pkg.ArgumentError, match="level 0: inv_diag entry 13 = "):
            make(inverse_diagonals=[d])
    with pytest.raises(pkg.ArgumentError, match="shift is not finite"):
        make(shift=np.nan)
    for kw in (dict(operators=[None]), dict(coarse=None), dict(operators=[np.ones((24, 24))]), dict(inverse_diagonals=None)):
        with pytest.raises(pkg.ArgumentError):
            make(**kw)
    for kw in (dict(shapes=[fine]), dict(bounds=[1.0, 2.0]), dict(inverse_diagonals=[np.ones(23)]), dict(inverse_diagonals=[])):
        with pytest.raises(pkg.DimensionMismatch):
            make(**kw)
    for op in (A, inner):
        with pytest.raises(pkg.ArgumentError, match="ks_operator_multigrid_info"):
            op.multigrid_info
    # source and destination must differ; closing the cycle leaves its operators usable
    M = make()
    ws = pkg.ArnoldiWorkspace(24, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(M, 1, 1)
    M.close()
    ws.set_col(0, np.arange(24.0))
    ws.apply(A, 0, 1)
    assert np.array_equal(ws.col(1), np.arange(24.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_bound_far_too_small_fails_or_slows_down_and_leaves_everything_usable(dtype, ctx):
    """lambda = 0.1 x the Gershgorin bound: the smoother's polynomial exceeds 1 on the upper spectrum, the cycle need not be positive
    definite.  pcg_operator then raises "the preconditioner is not positive definite" (or "did not converge"), or converges more
    slowly; either way the operators stay usable and nothing hangs."""
    H, mats, coarse = _case("three-level")
    bad, A = _device_cycle("three-level", dtype, ctx, bound_factor=0.1)
    good, _ = _device_cycle("three-level", dtype, ctx)
    b = cases.rhs("three-level", dtype)
    pcg = pkg.pcg_operator(A, bad, tol=cases.TOL, maxit=200)
    solve = Solver(pcg)
    try:
        y = solve(b)
        outcome = "converged in %d iterations" % pcg.pcg_info["last_iterations"]
        _assert_solution(mats[0], y, b, 0.0, cases.TOL)
    except pkg.HipError as e:
        outcome = str(e)
        assert "the preconditioner is not positive definite" in outcome or "did not converge" in outcome or "not positive definite" in outcome
    print("bound x 0.1: %s" % outcome)
    z = solve(np.zeros(b.size, dtype=dtype))
    assert not z.any() and pcg.pcg_info["last_iterations"] == 0
    assert np.all(np.isfinite(Solver(bad)(b)))
    ok = pkg.pcg_operator(A, good, tol=cases.TOL)
    _assert_solution(mats[0], Solver(ok)(b), b, 0.0, cases.TOL)
    assert abs(ok.pcg_info["last_iterations"] - cases.MODEL_ITS["three-level"]) <= cases.band("three-level")


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_shift_invert_with_the_multigrid_preconditioner_end_to_end(ctx):
    """The recipe of the README on 12 x 10 x 8: S = (A - sigma)^-1 by conjugate gradients preconditioned with
    extras.grid_multigrid_preconditioner, partialschur(S, nev=4, which="LM") -- the four eigenvalues the Jacobi recipe of
    tests/test_gpu_pcg_operator.py finds, within their residual bounds, in fewer inner iterations."""
    shape = pc.SHAPE
    c = pc.jump_coeff()
    taps, d = extras.diffusion_terms(shape, c, 1.0, None)
    Hm = pkg.host_grid_variable_matrix(shape, taps, c, d)
    n = Hm.shape[0]
    sigma = 0.0
    ev = sla.eigh(Hm.toarray(), eigvals_only=True)
    A = pkg.grid_variable_operator(shape, taps, c, d, ctx=ctx)
    M = extras.grid_multigrid_preconditioner(shape, c, shift=sigma, coarsest_rows=64, ctx=ctx)
    S = pkg.pcg_operator(A, M, shift=sigma, tol=1e-13)
    v1 = pkg.matrices.start_vector(n)
    P, hist = pkg.partialschur(S, v1=v1, nev=4, which="LM", tol=1e-10)
    assert hist.converged and P.nconverged >= 4, hist
    mu, X = pkg.partialeigen(P, device=True)
    assert np.all(np.imag(mu) == 0)
    lam = np.ascontiguousarray(extras.interior_eigenvalues(np.real(mu), sigma))
    r, _ = pkg.residuals(A, X, lam)
    xn = np.sqrt(np.real(np.diag(pkg.gram(X, X))))
    info = S.pcg_info
    print("%s; pcg %s; multigrid %s; lambda = %s, ||A x - lambda x|| = %s" % (hist, info, M.multigrid_info, lam, r))
    found = []
    for lj, rj, nj in zip(lam, r, xn):
        j = int(np.argmin(np.abs(ev - lj)))
        assert abs(ev[j] - lj) <= rj / nj, (lj, ev[j], rj / nj)
        found.append(j)
    order = np.argsort(-np.abs(np.real(mu)))[:4]
    assert sorted(found[i] for i in order) == [0, 1, 2, 3], found
    assert np.all(r / xn <= 1e-8)
    assert info["path"] == "generic" and info["worst_relres"] <= 1e-13 * (1.0 + 8 * EPS)
    assert info["preconditioner_applications"] == M.multigrid_info["applications"]
    SJ = pkg.pcg_operator(A, extras.jacobi_preconditioner(d, shift=sigma, ctx=ctx), shift=sigma, tol=1e-13)
    PJ, histJ = pkg.partialschur(SJ, v1=v1, nev=4, which="LM", tol=1e-10)
    muJ, _ = pkg.partialeigen(PJ, device=True)
    print("Jacobi: %s; %s" % (histJ, SJ.pcg_info))
    assert histJ.converged and PJ.nconverged >= 4
    lamJ = np.sort(extras.interior_eigenvalues(np.real(muJ), sigma))[:4]
    assert np.allclose(np.sort(lam)[:4], lamJ, rtol=1e-8, atol=0)
    assert info["iterations"] < SJ.pcg_info["iterations"], (info["iterations"], SJ.pcg_info["iterations"])
