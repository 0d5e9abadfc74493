"""`-m gpu`: the MINRES solve operator (`ks_operator_minres`, csrc/ks_minres.hpp) from its recurrence scalars up to interior
eigenvalues of a matrix-free operator by shift-invert with the shift inside the spectrum.

References: the host matrix of every operator, a dense host solve, and the numpy model of the recurrence (tests/minres_model.py;
tests/test_minres_model_cpu.py holds the model to the same bounds without a device).  Bounds: the true residual
||(A - sigma) y - b|| <= 2 tol ||b|| (the recurrence stops at tol ||b||; the model reached 1.02 tol ||b|| at most), the error
||y - y*|| <= 2 tol ||b|| / min |lambda - sigma|, the recurrence's own residual <= tol (1 + 8 eps), and the iteration count within
`minres_cases.band(case)` of the model's -- twice what summation order alone does to the model, measured by the CPU tests.
Conventions of every product test here: the destination is poisoned with NaN, KS_GUARD=1 puts canaries around the basis, the
right-hand side is unchanged bit for bit (`test_gpu_cg_operator.Solver`)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cg_cases
import grid_cases as gc
import minres_cases as cases
import minres_model as model
import test_gpu_cg_operator as cgt
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
TOL = cases.TOL
ROUND = 1.0 + 8 * np.finfo(np.float64).eps   # |phibar| <= fl(tol beta1), then a quotient: a few roundings above tol
Solver, _bits = cgt.Solver, cgt._bits


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in cgt.ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _assert_solves(mr, A, b, what, shift=0.0, tol=TOL, its_band=None, below=None):
    """The checks of the module docstring for one solve; returns y."""
    y = Solver(mr)(b)
    info = mr.minres_info
    ystar = np.linalg.solve(np.asarray(A.todense()) - shift * np.eye(A.shape[0]), b)
    res, res_bound, err, err_bound, nbelow = cases.bounds(A, y, ystar, b, tol, shift)
    _, its, _ = model.solve(A, b, shift=shift, tol=tol)
    print("%s: %d iterations (model %d, band %s), %d eigenvalues below the shift, recurrence residual %.3g, true residual %.3g <= %.3g, "
          "error %.3g <= %.3g" % (what, info["last_iterations"], its, its_band, nbelow, info["last_relres"], res, res_bound, err, err_bound))
    assert np.all(np.isfinite(y)), what
    assert below is None or nbelow == below, (what, nbelow, below)
    assert res <= res_bound, (what, res, res_bound)
    assert err <= err_bound, (what, err, err_bound)
    assert info["last_relres"] <= tol * ROUND, (what, info)
    if its_band is not None:
        assert abs(info["last_iterations"] - its) <= its_band, (what, info, its, its_band)
    return y


# ------------------------------------------------------------------------------------------------ 1. the recurrence scalars
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", cases.DIAG_SIZES)
@pytest.mark.parametrize("values", [cases.THREE, cases.FIVE], ids=["three", "five"])
def test_distinct_eigenvalues_take_exactly_that_many_iterations(values, n, dtype, ctx):
    """diag(1, -2, 4, ...) and diag(-3, -1, 1, 2, 4, ...), indefinite, at n = 37 (below one wave), 4096 (whole packs and workgroups)
    and 70001 (odd: a half-filled pack in Float64, a ragged last workgroup, 69 workgroups of partial sums): three and five iterations,
    as in exact arithmetic.  The third is the first to use eps and w__, the second the first to use beta, v_, delta and w_: a wrong
    role of a rotating buffer or a wrong sign in a rotation leaves a residual of order one after the last of them (the model: 0.37
    to 0.65 before the last step, 1.6e-15 after it)."""
    A, b = cases.cyclic_diag(values, n, dtype), cg_cases.rhs(n, dtype)
    mr = pkg.minres_operator(pkg.csr_operator(A, ctx), tol=TOL)
    y = Solver(mr)(b)
    info = mr.minres_info
    res = np.linalg.norm(A @ y - b)
    print("n = %d: %s, true residual %.3g" % (n, info, res))
    k = len(values)
    assert info["last_iterations"] == k and info["applications"] == 1 and info["iterations"] == k, info
    assert info["last_relres"] <= TOL * ROUND
    assert res <= 2 * TOL * np.linalg.norm(b)


@pytest.mark.parametrize("n", cases.PM_SIZES)
def test_a_step_without_progress(n, ctx):
    """diag(1, -1, ...) with b = ones: alpha_1 = 0, so c' = 0 and phi = 0 -- the first step moves nothing, the second solves.
    Conjugate gradients (and conjugate residuals) divide by that zero."""
    A, b = cases.cyclic_diag(cases.PLUS_MINUS, n), np.ones(n)
    op = pkg.csr_operator(A, ctx)
    mr = pkg.minres_operator(op, tol=TOL)
    y = Solver(mr)(b)
    info = mr.minres_info
    res = np.linalg.norm(A @ y - b)
    print("n = %d: %s, true residual %.3g" % (n, info, res))
    assert info["last_iterations"] == 2, info
    assert res <= 2 * TOL * np.linalg.norm(b)
    with pytest.raises(pkg.HipError, match="not positive definite"):
        Solver(pkg.cg_operator(op, tol=TOL))(b)


# ------------------------------------------------------------------------------------------------ 2. solves
def _laplace_v(ctx):
    return cgt._laplace_v(np.float64, ctx)


def _device_case(case, ctx):
    """(host matrix, device operator, dtype) of a case of minres_cases.SOLVES."""
    if case.startswith("laplace-v"):
        return _laplace_v(ctx) + (np.float64,)
    if case == "random-csr":
        return cgt._random_csr(np.float64, ctx) + (np.float64,)
    if case == "bloch-c64":
        return cgt._bloch(np.complex128, ctx) + (np.complex128,)
    return cgt._mass(np.float64, ctx) + (np.float64,)


@pytest.mark.parametrize("case", list(cases.SOLVES))
def test_solves_against_the_host_matrix(case, ctx):
    """Shifts inside the spectrum (6, 71, 10 and 6 eigenvalues below them) and one positive definite system.  Measured on an MI355X,
    device iterations (model): 153 (153), 800 (794), 267 (260), 162 (167), 61 (61); true residuals 2.9e-11 to 3.5e-11 against bounds
    of 6.4e-11 to 9.4e-11; errors 4.0e-11 to 4.9e-10 against bounds of 2.2e-9 to 3.8e-8."""
    shift, below = cases.SOLVES[case]
    A, op, dtype = _device_case(case, ctx)
    mr = pkg.minres_operator(op, shift=shift, tol=TOL)
    assert mr.shape == op.shape and mr.dtype == op.dtype and mr.base is op
    _assert_solves(mr, A, cg_cases.rhs(A.shape[0], dtype), case, shift=shift, its_band=cases.band(case), below=below)


@pytest.mark.parametrize("path", ["csr-fused", "csr-generic"])
def test_shift_through_a_stored_matrix(path, ctx, monkeypatch):
    """(A - 1.2 I)^-1 b with A stored: the shift fused into the product, and KS_SHIFT_FUSED=0, the product and a streaming pass."""
    A, _ = _laplace_v(ctx)
    if path == "csr-generic":
        monkeypatch.setenv("KS_SHIFT_FUSED", "0")
    mr = pkg.minres_operator(pkg.csr_operator(A, ctx), shift=1.2, tol=TOL)
    _assert_solves(mr, A, cg_cases.rhs(A.shape[0], np.float64), path, shift=1.2, its_band=cases.band("laplace-v-1.2"), below=6)


# ------------------------------------------------------------------------------------------------ 3. determinism and chunking
def test_result_does_not_depend_on_chunking_or_history(ctx):
    """The shift-1.2 case with check_every = the default, 1, 3, 64: the same bits and the same count.  The same right-hand side twice
    with another in between: the same bits.  b = 0: y = 0 after 0 iterations."""
    A, op = _laplace_v(ctx)
    n = A.shape[0]
    b, b2 = cg_cases.rhs(n, np.float64), cg_cases.rhs(n, np.float64, seed=23)
    want, want_its = None, None
    for every in (0, 1, 3, 64):
        mr = pkg.minres_operator(op, shift=1.2, tol=TOL, check_every=every)
        solve = Solver(mr)
        y = solve(b)
        its = mr.minres_info["last_iterations"]
        if want is None:
            want, want_its = y, its
            assert its > 64      # (more than one chunk of every length)
        assert np.array_equal(_bits(y), _bits(want)) and its == want_its, (every, its, want_its)
        y2 = solve(b2)
        its2 = mr.minres_info["last_iterations"]
        assert not np.array_equal(_bits(y2), _bits(want))
        assert np.array_equal(_bits(solve(b)), _bits(want)) and mr.minres_info["last_iterations"] == want_its, every
        z = solve(np.zeros(n))
        info = mr.minres_info
        assert not z.any() and np.all(np.isfinite(z)) and info["last_iterations"] == 0 and info["last_relres"] == 0.0, (every, info)
        assert info["applications"] == 4 and info["iterations"] == 2 * want_its + its2, info


# ------------------------------------------------------------------------------------------------ 4. failures
def test_singular_shift_raises_and_stays_usable(ctx):
    """(I - 1.0 I) = 0: q = 0 exactly, alpha = beta' = 0, gamma = 0 in the first iteration.  No right-hand side but zero is solvable at
    this shift, so the solve that follows is that one; a second operator on the same matrix with another shift solves a real one."""
    n = 4096
    eye = pkg.csr_operator(sp.identity(n, format="csr"), ctx)
    mr = pkg.minres_operator(eye, shift=1.0, tol=TOL)
    solve = Solver(mr)
    b = cg_cases.rhs(n, np.float64)
    with pytest.raises(pkg.HipError, match=r"singular: gamma = 0 at iteration 1"):
        solve(b)
    info = mr.minres_info
    assert info["last_iterations"] == 1 and info["last_relres"] == 1.0, info
    z = solve(np.zeros(n))
    assert not z.any() and mr.minres_info["last_iterations"] == 0
    with pytest.raises(pkg.HipError, match="singular"):
        solve(b)
    half = pkg.minres_operator(eye, shift=0.5, tol=TOL)
    y = Solver(half)(b)
    assert half.minres_info["last_iterations"] == 1 and np.linalg.norm(0.5 * y - b) <= 2 * TOL * np.linalg.norm(b)


def test_maxit_and_a_right_hand_side_that_is_not_finite_raise_and_stay_usable(ctx):
    A, op = _laplace_v(ctx)
    n = A.shape[0]
    b = cg_cases.rhs(n, np.float64)
    mr = pkg.minres_operator(op, shift=1.2, tol=TOL, maxit=10)
    solve = Solver(mr)
    with pytest.raises(pkg.HipError, match=r"did not converge: relative residual \d.* after 10 iterations"):
        solve(b)
    info = mr.minres_info
    _, _, relres = model.solve(A, b, shift=1.2, tol=TOL)
    # (ten iterations in: the trajectories differ by roundings only, 1e-10 is far above what they have grown to)
    assert info["last_iterations"] == 10 and abs(info["last_relres"] - relres[10]) <= 1e-10 * relres[10], (info, relres[10])
    # an eigenvector of the shifted matrix is solved in one iteration
    lam, X = np.linalg.eigh(A.toarray())
    y = solve(X[:, 3].copy())
    assert mr.minres_info["last_iterations"] == 1
    assert np.linalg.norm(A @ y - 1.2 * y - X[:, 3]) <= 2 * TOL
    assert mr.minres_info["worst_relres"] == info["last_relres"]
    # NaN in b
    full = pkg.minres_operator(op, shift=1.2, tol=TOL)
    bad = b.copy()
    bad[17] = np.nan
    ws = pkg.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.set_col(0, bad)
    with pytest.raises(pkg.HipError, match="the right-hand side is not finite"):
        ws.apply(full, 0, 1)
    assert full.minres_info["last_iterations"] == 0
    _assert_solves(full, A, b, "after a NaN", shift=1.2, its_band=cases.band("laplace-v-1.2"))


def test_wrong_use_is_refused(ctx):
    shape = (4, 3, 2)
    n = gc.size(shape)
    t = gc.taps(3, np.float64, symmetric=True)
    A = pkg.grid_operator(shape, t, ctx=ctx)
    # operators that cannot be enqueued ahead: a host callback, a solve of either kind, a product or filter of one
    host = pkg.host_operator(lambda y, x: np.copyto(y, x), n, ctx=ctx)
    inner_cg = pkg.cg_operator(A, tol=1e-10)
    inner = pkg.minres_operator(A, tol=1e-10)
    for bad in (host, inner_cg, inner, pkg.product_operator(inner, A, ctx=ctx), pkg.chebyshev_operator(inner, 0.0, 1.0, (0.5, 1.0))):
        with pytest.raises(pkg.ArgumentError, match="cannot be enqueued ahead"):
            pkg.minres_operator(bad)
    with pytest.raises(pkg.ArgumentError, match="cannot be enqueued ahead"):
        pkg.cg_operator(inner)
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="another context"):
        pkg.minres_operator(A, ctx=other)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.minres_operator(pkg.csr_operator(pkg.host_grid_matrix(shape, t), dctx))
    for tol in (0.0, 1.0, 2.0, -1e-3, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="tol"):
            pkg.minres_operator(A, tol=tol)
    with pytest.raises(pkg.ArgumentError, match="maxit = 0"):
        pkg.minres_operator(A, maxit=0)
    with pytest.raises(pkg.ArgumentError, match="check_every = -1"):
        pkg.minres_operator(A, check_every=-1)
    for shift in (np.nan, np.inf, -np.inf):
        with pytest.raises(pkg.ArgumentError, match="shift"):
            pkg.minres_operator(A, shift=shift)
    with pytest.raises(pkg.ArgumentError):
        pkg.minres_operator(pkg.host_grid_matrix(shape, t))
    for other_op in (A, inner_cg):
        with pytest.raises(pkg.ArgumentError, match="ks_operator_minres"):
            other_op.minres_info
    with pytest.raises(pkg.ArgumentError, match="ks_operator_cg"):
        inner.cg_info
    # source and destination must differ; closing the solve leaves the operator usable
    ws = pkg.ArnoldiWorkspace(n, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(inner, 1, 1)
    inner.close()
    ws.set_col(0, np.ones(n))
    ws.apply(A, 0, 1)
    assert np.all(np.isfinite(ws.col(1)))


# ------------------------------------------------------------------------------------------------ 5. where conjugate gradients stop
def test_solves_what_conjugate_gradients_refuse(ctx):
    A, b = cg_cases.indefinite(37)
    op = pkg.csr_operator(A, ctx)
    with pytest.raises(pkg.HipError, match="not positive definite"):
        Solver(pkg.cg_operator(op, tol=TOL))(b)
    mr = pkg.minres_operator(op, tol=TOL)
    _assert_solves(mr, A, b, "indefinite(37)", its_band=2, below=1)      # (four distinct eigenvalues: four iterations in the model)
    assert mr.minres_info["last_iterations"] == 4


# ------------------------------------------------------------------------------------------------ 6. composition
def test_composes_with_device_vectors_and_products(ctx):
    A, op = _laplace_v(ctx)
    n = A.shape[0]
    mr = pkg.minres_operator(op, shift=1.2, tol=TOL)
    solve = Solver(mr)
    B = np.stack([cg_cases.rhs(n, np.float64, seed=s) for s in (1, 2, 3)], axis=1)
    singles, its = [], []
    for j in range(3):
        singles.append(solve(B[:, j]))
        its.append(mr.minres_info["last_iterations"])
    Y = pkg.DeviceVectors.from_host(B, ctx).apply(mr).download()
    for j in range(3):
        assert np.array_equal(_bits(Y[:, j]), _bits(singles[j])), j
    info = mr.minres_info
    assert info["applications"] == 6 and info["iterations"] == 2 * sum(its) and info["last_iterations"] == its[2], (info, its)
    # (A - sigma)^-1 K x with K a stored matrix: the product operator against the two steps taken one by one, and within the bounds
    Kh = cg_cases.laplace_v(v=cg_cases.potential(seed=29))
    K = pkg.csr_operator(Kh, ctx)
    x = cg_cases.rhs(n, np.float64, seed=5)
    Kx = Solver(K)(x)
    want = solve(Kx)
    prod = pkg.product_operator(mr, K, ctx=ctx)
    got = Solver(prod)(x)
    assert np.array_equal(_bits(got), _bits(want))
    assert mr.minres_info["applications"] == 8
    M = A.toarray() - 1.2 * np.eye(n)
    res, res_bound, err, err_bound, _ = cases.bounds(A, got, np.linalg.solve(M, Kh @ x), Kh @ x, TOL, 1.2)
    # (K x on the device and on the host differ by roundings: eps ||K|| ||x|| on the right-hand side, far inside the factor 2)
    assert res <= res_bound and err <= err_bound, (res, res_bound, err, err_bound)


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_interior_eigenvalues_end_to_end(ctx):
    """The four eigenvalues of -Laplacian + V on 12 x 10 x 8 nearest sigma = 1.2 -- six lie below it -- by shift-invert through MINRES
    (inner tol 1e-13, outer tol 1e-10, which = LM) with every vector in HBM.  lambda = sigma + 1 / mu equals the four eigenvalues of
    the host matrix nearest sigma; A is Hermitian, so each lies within r_j / ||x_j|| of an eigenvalue, r_j = ||A x_j - lambda_j x_j||
    against the ORIGINAL operator, plus what numpy's eigvalsh itself is good for (n eps ||A|| = 2.6e-12).

    Measured on an MI355X: converged in 20 products, 3 125 inner iterations (133 in the last solve, worst recurrence residual
    9.9e-14); lambda = 1.17667701, 1.23612875, 1.12478146, 1.30622545 in the order of |mu|; ||A x - lambda x|| = 4.7e-15, 4.2e-15,
    4.6e-13, 1.8e-10; |lambda - eigvalsh| = 3.6e-15, 8.4e-15, 2.8e-14, 6.0e-14."""
    sigma = 1.2
    Ah, A = _laplace_v(ctx)
    n = Ah.shape[0]
    ev = np.linalg.eigvalsh(Ah.toarray())
    nearest = np.sort(np.argsort(np.abs(ev - sigma))[:4])
    assert np.allclose(ev[nearest], [1.12478146, 1.17667701, 1.23612875, 1.30622545], rtol=0, atol=5e-9)
    S = pkg.minres_operator(A, shift=sigma, tol=1e-13)
    P, hist = pkg.partialschur(S, v1=pkg.matrices.start_vector(n), nev=4, which="LM", tol=1e-10)
    assert hist.converged and P.nconverged >= 4, hist
    mu, X = pkg.partialeigen(P, device=True)
    assert np.all(np.imag(mu) == 0)
    lam = np.ascontiguousarray(extras.interior_eigenvalues(np.real(mu), sigma))
    r, _ = pkg.residuals(A, X, lam)
    xn = np.sqrt(np.real(np.diag(pkg.gram(X, X))))
    floor = n * np.finfo(np.float64).eps * np.abs(ev).max()
    radius = r / xn + floor
    info = S.minres_info
    print("%s; minres %s; lambda = %s, ||A x - lambda x|| = %s, inclusion radius = %s, |lambda - ev| = %s"
          % (hist, info, lam, r, radius, [float(np.abs(ev - lj).min()) for lj in lam]))
    found = []
    for lj, rad in zip(lam, radius):
        j = int(np.argmin(np.abs(ev - lj)))
        assert abs(ev[j] - lj) <= rad, (lj, ev[j], rad)
        found.append(j)
    order = np.argsort(-np.abs(np.real(mu)))[:4]
    assert sorted(found[i] for i in order) == list(nearest), (found, nearest)
    assert info["applications"] >= hist.mvproducts and info["worst_relres"] <= 1e-13 * ROUND
