"""`-m gpu`: the preconditioned conjugate-gradient solve operator (`ks_operator_pcg`, csrc/ks_pcg.hpp) and the diagonal operator
(`ks_operator_diagonal`), from the recurrence scalars up to a shift-invert eigenproblem on a coefficient jump.

References: the host matrix of every operator, a direct host solve, and the numpy models of the recurrences (tests/pcg_model.py,
tests/cg_model.py; tests/test_pcg_model_cpu.py holds the models to the same bounds without a device).  Bounds: those of
tests/test_gpu_cg_operator.py (`cg_cases.bounds`: true residual <= 2 tol ||b||, error <= 2 tol ||b|| / lambda_min), exact iteration
counts where exact arithmetic gives one, the bands of tests/pcg_cases.py elsewhere, and equal BITS between the fused Jacobi path and
the generic one.  Conventions of every product test here: the destination is poisoned with NaN, KS_GUARD=1 puts canaries around the
basis."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import cg_cases as cc
import cg_model
import pcg_cases as cases
import pcg_model as model
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
PATHS = ["jacobi", "generic"]
TOL = cc.TOL
ROUND = 1.0 + 8 * np.finfo(np.float64).eps   # rho' <= fl(fl(tol^2) rho0), then a quotient and a root: a few roundings above tol
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


def _pcg(A, M, path, monkeypatch, **kw):
    """pcg_operator on the asked path: a diagonal M is fused unless KS_PCG_FUSED=0 says otherwise at creation."""
    if path == "generic":
        monkeypatch.setenv("KS_PCG_FUSED", "0")
    op = pkg.pcg_operator(A, M, **kw)
    monkeypatch.delenv("KS_PCG_FUSED", raising=False)
    assert op.pcg_info["path"] == path and op.base is A and op.preconditioner is M and op.shape == A.shape and op.dtype == A.dtype
    return op


def _assert_bounds(op, A, b, what, shift=0.0, tol=TOL):
    """One solve against the host matrix: cg_cases.bounds and the recurrence's residual; returns (y, iterations)."""
    y = Solver(op)(b)
    info = op.pcg_info
    ystar = np.linalg.solve(np.asarray(A.todense()) - shift * np.eye(A.shape[0]), b)
    res, res_bound, err, err_bound = cc.bounds(A, y, ystar, b, tol, shift)
    print("%s: %s, true residual %.3g <= %.3g, error %.3g <= %.3g" % (what, info, res, res_bound, err, err_bound))
    assert np.all(np.isfinite(y)), what
    assert res <= res_bound, (what, res, res_bound)
    assert err <= err_bound, (what, err, err_bound)
    assert info["last_relres"] <= tol * ROUND, (what, info)
    return y, info["last_iterations"]


# ------------------------------------------------------------------------------------------------ 1. exact counts
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", cc.DIAG_SIZES)
def test_two_clusters_take_exactly_two_iterations_and_the_inverse_one(n, dtype, path, ctx, monkeypatch):
    """diag(1, 2, 4, ...) at n = 37 (below one wave), 4096 (whole packs and workgroups) and 70001 (odd: a half-filled pack in Float64,
    a ragged last workgroup, 69 workgroups of partial sums).  M = diag(1, 1, 1/2, ...) leaves the eigenvalues 1 and 2: two
    iterations as in exact arithmetic, where plain conjugate gradients take three and a wrong beta, or z and r mixed up, dozens.
    M = the inverse: one iteration and y = b / d to 4 ulp."""
    A, b, d = cc.diag3(n, dtype), cc.rhs(n, dtype), cases.diag3_entries(n)
    op = pkg.csr_operator(A, ctx)
    pcg = _pcg(op, pkg.diagonal_operator(cases.two_cluster_diagonal(n), dtype, ctx), path, monkeypatch, tol=TOL)
    y = Solver(pcg)(b)
    info = pcg.pcg_info
    res = np.linalg.norm(A @ y - b)
    print("n = %d, two clusters: %s, true residual %.3g" % (n, info, res))
    assert info["last_iterations"] == 2 and info["applications"] == 1 and info["iterations"] == 2, info
    assert res <= 2 * TOL * np.linalg.norm(b)
    # the start and one per iteration; the generic path also runs M for the rest of its chunk of 8, into z only
    assert info["preconditioner_applications"] == (3 if path == "jacobi" else 9), info
    inv = _pcg(op, pkg.diagonal_operator(1.0 / d, dtype, ctx), path, monkeypatch, tol=TOL)
    y = Solver(inv)(b)
    info = inv.pcg_info
    print("n = %d, inverse: %s" % (n, info))
    assert info["last_iterations"] == 1, info
    want = b / d
    ulp = np.finfo(np.float64).eps
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(y) - part(want)) <= 4 * ulp * np.abs(part(want)))


# ------------------------------------------------------------------------------------------------ 2. the two paths give the same bits
@functools.lru_cache(maxsize=None)
def _jump():
    """("jump" of pcg_cases) coefficient, taps, diagonal, host matrix, and per element type: b, y*, the models' counts."""
    c = cases.jump_coeff()
    taps, d = extras.diffusion_terms(cases.SHAPE, c, 1.0, None)
    H = pkg.host_grid_variable_matrix(cases.SHAPE, taps, c, d)
    ref = {}
    for dt in DTYPES:
        b = cc.rhs(H.shape[0], dt)
        _, its, _ = model.solve(H, lambda r: r / d, b, tol=cases.TOL)
        _, its_cg, _ = cg_model.solve(H, b, tol=cases.TOL, maxit=5000)
        ref[np.dtype(dt)] = (b, its, its_cg)
    return c, taps, d, H, ref


def _jump_operator(dtype, ctx):
    c, taps, d, H, ref = _jump()
    return pkg.grid_variable_operator(cases.SHAPE, taps, c, d, dtype=dtype, ctx=ctx), H, d, ref[np.dtype(dtype)]


def _both_paths(A, d, b, ctx, monkeypatch, **kw):
    out = []
    for path in PATHS:
        op = _pcg(A, pkg.diagonal_operator(d, A.dtype, ctx), path, monkeypatch, **kw)
        y = Solver(op)(b)
        info = op.pcg_info
        out.append((y, info["last_iterations"], info["last_relres"]))
    (y0, it0, rr0), (y1, it1, rr1) = out
    assert np.all(np.isfinite(y0))
    assert np.array_equal(_bits(y0), _bits(y1)) and it0 == it1 and rr0 == rr1, (it0, it1, rr0, rr1, np.abs(y0 - y1).max())
    return it0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", cc.DIAG_SIZES)
def test_fused_and_generic_jacobi_give_the_same_bits_on_diag3(n, dtype, ctx, monkeypatch):
    """... with a preconditioner that makes the solve take a dozen iterations with every kernel in its ordinary branch."""
    rng = np.random.default_rng(n)
    d = 1.0 / (cases.diag3_entries(n) * (0.5 + rng.random(n)))
    its = _both_paths(pkg.csr_operator(cc.diag3(n, dtype), ctx), d, cc.rhs(n, dtype), ctx, monkeypatch, tol=TOL)
    assert 5 <= its <= 40, its


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_and_generic_jacobi_give_the_same_bits_on_the_coefficient_jump(dtype, ctx, monkeypatch):
    A, H, d, (b, its_model, _) = _jump_operator(dtype, ctx)
    its = _both_paths(A, 1.0 / d, b, ctx, monkeypatch, tol=cases.TOL)
    assert abs(its - its_model) <= cases.band("jump")


# ------------------------------------------------------------------------------------------------ 3. M = I is conjugate gradients
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", ["laplace-v", "mass"])
def test_identity_preconditioner_follows_conjugate_gradients(case, dtype, path, ctx, monkeypatch):
    if case == "mass":
        mt = extras.q1_fem_taps(3)[1]
        H, A = pkg.host_grid_box_matrix(cc.MASS_SHAPE, mt), pkg.grid_box_operator(cc.MASS_SHAPE, mt, dtype=dtype, ctx=ctx)
    else:
        v = cc.potential()
        H, A = pkg.host_grid_matrix(cc.GRID_SHAPE, cc.LAPLACE, v), pkg.grid_operator(cc.GRID_SHAPE, cc.LAPLACE, v, dtype=dtype, ctx=ctx)
    n = H.shape[0]
    assert A.dtype == np.dtype(dtype)
    b = cc.rhs(n, dtype)
    cg = pkg.cg_operator(A, tol=TOL)
    Solver(cg)(b)
    pcg = _pcg(A, pkg.diagonal_operator(np.ones(n), dtype, ctx), path, monkeypatch, tol=TOL)
    _, its = _assert_bounds(pcg, H, b, case)
    assert abs(its - cg.cg_info["last_iterations"]) <= 1, (its, cg.cg_info)


# ------------------------------------------------------------------------------------------------ 4. Jacobi on a coefficient jump
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_jacobi_on_a_coefficient_jump(dtype, ctx):
    """-div(c grad) on 12 x 10 x 8 with a jump of 100 in c: the count lies within the band of the model's and is at most a third of
    the model's count for plain conjugate gradients (recorded in pcg_cases: 72 against 519)."""
    A, H, d, (b, its_model, its_cg) = _jump_operator(dtype, ctx)
    pcg = pkg.pcg_operator(A, extras.jacobi_preconditioner(d, dtype=dtype, ctx=ctx), tol=cases.TOL)
    assert pcg.pcg_info["path"] == "jacobi"
    _, its = _assert_bounds(pcg, H, b, "jump", tol=cases.TOL)
    print("jump: %d iterations, model %d (recorded %d), plain conjugate gradients %d (recorded %d)"
          % (its, its_model, cases.MODEL_ITS["jump"], its_cg, cases.CG_ITS["jump"]))
    assert abs(its - its_model) <= cases.band("jump"), (its, its_model)
    assert 3 * its <= its_cg, (its, its_cg)


# ------------------------------------------------------------------------------------------------ 5. other operators as M
@functools.lru_cache(maxsize=None)
def _aniso():
    t, v = cases.aniso_terms()
    H = pkg.host_grid_matrix(cases.SHAPE, t, v)
    T = sp.diags(list(extras.grid_line_terms(cases.SHAPE, t, v)), [-1, 0, 1]).tocsc()
    lu = spl.splu(T)
    ref = {}
    for dt in DTYPES:
        b = cc.rhs(H.shape[0], dt)
        line = (lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag)) if np.dtype(dt).kind == "c" else lu.solve
        _, its, _ = model.solve(H, line, b, tol=cases.TOL)
        _, its_cg, _ = cg_model.solve(H, b, tol=cases.TOL, maxit=5000)
        ref[np.dtype(dt)] = (b, its, its_cg)
    return t, v, H, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_line_preconditioner_on_an_anisotropic_grid(dtype, ctx):
    """Taps (z, y, x) = (1e-2, 1e-2, 1) (-1, 2, -1) plus a small potential: the x-line solve as M, through the generic path (16
    iterations against the 94 of plain conjugate gradients, and of the diagonal)."""
    t, v, H, ref = _aniso()
    b, its_model, its_cg = ref[np.dtype(dtype)]
    t, v = t.astype(dtype), v.astype(dtype)
    A = pkg.grid_operator(cases.SHAPE, t, v, ctx=ctx)
    M = extras.line_preconditioner(cases.SHAPE, t, v, ctx=ctx)
    assert A.dtype == M.dtype == np.dtype(dtype)
    pcg = pkg.pcg_operator(A, M, tol=cases.TOL)
    assert pcg.pcg_info["path"] == "generic"
    _, its = _assert_bounds(pcg, H, b, "aniso", tol=cases.TOL)
    print("aniso: %d iterations, model %d (recorded %d), plain conjugate gradients %d (recorded %d)"
          % (its, its_model, cases.MODEL_ITS["aniso"], its_cg, cases.CG_ITS["aniso"]))
    assert abs(its - its_model) <= cases.band("aniso"), (its, its_model)
    assert 3 * its <= its_cg, (its, its_cg)
    assert pcg.pcg_info["preconditioner_applications"] >= its + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_incomplete_factors_as_preconditioner(dtype, ctx):
    """`lu_operator` of scipy's incomplete LU (no pivoting, natural order) on the ragged random matrix: correctness only.  What was
    dropped leaves L U slightly unsymmetric, and with THAT M the numpy model stalls at a relative residual of 1e-10: M must be
    Hermitian, so it is L D L^T with L and D = diag(U) of the incomplete factors (the model: 8 iterations against 41)."""
    H = cc.random_spd()
    n = H.shape[0]
    ilu = spl.spilu(H.tocsc(), drop_tol=1e-2, fill_factor=5, permc_spec="NATURAL", diag_pivot_thresh=0.0)
    assert np.array_equal(ilu.perm_r, np.arange(n)) and np.array_equal(ilu.perm_c, np.arange(n))
    L, D = sp.csr_matrix(ilu.L), ilu.U.diagonal()
    assert D.min() > 0 and np.all(L.diagonal() == 1.0)
    A = pkg.csr_operator(H.astype(dtype), ctx)
    M = pkg.lu_operator(L.astype(dtype), sp.csr_matrix(sp.diags(D) @ L.T).astype(dtype), ctx=ctx)
    assert A.dtype == M.dtype == np.dtype(dtype)
    pcg = pkg.pcg_operator(A, M, tol=TOL)
    b = cc.rhs(H.shape[0], dtype)
    _, its = _assert_bounds(pcg, H, b, "ilu")
    cg = pkg.cg_operator(A, tol=TOL)
    Solver(cg)(b)
    assert its < cg.cg_info["last_iterations"], (its, cg.cg_info)


# ------------------------------------------------------------------------------------------------ 6. the shift
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["grid-fused-jacobi", "csr-fused-line", "csr-generic-line"])
def test_shift_below_the_spectrum(path, dtype, ctx, monkeypatch):
    """(A + 2 I)^-1 b on 12 x 10 x 8 with M built for A + 2 I: the grid operator and a stored matrix fuse the shift into their
    product, KS_SHIFT_FUSED=0 runs the product and a streaming pass."""
    v = cc.potential()
    H = pkg.host_grid_matrix(cc.GRID_SHAPE, cc.LAPLACE, v)
    if path == "csr-generic-line":
        monkeypatch.setenv("KS_SHIFT_FUSED", "0")
    if path == "grid-fused-jacobi":
        A = pkg.grid_operator(cc.GRID_SHAPE, cc.LAPLACE, v, dtype=dtype, ctx=ctx)
        M = extras.jacobi_preconditioner(H.diagonal(), shift=-2.0, dtype=dtype, ctx=ctx)
    else:
        A = pkg.csr_operator(H.astype(dtype), ctx)
        M = extras.line_preconditioner(cc.GRID_SHAPE, cc.LAPLACE.astype(dtype), v.astype(dtype), shift=-2.0, ctx=ctx)
    assert A.dtype == M.dtype == np.dtype(dtype)
    b = cc.rhs(H.shape[0], dtype)
    _, its = _assert_bounds(pkg.pcg_operator(A, M, shift=-2.0, tol=TOL), H, b, path, shift=-2.0)
    if path == "grid-fused-jacobi":
        M_host = lambda r: r / (H.diagonal() + 2.0)  # noqa: E731
    else:
        lu = spl.splu(sp.diags(list(extras.grid_line_terms(cc.GRID_SHAPE, cc.LAPLACE, v, shift=-2.0)), [-1, 0, 1]).tocsc())
        M_host = (lambda r: lu.solve(r.real) + 1j * lu.solve(r.imag)) if np.dtype(dtype).kind == "c" else lu.solve  # noqa: E731
    assert abs(its - model.solve(H, M_host, b, shift=-2.0, tol=TOL)[1]) <= 1


# ------------------------------------------------------------------------------------------------ 7. determinism and chunking
@pytest.mark.parametrize("path", ["jacobi", "generic", "line"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_result_does_not_depend_on_chunking_or_history(dtype, path, ctx, monkeypatch):
    """check_every = 1, 3, 64 and the default: the same bits and the same count.  The same right-hand side twice with another in
    between: the same bits.  b = 0: y = 0 after 0 iterations."""
    if path == "line":
        t, v, H, ref = _aniso()
        t, v = t.astype(dtype), v.astype(dtype)
        A, M = pkg.grid_operator(cases.SHAPE, t, v, ctx=ctx), extras.line_preconditioner(cases.SHAPE, t, v, ctx=ctx)
    else:
        A, H, d, _ = _jump_operator(dtype, ctx)
        M = extras.jacobi_preconditioner(d, dtype=dtype, ctx=ctx)
    n = H.shape[0]
    b, b2 = cc.rhs(n, dtype), cc.rhs(n, dtype, seed=23)
    want, want_its = None, None
    for every in (0, 1, 3, 64):
        pcg = _pcg(A, M, "jacobi" if path == "jacobi" else "generic", monkeypatch, tol=cases.TOL, check_every=every)
        solve = Solver(pcg)
        y = solve(b)
        its = pcg.pcg_info["last_iterations"]
        if want is None:
            want, want_its = y, its
            assert its > 8      # (more than one chunk of the default length)
        assert np.array_equal(_bits(y), _bits(want)) and its == want_its, (every, its, want_its)
        y2 = solve(b2)
        its2 = pcg.pcg_info["last_iterations"]
        assert not np.array_equal(_bits(y2), _bits(want))
        assert np.array_equal(_bits(solve(b)), _bits(want)) and pcg.pcg_info["last_iterations"] == want_its, every
        z = solve(np.zeros(n, dtype=dtype))
        info = pcg.pcg_info
        assert not z.any() and np.all(np.isfinite(z)) and info["last_iterations"] == 0 and info["last_relres"] == 0.0, (every, info)
        assert info["applications"] == 4 and info["iterations"] == 2 * want_its + its2, info


# ------------------------------------------------------------------------------------------------ 8. failures
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_negative_preconditioner_raises_at_iteration_0_and_stays_usable(dtype, path, ctx, monkeypatch):
    n = 4096
    A, b = pkg.csr_operator(cc.diag3(n, dtype), ctx), cc.rhs(n, dtype)
    pcg = _pcg(A, pkg.diagonal_operator(-np.ones(n), dtype, ctx), path, monkeypatch, tol=TOL)
    solve = Solver(pcg)
    with pytest.raises(pkg.HipError, match=r"the preconditioner is not positive definite: r\^H M r = -\d.* at iteration 0"):
        solve(b)
    assert pcg.pcg_info["last_iterations"] == 0
    z = solve(np.zeros(n, dtype=dtype))
    assert not z.any() and pcg.pcg_info["last_iterations"] == 0 and pcg.pcg_info["applications"] == 2
    # one negative entry, met later: the start is fine for a right-hand side without weight there ... and the solve too, the entry
    # is never touched
    d = np.ones(n)
    d[5] = -1e6
    pcg = _pcg(A, pkg.diagonal_operator(d, dtype, ctx), path, monkeypatch, tol=TOL)
    solve = Solver(pcg)
    with pytest.raises(pkg.HipError, match=r"the preconditioner is not positive definite: r\^H M r = -\d.* at iteration 0"):
        solve(b)
    good = b.copy()
    good[5] = 0.0
    y = solve(good)
    assert pcg.pcg_info["last_iterations"] == 3 and y[5] == 0.0
    assert np.linalg.norm(cc.diag3(n, dtype) @ y - good) <= 2 * TOL * np.linalg.norm(good)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_indefinite_operator_raises_and_stays_usable(dtype, path, ctx, monkeypatch):
    n = 4096
    H, b = cc.indefinite(n, dtype)
    pcg = _pcg(pkg.csr_operator(H, ctx), pkg.diagonal_operator(np.ones(n), dtype, ctx), path, monkeypatch, tol=TOL)
    assert pcg.dtype == np.dtype(dtype)
    solve = Solver(pcg)
    with pytest.raises(pkg.HipError, match=r"ks_operator_pcg: not positive definite: p\^H \(A - theta\) p = -\d.* at iteration 1"):
        solve(b)
    assert pcg.pcg_info["last_iterations"] == 1
    good = cc.rhs(n, dtype)
    good[5] = 0.0
    y = solve(good)
    assert pcg.pcg_info["last_iterations"] == 3 and y[5] == 0.0
    assert np.linalg.norm(H @ y - good) <= 2 * TOL * np.linalg.norm(good)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxit_and_a_nan_raise_and_stay_usable(dtype, path, ctx, monkeypatch):
    A, H, d, (b, its_model, _) = _jump_operator(dtype, ctx)
    pcg = _pcg(A, extras.jacobi_preconditioner(d, dtype=dtype, ctx=ctx), path, monkeypatch, tol=cases.TOL, maxit=5)
    solve = Solver(pcg)
    with pytest.raises(pkg.HipError, match=r"did not converge: relative residual \d.* after 5 iterations"):
        solve(b)
    info = pcg.pcg_info
    _, _, relres = model.solve(H, lambda r: r / d, b, tol=cases.TOL)
    # (sums of n = 960 terms in another order differ by at most n eps = 2.1e-13 relative; such an error in alpha or beta moves the
    # residual by at most ||M A|| / lambda_min(M A) times as much, below 1e4 here, in each of the five iterations)
    assert info["last_iterations"] == 5 and abs(info["last_relres"] - relres[5]) <= 1e-8 * relres[5], (info, relres[5])
    bad = b.copy()
    bad[17] = np.nan
    with pytest.raises(pkg.HipError, match="the right-hand side is not finite"):
        solve(bad)
    assert pcg.pcg_info["last_iterations"] == 0
    # the same operator and preconditioner with room to finish
    full = _pcg(A, extras.jacobi_preconditioner(d, dtype=dtype, ctx=ctx), path, monkeypatch, tol=cases.TOL)
    y = Solver(full)(b)
    assert abs(full.pcg_info["last_iterations"] - its_model) <= cases.band("jump") and np.all(np.isfinite(y))
    with pytest.raises(pkg.HipError, match="did not converge"):
        solve(b)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_wrong_use_is_refused(ctx):
    shape = (4, 3, 2)
    n = cc.size(shape)
    t = np.array([-1.0, -1.0, -1.0, 7.0, -1.0, -1.0, -1.0])
    A = pkg.grid_operator(shape, t, ctx=ctx)
    M = pkg.diagonal_operator(np.full(n, 1.0 / 7.0), ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="rows"):
        pkg.pcg_operator(A, pkg.diagonal_operator(np.ones(n + 1), ctx=ctx))
    with pytest.raises(pkg.ArgumentError, match="element type"):
        pkg.pcg_operator(A, pkg.diagonal_operator(np.ones(n), np.complex128, ctx=ctx))
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="preconditioner lives on another context"):
        pkg.pcg_operator(A, pkg.diagonal_operator(np.ones(n), ctx=other))
    with pytest.raises(pkg.ArgumentError, match="operator lives on another context"):
        pkg.pcg_operator(A, M, ctx=other)
    # a solve as preconditioner would need flexible conjugate gradients; so would a host callback
    host = pkg.host_operator(lambda y, x: np.copyto(y, x), n, ctx=ctx)
    inner = pkg.cg_operator(A, tol=1e-10)
    for bad in (inner, host, pkg.pcg_operator(A, M), pkg.product_operator(inner, A, ctx=ctx)):
        with pytest.raises(pkg.ArgumentError, match="preconditioner cannot be enqueued ahead"):
            pkg.pcg_operator(A, bad)
        with pytest.raises(pkg.ArgumentError, match="operator cannot be enqueued ahead"):
            pkg.pcg_operator(bad, M)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.pcg_operator(pkg.csr_operator(pkg.host_grid_matrix(shape, t), dctx), pkg.diagonal_operator(np.ones(n), ctx=dctx))
    for tol in (0.0, 1.0, -1e-3, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="tol"):
            pkg.pcg_operator(A, M, tol=tol)
    with pytest.raises(pkg.ArgumentError, match="maxit = 0"):
        pkg.pcg_operator(A, M, maxit=0)
    with pytest.raises(pkg.ArgumentError, match="check_every = -1"):
        pkg.pcg_operator(A, M, check_every=-1)
    with pytest.raises(pkg.ArgumentError, match="shift"):
        pkg.pcg_operator(A, M, shift=np.nan)
    for a, m in ((pkg.host_grid_matrix(shape, t), M), (A, None), (A, np.ones(n))):
        with pytest.raises(pkg.ArgumentError):
            pkg.pcg_operator(a, m)
    for op in (A, M, inner):
        with pytest.raises(pkg.ArgumentError, match="ks_operator_pcg"):
            op.pcg_info
    pcg = pkg.pcg_operator(A, M)
    with pytest.raises(pkg.ArgumentError, match="ks_operator_cg"):
        pcg.cg_info
    # source and destination must differ; closing the solve leaves the operator and the preconditioner usable
    ws = pkg.ArnoldiWorkspace(n, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(pcg, 1, 1)
    pcg.close()
    ws.set_col(0, np.ones(n))
    ws.apply(A, 0, 1)
    ws.apply(M, 1, 2)
    assert np.array_equal(ws.col(2), ws.col(1) * (1.0 / 7.0))
    with pytest.raises(pkg.ArgumentError, match="finite"):
        pkg.diagonal_operator([1.0, np.inf], ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        pkg.diagonal_operator([], ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        pkg.diagonal_operator(np.ones(3), np.float32, ctx=ctx)


# ------------------------------------------------------------------------------------------------ 10. the diagonal operator alone
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", cc.DIAG_SIZES)
def test_diagonal_operator_against_numpy(n, dtype, ctx):
    rng = np.random.default_rng(n)
    d = rng.standard_normal(n)
    d[::7] = 0.0
    x = cc.rhs(n, dtype, seed=3)
    D = pkg.diagonal_operator(d, dtype, ctx)
    assert D.shape == (n, n) and D.dtype == np.dtype(dtype) and np.array_equal(D.diagonal, d)
    y = Solver(D)(x)
    assert np.array_equal(_bits(y), _bits((d * x).astype(dtype)))
    # in place, through ks_operator_apply_raw (a workspace refuses equal columns): every element is read before it is written, by
    # the thread that owns it
    ws = pkg.ArnoldiWorkspace(n, 1, dtype, ctx=ctx)
    ws.set_col(1, x)
    lib, p = pkg._lib.load(), C.c_void_p()
    pkg._lib.check(lib.ks_workspace_col_ptr(ws._h, 1, C.byref(p)))
    pkg._lib.check(lib.ks_operator_apply_raw(D._h, p, p))
    ctx.synchronize()
    assert np.array_equal(_bits(ws.col(1)), _bits(y))


def test_diagonal_operator_composes(ctx):
    """Lumped-mass M^-1 K as a product, and DeviceVectors.apply column by column."""
    shape = cc.GRID_SHAPE
    n = cc.size(shape)
    v = cc.potential()
    K, Kh = pkg.grid_operator(shape, cc.LAPLACE, v, ctx=ctx), pkg.host_grid_matrix(shape, cc.LAPLACE, v)
    m = 0.5 + np.random.default_rng(2).random(n)
    Minv = pkg.diagonal_operator(1.0 / m, ctx=ctx)
    x = cc.rhs(n, np.float64, seed=5)
    Kx = Solver(K)(x)
    got = Solver(pkg.product_operator(Minv, K, ctx=ctx))(x)
    assert np.array_equal(_bits(got), _bits((1.0 / m) * Kx))
    assert np.allclose(got, (Kh @ x) / m, rtol=1e-14, atol=0)
    B = np.stack([cc.rhs(n, np.float64, seed=s) for s in (1, 2, 3)], axis=1)
    Y = pkg.DeviceVectors.from_host(B, ctx).apply(Minv).download()
    assert np.array_equal(_bits(Y), _bits(np.asfortranarray((1.0 / m)[:, None] * B)))
    # a Float64 diagonal on ComplexF64 vectors acts on both parts
    Bc = B[:, :2] + 1j * B[:, 1:]
    Yc = pkg.DeviceVectors.from_host(Bc, ctx).apply(Minv).download()
    assert np.array_equal(_bits(Yc), _bits(np.asfortranarray((1.0 / m)[:, None] * Bc)))
    # the Newton step of the s-step expansion: the default, product and streaming pass
    ws = pkg.ArnoldiWorkspace(n, 2, np.float64, ctx=ctx)
    ws.set_col(0, x)
    ws.apply_shifted(Minv, 0, 1, 0.25, 2.0)
    assert np.allclose(ws.col(1), 2.0 * (x / m - 0.25 * x), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ 11. end to end
def test_shift_invert_on_a_coefficient_jump_end_to_end(ctx):
    """The recipe of the README on 12 x 10 x 8: S = (A - sigma)^-1 by Jacobi-preconditioned conjugate gradients, sigma = 0 below the
    spectrum (lambda_min = 0.486), partialschur(S, nev=4, which="LM").  The four eigenvalues nearest sigma lie within their residual
    bounds ||A x - lambda x|| / ||x|| (a Hermitian A) of scipy.linalg.eigh of the host matrix, the residuals are those of the
    ORIGINAL operator, and the outer iteration takes the very steps it takes on cg_operator: both are the same linear map up to
    tol cond."""
    c, taps, d, H, _ = _jump()
    n = H.shape[0]
    sigma = 0.0
    ev = sla.eigh(H.toarray(), eigvals_only=True)
    assert ev[0] > sigma
    A = pkg.grid_variable_operator(cases.SHAPE, taps, c, d, ctx=ctx)
    S = pkg.pcg_operator(A, extras.jacobi_preconditioner(d, shift=sigma, ctx=ctx), shift=sigma, tol=1e-13)
    v1 = pkg.matrices.start_vector(n)
    P, hist = pkg.partialschur(S, v1=v1, nev=4, which="LM", tol=1e-10)
    assert hist.converged and P.nconverged >= 4, hist
    mu, X = pkg.partialeigen(P, device=True)
    assert np.all(np.imag(mu) == 0)
    lam = np.ascontiguousarray(extras.interior_eigenvalues(np.real(mu), sigma))
    r, _ = pkg.residuals(A, X, lam)
    xn = np.sqrt(np.real(np.diag(pkg.gram(X, X))))
    info = S.pcg_info
    print("%s; pcg %s; lambda = %s, ||A x - lambda x|| = %s" % (hist, info, lam, r))
    found = []
    for lj, rj, nj in zip(lam, r, xn):
        j = int(np.argmin(np.abs(ev - lj)))
        assert abs(ev[j] - lj) <= rj / nj, (lj, ev[j], rj / nj)
        found.append(j)
    order = np.argsort(-np.abs(np.real(mu)))[:4]
    assert sorted(found[i] for i in order) == [0, 1, 2, 3], found
    assert np.all(r / xn <= 1e-8)
    assert info["applications"] >= hist.mvproducts and info["worst_relres"] <= 1e-13 * ROUND and info["path"] == "jacobi"
    S0 = pkg.cg_operator(A, shift=sigma, tol=1e-13, maxit=5000)
    P0, hist0 = pkg.partialschur(S0, v1=v1, nev=4, which="LM", tol=1e-10)
    print("cg: %s; %s" % (hist0, S0.cg_info))
    assert (hist0.mvproducts, hist0.restarts, hist0.nconverged, hist0.converged) == (hist.mvproducts, hist.restarts, hist.nconverged, hist.converged)
    assert 3 * info["iterations"] <= S0.cg_info["iterations"]
