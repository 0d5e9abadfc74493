"""`-m gpu`: the conjugate-gradient solve operator (`ks_operator_cg`, csrc/ks_cg.hpp) from its recurrence scalars up to a generalized
eigenproblem K x = lambda M x solved with nothing but operator products.

References: the host matrix of every operator (host_grid_*_matrix, the scipy matrix of a csr_operator), a direct host solve, and the
numpy model of the recurrence (tests/cg_model.py; tests/test_cg_model_cpu.py holds the model to the same bounds without a device).
Bounds: the true residual ||(A - theta) y - b|| <= 2 tol ||b|| (the recurrence stops at tol ||b||; the factor 2 is the room for the
drift between the recurrence's residual and the true one), the error ||y - y*|| <= 2 tol ||b|| / lambda_min (||e|| <= ||A^-1|| ||r||),
the iteration count within one of the model's (the trajectories differ by summation order and fused multiply-adds only).
Conventions of every product test here: the destination is poisoned with NaN, KS_GUARD=1 puts canaries around the basis."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import cg_cases as cases
import cg_model as model
import grid_cases as gc
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
TOL = cases.TOL
ROUND = 1.0 + 8 * np.finfo(np.float64).eps   # rho' <= fl(fl(tol^2) rho0), then a quotient and a root: a few roundings above tol
ENV = ("KS_SHIFT_FUSED", "KS_SHIFT_PLAIN", "KS_SPMV_FORMAT", "KS_SSTEP")


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


def _assert_solves(cg, A, b, what, shift=0.0, tol=TOL):
    """The three checks of the module docstring for one solve; returns y."""
    y = Solver(cg)(b)
    info = cg.cg_info
    Ad = np.asarray(A.todense()) - shift * np.eye(A.shape[0])
    ystar = np.linalg.solve(Ad, b)
    res, res_bound, err, err_bound = cases.bounds(A, y, ystar, b, tol, shift)
    _, its, relres = model.solve(A, b, shift=shift, tol=tol)
    print("%s: %d iterations (model %d), recurrence residual %.3g, true residual %.3g <= %.3g, error %.3g <= %.3g"
          % (what, info["last_iterations"], its, info["last_relres"], res, res_bound, err, err_bound))
    assert np.all(np.isfinite(y)), what
    assert res <= res_bound, (what, res, res_bound)
    assert err <= err_bound, (what, err, err_bound)
    assert abs(info["last_iterations"] - its) <= 1, (what, info, its)
    assert info["last_relres"] <= tol * ROUND, (what, info)
    return y


# ------------------------------------------------------------------------------------------------ 1. the recurrence scalars
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", cases.DIAG_SIZES)
def test_three_eigenvalues_take_exactly_three_iterations(n, dtype, ctx):
    """diag(1, 2, 4, ...) at n = 37 (below one wave), 4096 (whole packs and workgroups) and 70001 (odd: a half-filled pack in Float64,
    a ragged last workgroup, 69 workgroups of partial sums): three iterations, as in exact arithmetic -- a wrong alpha or beta
    degrades to steepest descent, which needs dozens."""
    A, b = cases.diag3(n, dtype), cases.rhs(n, dtype)
    cg = pkg.cg_operator(pkg.csr_operator(A, ctx), tol=TOL)
    y = Solver(cg)(b)
    info = cg.cg_info
    res = np.linalg.norm(A @ y - b)
    print("n = %d: %s, true residual %.3g" % (n, info, res))
    assert info["last_iterations"] == 3 and info["applications"] == 1 and info["iterations"] == 3, info
    assert res <= 2 * TOL * np.linalg.norm(b)


# ------------------------------------------------------------------------------------------------ 2. solves
def _mass(dtype, ctx):
    mt = extras.q1_fem_taps(3)[1]
    return pkg.host_grid_box_matrix(cases.MASS_SHAPE, mt), pkg.grid_box_operator(cases.MASS_SHAPE, mt, ctx=ctx)


def _laplace_v(dtype, ctx):
    v = cases.potential()
    return pkg.host_grid_matrix(cases.GRID_SHAPE, cases.LAPLACE, v), pkg.grid_operator(cases.GRID_SHAPE, cases.LAPLACE, v, ctx=ctx)


def _bloch(dtype, ctx):
    """Periodic -Laplacian with Bloch phases plus V >= 1: Hermitian, ComplexF64, positive definite."""
    t = cases.LAPLACE.astype(np.complex128)
    w = extras.bloch_wrap(t, (0.7, -0.4, 1.1))
    v = cases.potential(lo=1.0).astype(np.complex128)
    per = (True, True, True)
    H = pkg.host_grid_matrix(cases.GRID_SHAPE, t, v, periodic=per, wrap=w)
    assert abs(H - H.conj().T).max() == 0 and H.dtype == np.complex128
    return H, pkg.grid_operator(cases.GRID_SHAPE, t, v, ctx=ctx, periodic=per, wrap=w)


def _random_csr(dtype, ctx):
    A = cases.random_spd()
    op = pkg.csr_operator(A, ctx)
    assert op.format["layout"] == "csr", op.format
    return A, op


SOLVES = {"mass-box": (_mass, np.float64), "laplace-v": (_laplace_v, np.float64), "bloch-c64": (_bloch, np.complex128),
          "random-csr": (_random_csr, np.float64)}


@pytest.mark.parametrize("case", list(SOLVES), ids=list(SOLVES))
def test_solves_against_the_host_matrix(case, ctx):
    make, dtype = SOLVES[case]
    A, op = make(dtype, ctx)
    cg = pkg.cg_operator(op, tol=TOL)
    assert cg.shape == op.shape and cg.dtype == op.dtype and cg.base is op
    _assert_solves(cg, A, cases.rhs(A.shape[0], dtype), case)


# ------------------------------------------------------------------------------------------------ 3. the shift
@pytest.mark.parametrize("path", ["grid-fused", "csr-fused", "csr-generic"])
def test_shift_below_the_spectrum(path, ctx, monkeypatch):
    """(A + 2 I)^-1 b on 12 x 10 x 8: the grid operator and a stored matrix fuse the shift into their product, KS_SHIFT_FUSED=0 runs
    the product and a streaming pass."""
    A, grid = _laplace_v(np.float64, ctx)
    if path == "csr-generic":
        monkeypatch.setenv("KS_SHIFT_FUSED", "0")
    op = grid if path == "grid-fused" else pkg.csr_operator(A, ctx)
    _assert_solves(pkg.cg_operator(op, shift=-2.0, tol=TOL), A, cases.rhs(A.shape[0], np.float64), path, shift=-2.0)


# ------------------------------------------------------------------------------------------------ 4. determinism and chunking
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_result_does_not_depend_on_chunking_or_history(dtype, ctx):
    """check_every = 1, 3, 64 and the default: the same bits and the same count.  The same right-hand side twice with another in
    between: the same bits.  b = 0: y = 0 after 0 iterations."""
    A, op = _bloch(dtype, ctx) if np.dtype(dtype).kind == "c" else _mass(dtype, ctx)
    n = A.shape[0]
    b, b2 = cases.rhs(n, dtype), cases.rhs(n, dtype, seed=23)
    want, want_its = None, None
    for every in (0, 1, 3, 64):
        cg = pkg.cg_operator(op, tol=TOL, check_every=every)
        solve = Solver(cg)
        y = solve(b)
        its = cg.cg_info["last_iterations"]
        if want is None:
            want, want_its = y, its
            assert its > 8      # (more than one chunk of the default length)
        assert np.array_equal(_bits(y), _bits(want)) and its == want_its, (every, its, want_its)
        y2 = solve(b2)
        its2 = cg.cg_info["last_iterations"]
        assert not np.array_equal(_bits(y2), _bits(want))
        assert np.array_equal(_bits(solve(b)), _bits(want)) and cg.cg_info["last_iterations"] == want_its, every
        z = solve(np.zeros(n, dtype=dtype))
        info = cg.cg_info
        assert not z.any() and np.all(np.isfinite(z)) and info["last_iterations"] == 0 and info["last_relres"] == 0.0, (every, info)
        assert info["applications"] == 4 and info["iterations"] == 2 * want_its + its2, info


# ------------------------------------------------------------------------------------------------ 5. failures
def test_indefinite_operator_raises_and_stays_usable(ctx):
    n = 4096
    A, b = cases.indefinite(n)
    cg = pkg.cg_operator(pkg.csr_operator(A, ctx), tol=TOL)
    solve = Solver(cg)
    with pytest.raises(pkg.HipError, match=r"not positive definite: p\^H \(A - theta\) p = -\d.* at iteration 1"):
        solve(b)
    assert cg.cg_info["last_iterations"] == 1
    # a right-hand side without weight on the negative entry never meets it: three eigenvalues, three iterations
    good = cases.rhs(n, np.float64)
    good[5] = 0.0
    y = solve(good)
    assert cg.cg_info["last_iterations"] == 3 and y[5] == 0.0
    assert np.linalg.norm(A @ y - good) <= 2 * TOL * np.linalg.norm(good)


def test_maxit_raises_and_stays_usable(ctx):
    A, op = _mass(np.float64, ctx)
    cg = pkg.cg_operator(op, tol=TOL, maxit=2)
    solve = Solver(cg)
    b = cases.rhs(A.shape[0], np.float64)
    with pytest.raises(pkg.HipError, match=r"did not converge: relative residual \d.* after 2 iterations"):
        solve(b)
    info = cg.cg_info
    _, _, relres = model.solve(A, b, tol=TOL)
    # (sums of n = 2079 non-negative terms in another order differ by at most n eps = 2.3e-13 relative; a few of them enter rho')
    assert info["last_iterations"] == 2 and abs(info["last_relres"] - relres[2]) <= 1e-11 * relres[2], (info, relres[2])
    # an eigenvector of the Kronecker product (sines along every axis) is solved in one iteration
    ax = [np.sin(np.pi * np.arange(1, m + 1) / (m + 1)) for m in cases.MASS_SHAPE]
    v = np.einsum("k,j,i->kji", ax[2], ax[1], ax[0]).ravel()
    y = solve(v)
    assert cg.cg_info["last_iterations"] == 1
    assert np.linalg.norm(A @ y - v) <= 2 * TOL * np.linalg.norm(v)
    assert cg.cg_info["worst_relres"] == info["last_relres"]


def test_wrong_use_is_refused(ctx):
    shape = (4, 3, 2)
    n = gc.size(shape)
    t = gc.taps(3, np.float64, symmetric=True)
    A = pkg.grid_operator(shape, t, ctx=ctx)
    # operators that cannot be enqueued ahead: a host callback, another solve, a product of one
    host = pkg.host_operator(lambda y, x: np.copyto(y, x), n, ctx=ctx)
    inner = pkg.cg_operator(A, tol=1e-10)
    for bad in (host, inner, pkg.product_operator(inner, A, ctx=ctx), pkg.chebyshev_operator(inner, 0.0, 1.0, (0.5, 1.0))):
        with pytest.raises(pkg.ArgumentError, match="cannot be enqueued ahead"):
            pkg.cg_operator(bad)
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="another context"):
        pkg.cg_operator(A, ctx=other)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.cg_operator(pkg.csr_operator(pkg.host_grid_matrix(shape, t), dctx))
    for tol in (0.0, 1.0, 2.0, -1e-3, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="tol"):
            pkg.cg_operator(A, tol=tol)
    with pytest.raises(pkg.ArgumentError, match="maxit = 0"):
        pkg.cg_operator(A, maxit=0)
    with pytest.raises(pkg.ArgumentError, match="check_every = -1"):
        pkg.cg_operator(A, check_every=-1)
    for shift in (np.nan, np.inf, -np.inf):
        with pytest.raises(pkg.ArgumentError, match="shift"):
            pkg.cg_operator(A, shift=shift)
    with pytest.raises(pkg.ArgumentError):
        pkg.cg_operator(pkg.host_grid_matrix(shape, t))
    with pytest.raises(pkg.ArgumentError, match="ks_operator_cg"):
        A.cg_info
    # source and destination must differ; closing the solve leaves the operator usable
    ws = pkg.ArnoldiWorkspace(n, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(inner, 1, 1)
    inner.close()
    ws.set_col(0, np.ones(n))
    ws.apply(A, 0, 1)
    assert np.all(np.isfinite(ws.col(1)))


# ------------------------------------------------------------------------------------------------ 6. composition
def test_composes_with_device_vectors_products_and_counters(ctx):
    shape = cases.GRID_SHAPE
    n = cases.size(shape)
    kt, mt = extras.q1_fem_taps(3)
    K, M = pkg.grid_box_operator(shape, kt, gc.harmonic(shape), ctx=ctx), pkg.grid_box_operator(shape, mt, ctx=ctx)
    cg = pkg.cg_operator(M, tol=TOL)
    solve = Solver(cg)
    B = np.stack([cases.rhs(n, np.float64, seed=s) for s in (1, 2, 3)], axis=1)
    singles, its = [], []
    for j in range(3):
        singles.append(solve(B[:, j]))
        its.append(cg.cg_info["last_iterations"])
    Y = pkg.DeviceVectors.from_host(B, ctx).apply(cg).download()
    for j in range(3):
        assert np.array_equal(_bits(Y[:, j]), _bits(singles[j])), j
    info = cg.cg_info
    assert info["applications"] == 6 and info["iterations"] == 2 * sum(its) and info["last_iterations"] == its[2], (info, its)
    # cg(M) K x: the product operator against the two steps taken one by one
    x = cases.rhs(n, np.float64, seed=5)
    Kx = Solver(K)(x)
    want = solve(Kx)
    prod = pkg.product_operator(cg, K, ctx=ctx)
    got = Solver(prod)(x)
    assert np.array_equal(_bits(got), _bits(want))
    assert cg.cg_info["applications"] == 8
    G = extras.generalized_cg_operator(K, M, tol=TOL)
    assert G.solve.base is M and G.factors == (G.solve, K)
    assert np.array_equal(_bits(Solver(G)(x)), _bits(want)) and G.solve.cg_info["applications"] == 1
    # sizes and format: those of the operator inside
    for op, inner in ((cg, M), (prod, None)):
        nn, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
        pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(nn), C.byref(nnz), C.byref(dt)))
        Mnnz = pkg.host_grid_box_matrix(shape, mt).nnz
        assert (nn.value, dt.value) == (n, pkg._lib.KS_F64) and nnz.value == (Mnnz if inner is not None else 2 * Mnnz)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")


# ------------------------------------------------------------------------------------------------ 7. end to end
@functools.lru_cache(maxsize=None)
def _pencil():
    shape = cases.GRID_SHAPE
    kt, mt = extras.q1_fem_taps(3)
    V = gc.harmonic(shape)
    Kh, Mh = pkg.host_grid_box_matrix(shape, kt, V), pkg.host_grid_box_matrix(shape, mt)
    mu = sla.eigh(Kh.toarray(), Mh.toarray(), eigvals_only=True)
    return shape, kt, mt, V, mu, float(np.linalg.eigvalsh(Mh.toarray())[0])


def test_generalized_problem_end_to_end(ctx):
    """K x = lambda M x, Q1 elements on 12 x 10 x 8 with a harmonic term in K (n = 960), through B^-1 A by conjugate gradients
    (inner tol 1e-13, outer tol 1e-10, which = SR).  Every lambda_j lies within r_j / (lambda_min(M) ||x_j||) of an eigenvalue of
    scipy.linalg.eigh(K, M) -- the residual bound of a definite pencil, |lambda - mu| <= ||M^-1/2 r|| / ||M^1/2 x|| -- and the four
    found are the four smallest.

    Measured on an MI355X: converged in 228 products, 15 250 inner iterations (61-67 per solve, worst recurrence residual 9.8e-14);
    lambda = 1.1019027, 1.90600516, 1.90859312, 1.93572845; ||K x - lambda M x|| = 1.1e-11, 4.8e-11, 3.5e-11, 5.7e-11; inclusion
    radii 2.7e-10 ... 1.3e-9 against a smallest gap of 2.6e-3 among the five lowest eigenvalues (lambda_min(M) = 0.042)."""
    shape, kt, mt, V, mu, m_min = _pencil()
    n = cases.size(shape)
    K, M = pkg.grid_box_operator(shape, kt, V, ctx=ctx), pkg.grid_box_operator(shape, mt, ctx=ctx)
    G = extras.generalized_cg_operator(K, M, tol=1e-13)
    dec, hist = pkg.partialschur(G, v1=pkg.matrices.start_vector(n), nev=4, which="SR", tol=1e-10)
    assert hist.converged and dec.nconverged >= 4, hist
    lam, X = pkg.partialeigen(dec, device=True)
    assert np.all(np.imag(lam) == 0)
    lam = np.ascontiguousarray(np.real(lam))
    r, _ = pkg.residuals(K, X, lam, M)
    xn = np.sqrt(np.real(np.diag(pkg.gram(X, X))))
    radius = r / (m_min * xn)
    print("%s; cg %s; lambda = %s, ||K x - lambda M x|| = %s, inclusion radius = %s, smallest gap of mu[0:5] = %.3g"
          % (hist, G.solve.cg_info, lam, r, radius, np.diff(mu[:5]).min()))
    found = []
    for lj, rad in zip(lam, radius):
        j = int(np.argmin(np.abs(mu - lj)))
        assert abs(mu[j] - lj) <= rad, (lj, mu[j], rad)
        found.append(j)
    assert sorted(found)[:4] == [0, 1, 2, 3], found
    info = G.solve.cg_info
    assert info["applications"] >= hist.mvproducts and info["worst_relres"] <= 1e-13 * ROUND
