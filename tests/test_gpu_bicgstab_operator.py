"""`-m gpu`: the BiCGStab(2) solve operator (`ks_operator_bicgstab`, csrc/ks_bicgstab.hpp) from its recurrence scalars up to the
eigenvalues nearest a shift of a matrix-free operator that is not Hermitian.

References: the host matrix of every operator and the numpy model of the recurrence (tests/bicgstab_model.py;
tests/test_bicgstab_model_cpu.py holds the model to tighter bounds without a device).  Bounds: the true residual
||(A - theta) y - b|| <= 2 tol ||b|| (the recurrence stops at tol ||b||; the model's true residual stays below 1.25 tol ||b|| on
every case here, in every ordering), the recurrence's own residual <= tol (1 + 8 eps), and the iteration count within
`bicgstab_cases.band(case)` of the model's -- twice what summation order alone does to the model, measured by the CPU tests.
Conventions of every product test here: the destination is poisoned with NaN, KS_GUARD=1 puts canaries around the basis, the
right-hand side is unchanged bit for bit (`test_gpu_cg_operator.Solver`)."""
import numpy as np
import pytest
import scipy.sparse as sp

import bicgstab_cases as cases
import bicgstab_model as model
import grid_cases as gc
import test_gpu_cg_operator as cgt
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402

TOL = cases.TOL
ROUND = 1.0 + 8 * np.finfo(np.float64).eps   # sqrt(rr) <= fl(tol beta1), then a quotient: a few roundings above tol
Solver, _bits = cgt.Solver, cgt._bits


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in cgt.ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _grid(kind, dtype, ctx):
    return pkg.grid_operator(cases.SHAPE, cases.taps(kind, dtype), cases.V.astype(dtype), ctx=ctx)


def _assert_solves(bs, A, b, what, shift=0.0, tol=TOL, model_its=None, its_band=None):
    """The checks of the module docstring for one solve; returns y."""
    before = bs.bicgstab_info
    y = Solver(bs)(b)
    info = bs.bicgstab_info
    res, nb = cases.true_residual(A, y, b, shift), float(np.linalg.norm(b))
    print("%s: %d iterations (model %s, band %s), recurrence residual %.3g, true residual %.3g <= %.3g"
          % (what, info["last_iterations"], model_its, its_band, info["last_relres"], res, 2 * tol * nb))
    assert np.all(np.isfinite(y)), what
    assert res <= 2 * tol * nb, (what, res, 2 * tol * nb)
    assert info["last_relres"] <= tol * ROUND, (what, info)
    assert info["applications"] == before["applications"] + 1 and info["iterations"] == before["iterations"] + info["last_iterations"], (before, info)
    assert info["worst_relres"] >= info["last_relres"]
    if its_band is not None:
        assert abs(info["last_iterations"] - model_its) <= its_band, (what, info, model_its, its_band)
    return y


# ------------------------------------------------------------------------------------------------ 1. the recurrence scalars
@pytest.mark.parametrize("n", cases.DIAG_SIZES)
@pytest.mark.parametrize("values,dtype", [(cases.THREE, np.float64), (cases.THREE, np.complex128), (cases.THREE_C, np.complex128)],
                         ids=["three-f64", "three-c64", "complex-c64"])
def test_three_eigenvalues_end_within_eight_iterations(values, dtype, n, ctx):
    """diag(1, -2, 4, ...) and diag(1 + i, 2 - i, -1 + i/2, ...) at n = 37 (below one wave), 4096 (whole packs and workgroups) and
    70001 (odd: a half-filled pack in Float64, a ragged last workgroup, 69 workgroups of partial sums): the second iteration ends
    the solve in exact arithmetic (the model: 2, at stage 1).  A wrong coefficient, a wrong role of one of the six vectors or a
    wrong conjugate leaves a method that needs dozens, or none that converges."""
    A, b = cases.cyclic_diag(values, n, dtype), cases.rhs(n, dtype)
    bs = pkg.bicgstab_operator(pkg.csr_operator(A, ctx), tol=TOL)
    y = Solver(bs)(b)
    info = bs.bicgstab_info
    res = cases.true_residual(A, y, b)
    print("n = %d: %s, true residual %.3g" % (n, info, res))
    assert 1 <= info["last_iterations"] <= cases.DIAG_MAX_ITS and info["applications"] == 1 and info["iterations"] == info["last_iterations"], info
    assert info["last_relres"] <= TOL * ROUND
    assert res <= 2 * TOL * np.linalg.norm(b)


@pytest.mark.parametrize("n,dtype", [(37, np.float64), (70001, np.float64), (4096, np.complex128)], ids=["37-f64", "70001-f64", "4096-c64"])
def test_twice_the_identity_finishes_in_the_half_step(n, dtype, ctx):
    """A = 2 I: alpha = 1/2 exactly and r0 = b - b = 0 after the first BiCG step: stage 1 of iteration 1 ends the solve with
    y = b / 2 exactly.  Every scalar behind it would be 0 / 0: the kernels behind the stage test must not run."""
    A, b = sp.identity(n, dtype=dtype, format="csr") * 2.0, cases.rhs(n, dtype)
    bs = pkg.bicgstab_operator(pkg.csr_operator(sp.csr_matrix(A), ctx), tol=TOL)
    solve = Solver(bs)
    y = solve(b)
    info = bs.bicgstab_info
    assert info["last_iterations"] == 1 and info["last_relres"] == 0.0, info
    assert np.array_equal(_bits(y), _bits(b / 2))
    # ... and again, into a destination and owned vectors that the first solve's idle products have filled
    assert np.array_equal(_bits(solve(b)), _bits(b / 2)) and bs.bicgstab_info["iterations"] == 2


# ------------------------------------------------------------------------------------------------ 2. solves
@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("case", list(cases.SOLVES))
def test_solves_against_the_host_matrix(case, path, ctx, monkeypatch):
    """Every case of bicgstab_cases.SOLVES: the grid cases through the matrix-free grid operator, the random matrix through CSR row
    blocks; the shift fused into the product, and KS_SHIFT_FUSED=0, the product and a streaming pass."""
    kind, dtype, shift = cases.SOLVES[case]
    A, b, _ = cases.host_case(case)
    if path == "generic":
        monkeypatch.setenv("KS_SHIFT_FUSED", "0")
    op = pkg.csr_operator(A, ctx) if kind == "random" else _grid(kind, dtype, ctx)
    bs = pkg.bicgstab_operator(op, shift=shift, tol=TOL)
    assert bs.shape == op.shape and bs.dtype == op.dtype and bs.base is op
    _assert_solves(bs, A, b, "%s/%s" % (case, path), shift=shift, model_its=cases.MODEL_ITS[case], its_band=cases.band(case))


@pytest.mark.parametrize("path", ["fused", "generic"])
@pytest.mark.parametrize("case", ["swirl-2.0", "swirl-c64"])
def test_swirl_through_a_stored_matrix(case, path, ctx, monkeypatch):
    A, b, shift = cases.host_case(case)
    if path == "generic":
        monkeypatch.setenv("KS_SHIFT_FUSED", "0")
    bs = pkg.bicgstab_operator(pkg.csr_operator(A, ctx), shift=shift, tol=TOL)
    _assert_solves(bs, A, b, "%s/csr-%s" % (case, path), shift=shift, model_its=cases.MODEL_ITS[case], its_band=cases.band(case))


# ------------------------------------------------------------------------------------------------ 3. determinism and chunking
@pytest.mark.parametrize("case", ["swirl-2.0", "swirl-c64"])
def test_result_does_not_depend_on_chunking_or_history(case, ctx):
    """check_every = the default, 1, 3, 64: the same bits and the same count (about fifty iterations: several chunks of 1, 3 and 8,
    one of 64 that runs idle past the end).  The same right-hand side twice with another in between: the same bits.  b = 0: y = 0
    after 0 iterations."""
    kind, dtype, shift = cases.SOLVES[case]
    A, b, _ = cases.host_case(case)
    op = _grid(kind, dtype, ctx)
    b2 = b[::-1].copy()
    want, want_its = None, None
    for every in (0, 1, 3, 64):
        bs = pkg.bicgstab_operator(op, shift=shift, tol=TOL, check_every=every)
        solve = Solver(bs)
        y = solve(b)
        its = bs.bicgstab_info["last_iterations"]
        if want is None:
            want, want_its = y, its
            assert its > 8
        assert np.array_equal(_bits(y), _bits(want)) and its == want_its, (every, its, want_its)
        y2 = solve(b2)
        its2 = bs.bicgstab_info["last_iterations"]
        assert not np.array_equal(_bits(y2), _bits(want))
        assert np.array_equal(_bits(solve(b)), _bits(want)) and bs.bicgstab_info["last_iterations"] == want_its, every
        z = solve(np.zeros(A.shape[0]))
        info = bs.bicgstab_info
        assert not z.any() and np.all(np.isfinite(z)) and info["last_iterations"] == 0 and info["last_relres"] == 0.0, (every, info)
        assert info["applications"] == 4 and info["iterations"] == 2 * want_its + its2, info


# ------------------------------------------------------------------------------------------------ 4. failures
def test_singular_shift_raises_and_stays_usable(ctx):
    """(I - 1.0 I) = 0: u1 = 0 exactly, gamma = <b, u1> = 0 in the first BiCG step.  No right-hand side but zero is solvable at this
    shift, so the solve that follows is that one; a second operator on the same matrix with another shift solves a real one."""
    n = 4096
    eye = pkg.csr_operator(sp.identity(n, format="csr"), ctx)
    bs = pkg.bicgstab_operator(eye, shift=1.0, tol=TOL)
    solve = Solver(bs)
    b = cases.rhs(n, np.float64)
    with pytest.raises(pkg.HipError, match=r"breakdown: gamma = 0 in stage 1 at iteration 1"):
        solve(b)
    info = bs.bicgstab_info
    assert info["last_iterations"] == 1 and info["last_relres"] == 1.0, info
    z = solve(np.zeros(n))
    assert not z.any() and bs.bicgstab_info["last_iterations"] == 0
    with pytest.raises(pkg.HipError, match="breakdown"):
        solve(b)
    half = pkg.bicgstab_operator(eye, shift=0.5, tol=TOL)
    y = Solver(half)(b)
    assert half.bicgstab_info["last_iterations"] == 1 and np.linalg.norm(0.5 * y - b) <= 2 * TOL * np.linalg.norm(b)
    # ComplexF64 (the identity and its eigenvalue again: (1 + 0i) x - (1 + 0i) x is exactly zero in every product path)
    cs = pkg.bicgstab_operator(pkg.csr_operator(sp.identity(n, dtype=np.complex128, format="csr"), ctx), shift=1.0, tol=TOL)
    with pytest.raises(pkg.HipError, match=r"breakdown: gamma = \(0, 0\) in stage 1 at iteration 1"):
        Solver(cs)(cases.rhs(n, np.complex128))


def test_maxit_and_a_right_hand_side_that_is_not_finite_raise_and_stay_usable(ctx):
    case = "convdiff-0.9936"
    A, b, shift = cases.host_case(case)
    op = _grid("convdiff", np.float64, ctx)
    n = A.shape[0]
    bs = pkg.bicgstab_operator(op, shift=shift, tol=TOL, maxit=2)
    solve = Solver(bs)
    with pytest.raises(pkg.HipError, match=r"did not converge: relative residual \d.* after 2 iterations"):
        solve(b)
    info = bs.bicgstab_info
    _, _, _, relres = model.solve(A, b, shift=shift, tol=TOL)
    # (two iterations in: the trajectories differ by roundings only, 1e-10 is far above what they have grown to)
    assert info["last_iterations"] == 2 and abs(info["last_relres"] - relres[2]) <= 1e-10 * relres[2], (info, relres[2])
    # an eigenvector (the spectrum of convdiff is real) is solved in the first half step: the model leaves 1.8e-15 ||x|| there
    lam, X = np.linalg.eig(A.toarray())
    j = int(np.argmax(lam.real))
    assert lam[j].imag == 0
    x = np.ascontiguousarray(X[:, j].real)
    y = solve(x)
    assert bs.bicgstab_info["last_iterations"] == 1
    assert cases.true_residual(A, y, x, shift) <= 2 * TOL * np.linalg.norm(x)
    assert bs.bicgstab_info["worst_relres"] == info["last_relres"]
    # NaN in b
    full = pkg.bicgstab_operator(op, shift=shift, tol=TOL)
    bad = b.copy()
    bad[17] = np.nan
    ws = pkg.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    ws.set_col(0, bad)
    with pytest.raises(pkg.HipError, match="the right-hand side is not finite"):
        ws.apply(full, 0, 1)
    assert full.bicgstab_info["last_iterations"] == 0
    _assert_solves(full, A, b, "after a NaN", shift=shift, model_its=cases.MODEL_ITS[case], its_band=cases.band(case))


def test_wrong_use_is_refused(ctx):
    shape = (4, 3, 2)
    n = gc.size(shape)
    t = gc.taps(3, np.float64)
    A = pkg.grid_operator(shape, t, ctx=ctx)
    Ac = pkg.grid_operator(shape, t.astype(np.complex128), ctx=ctx)
    # an imaginary shift needs a ComplexF64 operator
    with pytest.raises(pkg.ArgumentError, match="imaginary shift on a Float64 operator.*ComplexF64"):
        pkg.bicgstab_operator(A, shift=2.0 + 0.5j)
    pkg.bicgstab_operator(A, shift=2.0 + 0.0j).close()
    pkg.bicgstab_operator(Ac, shift=2.0 + 0.5j).close()
    # operators that cannot be enqueued ahead: a host callback, a solve of any kind, a product or filter of one
    host = pkg.host_operator(lambda y, x: np.copyto(y, x), n, ctx=ctx)
    inner_cg = pkg.cg_operator(A, tol=1e-10)
    inner_mr = pkg.minres_operator(A, tol=1e-10)
    inner = pkg.bicgstab_operator(A, tol=1e-10)
    for bad in (host, inner_cg, inner_mr, inner, pkg.product_operator(inner, A, ctx=ctx), pkg.chebyshev_operator(inner, 0.0, 1.0, (0.5, 1.0))):
        with pytest.raises(pkg.ArgumentError, match="cannot be enqueued ahead"):
            pkg.bicgstab_operator(bad)
    for solver in (pkg.cg_operator, pkg.minres_operator):
        with pytest.raises(pkg.ArgumentError, match="cannot be enqueued ahead"):
            solver(inner)
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="another context"):
        pkg.bicgstab_operator(A, ctx=other)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.bicgstab_operator(pkg.csr_operator(pkg.host_grid_matrix(shape, t), dctx))
    for tol in (0.0, 1.0, 2.0, -1e-3, np.nan, np.inf):
        with pytest.raises(pkg.ArgumentError, match="tol"):
            pkg.bicgstab_operator(A, tol=tol)
    with pytest.raises(pkg.ArgumentError, match="maxit = 0"):
        pkg.bicgstab_operator(A, maxit=0)
    with pytest.raises(pkg.ArgumentError, match="check_every = -1"):
        pkg.bicgstab_operator(A, check_every=-1)
    for shift in (np.nan, np.inf, -np.inf):
        with pytest.raises(pkg.ArgumentError, match="shift"):
            pkg.bicgstab_operator(A, shift=shift)
    with pytest.raises(pkg.ArgumentError, match="shift"):
        pkg.bicgstab_operator(Ac, shift=complex(1.0, np.inf))
    with pytest.raises(pkg.ArgumentError):
        pkg.bicgstab_operator(pkg.host_grid_matrix(shape, t))
    for other_op in (A, inner_cg, inner_mr):
        with pytest.raises(pkg.ArgumentError, match="ks_operator_bicgstab"):
            other_op.bicgstab_info
    with pytest.raises(pkg.ArgumentError, match="ks_operator_minres"):
        inner.minres_info
    # source and destination must differ; closing the solve leaves the operator usable
    ws = pkg.ArnoldiWorkspace(n, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(inner, 1, 1)
    inner.close()
    ws.set_col(0, np.ones(n))
    ws.apply(A, 0, 1)
    assert np.all(np.isfinite(ws.col(1)))


# ------------------------------------------------------------------------------------------------ 5. where the Hermitian solvers stop
def test_solves_what_minres_and_conjugate_gradients_cannot(ctx):
    """swirl is not Hermitian: the three-term recurrences of MINRES and conjugate gradients solve some other problem without a
    complaint (or stop on a curvature or at maxit) -- what they return has a true residual of the order of ||b||."""
    A, b, _ = cases.host_case("swirl-0")
    op = _grid("swirl", np.float64, ctx)
    nb = float(np.linalg.norm(b))
    for name, make in (("minres", pkg.minres_operator), ("cg", pkg.cg_operator)):
        try:
            y = Solver(make(op, tol=TOL, maxit=500))(b)
        except pkg.HipError as e:
            print("%s: raised %s" % (name, e))
            continue
        res = cases.true_residual(A, y, b)
        print("%s: returned with true residual %.3g ||b||" % (name, res / nb))
        assert res > 1e-3 * nb, (name, res / nb)
    bs = pkg.bicgstab_operator(op, tol=TOL)
    _assert_solves(bs, A, b, "swirl-0", model_its=cases.MODEL_ITS["swirl-0"], its_band=cases.band("swirl-0"))


# ------------------------------------------------------------------------------------------------ 6. composition
def test_composes_with_device_vectors_and_products(ctx):
    A, b, shift = cases.host_case("swirl-2.0")
    op = _grid("swirl", np.float64, ctx)
    n = A.shape[0]
    bs = pkg.bicgstab_operator(op, shift=shift, tol=TOL)
    solve = Solver(bs)
    rng = np.random.default_rng(11)
    B = np.asfortranarray(rng.standard_normal((n, 3)))
    singles, its = [], []
    for j in range(3):
        singles.append(solve(B[:, j]))
        its.append(bs.bicgstab_info["last_iterations"])
    Y = pkg.DeviceVectors.from_host(B, ctx).apply(bs).download()
    for j in range(3):
        assert np.array_equal(_bits(Y[:, j]), _bits(singles[j])), j
    info = bs.bicgstab_info
    assert info["applications"] == 6 and info["iterations"] == 2 * sum(its) and info["last_iterations"] == its[2], (info, its)
    # (A - sigma)^-1 K x with K a stored matrix: the product operator against the two steps taken one by one
    Kh = cases.grid_matrix("convdiff")
    K = pkg.csr_operator(Kh, ctx)
    x = rng.standard_normal(n)
    Kx = Solver(K)(x)
    want = solve(Kx)
    prod = pkg.product_operator(bs, K, ctx=ctx)
    got = Solver(prod)(x)
    assert np.array_equal(_bits(got), _bits(want))
    assert bs.bicgstab_info["applications"] == 8
    # (K x on the device and on the host differ by roundings: eps ||K|| ||x|| on the right-hand side, far inside the factor 2)
    assert cases.true_residual(A, got, Kh @ x, shift) <= 2 * TOL * np.linalg.norm(Kh @ x)


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_eigenvalues_nearest_a_shift_end_to_end(ctx):
    """The four eigenvalues of swirl nearest sigma = 2.0 -- two complex pairs, 2.844 +- 0.297 i and 3.055 +- 0.298 i -- by shift-invert
    through BiCGStab(2) (inner tol 1e-13, outer tol 1e-10, which = LM) with every vector in HBM: lambda = sigma + 1 / mu against
    numpy.linalg.eigvals of the host matrix to 1e-8, and ||A x - lambda x|| <= 1e-8 against the ORIGINAL operator."""
    sigma = 2.0
    Ah = pkg.host_grid_matrix(cases.SHAPE, cases.taps("swirl"), cases.V)
    A = _grid("swirl", np.float64, ctx)
    n = Ah.shape[0]
    ev = np.linalg.eigvals(Ah.toarray())
    nearest = ev[np.argsort(np.abs(ev - sigma))[:4]]
    assert np.allclose(np.sort_complex(nearest), [2.84436439 - 0.29708184j, 2.84436439 + 0.29708184j, 3.05478566 - 0.29834683j, 3.05478566 + 0.29834683j],
                       rtol=0, atol=5e-8)
    S = pkg.bicgstab_operator(A, shift=sigma, tol=1e-13)
    P, hist = pkg.partialschur(S, v1=pkg.matrices.start_vector(n), nev=4, which="LM", tol=1e-10)
    assert hist.converged and P.nconverged >= 4, hist
    mu, X = pkg.partialeigen(P, device=True)
    lam = np.ascontiguousarray(extras.interior_eigenvalues(mu, sigma))
    r, _ = pkg.residuals(A, X, lam)
    xn = np.sqrt(np.real(np.diag(pkg.gram(X, X))))
    info = S.bicgstab_info
    print("%s; bicgstab %s; lambda = %s, ||A x - lambda x|| = %s, ||x|| = %s, |lambda - ev| = %s"
          % (hist, info, lam, r, xn, [float(np.abs(ev - lj).min()) for lj in lam]))
    order = np.argsort(-np.abs(mu))[:4]
    got = np.sort_complex(lam[order])
    assert np.allclose(got, np.sort_complex(nearest), rtol=0, atol=1e-8), (got, nearest)
    assert np.all(r[order] <= 1e-8), r
    assert info["applications"] >= hist.mvproducts and info["worst_relres"] <= 1e-13 * ROUND
