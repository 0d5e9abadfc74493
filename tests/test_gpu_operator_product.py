"""`-m gpu`: products of device operators (`ks_operator_product`, csrc/ks_product.hpp): y = ops[0] ops[1] ... ops[k-1] x with every
intermediate vector resident in HBM.  The reference side is the composed LinearMaps of the user guide's recipes for generalized
problems: `mul!(temp, B, x); ldiv!(y, A_lu, temp)` (docs/src/index.md:273-287) and `M.L' \\ (M.A * (M.L \\ x))`
(docs/src/index.md:325-336), whose temporaries live on the host there.

A product launches exactly the kernels its factors launch, on the same inputs: it is compared BIT FOR BIT with the factors applied
one by one through the columns of a second workspace, and with the scipy product at 1e-12 relative to max|y| (forward products of
short sparse rows: a few eps).  Mixed products with a triangular solve use the tolerance and matrices of
tests/test_gpu_lu_operator.py (1e-11 against the host solve of the same factorisation)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from __graft_entry__ import ROOT, import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
extras = importlib.import_module(pkg.__name__ + ".extras")
TOL = 1e-11        # products with a triangular solve in them (tests/test_gpu_lu_operator.py)
TOL_MUL = 1e-12    # products of stored matrices only
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


def _lap2d(nx, ny):
    ex = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    ey = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(ny, ny))
    return (sp.kron(sp.identity(ny), ex) + sp.kron(ey, sp.identity(nx))).tocsc()


def _fem(n):
    return sp.diags([np.full(n - 1, 1.0 / 6.0), np.full(n, 4.0 / 6.0), np.full(n - 1, 1.0 / 6.0)], [-1, 0, 1])


def _random_matrix(n, cplx, seed):
    """(tests/test_gpu_lu_operator.py)"""
    A = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=seed, format="csc") + 4.0 * sp.identity(n)
    if cplx:
        A = A + 1j * sp.random(n, n, density=min(1.0, 3.0 / n), random_state=seed + 1, format="csc")
    return A.tocsc()


def _sparse(n, cplx, seed):
    """about five entries per row, no structure: two of these do not commute"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=min(1.0, 5.0 / n), random_state=rng, format="csr")
    if cplx:
        A = A + 1j * sp.random(n, n, density=min(1.0, 5.0 / n), random_state=rng, format="csr")
    return A.tocsr().astype(np.complex128 if cplx else np.float64)


def _vec(n, cplx, seed=0):
    rng = np.random.default_rng(77 + n + seed)
    return rng.random(n) + (1j * rng.random(n) if cplx else 0.0)


def _ws(n, dtype, ctx, k=3):
    return pkg.ArnoldiWorkspace(n, min(k, n), dtype, ctx=ctx)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 5000])
def test_order_and_ping_pong(ctx, n, cplx):
    dt = np.complex128 if cplx else np.float64
    mats = [_sparse(n, cplx, 10 * n + k) for k in range(3)]
    if n <= 300:
        rng = np.random.default_rng(n)
        mats.append((rng.random((n, n)) + (1j * rng.random((n, n)) if cplx else 0.0)).astype(dt))
    ops = [pkg.csr_operator(m, ctx) for m in mats[:3]] + ([pkg.dense_operator(mats[3], ctx)] if n <= 300 else [])
    last = len(ops) - 1   # the dense factor where there is one
    x = _vec(n, cplx).astype(dt)
    ws, ws2 = _ws(n, dt, ctx, 1), _ws(n, dt, ctx, 1)
    ws.set_col(0, x)
    for chain in ([0, 1], [0, last, 1], [0, 1, last, 0]):   # two, three and four factors (four: the first intermediate is used twice)
        prod = pkg.product_operator(*[ops[i] for i in chain], ctx=ctx)
        assert prod.factors == tuple(ops[i] for i in chain) and prod.dtype == dt and prod.shape == (n, n)
        assert prod.format["layout"] == "none" and prod.format["bytes_per_nnz"] == 0.0
        ws.apply(prod, 0, 1)
        y = ws.col(1)
        assert np.array_equal(ws.col(0), x)              # a basis column comes back untouched
        # the factors one by one, rightmost first, ping-pong between the two columns of another workspace
        ws2.set_col(0, x)
        src, want = 0, x
        for i in reversed(chain):
            ws2.apply(ops[i], src, 1 - src)
            src = 1 - src
            want = mats[i] @ want
        assert np.array_equal(y, ws2.col(src)), chain
        assert np.abs(y - want).max() <= TOL_MUL * np.abs(want).max(), chain
        for _ in range(3):
            ws.apply(prod, 0, 1)
            assert np.array_equal(ws.col(1), y)
        if n >= 63:                                      # (1 x 1 matrices commute)
            rev = pkg.product_operator(*[ops[i] for i in reversed(chain)], ctx=ctx)
            ws.apply(rev, 0, 1)
            assert not np.array_equal(ws.col(1), y), chain


@pytest.mark.parametrize("n,cplx", [(300, False), (300, True), (5000, False)], ids=["300-f64", "300-c128", "5000-f64"])
def test_triangular_solves_after_a_stored_matrix(ctx, n, cplx):
    """recipe 2 by hand: y = A^-1 (B x) from splu_operator and csr_operator, against the host lu.solve(B @ x).  (n = 5000 in Float64
    only: these random matrices fill in completely, and SuperLU alone takes ten seconds and more on the ComplexF64 one.)"""
    A, B = _random_matrix(n, cplx, seed=n), _random_matrix(n, cplx, seed=n + 7).tocsr()
    lu = spla.splu(A)
    solve, mul = pkg.splu_operator(lu, ctx), pkg.csr_operator(B, ctx)
    prod = pkg.product_operator(solve, mul, ctx=ctx)
    x = _vec(n, cplx).astype(prod.dtype)
    ws = _ws(n, prod.dtype, ctx)
    ws.set_col(0, x)
    ws.apply(prod, 0, 1)
    want = lu.solve(B @ x)
    assert np.abs(ws.col(1) - want).max() <= TOL * np.abs(want).max()
    L = pkg._lib.load()
    nl, nnz, dtc = C.c_int64(), C.c_int64(), C.c_int()
    sizes = []
    for op in (prod, solve, mul):
        pkg._lib.check(L.ks_operator_size(op._h, C.byref(nl), C.byref(nnz), C.byref(dtc)))
        sizes.append((nl.value, nnz.value, dtc.value))
    assert sizes[0] == (n, sizes[1][1] + sizes[2][1], sizes[1][2])      # nnz: the sum of the factors'


def test_the_same_factor_twice(ctx):
    n = 300
    A = _sparse(n, False, 5)
    op = pkg.csr_operator(A, ctx)
    prod = pkg.product_operator(op, op, ctx=ctx)
    x = _vec(n, False)
    ws = _ws(n, np.float64, ctx)
    ws.set_col(0, x)
    ws.apply(prod, 0, 1)
    want = A @ (A @ x)
    assert np.abs(ws.col(1) - want).max() <= TOL_MUL * np.abs(want).max()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_a_host_callback_in_the_middle(ctx, cplx):
    """A host-callback factor makes the product a host operator (one step per batch); the expansion hands it its input scale, which
    reaches the callback factor and cancels: the Arnoldi relation of five steps holds like that of any operator
    (tests/test_gpu_lu_operator.py: 1e-12 ||H||, sqrt(eps) / 100)."""
    n = 300
    dt = np.complex128 if cplx else np.float64
    A, B = _random_matrix(n, cplx, 3).tocsr(), _random_matrix(n, cplx, 4).tocsr()
    calls = []

    def cb(y, x):
        calls.append(np.linalg.norm(x))
        y[:] = B @ x

    opA = pkg.csr_operator(A, ctx)
    prod = pkg.product_operator(opA, pkg.host_operator(cb, n, dt, ctx), opA, ctx=ctx)
    x = _vec(n, cplx).astype(dt)
    ws = pkg.ArnoldiWorkspace(n, 6, dt, ctx=ctx)
    ws.set_col(0, x)
    ws.apply(prod, 0, 1)
    want = A @ (B @ (A @ x))
    assert np.abs(ws.col(1) - want).max() <= TOL_MUL * np.abs(want).max() and len(calls) == 1
    assert not prod.factors[1].errors
    ws.reinitialize(0, x)
    st = ws.iterate_arnoldi(prod, 1, 5)
    assert st["steps"] == 5 and st["breakdowns"] == 0 and len(calls) >= 6
    res, orth = ws.arnoldi_relation(prod, 5)
    hn = np.linalg.norm(ws.H)
    assert res <= 1e-12 * hn and orth <= np.sqrt(EPS) / 100, (res / hn, orth)


class _Boom(Exception):
    pass


def test_an_exception_in_a_callback_factor_surfaces_as_itself(ctx):
    n = 64

    def cb(y, x):
        raise _Boom("inside the factor")

    op = pkg.csr_operator(_sparse(n, False, 1), ctx)
    prod = pkg.product_operator(op, pkg.host_operator(cb, n, np.float64, ctx), op, ctx=ctx)
    ws = _ws(n, np.float64, ctx)
    ws.set_col(0, _vec(n, False))
    with pytest.raises(_Boom, match="inside the factor"):
        ws.apply(prod, 0, 1)
    # ... and the factors are none the worse for it
    ws.apply(op, 0, 1)
    assert np.abs(ws.col(1) - _sparse(n, False, 1) @ _vec(n, False)).max() <= TOL_MUL * np.abs(ws.col(1)).max()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_newton_step_of_a_product(ctx, cplx):
    """apply_shifted stays the base-class default: sigma (A x - theta x) from the product and one streaming pass"""
    n = 300
    dt = np.complex128 if cplx else np.float64
    ops = [pkg.csr_operator(_sparse(n, cplx, 20 + k), ctx) for k in range(3)]
    prod = pkg.product_operator(*ops, ctx=ctx)
    x = _vec(n, cplx).astype(dt)
    theta, sigma = (0.7 - 0.4j if cplx else 0.7), 1.3
    ws = _ws(n, dt, ctx)
    ws.set_col(0, x)
    ws.apply(prod, 0, 1)
    want = sigma * (ws.col(1) - theta * x)
    ws.apply_shifted(prod, 0, 2, theta, sigma)
    assert np.abs(ws.col(2) - want).max() <= 1e-13 * np.abs(want).max()
    assert np.array_equal(ws.col(0), x)


def test_products_stay_inside_the_workspace(ctx, monkeypatch):
    monkeypatch.setenv("KS_GUARD", "1")
    for n, cplx in ((65, False), (300, True), (5000, False)):
        dt = np.complex128 if cplx else np.float64
        mats = [_sparse(n, cplx, 30 + k) for k in range(3)]
        prod = pkg.product_operator(*[pkg.csr_operator(m, ctx) for m in mats], ctx=ctx)
        ws = pkg.ArnoldiWorkspace(n, 3, dt, ctx=ctx)
        x = _vec(n, cplx).astype(dt)
        want = mats[0] @ (mats[1] @ (mats[2] @ x))
        for src, dst in ((0, 3), (3, 0)):
            ws.set_col(src, x)
            ws.apply(prod, src, dst)
            assert np.abs(ws.col(dst) - want).max() <= TOL_MUL * np.abs(want).max()
            assert np.array_equal(ws.col(src), x)
        assert ws.guard_intact(), (n, cplx)


def test_destroying_the_product_leaves_the_factors_usable(ctx):
    n = 300
    A, B = _sparse(n, False, 40), _sparse(n, False, 41)
    a, b = pkg.csr_operator(A, ctx), pkg.csr_operator(B, ctx)
    prod = pkg.product_operator(a, b, ctx=ctx)
    x = _vec(n, False)
    ws = _ws(n, np.float64, ctx)
    ws.set_col(0, x)
    ws.apply(prod, 0, 1)
    prod.close()
    del prod
    for op, M in ((a, A), (b, B)):
        ws.apply(op, 0, 1)
        want = M @ x
        assert np.abs(ws.col(1) - want).max() <= TOL_MUL * np.abs(want).max()


# ------------------------------------------------------------------ the two recipes, end to end
_DENSE = {}


def _recipe2_problem(cplx):
    nx, ny = 30, 35
    n = nx * ny
    A = _lap2d(nx, ny)
    if cplx:
        A = (A.astype(np.complex128) + 1j * sp.diags(0.3 * np.random.default_rng(5).random(n))).tocsc()
    B = sp.kron(_fem(ny), _fem(nx)).tocsr()
    return n, A, B, (1.7 + 0.1j if cplx else 1.7)


def _recipe2_spectrum(cplx):
    """scipy.linalg.eigvals(A, B) of the dense pencil, RECORDED (tests/golden/make_recipe2_spectrum.py: the QZ iteration of the 1050 x
    1050 ComplexF64 pencil takes 17 s).  The record is tied to the matrices here by the trace: sum(lambda) = tr(B^-1 A)."""
    if cplx not in _DENSE:
        _, A, B, _ = _recipe2_problem(cplx)
        lam = np.load(os.path.join(ROOT, "tests", "golden", f"recipe2_pencil_eigvals_{'c128' if cplx else 'f64'}.npy"))
        tr = np.trace(np.linalg.solve(B.toarray(), A.toarray()))
        assert lam.shape == (A.shape[0],) and abs(lam.sum() - tr) <= 1e-10 * abs(tr)
        _DENSE[cplx] = lam
    return _DENSE[cplx]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_recipe_2_generalized_shift_invert(ctx, cplx):
    """docs/src/index.md:262-304 with the inverse and the product on the device: A the 2-D Laplacian (+ i diag), B the consistent mass
    of bilinear elements, the six eigenvalues of A x = B x lambda nearest sigma."""
    n, A, B, sigma = _recipe2_problem(cplx)
    op = extras.generalized_shift_invert(A, B, sigma, ctx)
    assert len(op.factors) == 2 and op.factor_residual <= 1e-10
    v1 = pkg.matrices.start_vector(n).astype(op.dtype)
    kw = dict(nev=6, which="LM", tol=1e-10, mindim=10, maxdim=20)
    dec, hist = pkg.partialschur_(op, pkg.ArnoldiWorkspace(v1, 20, ctx=ctx), **kw)
    assert hist.converged and dec.nconverged >= 6
    exact = _recipe2_spectrum(cplx)
    lam = sigma + 1.0 / np.asarray(dec.eigenvalues)
    dist = np.array([np.abs(exact - z).min() for z in lam])
    print(f"{hist.mvproducts} products, distance to the dense spectrum {dist.max():.2e}")
    assert dist.max() <= 1e-8
    # step by step: the trail of the same solve through a host callback around the same factorisation
    M = (sp.csc_matrix(A, dtype=op.dtype) - sigma * B.tocsc()).tocsc()
    lu = spla.splu(M, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))

    def cb(y, x):
        y[:] = lu.solve(B @ x)

    hop = pkg.host_operator(cb, n, op.dtype, ctx)
    ws = pkg.ArnoldiWorkspace(v1, 20, ctx=ctx)
    ws.set_sstep(0)
    dec1, hist1 = pkg.partialschur_(op, ws, **kw)
    dec2, hist2 = pkg.partialschur_(hop, pkg.ArnoldiWorkspace(v1, 20, ctx=ctx), **kw)
    assert hist1.converged and hist2.converged
    assert (hist1.mvproducts, hist1.nconverged) == (hist2.mvproducts, hist2.nconverged)


def test_recipe_3_b_orthonormal_schur_vectors(ctx):
    """docs/src/index.md:306-352 with a NON-diagonal B (the consistent mass; its Cholesky factor is bidiagonal: a chain of n dependent
    rows in both triangular solves): Q = L^-* Y is B-orthonormal and Q' A Q = R.  The reference's transcript for its diagonal B
    reads 3.9e-14 / 3.2e-15; the CPU oracle on this problem gives 1.2e-12 / 8e-15 in 213 products, the bounds are ~100x those."""
    n = 300
    B = _fem(n).toarray()
    L = sp.csr_matrix(np.linalg.cholesky(B))
    L.eliminate_zeros()
    A = (sp.random(n, n, 0.03, random_state=np.random.default_rng(11)) + sp.diags(np.linspace(1.0, 3.0, n))).tocsr()
    op, back = extras.b_orthonormal_operator(A, L, ctx)
    assert len(op.factors) == 3
    dec, hist = pkg.partialschur(op, nev=4, which="LM", tol=1e-10, v1=pkg.matrices.start_vector(n))
    assert hist.converged
    Q, R = back(dec.Q), np.array(dec.R)
    ra, rb = np.linalg.norm(Q.T @ (A @ Q) - R), np.linalg.norm(Q.T @ B @ Q - np.eye(Q.shape[1]))
    print(f"{hist.mvproducts} products: ||Q'AQ - R|| {ra:.2e}  ||Q'BQ - I|| {rb:.2e}")
    assert ra <= 1e-10 and rb <= 1e-12


def test_wrong_use_is_refused(ctx):
    n = 50
    a = pkg.csr_operator(_sparse(n, False, 1), ctx)
    with pytest.raises(pkg.ArgumentError, match="factors"):
        pkg.product_operator(a, ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="factors"):
        pkg.product_operator(*([a] * 9), ctx=ctx)
    pkg.product_operator(*([a] * 8), ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="factor 1 is null"):
        pkg.product_operator(a, None, ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="factor 2 has 51 rows"):
        pkg.product_operator(a, a, pkg.csr_operator(_sparse(n + 1, False, 1), ctx), ctx=ctx)
    with pytest.raises(pkg.ArgumentError, match="factor 1 does not have the element type"):
        pkg.product_operator(a, pkg.csr_operator(_sparse(n, True, 1), ctx), ctx=ctx)
    other = pkg.Context(0)
    with pytest.raises(pkg.ArgumentError, match="factor 1 lives on another context"):
        pkg.product_operator(a, pkg.csr_operator(_sparse(n, False, 2), other), ctx=ctx)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.product_operator(a, a, ctx=dctx)
