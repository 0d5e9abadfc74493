"""`-m gpu`: the fused tridiagonal pencil operator y = (K - sigma M)^-1 M x (`ks_operator_tridiag_pencil`, csrc/ks_tridiag.hpp):
T = K - sigma M factored once like `ks_operator_tridiag_solve` factors it, and level 0 of k_td_down forming M x while it stages its
right-hand side.  The reference side is the `ShiftAndInvert` LinearMap of docs/src/index.md:273-287 (`mul!(temp, B, x);
ldiv!(y, A_lu, temp)`) on a 1-D pencil (FEM stiffness and consistent mass).

Products are checked against the HOST path of the same pencil (`host_tridiagonal_pencil_solve`: the same T, M b in the same order,
the host walk of the same factors -- the difference is FMA contraction only; forming M b in another summation order moves the
solution by <= 1e-13 relative to max|y| on these families) at 1e-11 relative to max|y|, the project's product tolerance, and against
the pencil itself through the normwise backward error eta <= 64 eps of tests/test_tridiag_pencil_cpu.py (host path: <= 8.9e-16)."""
import numpy as np
import pytest
import scipy.sparse as sp

from __graft_entry__ import import_package
from pencil_cases import ETA_BOUND, FAMILIES, IDS, SIZES, default_levels, family, mass, pencil, pencil_eta, rhs, shifted

pytestmark = pytest.mark.gpu
pkg = import_package()
TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


def _apply(op, b, ctx):
    n = b.shape[0]
    ws = pkg.ArnoldiWorkspace(n, min(4, n - 1) if n > 1 else 1, op.dtype, ctx=ctx)
    ws.set_col(0, b.astype(op.dtype))
    ws.apply(op, 0, 1)
    return ws.col(1), ws


@pytest.mark.parametrize("kname,mname,cplx,sigma", FAMILIES, ids=IDS)
@pytest.mark.parametrize("n,block_rows", SIZES)
def test_product_matches_the_host_path_of_the_same_pencil(ctx, kname, mname, cplx, sigma, n, block_rows):
    K, M, sg = pencil(kname, mname, n, cplx, sigma)
    b = rhs(n, cplx)
    op = pkg.tridiagonal_pencil_operator(*K, *M, sigma=sg, ctx=ctx, block_rows=block_rows)
    y, ws = _apply(op, b, ctx)
    x, info = pkg.host_tridiagonal_pencil_solve(*K, *M, b, sigma=sg, block_rows=block_rows)
    e_dev, e_host = pencil_eta(K, M, sg, y, b), pencil_eta(K, M, sg, x, b)
    diff = np.abs(y - x).max() / np.abs(x).max()
    print(f"{kname} {mname} {'c128' if cplx else 'f64'} n={n} m={block_rows}: eta device {e_dev:.2e} host {e_host:.2e}  |dev - host| {diff:.2e}  {info}")
    assert np.abs(y - x).max() <= TOL * np.abs(x).max()
    assert e_dev <= ETA_BOUND
    assert op.tridiag_info == info
    assert info["levels"] == default_levels(n, block_rows)
    for _ in range(3):                                   # deterministic: bit-identical when repeated
        ws.apply(op, 0, 1)
        assert np.array_equal(ws.col(1), y)


@pytest.mark.parametrize("kname,cplx", [("b", True), ("d", False)])
@pytest.mark.parametrize("n,block_rows", SIZES)
def test_identity_mass_is_the_plain_operator_bit_for_bit(ctx, kname, cplx, n, block_rows):
    """M = I (md = 1, off-diagonals 0): the fused right-hand side is a pure pass-through (1 x + 0 x' + 0 x'' = x exactly) and
    T = K - sigma I is what the plain operator forms itself, so the product equals that of `tridiagonal_solve_operator(K, sigma)`
    bit for bit -- the solve behind the fused staging loop is the untouched one."""
    dl, d, du, sg = family(kname, n, cplx)
    b = rhs(n, cplx)
    want, _ = _apply(pkg.tridiagonal_solve_operator(dl, d, du, sigma=sg, ctx=ctx, block_rows=block_rows), b, ctx)
    got, _ = _apply(pkg.tridiagonal_pencil_operator(dl, d, du, *mass("identity", n, cplx), sigma=sg, ctx=ctx, block_rows=block_rows), b, ctx)
    assert np.array_equal(got, want)


def _tridiag_csr(dl, d, du):
    return sp.diags([dl, d, du], [-1, 0, 1], format="csr")


@pytest.mark.parametrize("kname,mname,cplx,sigma", [FAMILIES[0], FAMILIES[4]], ids=[IDS[0], IDS[4]])
@pytest.mark.parametrize("n,block_rows", [(341, 4), (4226, 0), (8449, 0), (70000, 0)])
def test_fused_against_composed(ctx, kname, mname, cplx, sigma, n, block_rows):
    """The same product from two launches more and one vector more: product_operator(tridiagonal_solve_operator(T, 0), csr_operator(M))."""
    K, M, sg = pencil(kname, mname, n, cplx, sigma)
    b = rhs(n, cplx)
    fused = pkg.tridiagonal_pencil_operator(*K, *M, sigma=sg, ctx=ctx, block_rows=block_rows)
    T = shifted(K, M, sg)
    solve = pkg.tridiagonal_solve_operator(*T, sigma=0.0, ctx=ctx, block_rows=block_rows)
    composed = pkg.product_operator(solve, pkg.csr_operator(_tridiag_csr(*M), ctx), ctx=ctx)
    assert fused.tridiag_info == solve.tridiag_info
    y, _ = _apply(fused, b, ctx)
    z, _ = _apply(composed, b, ctx)
    print(f"n={n}: |fused - composed| {np.abs(y - z).max() / np.abs(z).max():.2e}")
    assert np.abs(y - z).max() <= TOL * np.abs(z).max()


@pytest.mark.parametrize("n,block_rows", [(341, 4), (4226, 0)])
def test_products_stay_inside_the_workspace(ctx, n, block_rows, monkeypatch):
    """KS_GUARD=1 puts canary zones on both sides of the basis.  Column 0 as the source is the case an unguarded x[r - 1] load gets
    wrong (it would read the canary in front of the basis), the last column the one an unguarded x[r + 1] would."""
    monkeypatch.setenv("KS_GUARD", "1")
    for kname, mname, cplx, sigma in (FAMILIES[3], FAMILIES[4]):
        K, M, sg = pencil(kname, mname, n, cplx, sigma)
        op = pkg.tridiagonal_pencil_operator(*K, *M, sigma=sg, ctx=ctx, block_rows=block_rows)
        ws = pkg.ArnoldiWorkspace(n, 3, op.dtype, ctx=ctx)
        b = rhs(n, cplx)
        x, _ = pkg.host_tridiagonal_pencil_solve(*K, *M, b, sigma=sg, block_rows=block_rows)
        for src, dst in ((0, 3), (3, 0), (1, 2)):
            ws.set_col(src, b)
            ws.apply(op, src, dst)
            assert np.abs(ws.col(dst) - x).max() <= TOL * np.abs(x).max(), (src, dst)
            assert np.array_equal(ws.col(src), b.astype(op.dtype))
        assert ws.guard_intact(), (n, cplx)


def test_float64_whole_solve_against_the_analytic_spectrum(ctx):
    """K = laplace1d(1000), M the consistent mass: the pencil's eigenvalues are 6 (1 - c_k) / (2 + c_k), c_k = cos(k pi / (n + 1))
    (both matrices share the sine eigenvectors).  The four nearest sigma = 1; their gaps are 2.1e-3 and 4.9e-3."""
    n, sigma = 1000, 1.0
    K, M, _ = pencil("a", "fem", n, False, sigma)
    op = pkg.tridiagonal_pencil_operator(*K, *M, sigma=sigma, ctx=ctx)
    v1 = pkg.matrices.start_vector(n)
    ws = pkg.ArnoldiWorkspace(v1, 20, ctx=ctx)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="LM", tol=1e-13, mindim=10, maxdim=20)
    assert hist.converged and dec.nconverged >= 4
    c = np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
    exact = 6.0 * (1.0 - c) / (2.0 + c)
    want = exact[np.argsort(np.abs(exact - sigma))][:4]
    theta = dec.eigenvalues[np.argsort(-np.abs(dec.eigenvalues))][:4]
    lam = sigma + 1.0 / theta
    np.testing.assert_allclose(np.sort(lam.real), np.sort(want), atol=1e-8)
    assert np.abs(lam.imag).max() <= 1e-8
    dres, dorth = dec.workspace.residual_norms(op, dec.nconverged)
    print(f"residual {dres:.2e} orthogonality {dorth:.2e} nconverged {dec.nconverged} products {hist.mvproducts}")
    assert dres <= 1e-10 and dorth <= 1e-12


_ORACLE = {}


def _config4_pencil():
    from oracle import arnoldi as oa
    from oracle.matrices import laplace1d

    n = 400
    rng = np.random.default_rng(3)
    Kmat = (laplace1d(n) + 1j * sp.diags(0.3 * rng.random(n))).tocsc().astype(np.complex128)
    M = mass("fem", n)
    Mmat = _tridiag_csr(*M).tocsc().astype(np.complex128)
    sigma = 1.7 + 0.1j
    v1 = oa.uniform_hash(1, np.arange(n)) + 1j * oa.uniform_hash(2, np.arange(n))
    return n, Kmat, M, Mmat, sigma, v1


def _config4_oracle():
    """The oracle driven by host splu(K - sigma M) and M @ x, once for both runs."""
    if "c4" not in _ORACLE:
        import scipy.sparse.linalg as spla

        from oracle import arnoldi as oa

        n, Kmat, _, Mmat, sigma, v1 = _config4_pencil()
        lu = spla.splu((Kmat - sigma * Mmat).tocsc())

        class HostPencil:
            shape = (n, n)
            dtype = np.complex128

            def mul_(self, y, x):
                y[:] = lu.solve(Mmat @ x)

        _ORACLE["c4"] = oa.partialschur(HostPencil(), v1=v1, nev=6, which="LM", tol=1e-10, mindim=10, maxdim=20)
    return _ORACLE["c4"]


@pytest.mark.parametrize("sstep", [None, 0], ids=["blocks", "steps"])
def test_config4_whole_solve_on_the_pencil(ctx, sstep):
    """BASELINE config 4's matrix as K (laplace1d + i diag(0.3 rand)), the consistent mass as M, sigma = 1.7 + 0.1i: converged, the six
    eigenvalues of the pencil nearest sigma at 1e-8 against the dense generalized spectrum, eigenpairs of the pencil itself; step by
    step, the mat-vec count of the oracle driven by host splu(K - sigma M) and M @ x."""
    import scipy.linalg as sla

    n, Kmat, M, Mmat, sigma, v1 = _config4_pencil()
    op = pkg.tridiagonal_pencil_operator(Kmat.diagonal(-1), Kmat.diagonal(0), Kmat.diagonal(1), *M, sigma=sigma, ctx=ctx)
    ws = pkg.ArnoldiWorkspace(v1, 20, ctx=ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    dec, hist = pkg.partialschur_(op, ws, nev=6, which="LM", tol=1e-10, mindim=10, maxdim=20)
    ref, rhist = _config4_oracle()
    print(f"{'blocks' if sstep is None else 'steps'}: {hist.mvproducts} products (oracle {rhist.mvproducts})")
    assert hist.converged
    if sstep == 0:
        assert hist.mvproducts == rhist.mvproducts
    if "exact" not in _ORACLE:
        _ORACLE["exact"] = sla.eigvals(Kmat.toarray(), Mmat.toarray())
    exact = _ORACLE["exact"]
    want = exact[np.argsort(np.abs(exact - sigma))][:6]
    theta = dec.eigenvalues[np.argsort(-np.abs(dec.eigenvalues))][:6]
    np.testing.assert_allclose(np.sort_complex(sigma + 1.0 / theta), np.sort_complex(want), atol=1e-8)
    vals, vecs = pkg.partialeigen(dec)
    X, lam = np.asarray(vecs), sigma + 1.0 / np.asarray(vals)
    assert np.linalg.norm(Kmat @ X - (Mmat @ X) * lam[None, :]) <= 1e-8 * np.linalg.norm(Kmat.toarray())


def test_wrong_use_is_refused(ctx):
    K, M, sg = pencil("d", "rand", 100, False, 0.25)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.tridiagonal_pencil_operator(*K, *M, sigma=sg, ctx=dctx)
    # M's diagonals of the wrong lengths
    with pytest.raises(pkg.DimensionMismatch):
        pkg.tridiagonal_pencil_operator(*K, M[0], M[1][:-1], M[2], sigma=sg, ctx=ctx)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.tridiagonal_pencil_operator(*K, M[0][:-1], M[1], M[2], sigma=sg, ctx=ctx)
    # the refusals of the plain operator, before anything is uploaded
    with pytest.raises(pkg.ArgumentError):
        pkg.tridiagonal_pencil_operator(*K, *M, sigma=sg, ctx=ctx, block_rows=65)
    # a singular T: family c at an odd size (zero diagonal), M with a zero diagonal, so no shift moves it
    n = 401
    dl, d, du, _ = family("c", n, sigma="odd")
    with pytest.raises(pkg.ArgumentError):
        pkg.tridiagonal_pencil_operator(dl, d, du, np.full(n - 1, 1.0 / 6.0), np.zeros(n), np.full(n - 1, 1.0 / 6.0), sigma=0.0, ctx=ctx)
