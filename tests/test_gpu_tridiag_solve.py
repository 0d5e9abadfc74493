"""`-m gpu`: the library's own tridiagonal shift-invert operator (`ks_operator_tridiag_solve`, csrc/ks_tridiag.hpp): factored once
on the host at upload, applied by k_td_down / k_td_up with every vector resident in HBM.  The reference side is the LinearMap of
docs/src/index.md:234-259 -- `(y, x) -> ldiv!(y, factorize(A - sigma I), x)` -- on a 1-D operator.

Products are checked against the HOST path of the same factorisation (`ks_host_tridiag_solve` walks the same arrays in the same
order: the difference is FMA contraction only) at 1e-11 relative to max|y| -- tolerance and form of tests/test_gpu_lu_operator.py --
and against the matrix itself through the normwise backward error eta <= 64 eps of tests/test_tridiag_solve_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from __graft_entry__ import import_package
from tridiag_cases import ETA_BOUND, default_levels, eta, family, rhs

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


def _product_case(ctx, name, cplx, n, sigma, block_rows, expect_rows=None):
    dl, d, du, sg = family(name, n, cplx, sigma)
    b = rhs(n, cplx)
    op = pkg.tridiagonal_solve_operator(dl, d, du, sigma=sg, ctx=ctx, block_rows=block_rows)
    y, ws = _apply(op, b, ctx)
    x, info = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=block_rows)
    e_dev, e_host = eta(dl, d, du, sg, y, b), eta(dl, d, du, sg, x, b)
    diff = np.abs(y - x).max() / np.abs(x).max()
    print(f"{name} {'c128' if cplx else 'f64'} n={n} m={block_rows}: eta device {e_dev:.2e} host {e_host:.2e}  |dev - host| {diff:.2e}  {info}")
    assert e_dev <= ETA_BOUND
    assert np.abs(y - x).max() <= TOL * np.abs(x).max()
    assert op.tridiag_info == info                       # the operator reports what the host path reports for the same input
    assert info["levels"] == default_levels(n, block_rows)
    if expect_rows is not None:
        assert info["level_rows"] == expect_rows, info
    for _ in range(3):                                   # deterministic: bit-identical when repeated
        ws.apply(op, 0, 1)
        assert np.array_equal(ws.col(1), y)
    return op, ws


PRODUCTS = [(n, 4) for n in (1, 2, 5, 6, 11, 25, 26, 341)] + [(n, 0) for n in (64, 65, 66, 131, 4226, 70000)]


@pytest.mark.parametrize("name,cplx", [("b", True), ("b", False), ("d", False), ("d", True)])
@pytest.mark.parametrize("n,block_rows", PRODUCTS)
def test_product_matches_the_host_path_of_the_same_factorisation(ctx, name, cplx, n, block_rows):
    _product_case(ctx, name, cplx, n, None, block_rows)


@pytest.mark.parametrize("n,block_rows", [(400, 4), (70000, 0)])
@pytest.mark.parametrize("name,sigma", [("a", 1.7), ("a", 1.0), ("a", 2.0), ("c", None)])
def test_indefinite_and_zero_diagonal_products(ctx, name, sigma, n, block_rows):
    """Real indefinite T - sigma I and the zero diagonal (every pivot an interchange, shortened blocks on the reduced levels)."""
    _product_case(ctx, name, False, n, sigma, block_rows)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("n,block_rows,rows", [
    (129, 0, [129, 1]),             # level 1 has exactly one row
    (8384, 0, [8384, 128]),         # ... exactly the direct limit (2 x 64): 129 blocks = 3 workgroups, the last one with one block
    (8385, 0, [8385, 129, 1]),      # ... one more than the limit: a third level
    (8449, 0, [8449, 129, 1]),      # 130 blocks, the last a 64-row tail without separator
    (9, 4, [9, 1]),
    (44, 4, [44, 8]),
    (45, 4, [45, 9, 1]),
    (700, 4, [700, 140, 28, 5]),    # 140 blocks of 4: three workgroups at level 0, a ragged last one
])
def test_multi_workgroup_and_level_edges(ctx, n, block_rows, rows, cplx):
    _product_case(ctx, "d", cplx, n, None, block_rows, expect_rows=rows)


@pytest.mark.parametrize("n,block_rows", [(341, 4), (4226, 0)])
def test_products_stay_inside_the_workspace(ctx, n, block_rows, monkeypatch):
    """KS_GUARD=1 puts canary zones on both sides of the basis: products into its first and its last column leave them intact."""
    monkeypatch.setenv("KS_GUARD", "1")
    for cplx in (False, True):
        dl, d, du, sg = family("b", n, cplx)
        op = pkg.tridiagonal_solve_operator(dl, d, du, sigma=sg, ctx=ctx, block_rows=block_rows)
        ws = pkg.ArnoldiWorkspace(n, 3, op.dtype, ctx=ctx)
        b = rhs(n, cplx)
        x, _ = pkg.host_tridiagonal_solve(dl, d, du, b, sigma=sg, block_rows=block_rows)
        for src, dst in ((0, 3), (3, 0), (1, 2)):
            ws.set_col(src, b)
            ws.apply(op, src, dst)
            assert np.abs(ws.col(dst) - x).max() <= TOL * np.abs(x).max()
            assert np.array_equal(ws.col(src), b.astype(op.dtype))
        assert ws.guard_intact(), (n, cplx)


_ORACLE = {}


def _config4_oracle(n, sigma, A, v1):
    """The oracle driven by host splu, once for both runs."""
    if "c4" not in _ORACLE:
        import scipy.sparse.linalg as spla

        from oracle import arnoldi as oa

        lu = spla.splu((A - sigma * sp.identity(n)).tocsc())

        class HostLU:
            shape = (n, n)
            dtype = np.complex128

            def mul_(self, y, x):
                y[:] = lu.solve(x)

        _ORACLE["c4"] = oa.partialschur(HostLU(), v1=v1, nev=6, which="LM", tol=1e-10, mindim=10, maxdim=20)
    return _ORACLE["c4"]


@pytest.mark.parametrize("sstep", [None, 0], ids=["blocks", "steps"])
def test_config4_whole_solve_on_the_native_operator(ctx, sstep):
    """BASELINE config 4 with the inputs and assertions of test_config4_shift_invert_entirely_on_the_device, the rocSPARSE plug-in
    replaced by the library's own operator: converged, the mat-vec count of the oracle driven by host splu, lambda = sigma + 1/theta
    against the dense spectrum at 1e-8.  Once with the default (block) expansion, once step by step."""
    from oracle import arnoldi as oa
    from oracle.matrices import laplace1d

    n = 400
    rng = np.random.default_rng(3)
    A = (laplace1d(n) + 1j * sp.diags(0.3 * rng.random(n))).tocsc().astype(np.complex128)
    sigma = 1.7 + 0.1j
    op = pkg.tridiagonal_solve_operator(A.diagonal(-1), A.diagonal(0), A.diagonal(1), sigma=sigma, ctx=ctx)
    v1 = oa.uniform_hash(1, np.arange(n)) + 1j * oa.uniform_hash(2, np.arange(n))
    ws = pkg.ArnoldiWorkspace(v1, 20, ctx=ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    dec, hist = pkg.partialschur_(op, ws, nev=6, which="LM", tol=1e-10, mindim=10, maxdim=20)
    ref, rhist = _config4_oracle(n, sigma, A, v1)
    assert hist.converged and hist.mvproducts == rhist.mvproducts
    lam = sigma + 1.0 / dec.eigenvalues
    exact = np.linalg.eigvals(A.toarray())
    want = exact[np.argsort(np.abs(exact - sigma))][:6]
    np.testing.assert_allclose(np.sort_complex(lam), np.sort_complex(want), atol=1e-8)
    np.testing.assert_allclose(np.sort_complex(dec.eigenvalues), np.sort_complex(ref.eigenvalues), atol=1e-8)


def test_float64_whole_solve_against_the_analytic_spectrum(ctx):
    """laplace1d(1000) - I is indefinite; the four eigenvalues of laplace1d nearest 1 are 2 - 2 cos(k pi / 1001)."""
    n, sigma = 1000, 1.0
    dl, d, du, _ = family("a", n, sigma=sigma)
    op = pkg.tridiagonal_solve_operator(dl, d, du, sigma=sigma, ctx=ctx)
    v1 = pkg.matrices.start_vector(n)
    ws = pkg.ArnoldiWorkspace(v1, 20, ctx=ctx)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="LM", tol=1e-13, mindim=10, maxdim=20)
    assert hist.converged and dec.nconverged >= 4
    exact = 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
    want = exact[np.argsort(np.abs(exact - sigma))][:4]
    theta = dec.eigenvalues[np.argsort(-np.abs(dec.eigenvalues))][:4]
    lam = sigma + 1.0 / theta
    np.testing.assert_allclose(np.sort(lam.real), np.sort(want), atol=1e-8)
    assert np.abs(lam.imag).max() <= 1e-8
    dres, dorth = dec.workspace.residual_norms(op, dec.nconverged)
    print(f"residual {dres:.2e} orthogonality {dorth:.2e} nconverged {dec.nconverged} products {hist.mvproducts}")
    assert dres <= 1e-10 and dorth <= 1e-12


def test_wrong_use_is_refused(ctx):
    L = pkg._lib.load()
    dl, d, du, sg = family("d", 100)
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.tridiagonal_solve_operator(dl, d, du, sigma=sg, ctx=dctx)
    # the info call on another kind of operator
    csr = pkg.csr_operator(sp.identity(50, format="csr") * 2.0, ctx)
    lv = C.c_int()
    assert L.ks_operator_tridiag_info(csr._h, C.byref(lv), None, None, None, None) == pkg._lib.KS_ERR_ARGUMENT
    # the same refusals as the host path, before anything is uploaded
    with pytest.raises(pkg.ArgumentError):
        pkg.tridiagonal_solve_operator(np.ones(400), np.zeros(401), np.ones(400), ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        pkg.tridiagonal_solve_operator(dl, d, du, sigma=sg, ctx=ctx, block_rows=65)
