"""`-m gpu`: vectors that stay in HBM (`ks_vectors_*`, csrc/ks_vectors.hpp; `api.DeviceVectors`, `api.residuals`, `api.gram`): the last
two steps of the reference's recipes -- translate back to the original problem (docs/src/index.md:347) and show A x = x lambda,
A x = B x lambda, Q* A Q = R, Q* B Q = I for the ORIGINAL matrices (docs/src/index.md:258, 302, 350-351) -- without the download
`partialeigen` ends with.

Shapes are the smallest at which the code can go wrong: the 64-element pad, the 256-thread workgroup, a grid larger than the row
count, 8-column register groups (r = 8, 9), and r = 64 in ComplexF64 once for the chunked path of the residual kernel.  The numpy
reference and its bounds live in tests/test_device_vectors_cpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from __graft_entry__ import import_package
from test_device_vectors_cpu import exact_norms, gram_bound, integer_vectors, resid_bound, resid_model

pytestmark = pytest.mark.gpu
pkg = import_package()
api = pkg.api
EPS = np.finfo(np.float64).eps
TOL = 1e-11        # triangular solves against the host solve of the same factor (tests/test_gpu_lu_operator.py)

NS = (1, 2, 63, 64, 65, 255, 256, 257)
RS = (1, 2, 3, 8, 9, 20)
SHAPES = [(n, r) for n in NS for r in RS] + [(5000, 1), (5000, 20)]
DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c128"]


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


def norm_bound(n, ref):
    """a column norm against numpy's: an n-term sum of squares under a root is (n + 1) / 2 eps relative, doubled for slack like the
    same term of the residual bound, plus 3 eps for the model's own |x|, square and root"""
    return (n + 4) * EPS * np.asarray(ref)


def _rand(shape, cplx, seed):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1.0, 1.0, shape)
    if cplx:
        M = M + 1j * rng.uniform(-1.0, 1.0, shape)
    return np.asfortranarray(M)


def _device_image(X):
    """the whole allocation of X (ld x r, pads included) read back through col_ptr and torch"""
    import torch

    n, r = X.shape
    ld = X.ld
    assert ld % 64 == 0 and ld >= max(n, 64)
    dev = torch.device("cuda", X.ctx.device)
    t = torch.as_tensor(api._DevArray(X.col_ptr(0), ld * r, X.dtype), device=dev)
    img = t.cpu().numpy().reshape((ld, r), order="F")
    for j in (0, r - 1):
        assert X.col_ptr(j) == X.col_ptr(0) + j * ld * X.dtype.itemsize
    return img


def _pads_zero(X, want=None):
    img = _device_image(X)
    n = X.shape[0]
    assert not img[n:].any(), "pad rows written"
    if want is not None:
        assert np.array_equal(img[:n], want)
    return True


# ------------------------------------------------------------------ 1. round trip and pads
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_round_trip_and_pads(ctx, dtype):
    cplx = dtype is np.complex128
    for n, r in SHAPES + [(257, 64)]:
        M = _rand((n, r), cplx, 100 * n + r)
        X = pkg.DeviceVectors.from_host(M, ctx)
        assert X.shape == (n, r) and X.dtype == np.dtype(dtype) and X.ctx is ctx
        got = X.download()
        assert got.dtype == np.dtype(dtype) and np.array_equal(got, M), (n, r)
        assert _pads_zero(X, M)
        X.close()
    # a column range in the middle, through the C interface
    L = pkg._lib.load()
    X = pkg.DeviceVectors(65, 5, dtype, ctx)
    M = _rand((65, 2), cplx, 7)
    pkg._lib.check(L.ks_vectors_upload(X._h, 2, 2, M.ctypes.data, 65))
    want = np.zeros((65, 5), dtype=dtype)
    want[:, 2:4] = M
    assert np.array_equal(X.download(), want) and _pads_zero(X, want)
    out = np.empty((70, 2), dtype=dtype, order="F")
    pkg._lib.check(L.ks_vectors_download(X._h, 2, 2, out.ctypes.data, 70))
    assert np.array_equal(out[:65], M)
    nl, nc, dc, ld = C.c_int64(), C.c_int(), C.c_int(), C.c_int64()
    pkg._lib.check(L.ks_vectors_dims(X._h, C.byref(nl), C.byref(nc), C.byref(dc), C.byref(ld)))
    assert (nl.value, nc.value, dc.value, ld.value) == (65, 5, 1 if cplx else 0, 128)


def test_no_rows_is_legal_and_every_call_is_a_no_op(ctx):
    X = pkg.DeviceVectors(0, 3, np.float64, ctx)
    Y = pkg.DeviceVectors.from_host(np.zeros((0, 3)), ctx)
    assert X.download().shape == (0, 3) and X.ld == 64
    op = pkg.host_operator(lambda y, x: None, 0, np.float64, ctx)
    Z = X.apply(op)
    assert Z.shape == (0, 3)
    res, bn = pkg.vector_residuals(X, Y, np.ones(3))
    assert not res.any() and not bn.any()
    assert np.array_equal(pkg.gram(X, Y), np.zeros((3, 3)))
    assert not _device_image(X).any()


# ------------------------------------------------------------------ 2. the basis product, left on the device
def _laplace(n):
    return sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n), format="csr") if n > 1 else sp.csr_matrix(np.array([[2.0]]))


@pytest.mark.parametrize("combo", ["f64xf64", "f64xc128", "c128xc128"])
def test_basis_times_device_equals_basis_times(ctx, combo):
    vc, yc = combo.startswith("c128"), combo.endswith("xc128")
    vdt = np.complex128 if vc else np.float64
    for n in (1, 2, 63, 64, 65, 257, 5000):
        k = min(n, 21)
        ws = pkg.ArnoldiWorkspace(n, k, vdt, ctx=ctx)
        ws.set_cols(0, _rand((n, k + 1), vc, n))
        for c, r in ((k + 1, 1), (k + 1, 3), (max(k - 1, 1), 9), (k, 20)):
            Y = _rand((c, r), yc, 10 * c + r)
            X = ws.basis_times_device(c, Y)
            want = ws.basis_times(c, Y)
            assert X.dtype == want.dtype and X.shape == want.shape
            assert np.array_equal(X.download(), want), (n, c, r)
            assert _pads_zero(X, want)


@pytest.mark.parametrize("cplx", [False, True], ids=IDS)
def test_basis_times_device_right_after_an_expansion(ctx, cplx):
    """the workspace has just run iterate_arnoldi: its newest columns are still in factored (lazily normalised) form and the product
    has to materialise them itself"""
    n, k = 300, 12
    dt = np.complex128 if cplx else np.float64
    A = _laplace(n).astype(dt)
    if cplx:
        A = (A + 1j * sp.diags(np.linspace(0.0, 1.0, n))).tocsr()
    op = pkg.csr_operator(A, ctx)
    Y = _rand((k + 1, 5), cplx, 3)
    ws = pkg.ArnoldiWorkspace(n, k, dt, ctx=ctx)
    ws.reinitialize(0, pkg.matrices.start_vector(n).astype(dt))
    st = ws.iterate_arnoldi(op, 1, k)
    assert st["steps"] == k and st["breakdowns"] == 0
    X = ws.basis_times_device(k + 1, Y)          # first: nothing else has touched the basis since the expansion
    want = ws.basis_times(k + 1, Y)
    assert np.array_equal(X.download(), want) and _pads_zero(X)
    V = ws.V
    # against numpy on the downloaded basis: two (k + 1)-term inner products per entry, the library's and numpy's own
    assert np.all(np.abs(X.download() - V @ Y) <= 2 * (k + 3) * EPS * (np.abs(V) @ np.abs(Y)))


# ------------------------------------------------------------------ 3. apply
def _sparse(n, cplx, seed):
    """about five entries per row, no structure (tests/test_gpu_operator_product.py)"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=min(1.0, 5.0 / n), random_state=rng, format="csr")
    if cplx:
        A = A + 1j * sp.random(n, n, density=min(1.0, 5.0 / n), random_state=rng, format="csr")
    return A.tocsr().astype(np.complex128 if cplx else np.float64)


def _operators(n, cplx, ctx):
    """name -> Operator, one of every kind"""
    dt = np.complex128 if cplx else np.float64
    ops = {}
    S = _sparse(n, cplx, 11 * n + 1)
    ops["csr"] = pkg.csr_operator(S, ctx)
    ops["laplace"] = pkg.csr_operator(_laplace(n).astype(dt), ctx)
    if n <= 257:
        ops["dense"] = pkg.dense_operator(_rand((n, n), cplx, n + 5).astype(dt), ctx)
    rng = np.random.default_rng(n + 3)
    d = (4.0 + rng.random(n)).astype(dt) + (0.3j if cplx else 0.0)
    dl, du = -rng.random(max(n - 1, 0)).astype(dt), -rng.random(max(n - 1, 0)).astype(dt)
    ops["tridiag_solve"] = pkg.tridiagonal_solve_operator(dl, d, du, 0.25, ctx)
    S2 = _sparse(n, cplx, 11 * n + 2)
    ops["product"] = pkg.product_operator(ops["csr"], pkg.csr_operator(S2, ctx), ops["laplace"], ctx=ctx)
    ops["host"] = pkg.host_operator(lambda y, x: np.copyto(y, S2 @ x), n, dt, ctx)
    return ops


def _through_a_workspace(ws, op, x):
    ws.set_col(0, x)
    ws.apply(op, 0, 1)
    return ws.col(1)


@pytest.mark.parametrize("cplx", [False, True], ids=IDS)
@pytest.mark.parametrize("n", NS + (5000,))
def test_apply_is_the_operator_on_every_column(ctx, n, cplx):
    r = 3
    M = _rand((n, r), cplx, n)
    X = pkg.DeviceVectors.from_host(M, ctx)
    ws = pkg.ArnoldiWorkspace(n, 1, M.dtype, ctx=ctx)
    for name, op in _operators(n, cplx, ctx).items():
        Y = X.apply(op)
        got = Y.download()
        for i in range(r):
            assert np.array_equal(got[:, i], _through_a_workspace(ws, op, np.ascontiguousarray(M[:, i]))), (name, n, i)
        assert _pads_zero(Y, got) and _pads_zero(X, M), name          # `in` is unchanged
        assert Y.shape == X.shape and Y.dtype == X.dtype and Y.ctx is ctx


@pytest.mark.parametrize("n", NS + (5000,))
def test_a_real_operator_on_complex_vectors_acts_on_both_parts(ctx, n):
    r = 3
    M = _rand((n, r), True, n + 1)
    X = pkg.DeviceVectors.from_host(M, ctx)
    ws = pkg.ArnoldiWorkspace(n, 1, np.float64, ctx=ctx)
    for name, op in _operators(n, False, ctx).items():
        Y = X.apply(op)
        got = Y.download()
        assert got.dtype == np.complex128
        for i in range(r):
            assert np.array_equal(got[:, i].real, _through_a_workspace(ws, op, np.ascontiguousarray(M[:, i].real))), (name, n, i)
            assert np.array_equal(got[:, i].imag, _through_a_workspace(ws, op, np.ascontiguousarray(M[:, i].imag))), (name, n, i)
        assert _pads_zero(Y, got) and _pads_zero(X, M), name
        Y2 = X.apply(op)                                                  # the scratch columns of a fresh result start clean as well
        assert np.array_equal(Y2.download(), got)


class _Boom(Exception):
    pass


def test_an_exception_in_a_callback_surfaces_as_itself(ctx):
    n = 64

    def cb(y, x):
        raise _Boom("inside the callback")

    S = _sparse(n, False, 1)
    op = pkg.csr_operator(S, ctx)
    bad = pkg.host_operator(cb, n, np.float64, ctx)
    M = _rand((n, 2), False, 1)
    X = pkg.DeviceVectors.from_host(M, ctx)
    with pytest.raises(_Boom, match="inside the callback"):
        X.apply(bad)
    with pytest.raises(_Boom, match="inside the callback"):
        X.apply(pkg.product_operator(op, bad, op, ctx=ctx))
    with pytest.raises(_Boom, match="inside the callback"):
        pkg.DeviceVectors.from_host(M + 1j * M, ctx).apply(bad)
    # ... and the vectors and the other operator are none the worse for it
    want = S @ M
    assert np.abs(X.apply(op).download() - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ 4. residuals, exact
_EXACT_SHAPES = SHAPES + [(257, 64)]


def _coefficients(kind, r, cplx, seed):
    Cm = integer_vectors(r, r, cplx, seed)
    if kind == "diagonal":
        Cm = np.diag(np.diag(Cm))
    elif kind == "upper":
        Cm = np.triu(Cm)
    return np.asfortranarray(Cm)


@pytest.mark.parametrize("kind", ["diagonal", "upper", "full"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_residuals_are_exact_on_integer_data(ctx, dtype, kind):
    """entries in [-3, 3] (Gaussian integers in ComplexF64): every product and sum is exact in Float64 in any order -- the largest sum
    of squares, 2 * 5000 * (3 + 20 * 18)^2, is far below 2^53 -- so resid and bnorm equal np.sqrt of the exact integer sums BIT FOR BIT"""
    cplx = dtype is np.complex128
    for n, r in _EXACT_SHAPES:
        if r == 64 and not cplx:
            continue
        AX, BX = integer_vectors(n, r, cplx, 3 * n + r), integer_vectors(n, r, cplx, 3 * n + r + 1)
        Cm = _coefficients(kind, r, cplx, n + r)
        dAX, dBX = pkg.DeviceVectors.from_host(AX, ctx), pkg.DeviceVectors.from_host(BX, ctx)
        want_r, want_b = exact_norms(AX, BX, Cm)
        res, bn = pkg.vector_residuals(dAX, dBX, Cm if kind != "diagonal" else np.diag(Cm))
        assert np.array_equal(res, want_r), (n, r, res, want_r)
        assert np.array_equal(bn, want_b), (n, r, bn, want_b)
        for _ in range(2):
            res2, bn2 = pkg.vector_residuals(dAX, dBX, Cm)
            assert np.array_equal(res2, res) and np.array_equal(bn2, bn)
        # BX is AX's own object: both read streams on one allocation
        want_r, want_b = exact_norms(AX, AX, Cm)
        res, bn = pkg.vector_residuals(dAX, dAX, Cm)
        assert np.array_equal(res, want_r) and np.array_equal(bn, want_b), (n, r)
        assert _pads_zero(dAX, AX) and _pads_zero(dBX, BX)


# ------------------------------------------------------------------ 5. residuals, rounding
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_residuals_on_random_data_within_the_rounding_bound(ctx, dtype):
    cplx = dtype is np.complex128
    worst = 0.0
    for n, r in _EXACT_SHAPES:
        if r == 64 and not cplx:
            continue
        BX, Cm = _rand((n, r), cplx, 5 * n + r), _rand((r, r), cplx, n + 7 * r)
        for tiny in (False, True):
            AX = np.asfortranarray(BX @ Cm) if tiny else _rand((n, r), cplx, 5 * n + r + 1)   # tiny: the residual is rounding only
            dAX, dBX = pkg.DeviceVectors.from_host(AX, ctx), pkg.DeviceVectors.from_host(BX, ctx)
            res, bn = pkg.vector_residuals(dAX, dBX, Cm)
            ref, bref = resid_model(AX, BX, Cm)
            bound = resid_bound(AX, BX, Cm, ref)
            worst = max(worst, float((np.abs(res - ref) / bound).max()))
            assert np.all(np.abs(res - ref) <= bound), (n, r, tiny, res, ref, bound)
            assert np.all(np.abs(bn - bref) <= norm_bound(n, bref)), (n, r, bn, bref)
    print(f"largest |resid - model| / bound: {worst:.3f}")


# ------------------------------------------------------------------ 6. Gram
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gram(ctx, dtype):
    cplx = dtype is np.complex128
    for n, r in _EXACT_SHAPES:
        ry = {1: 3, 20: 9, 64: 17}.get(r, r)            # rectangular as well: tiles of both sides end at different columns
        X, Y = integer_vectors(n, r, cplx, n + r), integer_vectors(n, ry, cplx, n + r + 1)
        dX, dY = pkg.DeviceVectors.from_host(X, ctx), pkg.DeviceVectors.from_host(Y, ctx)
        G = pkg.gram(dX, dY)
        assert G.shape == (r, ry) and G.dtype == np.dtype(dtype)
        assert np.array_equal(G, X.conj().T @ Y), (n, r)       # exact: integers, sums below 2^53
        assert np.array_equal(pkg.gram(dX, dX), X.conj().T @ X)
        X, Y = _rand((n, r), cplx, n + r), _rand((n, ry), cplx, n + r + 1)
        dX, dY = pkg.DeviceVectors.from_host(X, ctx), pkg.DeviceVectors.from_host(Y, ctx)
        G = pkg.gram(dX, dY)
        assert np.all(np.abs(G - X.conj().T @ Y) <= gram_bound(X, Y)), (n, r)
        assert np.array_equal(pkg.gram(dX, dY), G)
        assert _pads_zero(dX, X) and _pads_zero(dY, Y)


# ------------------------------------------------------------------ 7. refusals
def _refused(rc, text):
    L = pkg._lib.load()
    assert rc == pkg._lib.KS_ERR_ARGUMENT, (rc, L.ks_last_error_string())
    msg = L.ks_last_error_string().decode()
    assert text in msg, msg


def test_wrong_use_is_refused(ctx):
    L = pkg._lib.load()
    n = 50
    a = pkg.csr_operator(_sparse(n, False, 1), ctx)
    ac = pkg.csr_operator(_sparse(n, True, 1), ctx)
    a51 = pkg.csr_operator(_sparse(n + 1, False, 1), ctx)
    other = pkg.Context(0)
    a_other = pkg.csr_operator(_sparse(n, False, 1), other)
    X, Y = pkg.DeviceVectors(n, 3, np.float64, ctx), pkg.DeviceVectors(n, 3, np.float64, ctx)
    W4, W51, Wc, W2 = (pkg.DeviceVectors(n, 4, np.float64, ctx), pkg.DeviceVectors(n + 1, 3, np.float64, ctx),
                       pkg.DeviceVectors(n, 3, np.complex128, ctx), pkg.DeviceVectors(n, 2, np.float64, ctx))
    Z = pkg.DeviceVectors(n, 3, np.float64, other)
    _refused(L.ks_vectors_apply(a._h, X._h, X._h), "the result must not be the input")
    _refused(L.ks_vectors_apply(a._h, X._h, W4._h), "shapes differ, (50, 3) and (50, 4)")
    _refused(L.ks_vectors_apply(a._h, X._h, W51._h), "shapes differ")
    _refused(L.ks_vectors_apply(a._h, X._h, Wc._h), "do not have one element type")
    _refused(L.ks_vectors_apply(a51._h, X._h, Y._h), "the operator has 51 rows, the vectors have 50")
    _refused(L.ks_vectors_apply(ac._h, X._h, Y._h), "a ComplexF64 operator needs ComplexF64 vectors")
    _refused(L.ks_vectors_apply(a._h, X._h, Z._h), "different contexts")
    _refused(L.ks_vectors_apply(a_other._h, X._h, Y._h), "the operator lives on another context")
    res, bn, Cm, G = np.zeros(3), np.zeros(3), np.asfortranarray(np.eye(3)), np.zeros((3, 3), order="F")
    dp = C.POINTER(C.c_double)
    rp, bp = res.ctypes.data_as(dp), bn.ctypes.data_as(dp)
    _refused(L.ks_vectors_residuals(X._h, Z._h, Cm.ctypes.data, 3, rp, bp), "different contexts")
    _refused(L.ks_vectors_residuals(X._h, W4._h, Cm.ctypes.data, 3, rp, bp), "shapes differ")
    _refused(L.ks_vectors_residuals(X._h, Wc._h, Cm.ctypes.data, 3, rp, bp), "do not have one element type")
    _refused(L.ks_vectors_gram(X._h, Z._h, G.ctypes.data, 3), "different contexts")
    _refused(L.ks_vectors_gram(X._h, W51._h, G.ctypes.data, 3), "shapes differ")
    _refused(L.ks_vectors_gram(X._h, Wc._h, G.ctypes.data, 3), "do not have one element type")
    h = C.c_void_p()
    for bad in (0, 65, -1):
        _refused(L.ks_vectors_create(ctx._h, n, bad, 0, C.byref(h)), "columns (1 to 64 are supported)")
        with pytest.raises(pkg.ArgumentError, match="1 to 64"):
            pkg.DeviceVectors(n, bad, np.float64, ctx)
    pkg.DeviceVectors(n, 64, np.float64, ctx).close()
    pkg.DeviceVectors(n, 1, np.float64, ctx).close()
    # the basis product
    ws = pkg.ArnoldiWorkspace(n, 5, np.float64, ctx=ctx)
    Yc = np.asfortranarray(np.ones((7, 3)))
    _refused(L.ks_basis_times_device(ws._h, 7, 3, Yc.ctypes.data, 7, 0, X._h), "bad shape")                     # c > maxdim + 1
    _refused(L.ks_basis_times_device(ws._h, 6, 3, Yc.ctypes.data, 7, 0, W2._h), "the product is (50, 3)")
    _refused(L.ks_basis_times_device(ws._h, 6, 3, Yc.ctypes.data, 7, 0, W51._h), "the product is (50, 3)")
    _refused(L.ks_basis_times_device(ws._h, 6, 3, Yc.ctypes.data, 7, 0, Wc._h), "element type of the coefficients")
    _refused(L.ks_basis_times_device(ws._h, 6, 3, Yc.ctypes.data, 7, 0, Z._h), "another context than the workspace")
    with pytest.raises(pkg.ArgumentError, match="bad shape"):
        ws.basis_times_device(7, np.ones((7, 3)))
    # the Python layer refuses before the library is asked
    with pytest.raises(pkg.ArgumentError, match="ComplexF64 operator needs ComplexF64 vectors"):
        X.apply(ac)
    with pytest.raises(pkg.ArgumentError, match="different contexts"):
        pkg.gram(X, Z)
    with pytest.raises(pkg.ArgumentError, match="complex coefficients need ComplexF64 vectors"):
        pkg.residuals(a, X, np.array([1.0, 1.0j, -1.0j]))
    # a multi-rank context (the collective code path, here with one rank)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU contexts only"):
        pkg.DeviceVectors(n, 3, np.float64, dctx)


# ------------------------------------------------------------------ 8. the recipes, end to end
def _agrees_with_numpy(res, bn, AXh, BXh, Cm, what):
    ref, bref = resid_model(AXh, BXh, Cm)
    bound = resid_bound(AXh, BXh, Cm, ref)
    print(f"{what}: resid {res}, numpy {ref}, |difference| / bound {np.abs(res - ref) / bound}")
    assert np.all(np.abs(res - ref) <= bound), (what, res, ref, bound)
    assert np.all(np.abs(bn - bref) <= norm_bound(AXh.shape[0], bref)), (what, bn, bref)


def test_recipe_shift_and_invert(ctx):
    """docs/src/index.md:234-259: the smallest eigenvalues of the 1-D Laplacian through x -> A^-1 x, lambda = 1 / theta, and then
    A x = x lambda shown for the ORIGINAL A on the device.  A symmetric: A^-1 x = theta x + rho with ||rho|| <= tol |theta| gives
    ||A x - lambda x|| <= ||A||_2 tol = 4e-10; the cap 1e-7 leaves a factor of 250 and only catches a wrong pairing of lambda and x."""
    n = 400
    A = _laplace(n)
    inv = pkg.tridiagonal_solve_operator(np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0), 0.0, ctx)
    dec, hist = pkg.partialschur(inv, nev=4, which="LM", tol=1e-10, v1=pkg.matrices.start_vector(n))
    assert hist.converged and dec.nconverged >= 4
    theta, X = pkg.partialeigen(dec, device=True)
    assert isinstance(X, pkg.DeviceVectors) and X.dtype == np.float64 and X.shape == (n, dec.nconverged)
    assert np.array_equal(X.download(), pkg.partialeigen(dec)[1])        # the default path, untouched, gives the same vectors
    lam = (1.0 / theta).real
    exact = 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
    assert np.abs(np.sort(lam)[:4] - exact[:4]).max() <= 1e-9
    res, bn = pkg.residuals(pkg.csr_operator(A, ctx), X, lam)
    Xh = X.download()
    _agrees_with_numpy(res, bn, A @ Xh, Xh, np.diag(lam), "shift-and-invert")
    assert res.max() <= 1e-7, res


def test_recipe_generalized_shift_and_invert(ctx):
    """docs/src/index.md:262-303: stiffness and consistent mass of linear elements, x -> K^-1 M x by the fused pencil operator, and
    K x = M x lambda shown for the ORIGINAL K and M on the device"""
    n = 400
    K = _laplace(n)
    M = sp.diags([np.full(n - 1, 1.0 / 6.0), np.full(n, 4.0 / 6.0), np.full(n - 1, 1.0 / 6.0)], [-1, 0, 1], format="csr")
    op = pkg.tridiagonal_pencil_operator(np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0), np.full(n - 1, 1.0 / 6.0),
                                         np.full(n, 4.0 / 6.0), np.full(n - 1, 1.0 / 6.0), 0.0, ctx)
    dec, hist = pkg.partialschur(op, nev=4, which="LM", tol=1e-10, v1=pkg.matrices.start_vector(n))
    assert hist.converged and dec.nconverged >= 4
    theta, X = pkg.partialeigen(dec, device=True)
    lam = 1.0 / theta
    if X.dtype.kind == "f":
        lam = lam.real
    res, bn = pkg.residuals(pkg.csr_operator(K, ctx), X, lam, B=pkg.csr_operator(M, ctx))
    Xh = X.download()
    _agrees_with_numpy(res, bn, K @ Xh, M @ Xh, np.diag(lam), "generalized shift-and-invert")
    assert np.all(np.abs(bn - np.linalg.norm(M @ Xh, axis=0)) <= norm_bound(n, bn))


def test_recipe_b_orthonormal_schur_vectors(ctx):
    """docs/src/index.md:306-352 with the problem of tests/test_gpu_operator_product.py (bidiagonal L): the back-transformation
    Q = L^-* Y by the device factor the product already holds, and Q* B Q = I, Q* A Q = R from two small Gram matrices"""
    extras = importlib.import_module(pkg.__name__ + ".extras")
    n = 300
    B = sp.diags([np.full(n - 1, 1.0 / 6.0), np.full(n, 4.0 / 6.0), np.full(n - 1, 1.0 / 6.0)], [-1, 0, 1], format="csr")
    L = sp.csr_matrix(np.linalg.cholesky(B.toarray()))
    L.eliminate_zeros()
    A = (sp.random(n, n, 0.03, random_state=np.random.default_rng(11)) + sp.diags(np.linspace(1.0, 3.0, n))).tocsr()
    op, back = extras.b_orthonormal_operator(A, L, ctx)
    assert back.operator is op.factors[2]
    dec, hist = pkg.partialschur(op, nev=4, which="LM", tol=1e-10, v1=pkg.matrices.start_vector(n))
    assert hist.converged
    Y = pkg.schur_vectors(dec)
    assert np.array_equal(Y.download(), dec.Q)
    Q = Y.apply(back.operator)
    Qh, want = Q.download(), back(dec.Q)
    assert np.abs(Qh - want).max() <= TOL * np.abs(want).max()
    R = np.array(dec.R)
    BQ, AQ = Q.apply(pkg.csr_operator(B, ctx)), Q.apply(pkg.csr_operator(A, ctx))
    for what, P, target in (("Q*BQ - I", BQ, np.eye(Q.shape[1])), ("Q*AQ - R", AQ, R)):
        G, Ph = pkg.gram(Q, P), P.download()
        G_np = Qh.conj().T @ Ph
        print(f"||{what}|| = {np.linalg.norm(G - target):.2e} (numpy on the downloads: {np.linalg.norm(G_np - target):.2e})")
        assert np.all(np.abs((G - target) - (G_np - target)) <= gram_bound(Qh, Ph)), what


def test_recipe_real_matrix_with_conjugate_pairs(ctx):
    """a real non-symmetric matrix whose dominant eigenvalues are three planted complex-conjugate pairs: complex eigenvectors of a
    Float64 problem, the Float64 operator applied to their real and imaginary parts, complex eigenvalues in the residual"""
    n = 300
    planted = [(5.0, 3.0), (4.0, -2.5), (-6.0, 1.0)]
    A = pkg.matrices.hashed_nonsymmetric_csr(n, seed=7, planted=planted)
    op = pkg.csr_operator(A, ctx)
    assert op.dtype == np.float64
    dec, hist = pkg.partialschur(op, nev=6, which="LM", tol=1e-10, v1=pkg.matrices.start_vector(n))
    assert hist.converged and dec.nconverged >= 6
    lam, X = pkg.partialeigen(dec, device=True)
    assert X.dtype == np.complex128 and np.count_nonzero(np.abs(lam.imag) > 0.5) >= 6
    exact = np.array([complex(a, s * b) for a, b in planted for s in (1, -1)])
    assert max(np.abs(lam - z).min() for z in exact) <= 1e-8
    res, bn = pkg.residuals(op, X, lam)
    Xh = X.download()
    _agrees_with_numpy(res, bn, A @ Xh, Xh, np.diag(lam), "conjugate pairs")
    with pytest.raises(pkg.ArgumentError, match="complex coefficients need ComplexF64 vectors"):
        pkg.residuals(op, pkg.schur_vectors(dec), lam)
