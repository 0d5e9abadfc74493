"""`-m "not gpu"`: the host side of the device-resident vectors (`api.DeviceVectors`, `api.residuals`, `api.gram`;
`ks_vectors_*`, include/kschur.h) -- what can be checked without a device:

  * the expansion of eigenvalues to the coefficient block C of `ks_vectors_residuals` (`api.residual_coefficients`): a 1-D `lam`
    becomes diag(lam) in the vectors' element type, a 2-D block (R of a Schur decomposition, a real 2 x 2 block that carries a
    complex-conjugate pair) is taken as it is;
  * the argument errors `api.residuals` / `api.gram` / `DeviceVectors.apply` raise BEFORE any device call (no context exists on a
    box without a GPU: the stand-ins below carry shape, element type and context only);
  * the numpy models `resid_model` / `resid_bound` / `gram_bound` that tests/test_gpu_device_vectors.py uses as its reference.
"""
import numpy as np
import pytest

from __graft_entry__ import import_package

pkg = import_package()
api = pkg.api
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------ the reference of the GPU tests
def resid_model(AX, BX, C):
    """(resid, bnorm): resid[i] = ||AX[:, i] - sum_j BX[:, j] C[j, i]||_2, bnorm[i] = ||BX[:, i]||_2, in numpy."""
    AX, BX, C = np.asarray(AX), np.asarray(BX), np.asarray(C)
    E = AX - BX @ C
    return np.sqrt((np.abs(E) ** 2).sum(axis=0)), np.sqrt((np.abs(BX) ** 2).sum(axis=0))


def resid_bound(AX, BX, C, r_ref):
    """How far a residual evaluated in Float64 in ANY order, with or without FMA, may be from `r_ref`:
        2 (r + 2) eps || |AX_i| + |BX| |C_i| ||_2     an (r + 1)-term inner product per row
      + n eps r_ref                                    an n-term sum of squares, halved by the root, doubled for slack"""
    AX, BX, C = np.asarray(AX), np.asarray(BX), np.asarray(C)
    n, r = AX.shape
    mag = np.abs(AX) + np.abs(BX) @ np.abs(C)
    return 2 * (r + 2) * EPS * np.sqrt((mag ** 2).sum(axis=0)) + n * EPS * np.asarray(r_ref)


def gram_bound(X, Y):
    """entrywise bound of an n-term inner product: (n + 2) eps |X|^H |Y|"""
    X, Y = np.asarray(X), np.asarray(Y)
    return (X.shape[0] + 2) * EPS * (np.abs(X).T @ np.abs(Y))


def integer_vectors(n, r, cplx, seed):
    """entries in [-3, 3] (Gaussian integers when cplx): every product and sum of the residual is exact in Float64"""
    rng = np.random.default_rng(seed)
    M = rng.integers(-3, 4, size=(n, r)).astype(np.float64)
    if cplx:
        M = M + 1j * rng.integers(-3, 4, size=(n, r))
    return np.asfortranarray(M)


def exact_norms(AX, BX, C):
    """np.sqrt of the EXACT integer sums of squares (int64 arithmetic) for integer data"""
    def ints(M):
        M = np.asarray(M)
        return np.rint(M.real).astype(np.int64), np.rint(M.imag).astype(np.int64)

    ar, ai = ints(AX)
    br, bi = ints(BX)
    cr, ci = ints(C)
    er = ar - (br @ cr - bi @ ci)
    ei = ai - (br @ ci + bi @ cr)
    r2 = (er * er + ei * ei).sum(axis=0)
    b2 = (br * br + bi * bi).sum(axis=0)
    assert r2.max(initial=0) < 2 ** 53 and b2.max(initial=0) < 2 ** 53
    return np.sqrt(r2.astype(np.float64)), np.sqrt(b2.astype(np.float64))


# ------------------------------------------------------------------ the models themselves
def test_models_agree_with_a_column_by_column_evaluation():
    rng = np.random.default_rng(1)
    for cplx in (False, True):
        n, r = 37, 5
        AX, BX, C = (rng.uniform(-1, 1, s) + (1j * rng.uniform(-1, 1, s) if cplx else 0.0) for s in ((n, r), (n, r), (r, r)))
        res, bn = resid_model(AX, BX, C)
        for i in range(r):
            e = AX[:, i] - sum(BX[:, j] * C[j, i] for j in range(r))
            assert abs(res[i] - np.linalg.norm(e)) <= 4 * EPS * res[i]
            assert abs(bn[i] - np.linalg.norm(BX[:, i])) <= 4 * EPS * bn[i]
        assert np.all(resid_bound(AX, BX, C, res) > 0) and resid_bound(AX, BX, C, res).shape == (r,)
        G = gram_bound(AX, BX)
        assert G.shape == (r, r) and np.all(G > 0)


def test_exact_norms_on_integer_data():
    for cplx in (False, True):
        AX, BX, C = integer_vectors(50, 4, cplx, 1), integer_vectors(50, 4, cplx, 2), integer_vectors(4, 4, cplx, 3)
        assert np.abs(AX.real).max() <= 3 and np.array_equal(AX, np.rint(AX.real) + 1j * np.rint(AX.imag))
        res, bn = exact_norms(AX, BX, C)
        mres, mbn = resid_model(AX, BX, C)
        assert np.allclose(res, mres, rtol=1e-14, atol=0) and np.allclose(bn, mbn, rtol=1e-14, atol=0)


# ------------------------------------------------------------------ lam -> C
def test_eigenvalues_become_a_diagonal_block_in_the_vectors_type():
    lam = np.array([1.5, -2.0, 0.25])
    C = api.residual_coefficients(lam, 3, np.float64)
    assert C.dtype == np.float64 and C.flags.f_contiguous and np.array_equal(C, np.diag(lam))
    C = api.residual_coefficients(lam, 3, np.complex128)
    assert C.dtype == np.complex128 and np.array_equal(C, np.diag(lam))
    lamc = np.array([1.0 + 2.0j, 1.0 - 2.0j])
    C = api.residual_coefficients(lamc, 2, np.complex128)
    assert C.dtype == np.complex128 and np.array_equal(C, np.diag(lamc))
    assert api.residual_coefficients([2, 3], 2, np.float64).dtype == np.float64   # integers are promoted


def test_a_real_2x2_block_carries_a_conjugate_pair():
    a, b = 0.5, 2.0
    blk = np.array([[a, b], [-b, a]])
    C = api.residual_coefficients(blk, 2, np.float64)
    assert C.dtype == np.float64 and C.flags.f_contiguous and np.array_equal(C, blk)
    # x = u + i v with A x = (a + i b) x  <=>  A [u v] = [u v] [[a, b], [-b, a]]: the model sees a zero residual for it
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6, 2))
    res, _ = resid_model(X @ blk, X, C)
    assert res.max() <= 1e-14
    R = np.triu(rng.standard_normal((4, 4)))
    assert np.array_equal(api.residual_coefficients(R, 4, np.complex128), R.astype(np.complex128))


def test_coefficient_errors():
    with pytest.raises(pkg.ArgumentError, match="complex coefficients need ComplexF64 vectors"):
        api.residual_coefficients(np.array([1.0 + 1.0j, 2.0]), 2, np.float64)
    with pytest.raises(pkg.ArgumentError, match="complex coefficients"):
        api.residual_coefficients(np.eye(2, dtype=np.complex128), 2, np.float64)
    with pytest.raises(pkg.DimensionMismatch, match="3 eigenvalues for 2 vectors"):
        api.residual_coefficients(np.ones(3), 2, np.float64)
    with pytest.raises(pkg.DimensionMismatch, match="coefficient block"):
        api.residual_coefficients(np.ones((2, 3)), 2, np.float64)
    with pytest.raises(pkg.DimensionMismatch, match="coefficient block"):
        api.residual_coefficients(np.ones((2, 2, 2)), 2, np.float64)


# ------------------------------------------------------------------ errors before any device call
class _Ctx:
    """stands for a context: only its identity matters to the checks"""
    _h = None


def _vectors(n, r, dtype, ctx):
    X = api.DeviceVectors.__new__(api.DeviceVectors)   # no device: shape, element type and context only
    X.shape, X.dtype, X.ctx, X._h = (n, r), np.dtype(dtype), ctx, None
    return X


def _operator(n, dtype, ctx):
    return api.Operator(ctx, None, (n, n), dtype)


def test_residuals_argument_errors_come_before_the_device():
    c1, c2 = _Ctx(), _Ctx()
    X = _vectors(10, 3, np.float64, c1)
    A = _operator(10, np.float64, c1)
    with pytest.raises(pkg.DimensionMismatch, match="the operator has 11 rows, the vectors have 10"):
        api.residuals(_operator(11, np.float64, c1), X, np.ones(3))
    with pytest.raises(pkg.ArgumentError, match="different contexts"):
        api.residuals(_operator(10, np.float64, c2), X, np.ones(3))
    with pytest.raises(pkg.ArgumentError, match="ComplexF64 operator needs ComplexF64 vectors"):
        api.residuals(_operator(10, np.complex128, c1), X, np.ones(3))
    with pytest.raises(pkg.ArgumentError, match="complex coefficients need ComplexF64 vectors"):
        api.residuals(A, X, np.array([1.0, 2.0 + 1.0j, 2.0 - 1.0j]))
    with pytest.raises(pkg.DimensionMismatch, match="2 eigenvalues for 3 vectors"):
        api.residuals(A, X, np.ones(2))
    with pytest.raises(pkg.DimensionMismatch, match="the operator has 9 rows"):
        api.residuals(A, X, np.ones(3), B=_operator(9, np.float64, c1))
    with pytest.raises(pkg.ArgumentError, match="different contexts"):
        api.residuals(A, X, np.ones(3), B=_operator(10, np.float64, c2))
    with pytest.raises(pkg.ArgumentError, match="expected DeviceVectors"):
        api.residuals(A, np.ones((10, 3)), np.ones(3))
    with pytest.raises(pkg.ArgumentError, match="expected an Operator"):
        api.residuals(np.eye(10), X, np.ones(3))
    with pytest.raises(pkg.ArgumentError, match="ComplexF64 operator needs ComplexF64 vectors"):
        X.apply(_operator(10, np.complex128, c1))


def test_gram_argument_errors_come_before_the_device():
    c1, c2 = _Ctx(), _Ctx()
    X = _vectors(10, 3, np.float64, c1)
    with pytest.raises(pkg.DimensionMismatch, match=r"shapes \(10, 3\) and \(11, 3\)"):
        api.gram(X, _vectors(11, 3, np.float64, c1))
    with pytest.raises(pkg.ArgumentError, match="element types float64 and complex128"):
        api.gram(X, _vectors(10, 2, np.complex128, c1))
    with pytest.raises(pkg.ArgumentError, match="different contexts"):
        api.gram(X, _vectors(10, 2, np.float64, c2))
    with pytest.raises(pkg.ArgumentError, match="expected DeviceVectors"):
        api.gram(X, np.ones((10, 2)))
    # products that already exist: the column counts must agree as well
    with pytest.raises(pkg.DimensionMismatch, match="shapes"):
        api.vector_residuals(X, _vectors(10, 2, np.float64, c1), np.ones(3))


def test_the_public_names_exist():
    for name in ("DeviceVectors", "residuals", "vector_residuals", "gram", "schur_vectors"):
        assert hasattr(pkg, name) and name in pkg.__all__
    import inspect

    assert inspect.signature(pkg.partialeigen).parameters["device"].default is False
    for sym in ("ks_vectors_create", "ks_vectors_destroy", "ks_vectors_dims", "ks_vectors_upload", "ks_vectors_download",
                "ks_vectors_col_ptr", "ks_basis_times_device", "ks_vectors_apply", "ks_vectors_residuals", "ks_vectors_gram"):
        assert sym in pkg._lib.PROTOTYPES and hasattr(pkg._lib.load(), sym)
