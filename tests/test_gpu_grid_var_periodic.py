"""`-m gpu`: the matrix-free variable-coefficient grid operator with periodic axes (`ks_operator_grid_var_periodic`, the periodic
instantiation of k_grid_var, csrc/ks_grid_var.hpp) -- mul!(y, A, x), src/expansion.jl:121, for A = -div(c(x) grad) + V(x) on a torus
or with Bloch phases on the links that cross the cell boundary, nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_variable_matrix(..., periodic=, wrap=)` returns (tests/test_grid_var_periodic_cpu.py
pins that matrix to an independent assembly), so a plain product must carry the bits of `seq_matvec` on that matrix and of
`csr_operator` applied to it.  The random coefficient makes every link's entry its own: a kernel that wraps x but not c (the halo
cell, the owned point beyond a partial last tile, plane -1 or plane nz), or sums a wrap link at the place of the interior link of its
direction, fails there.  Conventions of tests/test_gpu_grid_var.py: the `Checked` wrapper, a NaN-poisoned destination, KS_GUARD=1 and
`guard_intact()` after every product, x unchanged."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_periodic_cases as gp
import grid_var_cases as vc
import grid_var_periodic_cases as vp
import spmv_reference as ref
from __graft_entry__ import import_package
from test_gpu_grid_operator import Checked
from test_gpu_shifted_product import PAIRS, _assert_bound, _assert_plain_bits, _bits

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
ENV = ("KS_SHIFT_FUSED", "KS_SHIFT_PLAIN", "KS_SPMV_FORMAT", "KS_SSTEP")
COUNTS = ("mvproducts", "nconverged", "converged", "nev", "restarts", "reorth", "breakdowns", "explicit_steps")


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _check_plain(shape, per, dtype, ctx, x=None):
    """With and without a potential, wrap = None and distinct values: bits of seq_matvec on the host matrix, and of csr_operator
    of that matrix on the same x."""
    ndim = len(shape)
    t = gc.taps(ndim, dtype)
    c = vc.random_coeff(shape)
    x = gc.vector(shape, dtype) if x is None else x
    want = None
    for w in (None, gp.wrap(ndim, dtype)):
        for v in (None, gc.potential(shape, dtype)):
            A = pkg.host_grid_variable_matrix(shape, t, c, v, periodic=per, wrap=w)
            assert A.nnz == gp.nnz(shape, per)
            want = ref.seq_matvec(A, x)
            op = pkg.grid_variable_operator(shape, t, c, v, ctx=ctx, periodic=per, wrap=w)
            what = "variable grid %s periodic=%s %s potential=%s wrap=%s" % (shape, per, np.dtype(dtype).name, v is not None, w is not None)
            assert op.shape == A.shape and op.dtype == np.dtype(dtype)
            assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
            y = Checked(op, x).plain()
            _assert_plain_bits(y, want, what)
            stored = Checked(pkg.csr_operator(A, ctx), x).plain()
            _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
            assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("group", list(vp.GROUPS), ids=list(vp.GROUPS))
def test_plain_product_bit_for_bit(group, dtype, ctx):
    for shape, per in vp.GROUPS[group]:
        _check_plain(shape, per, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_new_entry_point_without_a_periodic_axis_is_the_open_operator(shape, dtype, ctx):
    ndim = len(shape)
    t, c = gc.taps(ndim, dtype), vc.random_coeff(shape)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        old = Checked(pkg.grid_variable_operator(shape, t, c, v, ctx=ctx), x).plain()
        for per, w in ((False, None), ((False,) * ndim, gp.wrap(ndim, dtype))):
            op = pkg.grid_variable_operator(shape, t, c, v, ctx=ctx, periodic=per, wrap=w)
            assert op.grid_info["periodic"] == (False,) * ndim and op.grid_info["variable"] is True
            assert np.array_equal(_bits(Checked(op, x).plain()), _bits(old))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.EDGE_CASES, ids=gp.case_id)
def test_unit_coefficient_gives_the_bits_of_the_constant_coefficient_periodic_operator(case, dtype, ctx):
    shape, per = case
    ndim = len(shape)
    t, w = gc.taps(ndim, dtype), gp.wrap(ndim, dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        const = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, periodic=per, wrap=w), x).plain()
        var = Checked(pkg.grid_variable_operator(shape, t, np.ones(gc.size(shape)), v, ctx=ctx, periodic=per, wrap=w), x).plain()
        assert np.array_equal(_bits(var), _bits(const))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.EDGE_CASES_X, ids=gp.case_id)
def test_non_finite_x_reaches_exactly_the_periodic_neighbours(case, dtype, ctx):
    """NaN at the corner point 0, Inf at the last point of the grid: the non-finite rows of y are exactly the periodic neighbour
    sets, wrap neighbours included."""
    shape, per = case
    n = gc.size(shape)
    x = gc.vector(shape, dtype)
    x[0], x[n - 1] = np.nan, np.inf
    want = _check_plain(shape, per, dtype, ctx, x)
    hit = np.zeros(n, dtype=bool)
    hit[list(gp.neighbours(shape, per, 0) | gp.neighbours(shape, per, n - 1))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.EDGE_CASES, ids=gp.case_id)
def test_newton_step_within_its_forward_error_bound(case, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of the periodic k_grid_var) and with KS_SHIFT_FUSED=0 (the product and a streaming pass):
    both (theta, sigma) pairs, both stores, with and without a potential, distinct wrap values; the two stores of the fused form
    carry the same values."""
    shape, per = case
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t, w = gc.taps(len(shape), dtype), gp.wrap(len(shape), dtype)
    c = vc.random_coeff(shape)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_variable_matrix(shape, t, c, v, periodic=per, wrap=w)
        P = Checked(pkg.grid_variable_operator(shape, t, c, v, ctx=ctx, periodic=per, wrap=w), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.all(hp[2] == 2 * len(shape) + 1)      # L: the row length, wrap links included
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "variable grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        # the plain product after shifted ones is still the plain product
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ whole solves
def _solve(op, sstep, dtype=np.float64):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, dtype, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n).astype(dtype)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


@pytest.fixture(scope="module")
def terms():
    """-div(c grad) + the harmonic potential on the 12 x 10 x 9 torus, the smooth coefficient with a jump: (c, taps, diagonal)."""
    c = vc.coeff(vp.SOLVE_SHAPE)
    taps, diag = extras.diffusion_terms(vp.SOLVE_SHAPE, c, potential=vp.solve_potential(), periodic=True)
    return c, taps, diag


def test_whole_solve_real_is_interchangeable_with_the_stored_matrix(terms, ctx):
    """:SR, nev = 4.  set_sstep(0): the products are bit-identical, so eigenvalues, R and the History counts must be; the default
    s-step run takes the fused Newton step of the periodic kernel: same counts, eigenvalues within 1e-10."""
    c, taps, diag = terms
    shape = vp.SOLVE_SHAPE
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True)
    assert np.all(np.diff(A.indptr) == 7) and (A - A.T).nnz == 0
    grid = pkg.grid_variable_operator(shape, taps, c.reshape(shape[::-1]), diag.reshape(shape[::-1]), ctx=ctx, periodic=True)
    stored = pkg.csr_operator(A, ctx)
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, k) for k in COUNTS] == [getattr(hs, k) for k in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    (db, hb, wb), (dsb, hsb, _) = _solve(grid, None), _solve(stored, None)
    assert (hb.mvproducts, hb.restarts, hb.nconverged) == (hsb.mvproducts, hsb.restarts, hsb.nconverged), (hb, hsb)
    assert np.abs(np.sort_complex(db.eigenvalues) - np.sort_complex(dsb.eigenvalues)).max() <= 1e-10
    assert wb.sstep_info["blocks"] > 0, wb.sstep_info      # (otherwise this ran the step-by-step path)


def test_whole_solve_bloch_matches_the_dense_spectrum(terms, ctx):
    """The same grid at the k-point theta = (0.7, 1.1, 1.9), ComplexF64, :SR, nev = 4, tol 1e-10: real eigenvalues, the four smallest
    of a dense eigvalsh of the host matrix."""
    c, taps, diag = terms
    shape = vp.SOLVE_SHAPE
    w = extras.bloch_wrap(taps, vp.SOLVE_THETA)
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True, wrap=w)
    assert A.dtype == np.complex128 and (A - A.conj().T).nnz == 0
    exact = np.linalg.eigvalsh(A.toarray())[:4]
    op = pkg.grid_variable_operator(shape, taps, c, diag, ctx=ctx, periodic=True, wrap=w)
    assert op.dtype == np.complex128
    dec, hist, _ = _solve(op, None, np.complex128)
    assert hist.nconverged >= 4
    lam = np.sort_complex(dec.eigenvalues)[:4]
    print("Bloch eigenvalues:", lam, "dense:", exact)
    assert np.abs(lam.imag).max() <= 1e-10
    assert np.abs(lam.real - exact).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ composition, size, refusals
def test_composes_with_device_vectors_residuals_and_products(ctx):
    shape, dtype = (33, 7, 9), np.complex128
    c = vc.coeff(shape)
    taps, diag = extras.diffusion_terms(shape, c, potential=gc.harmonic(shape), periodic=True)
    w = extras.bloch_wrap(taps, (0.7, 1.1, 1.9))
    A = pkg.host_grid_variable_matrix(shape, taps, c, diag, periodic=True, wrap=w)
    op = pkg.grid_variable_operator(shape, taps, c, diag, ctx=ctx, periodic=True, wrap=w)
    assert A.dtype == op.dtype == np.dtype(dtype)
    x = gc.vector(shape, dtype)
    y1 = Checked(op, x).plain()
    y2 = Checked(op, y1).plain()
    prod = pkg.product_operator(op, op, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two periodic variable-coefficient operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(A, ref.seq_matvec(A, x))))
    dec, hist = pkg.partialschur(op, v1=gc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    AQ = Q.apply(op)
    assert np.abs(AQ.download() - A @ Q.download()).max() <= 1e-12 * abs(A).sum(axis=1).max()
    resid, qn = pkg.residuals(op, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_size_and_grid_info(dtype, ctx):
    code = pkg._lib.KS_F64 if np.dtype(dtype).kind == "f" else pkg._lib.KS_C64
    for shape, per in [((5, 4, 3), (True, False, True)), ((9, 2, 11), (True, False, True)), ((7,), (True,)), ((3, 12), (True, True))]:
        ndim = len(shape)
        t, c, w = gc.taps(ndim, dtype), vc.coeff(shape), gp.wrap(ndim, dtype)
        for v in (None, gc.potential(shape, dtype)):
            for wv in (None, w):
                op = pkg.grid_variable_operator(shape, t, c, v, ctx=ctx, periodic=per, wrap=wv)
                n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
                pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
                assert (n.value, nnz.value, dt.value) == (gc.size(shape), gp.nnz(shape, per), code)
                assert nnz.value == pkg.host_grid_variable_matrix(shape, t, c, v, periodic=per, wrap=wv).nnz
                info = op.grid_info
                assert info["shape"] == tuple(shape) and info["variable"] is True and info["has_potential"] == (v is not None)
                assert info["periodic"] == tuple(per) and np.array_equal(info["taps"], t)
                assert (info["wrap"] is None) if wv is None else np.array_equal(info["wrap"], wv)
                assert info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2) + 8
    # a complex wrap promotes the element type; `periodic=None` keeps the open operator's info
    op = pkg.grid_variable_operator((5,), np.array([-1.0, 0.0, -1.0]), np.ones(5), ctx=ctx, periodic=True, wrap=np.array([-1j, 1j]))
    assert op.dtype == np.complex128
    assert "periodic" not in pkg.grid_variable_operator((5,), np.array([-1.0, 0.0, -1.0]), np.ones(5), ctx=ctx).grid_info


def test_wrong_use_is_refused(ctx):
    t, c = gc.taps(3, np.float64), np.ones(36)
    with pytest.raises(pkg.ArgumentError, match="periodic axis 1.*extent 2"):
        pkg.grid_variable_operator((4, 2, 3), t, np.ones(24), ctx=ctx, periodic=(True, True, False))
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_variable_operator((4, 3, 3), t, c, ctx=dctx, periodic=True)
    w = gp.wrap(3, np.float64)
    w[2] = np.inf
    with pytest.raises(pkg.ArgumentError, match="wrap value 2"):
        pkg.grid_variable_operator((4, 3, 3), t, c, ctx=ctx, periodic=True, wrap=w)
    assert pkg.grid_variable_operator((4, 3, 3), t, c, ctx=ctx, periodic=(False, True, True), wrap=w).shape == (36, 36)   # (x does not wrap: not read)
    with pytest.raises(pkg.ArgumentError, match="coeff"):
        pkg.grid_variable_operator((4, 3, 3), t, c + 0j, ctx=ctx, periodic=True)
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.grid_variable_operator((4, 3, 3), t, c, dtype=np.float64, ctx=ctx, periodic=True, wrap=gp.wrap(3, np.complex128))
    bad = c.copy()
    bad[13] = np.nan
    with pytest.raises(pkg.ArgumentError, match="coefficient entry 13"):
        pkg.grid_variable_operator((4, 3, 3), t, bad, ctx=ctx, periodic=True)
