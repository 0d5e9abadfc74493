"""`-m gpu`: star stencils of radius 2, 3, 4 with PERIODIC axes for the matrix-free grid operator
(`ks_operator_grid_star_periodic`, k_grid_star_per of csrc/ks_grid.hpp) -- mul!(y, A, x), src/expansion.jl:121, for central
differences of order 4, 6, 8 on a torus or with Bloch phases on the links that cross the cell boundary, with nothing stored per
non-zero.

The operator is DEFINED by the matrix `host_grid_star_matrix` returns (tests/test_grid_star_periodic_cpu.py pins that matrix to an
independent assembly and the place of every wrapped entry to the header's row order), so a plain product must carry the bits of
`seq_matvec` on that matrix and of `csr_operator` applied to it; the Newton step is held to the bound of its operation sequence,
(L + 3) eps w with L = 2 ndim R + 1 the row length, never to a measured number.  Conventions of tests/test_gpu_grid_star.py:
NaN-poisoned destination, KS_GUARD=1 and `guard_intact()` after every product, x unchanged.

Shapes (tests/grid_star_periodic_cases.py): with t the tile extent (32; 1024 where ny == 1; 16 and 512 for half tiles) and zc = 8 R,
periodic axes at 2 R + 1, 2 R + 2 (where a double wrap or a coinciding link would show), t - R, t - 1, t, t + 1, t + R, 2 t + 1 -- a
partial last tile is where up to R slots of owned points hold wrap images -- and z at 2 R + 1, 2 R + 2, zc - 1 ... 2 zc + 1."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_periodic_cases as gp
import grid_star_cases as sc
import grid_star_periodic_cases as sp_
import spmv_reference as ref
from __graft_entry__ import import_package
from test_gpu_grid_operator import COUNTS, Checked
from test_gpu_shifted_product import PAIRS, _assert_bound, _assert_plain_bits, _bits

pytestmark = pytest.mark.gpu
pkg = import_package()
from arnoldimethod_jl_amd import extras  # noqa: E402  (imported on demand: after the package is registered)

DTYPES = [np.float64, np.complex128]
IDS = ["f64", "c64"]
ENV = ("KS_SHIFT_FUSED", "KS_SHIFT_PLAIN", "KS_SPMV_FORMAT", "KS_SSTEP")


@pytest.fixture(scope="module")
def ctx():
    return pkg.Context(0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KS_GUARD", "1")


def _check_plain(shape, per, R, dtype, ctx, x=None, wraps=(False, True)):
    """With and without a potential, wrap = None and distinct values: bits of seq_matvec on the host matrix, and of csr_operator
    of that matrix on the same x."""
    ndim = len(shape)
    t = sc.taps(ndim, R, dtype)
    x = sc.vector(shape, dtype) if x is None else x
    want = None
    for given in wraps:
        w = sp_.wrap(ndim, R, dtype) if given else None
        for v in (None, sc.potential(shape, dtype)):
            A = pkg.host_grid_star_matrix(shape, t, R, v, periodic=per, wrap=w)
            assert A.nnz == sp_.nnz(shape, per, R)
            want = ref.seq_matvec(A, x)
            op = pkg.grid_star_operator(shape, t, R, v, ctx=ctx, periodic=per, wrap=w)
            what = "star %s periodic=%s R=%d %s potential=%s wrap=%s" % (shape, per, R, np.dtype(dtype).name, v is not None, given)
            assert op.shape == A.shape and op.dtype == np.dtype(dtype)
            info = op.grid_info
            assert info["shape"] == tuple(shape) and info["radius"] == R and info["has_potential"] == (v is not None)
            assert info["periodic"] == tuple(per)
            assert info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2)
            assert (info["wrap"] is None) if w is None else np.array_equal(info["wrap"], w)
            assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
            y = Checked(op, x).plain()
            _assert_plain_bits(y, want, what)
            stored = Checked(pkg.csr_operator(A, ctx), x).plain()
            _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
            assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("group", list(sp_.GROUPS), ids=list(sp_.GROUPS))
@pytest.mark.parametrize("R", sc.RADII)
def test_plain_product_bit_for_bit(R, group, dtype, ctx):
    for shape, per in sp_.GROUPS[group](R):
        _check_plain(shape, per, R, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", sp_.EDGE_CASES_X, ids=sp_.case_id)
@pytest.mark.parametrize("R", sc.RADII)
def test_non_finite_x_reaches_exactly_the_periodic_neighbours(R, case, dtype, ctx):
    """NaN at the corner point 0, Inf at the last point of the grid: the non-finite rows of y are exactly the periodic neighbour
    sets, wrap neighbours included.  A kernel that takes a wrapped neighbour from the next line, wraps twice, or multiplies a slot
    it should skip puts a non-finite value into a row that is no neighbour (or a finite one into a neighbour)."""
    shape, per = case
    n = sc.size(shape)
    x = sc.vector(shape, dtype)
    x[0], x[n - 1] = np.nan, np.inf
    want = _check_plain(shape, per, R, dtype, ctx, x)
    hit = np.zeros(n, dtype=bool)
    hit[list(sp_.neighbours(shape, per, 0, R) | sp_.neighbours(shape, per, n - 1, R))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself)
    nx = shape[0]
    assert all(hit[nx - d] and hit[n - nx + d - 1] for d in range(1, R + 1))   # the wrap neighbours along x: the other end of the SAME line
    if len(shape) > 1 and not per[1]:
        assert np.all(np.isfinite(want[2 * nx - R : 2 * nx]))                  # the end of the next line is no neighbour of point 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", sp_.EDGE_CASES_X, ids=sp_.case_id)
@pytest.mark.parametrize("R", sc.RADII)
def test_newton_step_within_its_forward_error_bound(R, case, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid_star_per) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both
    (theta, sigma) pairs, both stores, with and without a potential, distinct wrap values; the two stores of the fused form carry
    the same values."""
    shape, per = case
    ndim = len(shape)
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t, w = sc.taps(ndim, R, dtype), sp_.wrap(ndim, R, dtype)
    x = sc.vector(shape, dtype)
    for v in (None, sc.potential(shape, dtype)):
        A = pkg.host_grid_star_matrix(shape, t, R, v, periodic=per, wrap=w)
        P = Checked(pkg.grid_star_operator(shape, t, R, v, ctx=ctx, periodic=per, wrap=w), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.array_equal(hp[2], np.diff(A.indptr)) and hp[2].max() == 2 * ndim * R + 1   # L: the row length, wrap links included
            if all(per):
                assert hp[2].min() == 2 * ndim * R + 1
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "star %s %s R=%d %s potential=%s theta=%s fused=%s cacheable=%d"
                                  % (shape, per, R, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R", sc.RADII)
def test_without_a_periodic_axis_it_is_the_open_star_operator(R, dtype, ctx):
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    th, sg = PAIRS[kind][0]
    for shape in sc.EDGE_SHAPES:
        ndim = len(shape)
        t, v, x = sc.taps(ndim, R, dtype), sc.potential(shape, dtype), sc.vector(shape, dtype)
        old = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, radius=R), x)
        want, want_s = old.plain(), old.shifted(th, sg, False)
        for kw in (dict(), dict(periodic=False), dict(periodic=(False,) * ndim, wrap=sp_.wrap(ndim, R, dtype))):
            op = pkg.grid_star_operator(shape, t, R, v, ctx=ctx, **kw)
            assert op.grid_info["periodic"] == (False,) * ndim
            new = Checked(op, x)
            assert np.array_equal(_bits(new.plain()), _bits(want))
            assert np.array_equal(_bits(new.shifted(th, sg, False)), _bits(want_s))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_radius_one_is_the_existing_periodic_operator(dtype, ctx):
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    th, sg = PAIRS[kind][0]
    for shape, per in gp.EDGE_CASES_X:
        ndim = len(shape)
        t, v, w, x = gc.taps(ndim, dtype), gc.potential(shape, dtype), gp.wrap(ndim, dtype), gc.vector(shape, dtype)
        old = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, periodic=per, wrap=w), x)
        new = Checked(pkg.grid_star_operator(shape, t, 1, v, ctx=ctx, periodic=per, wrap=w), x)
        assert np.array_equal(_bits(new.plain()), _bits(old.plain()))
        assert np.array_equal(_bits(new.shifted(th, sg, False)), _bits(old.shifted(th, sg, False)))


# ------------------------------------------------------------------------------------------------ whole solves
SOLVE_SHAPE = (12, 10, 9)     # 9 = 2 * 4 + 1: the shortest periodic axis of radius 4


def _solve(op, sstep, dtype=np.float64):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, dtype, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n).astype(dtype)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


@pytest.mark.parametrize("R", [2, 4])
def test_whole_solve_real_is_interchangeable_with_the_stored_matrix(R, ctx):
    """Central differences of order 2 R + harmonic potential on the 12 x 10 x 9 torus, :SR, nev = 4.  set_sstep(0): the products are
    bit-identical, so eigenvalues, R and the History counts must be; the default s-step run takes the fused Newton step of the
    periodic kernel: same counts, eigenvalues within 1e-10."""
    v = gc.harmonic(SOLVE_SHAPE)
    t = extras.fd_laplacian_taps(3, 2 * R)
    A = pkg.host_grid_star_matrix(SOLVE_SHAPE, t, R, v, periodic=True)
    assert np.all(np.diff(A.indptr) == 6 * R + 1)
    grid = pkg.grid_star_operator(SOLVE_SHAPE, t, R, v.reshape(SOLVE_SHAPE[::-1]), ctx=ctx, periodic=True)
    stored = pkg.csr_operator(A, ctx)
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, c) for c in COUNTS] == [getattr(hs, c) for c in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    (db, hb, wb), (dsb, hsb, _) = _solve(grid, None), _solve(stored, None)
    assert (hb.mvproducts, hb.restarts, hb.nconverged) == (hsb.mvproducts, hsb.restarts, hsb.nconverged), (hb, hsb)
    assert np.abs(np.sort_complex(db.eigenvalues) - np.sort_complex(dsb.eigenvalues)).max() <= 1e-10
    assert wb.sstep_info["blocks"] > 0, wb.sstep_info      # (otherwise this ran the step-by-step path)


BANDS = {2: (0.06007, 0.25255, 0.27303, 0.31641, 0.39489), 4: (0.06007, 0.25269, 0.27314, 0.31662, 0.39531)}


@pytest.mark.parametrize("R", [2, 4])
def test_whole_solve_bloch_matches_the_analytic_band_energies(R, ctx):
    """Central differences of order 2 R on 12 x 10 x 9 with Bloch phases theta = (0.7, 1.1, 1.9), ComplexF64, no potential, :SR,
    nev = 4, tol 1e-10: the eigenvalues are sum_a [w_0 + 2 sum_d w_d cos(d (2 pi k_a + theta_a) / m_a)]; the lowest five are BANDS[R]
    (smallest gap among the lowest six 0.020: nothing is degenerate)."""
    theta = (0.7, 1.1, 1.9)
    w1 = extras.fd_laplacian_taps(1, 2 * R)     # [w_R ... w_1, w_0, w_1 ... w_R]
    one = []
    for m, th in zip(SOLVE_SHAPE, theta):
        q = (2.0 * np.pi * np.arange(m) + th) / m
        one.append(w1[R] + 2.0 * sum(w1[R + d] * np.cos(d * q) for d in range(1, R + 1)))
    exact = np.sort((one[0][:, None, None] + one[1][None, :, None] + one[2][None, None, :]).ravel())
    assert np.abs(exact[:5] - np.array(BANDS[R])).max() <= 5e-5 and np.diff(exact[:6]).min() >= 0.020
    t = extras.fd_laplacian_taps(3, 2 * R)
    op = pkg.grid_star_operator(SOLVE_SHAPE, t, R, ctx=ctx, periodic=True, wrap=extras.bloch_wrap(t, theta, radius=R))
    assert op.dtype == np.complex128
    dec, hist, _ = _solve(op, None, np.complex128)
    assert hist.nconverged >= 4
    lam = np.sort_complex(dec.eigenvalues)[:4]
    print("Bloch eigenvalues:", lam, "exact:", exact[:4])
    assert np.abs(lam - exact[:4]).max() <= 1e-8
    resid, _qn = pkg.residuals(op, pkg.schur_vectors(dec), np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8)


# ------------------------------------------------------------------------------------------------ composition, refusals, size
def test_composes_with_device_vectors_residuals_and_products(ctx):
    """ComplexF64, Hermitian: symmetric taps, a real harmonic potential and Bloch phases on the wrapped links."""
    shape, R, dtype = (33, 9, 9), 3, np.complex128
    t = sc.taps(3, R, dtype, symmetric=True)
    v = gc.harmonic(shape).astype(dtype)
    w = extras.bloch_wrap(t, (0.7, 1.1, 1.9), radius=R)
    A = pkg.host_grid_star_matrix(shape, t, R, v, periodic=True, wrap=w)
    assert (A != A.conj().T).nnz == 0
    op = pkg.grid_star_operator(shape, t, R, v, ctx=ctx, periodic=True, wrap=w)
    x = sc.vector(shape, dtype)
    y1 = Checked(op, x).plain()
    y2 = Checked(op, y1).plain()
    prod = pkg.product_operator(op, op, ctx=ctx)
    _assert_plain_bits(Checked(prod, x).plain(), y2, "product of two periodic star operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(A, ref.seq_matvec(A, x))))
    dec, hist = pkg.partialschur(op, v1=sc.vector(shape, dtype, seed=3), nev=3, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    AQ = Q.apply(op)
    assert np.abs(AQ.download() - A @ Q.download()).max() <= 1e-12 * abs(A).sum(axis=1).max()
    resid, qn = pkg.residuals(op, Q, np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8) and np.all(np.abs(qn - 1.0) <= 1e-12)


@pytest.mark.parametrize("R", sc.RADII)
def test_wrong_use_is_refused_and_size_reports_the_nnz(R, ctx):
    t = sc.taps(3, R, np.float64)
    m = 2 * R + 1
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_star_operator((m, m, m), t, R, ctx=dctx, periodic=True)
    with pytest.raises(pkg.ArgumentError, match=r"(?s)periodic axis 1.*extent %d.*radius %d" % (2 * R, R)):
        pkg.grid_star_operator((m, 2 * R, m), t, R, ctx=ctx, periodic=(True, True, False))
    w = sp_.wrap(3, R, np.float64)
    w[2 * R] = np.inf
    with pytest.raises(pkg.ArgumentError, match=r"wrap value %d\b" % (2 * R)):
        pkg.grid_star_operator((m, m, m), t, R, ctx=ctx, periodic=True, wrap=w)
    assert pkg.grid_star_operator((m, m, m), t, R, ctx=ctx, periodic=(False, True, True), wrap=w).shape == (m ** 3,) * 2   # (x does not wrap: not read)
    for shape, per in [((m, 4, m + 2), (True, False, True)), ((m + 1, m), (True, True)), ((2 * m,), (True,)), ((m, m, m), sp_.ALL)]:
        tt = sc.taps(len(shape), R, np.float64)
        op = pkg.grid_star_operator(shape, tt, R, ctx=ctx, periodic=per)
        n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
        pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
        assert (n.value, nnz.value, dt.value) == (sc.size(shape), sp_.nnz(shape, per, R), pkg._lib.KS_F64)
        assert nnz.value == pkg.host_grid_star_matrix(shape, tt, R, periodic=per).nnz
