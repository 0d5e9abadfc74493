"""`-m gpu`: the matrix-free grid operator with periodic axes (`ks_operator_grid_periodic`, csrc/ks_grid.hpp: the periodic
instantiations of k_grid) -- mul!(y, A, x), src/expansion.jl:121, on a torus or with Bloch phases on the links that cross the cell
boundary, still with nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_matrix(..., periodic=, wrap=)` returns (tests/test_grid_periodic_cpu.py pins that
matrix to an independent assembly): a row is summed in the 13-slot order of include/kschur.h (ix), a wrap link at another place
than the interior link of its direction, so a plain product must carry the bits of `seq_matvec` on that matrix
(tests/spmv_reference.py) and of `csr_operator` applied to it; the Newton step is held to the bound of its operation sequence,
(L + 3) eps w with L the row length including the wrap links (x 4 in modulus for complex), never to a measured number.
Conventions as in tests/test_gpu_grid_operator.py: the destination column is poisoned with NaN, KS_GUARD=1 puts canary zones around
the basis and `guard_intact()` is asserted after every product, and x is asserted unchanged.

Shapes (tests/grid_periodic_cases.py): with t the tile extent along an axis, periodic axes at 3, t - 1, t, t + 1, 2 t + 1 -- a
partial last tile is where the +x / +y wrap neighbour is no halo cell but the LDS slot of an owned point outside the grid."""
import ctypes as C

import numpy as np
import pytest

import grid_cases as gc
import grid_periodic_cases as gp
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


def _check_plain(shape, per, dtype, ctx, x=None, wraps=(False, True)):
    """With and without a potential, wrap = None and distinct values: bits of seq_matvec on the host matrix, and of csr_operator
    of that matrix on the same x."""
    ndim = len(shape)
    t = gc.taps(ndim, dtype)
    x = gc.vector(shape, dtype) if x is None else x
    want = None
    for given in wraps:
        w = gp.wrap(ndim, dtype) if given else None
        for v in (None, gc.potential(shape, dtype)):
            A = pkg.host_grid_matrix(shape, t, v, periodic=per, wrap=w)
            assert A.nnz == gp.nnz(shape, per)
            want = ref.seq_matvec(A, x)
            op = pkg.grid_operator(shape, t, v, ctx=ctx, periodic=per, wrap=w)
            what = "grid %s periodic=%s %s potential=%s wrap=%s" % (shape, per, np.dtype(dtype).name, v is not None, given)
            assert op.shape == A.shape and op.dtype == np.dtype(dtype)
            info = op.grid_info
            assert info["shape"] == tuple(shape) and info["has_potential"] == (v is not None) and info["periodic"] == tuple(per)
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
@pytest.mark.parametrize("group", list(gp.GROUPS), ids=list(gp.GROUPS))
def test_plain_product_bit_for_bit(group, dtype, ctx):
    for shape, per in gp.GROUPS[group]:
        _check_plain(shape, per, dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_new_entry_point_without_a_periodic_axis_is_the_open_operator(shape, dtype, ctx):
    ndim = len(shape)
    t = gc.taps(ndim, dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        old = Checked(pkg.grid_operator(shape, t, v, ctx=ctx), x).plain()
        for per, w in ((False, None), ((False,) * ndim, gp.wrap(ndim, dtype))):
            op = pkg.grid_operator(shape, t, v, ctx=ctx, periodic=per, wrap=w)
            assert op.grid_info["periodic"] == (False,) * ndim
            assert np.array_equal(_bits(Checked(op, x).plain()), _bits(old))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.EDGE_CASES_X, ids=gp.case_id)
def test_non_finite_x_reaches_exactly_the_periodic_neighbours(case, dtype, ctx):
    """NaN at the corner point 0, Inf at the last point of the grid: the non-finite rows of y are exactly the periodic neighbour
    sets, wrap neighbours included.  A kernel that takes the +x neighbour of the last point of a line from the next line, or that
    multiplies a slot it should skip, puts a non-finite value into a row that is no neighbour (or a finite one into a neighbour)."""
    shape, per = case
    n = gc.size(shape)
    x = gc.vector(shape, dtype)
    x[0], x[n - 1] = np.nan, np.inf
    want = _check_plain(shape, per, dtype, ctx, x)
    hit = np.zeros(n, dtype=bool)
    hit[list(gp.neighbours(shape, per, 0) | gp.neighbours(shape, per, n - 1))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself)
    nx = shape[0]
    assert hit[nx - 1] and hit[n - nx]                 # the wrap neighbours along x: the other end of the SAME line
    if len(shape) > 1 and not per[1]:
        assert np.isfinite(want[2 * nx - 1])           # the last point of the next line is no neighbour of point 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", gp.EDGE_CASES, ids=gp.case_id)
def test_newton_step_within_its_forward_error_bound(case, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both (theta,
    sigma) pairs, both stores, with and without a potential, distinct wrap values; the two stores of the fused form carry the same
    values."""
    shape, per = case
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t, w = gc.taps(len(shape), dtype), gp.wrap(len(shape), dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_matrix(shape, t, v, periodic=per, wrap=w)
        P = Checked(pkg.grid_operator(shape, t, v, ctx=ctx, periodic=per, wrap=w), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.all(hp[2] == 2 * len(shape) + 1)      # L: the row length, wrap links included
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
                    got[fused, cacheable] = y
            monkeypatch.delenv("KS_SHIFT_FUSED")
            assert np.array_equal(_bits(got["1", False]), _bits(got["1", True]))
        _assert_plain_bits(P.plain(), ref.seq_matvec(A, x), "plain after shifted")


# ------------------------------------------------------------------------------------------------ whole solves
SOLVE_SHAPE = (12, 10, 9)
LAPLACE = np.array([-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0])


def _solve(op, sstep, dtype=np.float64):
    n = op.shape[0]
    ws = pkg.ArnoldiWorkspace(n, 20, dtype, ctx=op.ctx)
    if sstep is not None:
        ws.set_sstep(sstep)
    ws._v1 = pkg.matrices.start_vector(n).astype(dtype)
    dec, hist = pkg.partialschur_(op, ws, nev=4, which="SR", tol=1e-10)
    assert hist.converged and ws.guard_intact(), hist
    return dec, hist, ws


def test_whole_solve_real_is_interchangeable_with_the_stored_matrix(ctx):
    """-Laplacian + harmonic potential on the 12 x 10 x 9 torus, :SR, nev = 4.  set_sstep(0): the products are bit-identical, so
    eigenvalues, R and the History counts must be; the default s-step run takes the fused Newton step of the periodic kernel:
    same counts, eigenvalues within 1e-10."""
    v = gc.harmonic(SOLVE_SHAPE)
    A = pkg.host_grid_matrix(SOLVE_SHAPE, LAPLACE, v, periodic=True)
    assert np.all(np.diff(A.indptr) == 7)
    grid = pkg.grid_operator(SOLVE_SHAPE, LAPLACE, v.reshape(SOLVE_SHAPE[::-1]), ctx=ctx, periodic=True)
    stored = pkg.csr_operator(A, ctx)
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, c) for c in COUNTS] == [getattr(hs, c) for c in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    (db, hb, wb), (dsb, hsb, _) = _solve(grid, None), _solve(stored, None)
    assert (hb.mvproducts, hb.restarts, hb.nconverged) == (hsb.mvproducts, hsb.restarts, hsb.nconverged), (hb, hsb)
    assert np.abs(np.sort_complex(db.eigenvalues) - np.sort_complex(dsb.eigenvalues)).max() <= 1e-10
    assert wb.sstep_info["blocks"] > 0, wb.sstep_info      # (otherwise this ran the step-by-step path)


def test_whole_solve_bloch_matches_the_analytic_band_energies(ctx):
    """-Laplacian on 12 x 10 x 9 with Bloch phases theta = (0.7, 1.1, 1.9), ComplexF64, :SR, nev = 4, tol 1e-10: the eigenvalues
    are sum_a 2 - 2 cos((2 pi k_a + theta_a) / m_a); the lowest five are 0.0599, 0.2480, 0.2691, 0.3105, 0.3857 (smallest gap
    0.021: nothing is degenerate)."""
    theta = (0.7, 1.1, 1.9)
    one = [2.0 - 2.0 * np.cos((2.0 * np.pi * np.arange(m) + th) / m) for m, th in zip(SOLVE_SHAPE, theta)]
    exact = np.sort((one[0][:, None, None] + one[1][None, :, None] + one[2][None, None, :]).ravel())
    assert np.abs(exact[:5] - np.array([0.0599, 0.2480, 0.2691, 0.3105, 0.3857])).max() <= 5e-5 and np.diff(exact[:5]).min() >= 0.021
    op = pkg.grid_operator(SOLVE_SHAPE, LAPLACE, ctx=ctx, periodic=True, wrap=extras.bloch_wrap(LAPLACE, theta))
    assert op.dtype == np.complex128
    dec, hist, _ = _solve(op, None, np.complex128)
    assert hist.nconverged >= 4
    lam = np.sort_complex(dec.eigenvalues)[:4]
    print("Bloch eigenvalues:", lam, "exact:", exact[:4])
    assert np.abs(lam - exact[:4]).max() <= 1e-8
    resid, _qn = pkg.residuals(op, pkg.schur_vectors(dec), np.array(dec.R))
    print("Schur residuals on the device:", resid)
    assert np.all(resid <= 1e-8)


# ------------------------------------------------------------------------------------------------ refusals
def test_wrong_use_is_refused_and_size_reports_the_nnz(ctx):
    t = gc.taps(3, np.float64)
    with pytest.raises(pkg.ArgumentError, match="periodic axis 1.*extent 2"):
        pkg.grid_operator((4, 2, 3), t, ctx=ctx, periodic=(True, True, False))
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_operator((4, 3, 3), t, ctx=dctx, periodic=True)
    w = gp.wrap(3, np.float64)
    w[2] = np.inf
    with pytest.raises(pkg.ArgumentError, match="wrap value 2"):
        pkg.grid_operator((4, 3, 3), t, ctx=ctx, periodic=True, wrap=w)
    assert pkg.grid_operator((4, 3, 3), t, ctx=ctx, periodic=(False, True, True), wrap=w).shape == (36, 36)   # (x does not wrap: not read)
    shape, per = (5, 4, 3), (True, False, True)
    op = pkg.grid_operator(shape, t, ctx=ctx, periodic=per)
    n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
    pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
    assert (n.value, nnz.value, dt.value) == (60, gp.nnz(shape, per), pkg._lib.KS_F64)
    assert nnz.value == pkg.host_grid_matrix(shape, t, periodic=per).nnz
