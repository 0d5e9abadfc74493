"""`-m gpu`: the matrix-free box-stencil grid operator with periodic axes (`ks_operator_grid_box_periodic`, k_grid_box_per of
csrc/ks_grid_box.hpp) -- mul!(y, A, x), src/expansion.jl:121, for the 9- / 27-point stencil on a torus with one entry per class of
boundary-crossing link (Bloch phases: a crystal in a non-orthogonal cell), nothing stored per non-zero.

The operator is DEFINED by the matrix `host_grid_box_matrix(..., periodic=, links=)` returns (tests/test_grid_box_periodic_cpu.py
pins that matrix to an independent assembly), so a plain product must carry the bits of `seq_matvec` on that matrix and of
`csr_operator` applied to it.  All taps and all link values are distinct with full mantissas, so a kernel that takes the entry of
another class, loads a wrap image from the wrong end (or the corner image from a point other than (0, 0)), adds the terms of an
edge row in the interior order, or adds the links to plane 0 / plane nz - 1 at the wrong end of a row fails there.  Conventions of
tests/test_gpu_grid_box.py: NaN-poisoned destination, KS_GUARD=1 and `guard_intact()` after every product, x unchanged.

Cases: tests/grid_box_periodic_cases.py."""
import ctypes as C

import numpy as np
import pytest

import grid_box_periodic_cases as pc
import grid_cases as gc
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


def _check_plain(shape, flags, dtype, ctx, x=None):
    """With and without a potential, distinct link values: bits of seq_matvec on the host matrix, and of csr_operator of that
    matrix on the same x."""
    ndim = len(shape)
    t, w = pc.taps(ndim, dtype), pc.links(ndim, dtype)
    x = gc.vector(shape, dtype) if x is None else x
    want = None
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_box_matrix(shape, t, v, periodic=flags, links=w)
        assert A.nnz == pc.nnz(shape, flags)
        want = ref.seq_matvec(A, x)
        op = pkg.grid_box_operator(shape, t, v, ctx=ctx, periodic=flags, links=w)
        what = "box grid %s periodic=%s %s potential=%s" % (shape, flags, np.dtype(dtype).name, v is not None)
        assert op.shape == A.shape and op.dtype == np.dtype(dtype)
        assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
        y = Checked(op, x).plain()
        _assert_plain_bits(y, want, what)
        stored = Checked(pkg.csr_operator(A, ctx), x).plain()
        _assert_plain_bits(y, np.where(np.isfinite(want), stored, np.nan), what + " against csr_operator")
        assert np.array_equal(np.isfinite(stored), np.isfinite(y))
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_plain_product_bit_for_bit(case, dtype, ctx):
    _check_plain(case[0], case[1], dtype, ctx)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", gc.EDGE_SHAPES, ids=["1d", "2d", "3d"])
def test_new_entry_point_without_a_periodic_axis_is_the_open_operator(shape, dtype, ctx):
    ndim = len(shape)
    t, w = pc.taps(ndim, dtype), pc.links(ndim, dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        old = Checked(pkg.grid_box_operator(shape, t, v, ctx=ctx), x).plain()
        for flags, wv in ((False, None), ((False,) * ndim, w)):
            op = pkg.grid_box_operator(shape, t, v, ctx=ctx, periodic=flags, links=wv)
            assert op.grid_info["periodic"] == (False,) * ndim and op.grid_info["box"] is True
            assert np.array_equal(_bits(Checked(op, x).plain()), _bits(old))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.case_id)
def test_non_finite_x_reaches_exactly_the_periodic_neighbours(case, dtype, ctx):
    """NaN at the last point of an x-line, Inf at corner 0: the non-finite rows of y are exactly the neighbour sets, wrap images
    included -- a kernel that multiplies an absent slot, or reads an image that is no neighbour, puts a non-finite value elsewhere."""
    shape, flags = case
    nx, ny, nz = list(shape) + [1] * (3 - len(shape))
    x = gc.vector(shape, dtype)
    p_nan = (nx - 1) + nx * ((1 if ny > 1 else 0) + ny * (1 if nz > 1 else 0))
    p_inf = 0
    x[p_nan], x[p_inf] = np.nan, np.inf
    want = _check_plain(shape, flags, dtype, ctx, x)
    hit = np.zeros(gc.size(shape), dtype=bool)
    hit[list(pc.neighbours(shape, flags, p_nan) | pc.neighbours(shape, flags, p_inf))] = True
    assert np.array_equal(~np.isfinite(want), hit)     # (the reference itself)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.case_id)
def test_newton_step_within_its_forward_error_bound(case, dtype, ctx, monkeypatch):
    """ws.apply_shifted, fused (one launch of k_grid_box_per) and with KS_SHIFT_FUSED=0 (the product and a streaming pass): both
    (theta, sigma) pairs, both stores, with and without a potential; the bound is (L + 3) eps w with L the row length, 3^ndim on
    a full torus; the two stores of the fused form carry the same values."""
    shape, flags = case
    kind = "c" if np.dtype(dtype).kind == "c" else "f"
    t, w = pc.taps(len(shape), dtype), pc.links(len(shape), dtype)
    x = gc.vector(shape, dtype)
    for v in (None, gc.potential(shape, dtype)):
        A = pkg.host_grid_box_matrix(shape, t, v, periodic=flags, links=w)
        P = Checked(pkg.grid_box_operator(shape, t, v, ctx=ctx, periodic=flags, links=w), x)
        for th, sg in PAIRS[kind]:
            hp = ref.hp_shifted(A, x, th, sg)
            assert np.array_equal(hp[2], np.diff(A.indptr)) and np.all(hp[2] == 3 ** len(shape))   # L: the row length on the torus
            got = {}
            for fused in ("1", "0"):
                monkeypatch.setenv("KS_SHIFT_FUSED", fused)
                for cacheable in (False, True):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "periodic box grid %s %s potential=%s theta=%s fused=%s cacheable=%d" % (shape, kind, v is not None, th, fused, cacheable))
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


def test_whole_solve_real_is_interchangeable_with_the_stored_matrix(ctx):
    """-div(D grad) + the harmonic potential on the 12 x 10 x 9 torus with a full tensor D, :SR, nev = 4.  set_sstep(0): the products
    are bit-identical, so eigenvalues, R and the History counts must be; the default s-step run takes the fused Newton step of the
    periodic kernel: same counts, eigenvalues within 1e-10."""
    shape = pc.SOLVE_SHAPE
    taps, V = extras.tensor_laplacian_taps(pc.SOLVE_TENSOR), pc.solve_potential()
    A = pkg.host_grid_box_matrix(shape, taps, V, periodic=True)
    assert np.all(np.diff(A.indptr) == 27) and (A - A.T).nnz == 0
    grid = pkg.grid_box_operator(shape, taps.reshape(3, 3, 3), V.reshape(shape[::-1]), ctx=ctx, periodic=True)
    stored = pkg.csr_operator(A, ctx)
    (dg, hg, _), (ds, hs, _) = _solve(grid, 0), _solve(stored, 0)
    assert [getattr(hg, k) for k in COUNTS] == [getattr(hs, k) for k in COUNTS], (hg, hs)
    assert np.array_equal(_bits(dg.eigenvalues), _bits(ds.eigenvalues))
    assert np.array_equal(_bits(np.array(dg.R)), _bits(np.array(ds.R)))
    (db, hb, wb), (dsb, hsb, _) = _solve(grid, None), _solve(stored, None)
    assert (hb.mvproducts, hb.restarts, hb.nconverged) == (hsb.mvproducts, hsb.restarts, hsb.nconverged), (hb, hsb)
    assert np.abs(np.sort_complex(db.eigenvalues) - np.sort_complex(dsb.eigenvalues)).max() <= 1e-10
    assert wb.sstep_info["blocks"] > 0, wb.sstep_info      # (otherwise this ran the step-by-step path)


def test_whole_solve_bloch_matches_eigsh(ctx):
    """The same grid at the k-point theta = (0.7, 1.1, 1.9) with `box_bloch_links`, ComplexF64, :SR, nev = 4, tol 1e-10: real
    eigenvalues, the four smallest of scipy's eigsh of the host matrix."""
    import scipy.sparse.linalg as spla

    shape = pc.SOLVE_SHAPE
    taps, V = extras.tensor_laplacian_taps(pc.SOLVE_TENSOR), pc.solve_potential()
    w = extras.box_bloch_links(taps, pc.SOLVE_THETA)
    A = pkg.host_grid_box_matrix(shape, taps, V, periodic=True, links=w)
    assert A.dtype == np.complex128 and (A - A.conj().T).nnz == 0
    exact = np.sort(spla.eigsh(A.tocsc(), k=4, sigma=0.0, which="LM", return_eigenvectors=False))
    op = pkg.grid_box_operator(shape, taps, V, ctx=ctx, periodic=True, links=w.reshape(5, 5, 5))
    assert op.dtype == np.complex128
    dec, hist, _ = _solve(op, None, np.complex128)
    assert hist.nconverged >= 4
    lam = np.sort_complex(dec.eigenvalues)[:4]
    print("Bloch eigenvalues:", lam, "eigsh:", exact)
    assert np.abs(lam.imag).max() <= 1e-10
    assert np.abs(lam.real - exact).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ composition, size, refusals
def test_generalized_residuals_of_the_periodic_q1_pencil(ctx):
    """Periodic Q1 stiffness (plus a harmonic term that separates its lowest eigenvalues) and mass matrix with Bloch links on
    (33, 7, 9): ||K x - lambda M x|| from the two device operators against the same quantity from the two host matrices."""
    shape, dtype = (33, 7, 9), np.complex128
    kt, mt = extras.q1_fem_taps(3)
    V = 4.0 * gc.harmonic(shape)
    wk, wm = extras.box_bloch_links(kt, pc.SOLVE_THETA), extras.box_bloch_links(mt, pc.SOLVE_THETA)
    K = pkg.host_grid_box_matrix(shape, kt, V, periodic=True, links=wk)
    M = pkg.host_grid_box_matrix(shape, mt, periodic=True, links=wm)
    opK = pkg.grid_box_operator(shape, kt, V, ctx=ctx, periodic=True, links=wk)
    opM = pkg.grid_box_operator(shape, mt, ctx=ctx, periodic=True, links=wm)
    assert K.dtype == M.dtype == opK.dtype == opM.dtype == np.dtype(dtype)
    assert (K - K.conj().T).nnz == 0 and (M - M.conj().T).nnz == 0
    x = gc.vector(shape, dtype)
    y1 = Checked(opK, x).plain()
    y2 = Checked(opK, y1).plain()
    _assert_plain_bits(Checked(pkg.product_operator(opK, opK, ctx=ctx), x).plain(), y2, "product of two periodic box operators")
    assert np.array_equal(_bits(y2), _bits(ref.seq_matvec(K, ref.seq_matvec(K, x))))
    dec, hist = pkg.partialschur(opK, v1=gc.vector(shape, dtype, seed=3), nev=2, which="SR", tol=1e-10, maxdim=24)
    assert hist.converged
    Q = pkg.schur_vectors(dec)
    Qh = Q.download()
    lam = np.asarray(dec.eigenvalues)[: Qh.shape[1]].astype(dtype)
    resid, bn = pkg.residuals(opK, Q, lam, opM)
    MQ = M @ Qh
    want = np.linalg.norm(K @ Qh - MQ * lam[None, :], axis=0)
    tol = 1e-12 * (abs(K).sum(axis=1).max() + np.abs(lam).max() * abs(M).sum(axis=1).max())
    print("generalized residuals on the device:", resid, "on the host:", want, "tolerance", tol)
    assert np.abs(resid - want).max() <= tol and np.abs(bn - np.linalg.norm(MQ, axis=0)).max() <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_size_and_grid_info(dtype, ctx):
    code = pkg._lib.KS_F64 if np.dtype(dtype).kind == "f" else pkg._lib.KS_C64
    for shape, flags in [((5, 4, 3), (True, False, True)), ((9, 2, 11), (True, False, True)), ((7,), (True,)), ((3, 12), (True, True))]:
        ndim = len(shape)
        t, w = pc.taps(ndim, dtype), pc.links(ndim, dtype)
        for v in (None, gc.potential(shape, dtype)):
            for wv in (None, w.reshape((5,) * ndim)):
                op = pkg.grid_box_operator(shape, t, v, ctx=ctx, periodic=flags, links=wv)
                n, nnz, dt = C.c_int64(), C.c_int64(), C.c_int()
                pkg._lib.check(pkg._lib.load().ks_operator_size(op._h, C.byref(n), C.byref(nnz), C.byref(dt)))
                assert (n.value, nnz.value, dt.value) == (gc.size(shape), pc.nnz(shape, flags), code)
                assert nnz.value == pkg.host_grid_box_matrix(shape, t, v, periodic=flags, links=wv).nnz
                assert op.format == dict(bytes_per_nnz=0.0, ndict=0, layout="none")
                info = op.grid_info
                assert info["shape"] == tuple(shape) and info["box"] is True and info["has_potential"] == (v is not None)
                assert info["periodic"] == tuple(flags) and np.array_equal(info["taps"], t)
                assert (info["links"] is None) if wv is None else (info["links"].shape == (5 ** ndim,) and np.array_equal(info["links"], w))
                assert info["bytes_per_row"] == np.dtype(dtype).itemsize * (3 if v is not None else 2)
    # a complex table promotes the element type; `periodic=None` keeps the open operator's info
    op = pkg.grid_box_operator((5,), np.array([-1.0, 2.0, -1.0]), ctx=ctx, periodic=True, links=np.array([-1j, 0, 0, 0, 1j]))
    assert op.dtype == np.complex128
    assert "periodic" not in pkg.grid_box_operator((5,), np.array([-1.0, 2.0, -1.0]), ctx=ctx).grid_info


def test_wrong_use_is_refused(ctx):
    t, w = pc.taps(3, np.float64), pc.links(3, np.float64)
    dctx = pkg.Context(0, rank=0, nranks=1, hostcomm=(lambda buf: None, lambda peers, sbufs, rbufs: None))
    with pytest.raises(pkg.ArgumentError, match="single-GPU"):
        pkg.grid_box_operator((4, 3, 3), t, ctx=dctx, periodic=True)
    with pytest.raises(pkg.DimensionMismatch, match="125 link values"):
        pkg.grid_box_operator((4, 3, 3), t, ctx=ctx, periodic=True, links=w[:25])
    with pytest.raises(pkg.DimensionMismatch, match="link values"):
        pkg.grid_box_operator((4, 3, 3), t, ctx=ctx, periodic=True, links=w.reshape(5, 25))
    bad = w.copy()
    bad[4] = np.inf          # (e_z, e_y, e_x) = (0, 0, 4): read on the full torus
    with pytest.raises(pkg.ArgumentError, match="link value 4 is not finite"):
        pkg.grid_box_operator((4, 3, 3), t, ctx=ctx, periodic=True, links=bad)
    assert pkg.grid_box_operator((4, 3, 3), t, ctx=ctx, periodic=(False, True, True), links=bad).shape == (36, 36)   # (x does not wrap: not read)
    with pytest.raises(pkg.ArgumentError, match=r"periodic axis 1 \(y\) has extent 2"):
        pkg.grid_box_operator((4, 2, 3), t, ctx=ctx, periodic=(True, True, False))
    with pytest.raises(pkg.ArgumentError, match="imaginary"):
        pkg.grid_box_operator((4, 3, 3), t, dtype=np.float64, ctx=ctx, periodic=True, links=pc.links(3, np.complex128))
    op = pkg.grid_box_operator((4, 3, 3), t, ctx=ctx, periodic=True, links=w)
    ws = pkg.ArnoldiWorkspace(36, 2, np.float64, ctx=ctx)
    with pytest.raises(pkg.ArgumentError):
        ws.apply(op, 1, 1)                                   # x and y of a product are distinct
