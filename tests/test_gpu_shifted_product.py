"""`-m gpu`: the Newton step y = sigma (A x - theta x) of the s-step expansion (the shifted form of mul!(y, A, x),
src/expansion.jl:121), product by product through ks_debug_apply_shifted, and every path of the marching stencil kernels
(csrc/ks_spmv_march.hpp) at the smallest sizes where each can go wrong.

References (tests/spmv_reference.py, plain numpy): seq_matvec gives the BITS of a plain product (each product rounded on its own,
added to +0.0 in stored order); hp_shifted the shifted product in extended precision with the scale w and the row lengths L of
its forward-error bound |y - hp| <= (L + 3) eps w (x 4 in modulus for complex) -- the bound of the operation sequence itself,
contracted or not, so no tolerance here is a measured number.  The destination column is poisoned with NaN before every product:
a tile that is never stored cannot hide behind the previous, identical result."""
import numpy as np
import pytest

import layout_cases as lc
import spmv_reference as ref
import stencil_cases as sc
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
EPS = ref.EPS
ENV = lc.LAYOUT_ENV + ("KS_MARCH_Z", "KS_MARCH_WINDOW", "KS_STENCIL_MARCH", "KS_MARCH_S", "KS_MARCH_ZR", "KS_SHIFT_FUSED", "KS_GUARD")
# (theta, sigma): a large shift -- theta x dwarfs A x, the subtraction cancels it --, and a scale that is no power of two
PAIRS = {"f": ((1234.56789, 2.0 ** -10), (-0.6180339887, 0.3)), "c": ((1234.56789 - 77.25j, 2.0 ** -10), (-0.6180339887 + 0.35j, 0.3))}
S_VALUES = (None, "1", "2", "3")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _first(bad):
    return int(np.flatnonzero(bad)[0]) if np.any(bad) else -1


class Product:
    """One operator on one workspace: column 0 = x, column 1 = the (poisoned) destination."""

    def __init__(self, op, x, ncols=2):
        self.op, self.x = op, np.asarray(x, dtype=op.dtype)
        self.ws = pkg.ArnoldiWorkspace(len(x), ncols, op.dtype, ctx=op.ctx)
        self.ws.set_col(0, self.x)
        self.poison = np.full(len(x), np.nan, dtype=op.dtype)

    def plain(self):
        self.ws.set_col(1, self.poison)
        self.ws.apply(self.op, 0, 1)
        return self.ws.col(1)

    def shifted(self, theta, sigma, cacheable):
        self.ws.set_col(1, self.poison)
        self.ws.apply_shifted(self.op, 0, 1, theta, sigma, cacheable)
        return self.ws.col(1)


def _assert_plain_bits(y, want, what, rows=None):
    """Where the reference is finite: the same bits; elsewhere: not finite either."""
    fin = np.isfinite(want)
    bad = np.isfinite(y) != fin
    assert not np.any(bad), (what, "finite / non-finite pattern, first row", _first(bad))
    sel = fin if rows is None else fin & rows
    bad = np.zeros(len(y), dtype=bool)
    bad[sel] = np.any(_bits(y[sel]).reshape(int(sel.sum()), -1) != _bits(want[sel]).reshape(int(sel.sum()), -1), axis=1)
    assert not np.any(bad), (what, "first wrong row", _first(bad), y[_first(bad)], want[_first(bad)])


def _assert_bound(y, hp, what, extra=0):
    """|y - hp| <= (L + 3 + extra) eps w componentwise (modulus and a factor 4 for complex), on the rows where hp is finite."""
    yh, w, L = hp
    fin = np.isfinite(yh)
    bad = np.isfinite(y) != fin
    assert not np.any(bad), (what, "finite / non-finite pattern, first row", _first(bad))
    fac = 4 if np.iscomplexobj(yh) else 1
    err = np.abs(y[fin].astype(yh.dtype) - yh[fin])
    bound = fac * (L[fin] + 3 + extra) * np.longdouble(EPS) * w[fin]
    print("%s: max |y - hp| / bound = %.3f" % (what, float(np.max(err / np.where(bound > 0, bound, 1), initial=0.0))))
    bad = np.zeros(len(y), dtype=bool)
    bad[fin] = err > bound
    i = _first(bad)
    assert i < 0, (what, "first row outside the bound", i, y[i], complex(yh[i]), float(w[i]), int(L[i]))


def _forms(fam):
    """form name -> environment; each with the KS_MARCH_S values that change what it runs."""
    out = [("default", {}, (None,) if fam.kernel.startswith("marchz") else S_VALUES)]
    out += [(name, env, S_VALUES) for name, env in fam.forms.items()]
    out.append(("stencil2", {"KS_STENCIL_MARCH": "0"}, (None,)))
    return out


def _check_stencil_case(fam, n, knock, monkeypatch, ctx, x_edit=None, s_values=None):
    A, x, removed = sc.build(fam.name, n, knock)
    if x_edit is not None:
        x = x_edit(x.copy(), removed)
    want = ref.seq_matvec(A, x)
    hps = [ref.hp_shifted(A, x, th, sg) for th, sg in PAIRS["f"]]
    tag = "%s n=%d%s" % (fam.name, n, " knocked" if knock else "")
    _setenv(monkeypatch, {"KS_SPMV_FORMAT": "csr"})
    rows = pkg.csr_operator(A, ctx)
    assert rows.format["layout"] == "csr"
    _assert_plain_bits(Product(rows, x).plain(), want, tag + " csr")
    _setenv(monkeypatch, {})
    op = pkg.csr_operator(A, rows.ctx)
    assert op.format["layout"] == "stencil" and op.format["ndict"] == len(fam.deltas), op.format
    P = Product(op, x)
    first = None
    for form, env, svals in _forms(fam):
        for S in (svals if s_values is None else [s for s in svals if s in s_values]):
            _setenv(monkeypatch, dict(env, KS_MARCH_S=S))
            what = "%s %s S=%s" % (tag, form, S)
            _assert_plain_bits(P.plain(), want, what)
            got = []
            for cacheable in (False, True):
                for (th, sg), hp in zip(PAIRS["f"], hps):
                    y = P.shifted(th, sg, cacheable)
                    _assert_bound(y, hp, "%s theta=%g cacheable=%d" % (what, th, cacheable))
                    got.append(y)
            if first is None:
                first = got
                # the two stores of one form carry the same values
                for k in range(len(PAIRS["f"])):
                    _assert_plain_bits(got[len(PAIRS["f"]) + k], np.where(np.isfinite(hps[k][0]), got[k], np.nan), what + " cacheable vs streaming store")
            for k, y in enumerate(got):
                _assert_plain_bits(y, np.where(np.isfinite(hps[k % 2][0]), first[k], np.nan), what + " shifted bits vs the first form, product %d" % k)
    return rows.ctx


@pytest.mark.parametrize("fam", sc.FAMILIES, ids=lambda f: f.name)
def test_marching_paths_plain_bits_and_newton_step(fam, monkeypatch):
    """(a) Every size and knock-out variant of one family, every form it can take (its marching kernel, the register form behind a
    window form, k_spmv_stencil2), KS_MARCH_S unset / 1 / 2 / 3: on 28-29 tiles a workgroup then walks 1, 2, 3 or 4 tiles, so both
    register sets, both loop exits and every wait count of the software pipeline run.  Plain y == seq_matvec bit for bit (and ==
    the CSR row blocks); the Newton step within its forward-error bound for both stores and both (theta, sigma); the shifted
    bits identical across all forms and S (the solver's bit-identical H across forms rests on that)."""
    ctx = None
    for n, knock in fam.cases():
        ctx = _check_stencil_case(fam, n, knock, monkeypatch, ctx)


def test_large_grid_z_marching_window_and_register_forms(monkeypatch):
    """(a) 182 x 182 x 9, non-symmetric coefficients, knock-outs: the z-marching form by default, the window and the register form
    behind it with 583 tiles on 8 x S workgroups (S = 1: 73 tiles per workgroup), k_spmv_stencil2."""
    _check_stencil_case(sc.BIG, sc.BIG_N, True, monkeypatch, None)


@pytest.mark.parametrize("name", ["grid3d-20x15", "eight-wide", "six-hollow", "line3"])
def test_absent_slots_of_interior_tiles_are_never_multiplied(name, monkeypatch):
    """(b) x holds Inf at one column and NaN at another which rows of INTERIOR tiles lack (knocked-out entries): the and-mask of the
    unclamped path must turn the product of an absent slot into +0.0.  The finite entries of y are exactly the reference's, and
    they obey the checks of (a)."""
    fam = sc.BY_NAME[name]
    n = fam.sizes()[2]

    def edit(x, removed):
        r, c = removed
        t = r // sc.TILE
        pick = np.flatnonzero((t >= 3) & (t < sc.KTILES - 3))
        assert pick.size >= 2
        i, j = pick[0], pick[pick.size // 2]
        assert c[i] != c[j]
        x[c[i]], x[c[j]] = np.inf, np.nan
        return x

    A, x0, removed = sc.build(fam.name, n, True)
    x = edit(x0.copy(), removed)
    want = ref.seq_matvec(A, x)
    lost = np.isin(np.arange(n), removed[0][~np.isfinite(x[removed[1]])])
    assert np.any(lost & np.isfinite(want)) and np.any(~np.isfinite(want))     # rows that lack the column stay finite, others do not
    _check_stencil_case(fam, n, True, monkeypatch, None, x_edit=edit, s_values=(None, "2"))


# ------------------------------------------------------------------------------------------------ (c) every other layout
def _check_layout(A, x, env, layout, monkeypatch, ctx, tag, tree_rows=None):
    """Plain bits against seq_matvec (rows in `tree_rows` -- rows cut into chunks, summed by a fixed tree instead of stored order --
    against the bound of any summation order), the Newton step against hp_shifted for both stores and both (theta, sigma)."""
    kind = "c" if np.iscomplexobj(A.data) else "f"
    _setenv(monkeypatch, env)
    op = pkg.csr_operator(A, ctx)
    assert op.format["layout"] == layout, (tag, op.format)
    P = Product(op, x)
    y = P.plain()
    what = "%s %s %s" % (tag, kind, env)
    _assert_plain_bits(y, ref.seq_matvec(A, x), what, rows=None if tree_rows is None else ~tree_rows)
    if tree_rows is not None:
        _assert_bound(y, ref.hp_shifted(A, x, 0.0, 1.0), what + " plain, chunked rows")
    for th, sg in PAIRS[kind]:
        hp = ref.hp_shifted(A, x, th, sg)
        for cacheable in (False, True):
            _assert_bound(P.shifted(th, sg, cacheable), hp, "%s theta=%s cacheable=%d" % (what, th, cacheable))
    return op.ctx


def _stencil7(dtype):
    fam = sc.BY_NAME["grid3d-21x15"]
    A, x, _ = sc.build(fam.name, fam.sizes()[2], True, np.dtype(dtype).name)
    return A, x


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_newton_step_on_csr_row_blocks_and_column_blocks(dtype, monkeypatch):
    """csr: fused (a scattered matrix with empty rows) and the unfused fallback of a matrix with rows cut into chunks (skewed_case:
    nlong > 0); csr-cb: one launch per block, and the single launch with 1 and 16 sub-tiles per workgroup."""
    A, x, _rng = lc.colblock_matrix(dtype)
    ctx = _check_layout(A, x, {"KS_SPMV_FORMAT": "csr", "KS_SPMV_COLBLOCKS": "0"}, "csr", monkeypatch, None, "colblock")
    _check_layout(A, x, {"KS_SPMV_FORMAT": "csr", "KS_SPMV_COLBLOCKS": "3"}, "csr-cb", monkeypatch, ctx, "colblock 3 launches")
    for rpt in ("1", "16"):
        _check_layout(A, x, {"KS_SPMV_FORMAT": "csr", "KS_SPMV_COLBLOCKS": "5", "KS_SPMV_CB_RPT": rpt}, "csr-cb", monkeypatch, ctx, "colblock single launch")
    B, xb = lc.skewed_case(dtype)
    long_rows = np.diff(B.indptr) > 4096       # (longer than any block: ni <= 16 sub-tiles of 256 entries)
    assert long_rows.sum() == 3
    _check_layout(B, xb, {"KS_SPMV_FORMAT": "csr"}, "csr", monkeypatch, ctx, "skewed", tree_rows=long_rows)
    _check_layout(A, x, {"KS_SPMV_FORMAT": "csr", "KS_SPMV_COLBLOCKS": "0", "KS_SHIFT_FUSED": "0"}, "csr", monkeypatch, ctx, "colblock unfused")


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_newton_step_on_dictionary_and_sliced_layouts(dtype, monkeypatch):
    """vi, dvi with 1 / 2 / 4 rows per thread, the complex / unfused stencil kernels on a knocked-out non-symmetric 7-point matrix;
    sell and sell-vi with sigma = 1 and 256 on the ragged matrix (rows permuted inside a window: the own entry x[row] must be the
    unpermuted row's; Inf in x next to padding); the 19-slot stencil with 32-bit masks."""
    A, x = _stencil7(dtype)
    ctx = _check_layout(A, x, {"KS_SPMV_FORMAT": "vi"}, "csr-vi", monkeypatch, None, "stencil7")
    for rpt in ("1", "2", "4"):
        _check_layout(A, x, {"KS_SPMV_FORMAT": "dvi", "KS_DVI_RPT": rpt}, "csr-dvi", monkeypatch, ctx, "stencil7")
    _check_layout(A, x, {}, "stencil", monkeypatch, ctx, "stencil7")
    _check_layout(A, x, {"KS_SHIFT_FUSED": "0"}, "stencil", monkeypatch, ctx, "stencil7 unfused")
    _A, _x, R, xr = lc.varcoef_and_ragged(dtype)
    for fmt, layout in (("sell", "sell"), ("sellvi", "sell-vi")):
        for sigma in ("1", "256"):
            _check_layout(R, xr, {"KS_SPMV_FORMAT": fmt, "KS_SELL_SIGMA": sigma}, layout, monkeypatch, ctx, "ragged")
    S, xs, _rng = lc.stencil19(dtype)
    _check_layout(S, xs, {}, "stencil", monkeypatch, ctx, "stencil19")


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_newton_step_of_operators_without_a_fused_form(dtype, monkeypatch):
    """A dense operator (n = 130) and the tridiagonal shift-invert operator (n = 100) take ks_operator::apply_shifted: the product,
    then one streaming pass.  No bit contract for their products: the step is held to the operator's OWN plain result,
    |y - (y_plain - theta x) sigma| <= 3 eps (|y_plain| + |theta| |x|) |sigma| (x 4 in modulus for complex)."""
    cplx = np.dtype(dtype).kind == "c"
    rng = np.random.default_rng(17)
    D = lc.rnd(rng, dtype, 130, 130)
    n = 100
    dl, du, d = lc.rnd(rng, dtype, n - 1), lc.rnd(rng, dtype, n - 1), lc.rnd(rng, dtype, n) + 4.0
    ctx = pkg.default_context()
    for op in (pkg.dense_operator(D, ctx), pkg.tridiagonal_solve_operator(dl, d, du, sigma=(0.25 + 0.5j if cplx else 0.25), ctx=ctx)):
        m = op.shape[0]
        x = lc.rnd(rng, dtype, m)
        P = Product(op, x)
        hp = np.clongdouble if cplx else np.longdouble
        y0 = P.plain()
        assert np.all(np.isfinite(y0))
        for th, sg in PAIRS["c" if cplx else "f"]:
            want = (y0.astype(hp) - hp(th) * x.astype(hp)) * np.longdouble(sg)
            bound = (4 if cplx else 1) * 3 * np.longdouble(EPS) * (np.abs(y0.astype(hp)) + abs(th) * np.abs(x.astype(hp))) * abs(sg)
            for cacheable in (False, True):
                y = P.shifted(th, sg, cacheable)
                bad = ~(np.abs(y.astype(hp) - want) <= bound)
                assert not np.any(bad), (m, th, cacheable, "first row outside the bound", _first(bad))


# ------------------------------------------------------------------------------------------------ (d) hygiene
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_shifted_product_writes_its_destination_only(dtype, monkeypatch):
    """Only column jdst changes (the others bit for bit, the first and the last column of the basis as destinations included), the
    canary zones of KS_GUARD=1 around the basis stay intact, and the library no longer vouches for the factorisation.  Fused
    stencil kernels (n odd: the last pair is half a pair), the unfused pass over ld elements, a dense operator."""
    monkeypatch.setenv("KS_GUARD", "1")
    cplx = np.dtype(dtype).kind == "c"
    th, sg = PAIRS["c" if cplx else "f"][1]
    fam = sc.BY_NAME["grid3d-20x15"]
    A, x = sc.build(fam.name, sc.ODD_N, True, np.dtype(dtype).name)[:2]
    rng = np.random.default_rng(23)
    ops = [("fused", {}, pkg.csr_operator(A), x)]
    ops.append(("unfused", {"KS_SHIFT_FUSED": "0"}, ops[0][2], x))
    ops.append(("dense", {}, pkg.dense_operator(lc.rnd(rng, dtype, 131, 131), ops[0][2].ctx), lc.rnd(rng, dtype, 131)))
    for name, env, op, xv in ops:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = len(xv)
        ws = pkg.ArnoldiWorkspace(m, 3, dtype, ctx=op.ctx)
        V = np.asfortranarray(lc.rnd(rng, dtype, m, 4))
        V[:, 1] = xv
        for src, dst in ((1, 2), (1, 0), (1, 3)):
            ws.set_cols(0, V)
            ws.apply_shifted(op, src, dst, th, sg, cacheable=(dst == 3))
            got = ws.cols(0, 4)
            for j in range(4):
                if j != dst:
                    assert np.array_equal(_bits(got[:, j]), _bits(V[:, j])), (name, src, dst, j)
            assert not np.array_equal(got[:, dst], V[:, dst]) and np.all(np.isfinite(got[:, dst])), (name, dst)
            assert ws.provenance == -1
        assert ws.guard_intact(), name
        for k in env:
            monkeypatch.delenv(k)
    # a real workspace refuses a complex shift, and the two columns must differ
    if not cplx:
        with pytest.raises(pkg.ArgumentError):
            ws.apply_shifted(op, 1, 2, 1.0 + 2.0j, 1.0)
    with pytest.raises(pkg.ArgumentError):
        ws.apply_shifted(op, 1, 1, 1.0, 1.0)
