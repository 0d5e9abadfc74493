"""`-m gpu`: the kernel forms that only large problems select, run at small sizes.

Several hot kernels change form with the problem size -- deep write-back staging of k_axpy_dots_cs from 24 MiB columns on, the
wrap of its staging ring once a workgroup sees more tiles than it stages, non-temporal loads of the basis above 352 MB, the
8-pack k_axpy above 3072 packs per workgroup, second and later trips of the per-lane loops of the fixed-grid kernels -- and the
headline benchmark runs exactly those forms.  KS_GRID_CAP (upper bound on the workgroups of every row-streaming launch),
KS_FUSED_WB and KS_V_NT, all read when a workspace is created, select them at 16 461 rows.  A "form" below is such an
environment, set before the workspace is made.

The data (tests/headline_forms_cases.py) is chosen so that every projection is EXACT in Float64 in any summation order:
H columns, projected vectors and rotated columns are compared bit for bit (tests/test_headline_forms_cases_cpu.py guards the
reference).  Only norms are rounded: rel 1e-13, the bound of test_gemv_t_and_gemv_n for a re-ordered sum."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import headline_forms_cases as hc
from __graft_entry__ import import_package
from oracle import arnoldi as oa
from oracle.matrices import laplace3d

pytestmark = pytest.mark.gpu
pkg = import_package()
EPS = hc.EPS
KNOBS = ("KS_GRID_CAP", "KS_FUSED_WB", "KS_FUSED_WB_MIN_MB", "KS_V_NT", "KS_V_NT_MB", "KS_BPC", "KS_ROTATE", "KS_ROTATE_VALU",
         "KS_PASSES", "KS_SSTEP")


def _form(cap=None, wb=None, nt=None):
    env = {}
    if cap is not None:
        env["KS_GRID_CAP"] = str(cap)
    if wb is not None:
        env["KS_FUSED_WB"] = str(wb)
    if nt is not None:
        env["KS_V_NT"] = str(nt)
    return pytest.param(env, id="-".join(f"{k[3:].lower()}{v}" for k, v in env.items()) or "default")


CAPPED = [(cap, wb, nt) for cap in (1, 3) for wb in (8, 24) for nt in (0, 1)]
FORMS = [_form()] + [_form(*f) for f in CAPPED]
FORMS_CAP3 = [_form(*f) for f in CAPPED if f[0] == 3]
FORMS_CAP_NT = [_form(cap, None, nt) for cap in (1, 3) for nt in (0, 1)]


def _enter(monkeypatch, env, **more):
    """The form's environment (and nothing else of the knobs), with the guard bands around the basis switched on."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {**env, **more, "KS_GUARD": "1"}.items():
        monkeypatch.setenv(k, str(v))


def _cap(env):
    return int(env.get("KS_GRID_CAP", 0))


def _parts(a):
    """Real view of an array: real and imaginary parts are compared one by one."""
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


def _check_step(ws, shape, j, dtype, which, V):
    """orthogonalize(j) on the exact data: what the issue of this module pins, in its order."""
    st = hc.step(shape, j, dtype, which)
    ws.set_col(j, st.w)
    ok = ws.orthogonalize(j)
    H = np.array(ws.H)
    tag = (j, which)
    assert ok, tag
    assert np.array_equal(H[:j, j - 1], st.hcol), (tag, np.abs(H[:j, j - 1] - st.hcol).max())
    beta = H[j, j - 1]
    assert np.imag(beta) == 0 and abs(np.real(beta) - st.beta) <= 1e-13 * st.beta, (tag, beta, st.beta)
    # reciprocal, scaling and this product: three roundings, every row pinned (atol = 0)
    np.testing.assert_allclose(_parts(ws.col(j) * np.real(beta)), _parts(st.vec), rtol=4 * EPS, atol=0, err_msg=str(tag))
    assert np.array_equal(ws.cols(0, j), V[:, :j]), tag
    assert ws.guard_intact(), tag
    if j < V.shape[1]:
        ws.set_col(j, V[:, j])       # column j belongs to the basis of the wider steps


def test_shapes_meet_the_coverage_condition():
    """For each (U, WB) of k_axpy_dots_cs and each type some case below gives one workgroup more than WB tiles of 64 U packs, a
    tile count that is no multiple of WB, and a partial last tile -- computed from n, the cap and U, so that a change of shapes
    cannot lose it silently.  (ComplexF64 at U = 2: 16 512 packs are exactly 129 tiles, the large shape has the partial one.)"""
    cases = [(hc.nrows(hc.SMALL), _cap(f.values[0])) for f in FORMS] + [(hc.nrows(hc.LARGE), 3)]
    for dtype in hc.DTYPES:
        for U, WB in hc.FUSED_UWB:
            assert any(cap and hc.ring_wrap_covered(n, dtype, cap, U, WB) for n, cap in cases), (dtype, U, WB)
        # cap 1: k_axpy<D, 8> with its 8-pack main loop and its one-pack remainder loop
        ppb = hc.axpy_packs_per_workgroup(hc.nrows(hc.SMALL), dtype, 1)
        assert ppb >= 3072 and ppb % (8 * hc.KBLOCK) != 0
        for kind, (trips, partial) in hc.rot_trips(hc.ROT_ROWS[np.dtype(dtype)], dtype).items():
            assert trips >= 3 and partial, (dtype, kind)
    assert min(hc.J_FUSED_LARGE) <= 40 < max(hc.J_FUSED_LARGE)     # both U = 4 and U = 2 run on the large shape


# ------------------------------------------------------------------------------------------------ A: one fused step
@pytest.mark.parametrize("which", hc.VECTORS)
@pytest.mark.parametrize("env", FORMS)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_fused_step_is_exact(dtype, env, which, monkeypatch):
    """k_dots -> k_fin_dots_def -> k_axpy_dots_cs -> k_fin_mid_def -> k_axpy (maxdim 64) at every column count that matters."""
    _enter(monkeypatch, env)
    if _cap(env) == 1:
        assert hc.axpy_packs_per_workgroup(hc.nrows(hc.SMALL), dtype, 1) >= 3072     # vector (b) takes k_axpy<D, 8>
    V = hc.basis(hc.SMALL, hc.MAXDIM_FUSED, dtype)
    ws = pkg.ArnoldiWorkspace(hc.nrows(hc.SMALL), hc.MAXDIM_FUSED, dtype)
    ws.set_cols(0, V)
    for j in hc.J_FUSED:
        _check_step(ws, hc.SMALL, j, dtype, which, V)


@pytest.mark.parametrize("which", hc.VECTORS)
@pytest.mark.parametrize("env", FORMS_CAP3)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_fused_step_is_exact_three_workgroups_wrap_the_ring(dtype, env, which, monkeypatch):
    """66 049 rows over three workgroups: 44 / 87 tiles per workgroup in Float64, 87 / 173 in ComplexF64 (U = 4 / 2)."""
    _enter(monkeypatch, env)
    V = hc.basis(hc.LARGE, hc.MAXDIM_FUSED, dtype)
    ws = pkg.ArnoldiWorkspace(hc.nrows(hc.LARGE), hc.MAXDIM_FUSED, dtype)
    ws.set_cols(0, V)
    for j in hc.J_FUSED_LARGE:
        _check_step(ws, hc.LARGE, j, dtype, which, V)


# ------------------------------------------------------------------------------------------------ B: the eager sequence
@pytest.mark.parametrize("which", hc.VECTORS)
@pytest.mark.parametrize("env", FORMS_CAP_NT)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_eager_step_is_exact(dtype, env, which, monkeypatch):
    """maxdim > 64: k_dots in 40-column chunks, k_axpy across its 128-column chunk, k_scale."""
    _enter(monkeypatch, env)
    V = hc.basis(hc.SMALL, hc.MAXDIM_EAGER, dtype)
    ws = pkg.ArnoldiWorkspace(hc.nrows(hc.SMALL), hc.MAXDIM_EAGER, dtype)
    ws.set_cols(0, V)
    for j in hc.J_EAGER:
        _check_step(ws, hc.SMALL, j, dtype, which, V)


# ------------------------------------------------------------------------------------------------ C: the two verbs
@pytest.mark.parametrize("env", FORMS_CAP_NT)
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_gemv_verbs_are_exact(dtype, env, monkeypatch):
    _enter(monkeypatch, env)
    V = hc.basis(hc.SMALL, hc.MAXDIM_EAGER, dtype)
    jv = hc.MAXDIM_EAGER
    ws = pkg.ArnoldiWorkspace(hc.nrows(hc.SMALL), hc.MAXDIM_EAGER, dtype)
    ws.set_cols(0, V)
    for j in hc.J_GEMV:
        w, g, h, wg = hc.gemv_case(j, dtype)
        ws.set_col(jv, w)
        assert np.array_equal(ws.gemv_t(j, jv), h), j
        ws.gemv_n_sub(j, jv, g)
        assert np.array_equal(ws.col(jv), wg), j
        assert np.array_equal(ws.cols(0, jv), V), j
        assert ws.guard_intact(), j


# ------------------------------------------------------------------------------------------------ D: rotations
ROT_MODES = [pytest.param(np.float64, {"KS_ROTATE": "fma", "KS_V_NT": "0"}, id="f64-fma-nt0"),
             pytest.param(np.float64, {"KS_ROTATE": "fma", "KS_V_NT": "1"}, id="f64-fma-nt1"),
             pytest.param(np.float64, {"KS_ROTATE": "mfma"}, id="f64-mfma"),
             pytest.param(np.float64, {"KS_ROTATE_VALU": "1"}, id="f64-valu"),
             pytest.param(np.complex128, {}, id="c64-default")]


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("dtype,mode", ROT_MODES)
def test_rotations_are_exact_on_small_integers(dtype, mode, cap, monkeypatch):
    """V[:, c0 : c0 + r) <- V[:, c0 : c0 + c) Q on integers |.| <= 7: every kernel (vector-ALU, matrix-instruction, generic, the
    out-of-place product above 64 columns) must equal the int64 product bit for bit, at every width at which the dispatch in
    rotate_device changes, with several trips of the row loop per lane and a partial last one; nothing else may change."""
    _enter(monkeypatch, {"KS_GRID_CAP": cap}, **mode)
    n = hc.ROT_ROWS[np.dtype(dtype)]
    rng = np.random.default_rng(77)
    V = hc.small_ints(rng, dtype, n, hc.ROT_MAXDIM + 1)
    ws = pkg.ArnoldiWorkspace(n, hc.ROT_MAXDIM, dtype)
    ws.set_cols(0, V)
    for c, c0 in itertools.product(hc.ROT_C, hc.ROT_C0):
        for r in hc.rot_widths(c):
            Q = hc.small_ints(rng, dtype, c, r)
            want = V.copy(order="F")
            want[:, c0 : c0 + r] = hc.int_product(V[:, c0 : c0 + c], Q)
            ws.rotate(c0, Q)
            got = ws.V
            bad = np.flatnonzero((got != want).any(axis=0))
            assert bad.size == 0, (c, r, c0, bad[:8])
            ws.set_cols(c0, V[:, c0 : c0 + r])
    assert ws.guard_intact()


# ------------------------------------------------------------------------------------------------ E: many steps
E_SHAPE = (9, 31, 59)      # 16 461 rows


def _operator(dtype):
    """The operator of test_gpu_fused_variants.py at 16 461 rows."""
    A = laplace3d(*E_SHAPE)
    n = A.shape[0]
    if hc.is_complex(dtype):
        A = (A + 1j * sp.diags(0.25 * np.cos(np.arange(n))) + 0.1j * sp.diags(np.ones(n - 1), 1)).tocsr()
    return A.astype(dtype), n


def _start(dtype, n, seed=oa.DEFAULT_SEED):
    v = oa.uniform_hash(seed, np.arange(n))
    if hc.is_complex(dtype):
        v = v + 1j * oa.uniform_hash(seed + 1, np.arange(n))
    return v.astype(dtype)


_ORACLE = {}


def _oracle(dtype):
    """64 steps of the oracle, once per type (the first m steps of it are the m-step expansion)."""
    key = np.dtype(dtype)
    if key not in _ORACLE:
        A, n = _operator(dtype)
        v1 = _start(dtype, n)
        ows = oa.ArnoldiWorkspace.from_vector(v1, 64)
        oa.reinitialize(ows, 0, lambda v: v.__setitem__(slice(None), v1))
        oa.iterate_arnoldi(A, ows, 1, 64, {})
        _ORACLE[key] = (A, v1, np.array(ows.H), np.array(ows.V))
    return _ORACLE[key]


@pytest.mark.parametrize("sstep", ["0", "20"])
@pytest.mark.parametrize("passes", ["2", "3"])
@pytest.mark.parametrize("m", [24, 40, 64])
@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_expansion_under_the_large_problem_forms(dtype, m, passes, sstep, monkeypatch):
    """iterate_arnoldi 1..m.  Within one grid cap H and the basis are bit-identical across staging depth and load policy (they move
    data only; the cap fixes the partial sums); every form agrees with the oracle to the tolerances of
    test_expansion_matches_oracle_H and keeps the relation / orthogonality bounds of test_full_size_properties_1e6."""
    A, v1, Ho, Vo = _oracle(dtype)
    n = A.shape[0]
    out = {}
    for f in FORMS:
        env = f.values[0]
        _enter(monkeypatch, env, KS_PASSES=passes, KS_SSTEP=sstep)
        op = pkg.csr_operator(A)
        ws = pkg.ArnoldiWorkspace(n, m, dtype, ctx=op.ctx)
        ws.reinitialize(0, v1)
        st = ws.iterate_arnoldi(op, 1, m)
        assert st["steps"] == m and st["breakdowns"] == 0, f.id
        H = np.array(ws.H)
        res, orth = ws.arnoldi_relation(op, m)
        V = ws.V
        print(f"{f.id}: |H - oracle| {np.abs(H - Ho[: m + 1, :m]).max():.2e}  |V - oracle| {np.abs(V - Vo[:, : m + 1]).max():.2e}  "
              f"relation {res / np.linalg.norm(H):.2e}  orthogonality {orth:.2e}")
        np.testing.assert_allclose(H, Ho[: m + 1, :m], atol=1e-11, err_msg=f.id)
        np.testing.assert_allclose(V, Vo[:, : m + 1], atol=1e-9, err_msg=f.id)
        assert res <= 1e-12 * np.linalg.norm(H) and orth <= np.sqrt(EPS) / 100, (f.id, res, orth)
        # one restart and the expansion on top of it: only now are there Ritz values, so only this one can run in blocks
        # (compared across forms and through the same two bounds; the oracle comparison above is the issue's)
        r = ws.restart(0, 6, "LM" if hc.is_complex(dtype) else "SR", 1e-10, m // 2, m)
        ws.iterate_arnoldi(op, r["k"] + 1, m)
        H2 = np.array(ws.H)
        res2, orth2 = ws.arnoldi_relation(op, m)
        V2 = ws.V
        blocks = ws.sstep_info["blocks"]
        print(f"{f.id}: after a restart to {r['k']} columns: blocks {blocks}  relation {res2 / np.linalg.norm(H2):.2e}  orthogonality {orth2:.2e}")
        assert (blocks > 0) == (passes == "2" and sstep != "0"), (f.id, blocks)     # the block kernels did run where they can
        assert res2 <= 1e-12 * np.linalg.norm(H2) and orth2 <= np.sqrt(EPS) / 100, (f.id, res2, orth2)
        assert ws.guard_intact(), f.id
        out.setdefault(_cap(env), []).append((f.id, H, V, H2, V2, blocks))
    for cap in (1, 3):
        first, rest = out[cap][0], out[cap][1:]
        assert len(rest) == 3
        for other in rest:
            assert all(np.array_equal(a, b) for a, b in zip(first[1:], other[1:])), (first[0], other[0])
