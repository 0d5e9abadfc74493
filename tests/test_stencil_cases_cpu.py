"""`-m "not gpu"`: the stencil families of tests/stencil_cases.py plan to the stencil-mask layout with the slot order -- and so
the marching kernel -- each of them is meant to reach (ks_host_csr_plan, no device), and the references of
tests/spmv_reference.py are what they claim to be: seq_matvec against scipy and against the naive loop, hp_shifted against
exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import layout_cases as lc
import spmv_reference as ref
import stencil_cases as sc
from test_csr_layout_cpu import plan

EPS = ref.EPS


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in lc.LAYOUT_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("fam", sc.FAMILIES + [sc.BIG], ids=lambda f: f.name)
def test_every_case_plans_as_the_intended_stencil(fam):
    """Every size, without and with knock-outs: KS_LAYOUT_STENCIL, one slot per tap in ascending offset, 1-byte masks; the
    kernel launch_march picks for that slot order is the one the family is named for, and the sizes straddle its bound."""
    cases = [(sc.BIG_N, True)] if fam is sc.BIG else fam.cases()
    for n, knock in cases:
        A, _x, removed = sc.build(fam.name, n, knock)
        f = plan(A, np.float64)
        assert f["layout"] == "stencil" and f["nstencil"] == len(fam.deltas) and f["ndict"] == len(fam.deltas), (n, knock, f)
        assert f["stencil_delta"] == fam.deltas and f["stencil_mask_bytes"] == 1, (n, knock, f)
        assert sc.expected_kernel(f["stencil_delta"], n) == fam.kernel, (n, knock)
        for form, env in fam.forms.items():
            assert sc.expected_kernel(f["stencil_delta"], n, env) not in (fam.kernel, "stencil2"), form
        if knock:
            # about a tenth of the entries is gone, and rows of the interior tiles are among those that lost one
            total = A.nnz + removed[0].size
            assert 0.08 * total < removed[0].size < 0.12 * total
            t = removed[0] // sc.TILE
            assert np.any((t >= 2) & (t < sc.KTILES - 1))
        else:
            assert removed[0].size == 0
    if fam is not sc.BIG:
        # tile 26 is interior at all three sizes around the bound, tile 27 only from the middle one on
        base = fam.sizes()[1]
        interior = lambda t, n: sc.TILE * t + fam.bound <= n  # noqa: E731
        assert [interior(sc.KTILES - 1, n) for n in (base - 1, base, base + 1)] == [False, True, True]
        assert not interior(sc.KTILES, base + 1) and fam.sizes()[3] % 2 == 1
        if fam.name == "eight-wide":
            assert (-fam.dmin + sc.TILE - 1) // sc.TILE == 2      # two clamped tiles at the low end, two at the high end
            assert not interior(sc.KTILES, base + 1) and sc.TILE * (sc.KTILES + 1) < base + 1


def test_the_families_reach_every_instantiation_of_the_register_form():
    got = {f.kernel for f in sc.FAMILIES} | {sc.expected_kernel(f.deltas, f.sizes()[0], env) for f in sc.FAMILIES for env in f.forms.values()}
    want = {"march<%d,-1>" % k for k in range(1, 9)} | {"march<3,1>", "march<5,2>", "march<7,3>", "window<0x14>", "window<0x36>", "window<0x3e>"}
    assert got == want
    assert sc.BIG.kernel == "marchz<0x14>"


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_seq_matvec_is_the_stored_order_sum(dtype):
    """Against scipy to L eps |A||x| componentwise (ragged rows, empty rows, rows of thousands of entries); bit for bit against
    the naive loop on a small matrix and on the first rows of a stencil."""
    A, x = lc.skewed_case(dtype)
    y = ref.seq_matvec(A, x)
    w, L = ref.abs_matvec(A, x)
    fac = 4 if np.dtype(dtype).kind == "c" else 1
    assert np.all(np.abs(y - A @ x) <= fac * L * EPS * w.astype(np.float64))
    assert np.all(y[L == 0] == 0) and not np.any(np.signbit(y[L == 0].real))
    S, xs, _rng = lc.stencil19(dtype)
    assert np.array_equal(ref.seq_matvec(S, xs).view(np.uint64), ref.seq_matvec_loop(S, xs).view(np.uint64))
    _A7, _x7, R, xr = lc.varcoef_and_ragged(dtype)
    ys, yl = ref.seq_matvec(R, xr), ref.seq_matvec_loop(R, xr)   # (Inf in xr, -0.0 among the values, empty rows)
    assert np.array_equal(np.isfinite(ys), np.isfinite(yl))
    fin = np.isfinite(ys)
    assert np.array_equal(ys[fin].view(np.uint64), yl[fin].view(np.uint64))


def _exact_row(A, x, i, theta, sigma):
    """Row i of sigma (A x - theta x) in rational arithmetic: (real part, imaginary part)."""
    def fr(z):
        z = complex(z)
        return Fraction(z.real), Fraction(z.imag)

    sr, si = Fraction(0), Fraction(0)
    for p in range(A.indptr[i], A.indptr[i + 1]):
        (ar, ai), (br, bi) = fr(A.data[p]), fr(x[A.indices[p]])
        sr, si = sr + ar * br - ai * bi, si + ar * bi + ai * br
    (tr, ti), (xr, xi) = fr(theta), fr(x[i])
    sr, si = sr - (tr * xr - ti * xi), si - (tr * xi + ti * xr)
    return Fraction(float(sigma)) * sr, Fraction(float(sigma)) * si


@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_hp_shifted_agrees_with_rational_arithmetic(dtype):
    """200 sampled rows of a knocked-out 7-point case and of the skewed matrix: the extended-precision value is within
    (L + 3) 2^-63 w of the exact one -- 2^-11 of the bound the Float64 kernels are held to."""
    cplx = np.dtype(dtype).kind == "c"
    theta, sigma = (1234.56789 - 77.25j if cplx else 1234.56789), 0.3
    fam = sc.BY_NAME["grid3d-20x15"]
    A, x, _ = sc.build(fam.name, fam.sizes()[2], True, np.dtype(dtype).name)
    B, xb = lc.skewed_case(dtype)
    for M, xv in ((A, x), (B, xb)):
        y, w, L = ref.hp_shifted(M, xv, theta, sigma)
        assert y.dtype == (np.clongdouble if cplx else np.longdouble) and np.array_equal(L, np.diff(M.indptr))
        rows = np.random.default_rng(3).choice(M.shape[0], 200, replace=False)
        rows[:3] = np.argsort(-L)[:3]      # the longest rows among them
        for i in rows:
            er, ei = _exact_row(M, xv, int(i), theta, sigma)
            # (the difference to the exact value, formed in extended precision from the leading and trailing parts of the fraction)
            dr = _ld_diff(np.real(y[i]), er)
            di = _ld_diff(np.imag(y[i]), ei) if cplx else np.longdouble(0)
            err = np.sqrt(dr * dr + di * di)
            assert err <= (4 if cplx else 1) * (L[i] + 3) * np.longdouble(2.0) ** -63 * w[i], (int(i), float(err), float(w[i]))
        # the scale itself: |sigma| (sum |a||x| + |theta||x_i|) to a few units of Float64
        i = int(rows[0])
        wi = abs(sigma) * (sum(abs(complex(M.data[p])) * abs(complex(xv[M.indices[p]])) for p in range(M.indptr[i], M.indptr[i + 1])) + abs(theta) * abs(complex(xv[i])))
        assert abs(float(w[i]) - wi) <= 1e-13 * wi


def _ld_diff(v, exact):
    """v - exact for a longdouble v and a Fraction: v is split into two doubles, which are exact rationals."""
    hi = float(v)
    lo = float(v - np.longdouble(hi))
    assert np.longdouble(hi) + np.longdouble(lo) == v
    return np.longdouble(float(Fraction(hi) + Fraction(lo) - exact))
