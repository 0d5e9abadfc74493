"""`-m "not gpu"`: the host decision of csrc/ks_defl_plan.hpp -- which leading locked columns a Newton chain is deflated against
(HipBackend::defl_plan calls it) -- in a stand-alone host program under the address and undefined-behaviour sanitizers
(tests/defl_plan_check.cpp), case by case against tests/sstep_model.py: defl_plan: the same column count, the same excluded
eigenvalues to 1e-12.  That is what makes "sm.defl_plan = HipBackend::defl_plan" (tests/test_sstep_model.py) a checked statement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT

import sstep_model as sm


def _host_compiler():
    for cand in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        cc = shutil.which(cand)
        if cc:
            return cc
    return None


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++, c++, clang++) found")
    exe = str(tmp_path_factory.mktemp("defl_plan") / "defl_plan_check")
    src = os.path.join(ROOT, "tests", "defl_plan_check.cpp")
    # (GCC links the sanitizer runtimes as shared libraries unless told otherwise, and a shared ASan runtime refuses to start behind
    # any other preloaded library; clang links them statically)
    gnu = "clang" not in subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    b = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                       + (["-static-libasan", "-static-libubsan"] if gnu else []) + [src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _num(x):
    return repr(float(x))


def _run(exe, cases):
    """cases: (H, j0, ritz, steps[, nmax, ratio]) -> [(nd, [excluded eigenvalues])] from the C++ function"""
    lines = []
    for c in cases:
        H, j0, ritz, steps = c[:4]
        nmax, ratio = (c[4:] + (16, 1.5)[len(c) - 4:])
        H = np.asarray(H)
        cplx = H.dtype.kind == "c"
        m = max(j0 - 1, 0)
        lines.append(f"{'c' if cplx else 'r'} {j0} {steps} {nmax} {_num(ratio)} {len(ritz)}")
        ent = H[:m, :m].flatten(order="F")
        lines.append(" ".join(f"{_num(z.real)} {_num(z.imag)}" for z in ent) if cplx else " ".join(_num(z) for z in ent))
        lines.append(" ".join(f"{_num(complex(z).real)} {_num(complex(z).imag)}" for z in ritz))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"DEFL_PLAN_CHECK_OK {len(cases)}" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = []
    for ln in r.stdout.splitlines()[: len(cases)]:
        f = ln.split()
        nd, ne = int(f[0]), int(f[1])
        out.append((nd, [complex(float(f[2 + 2 * i]), float(f[3 + 2 * i])) for i in range(ne)]))
    return out


def _same(exe, cases):
    got = _run(exe, cases)
    want = []
    for c, (nd, ex) in zip(cases, got):
        H, j0, ritz, steps = c[:4]
        nmax, ratio = (c[4:] + (16, 1.5)[len(c) - 4:])
        nd0, ex0 = sm.defl_plan(np.asarray(H), j0, np.asarray(ritz, dtype=np.complex128) if len(ritz) else None, ratio=ratio, nmax=nmax, steps=steps)
        want.append(nd0)
        assert nd == nd0 and len(ex) == len(ex0) == nd0, (nd, nd0, ex, ex0)
        for a, b in zip(ex, ex0):
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (ex, ex0)
    return want


def _fixed():
    """the matrix of test_sstep_model.py::test_deflation_plan_takes_the_leading_dominant_locked_columns"""
    rng = np.random.default_rng(0)
    m = 12
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    H[:4, :4] = np.triu(H[:4, :4])
    H[0, 0] = 50.0
    H[1:3, 1:3] = [[30.0, 10.0], [-10.0, 30.0]]
    H[3, 3] = 2.5
    H[4:, :4] = 0.0
    H[1, 0] = 0.0
    H[3, 2] = 0.0
    active = np.linalg.eigvals(H[4:m, 4:m])
    active = 1.2 * active / np.abs(active).max()
    return H, m, np.concatenate([[50.0, 30 + 10j, 30 - 10j, 2.5], active])


def test_the_fixed_matrix_of_the_model_test(plan_exe):
    H, m, ritz = _fixed()
    assert _same(plan_exe, [(H, m, ritz, 8), (H, m, ritz, 20), (H, m, ritz, 2)]) == [3, 4, 0]


def _random_case(rng, cplx):
    """a quasi-triangular locked prefix (1 x 1 and, in real arithmetic, 2 x 2 blocks; magnitudes from far above to below the
    rest), a general Hessenberg active part behind it, Ritz values = the locked ones, the rest, and now and then an infinite one"""
    m = int(rng.integers(6, 30))
    nl = int(rng.integers(1, min(m - 3, 20) + 1))
    H = np.triu(rng.standard_normal((m + 1, m)) + (1j * rng.standard_normal((m + 1, m)) if cplx else 0), -1)
    H[np.arange(1, m + 1), np.arange(m)] = np.abs(H[np.arange(1, m + 1), np.arange(m)]) + 0.1
    lam, j = [], 0
    while j < nl:
        mag = float(10.0 ** rng.uniform(-0.3, 1.8))
        if not cplx and j + 1 < nl and rng.integers(0, 3) == 0:
            th = rng.uniform(0.1, 1.2)
            a, b = mag * np.cos(th), mag * np.sin(th)
            g = float(rng.uniform(0.5, 2.0))                       # (a non-normalised 2 x 2 block: [[a, b g], [-b / g, a]])
            H[j:j + 2, j:j + 2] = [[a, b * g], [-b / g, a]]
            if j > 0:
                H[j, j - 1] = 0.0
            lam += [complex(a, b), complex(a, -b)]
            j += 2
        else:
            H[j, j] = mag * (np.exp(1j * rng.uniform(-3, 3)) if cplx else rng.choice([-1.0, 1.0]))
            if j > 0:
                H[j, j - 1] = 0.0
            lam.append(complex(H[j, j]))
            j += 1
    H[nl, nl - 1] = 0.0
    H[nl + 1:, :nl] = 0.0
    rest = (10.0 ** rng.uniform(-0.5, 0.5)) * np.exp(1j * rng.uniform(-3, 3, int(rng.integers(1, 8)))) * rng.uniform(0.2, 1.0)
    ritz = list(lam) + list(rest) + ([np.inf] if rng.integers(0, 5) == 0 else [])
    j0 = int(rng.integers(nl + 2, m + 1))
    return H, j0, ritz, int(rng.integers(1, 21))


@pytest.mark.parametrize("cplx", [False, True])
def test_random_quasi_triangular_prefixes(plan_exe, cplx):
    rng = np.random.default_rng(77 + cplx)
    cases = [_random_case(rng, cplx) for _ in range(200)]
    nds = _same(plan_exe, cases)
    assert sum(n > 0 for n in nds) >= 50 and sum(n == 0 for n in nds) >= 20 and max(nds) >= 4, nds     # (the sweep sees both answers)


def _dominant(n, m=24, pair_at=None):
    """n locked real eigenvalues 100, 99, ... (all far above a rest of radius 1); `pair_at` = j: a 2 x 2 block at columns j, j + 1"""
    H = np.triu(np.random.default_rng(3).standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = 0.5
    H[:n, :n] = np.triu(H[:n, :n])
    H[np.arange(n), np.arange(n)] = 100.0 - np.arange(n)
    if pair_at is not None:
        H[pair_at:pair_at + 2, pair_at:pair_at + 2] = [[80.0, 20.0], [-20.0, 80.0]]
    H[n:, :n] = 0.0
    lam = [complex(H[j, j]) for j in range(n)]
    if pair_at is not None:
        lam[pair_at:pair_at + 2] = [80 + 20j, 80 - 20j]
    return H, m, lam + [1.0, -0.5 + 0.5j, -0.5 - 0.5j]


def test_edges(plan_exe):
    H16 = _dominant(16)
    H17 = _dominant(17)
    Hp = _dominant(18, pair_at=15)                         # a 2 x 2 block at positions 15-16: taken whole or not at all -> 15
    Hfirst = _dominant(5)
    Hfirst[0][0, 0] = 1.2                                   # the FIRST locked column does not dominate: nothing, whatever follows
    Hfirst = (Hfirst[0], Hfirst[1], [1.2] + Hfirst[2][1:])
    Hlocked_only = (H16[0], H16[1], H16[2][:16] + [np.inf, np.nan])    # no finite Ritz value outside the locked set
    Hn = _dominant(4)
    Hn[0][np.arange(1, 5), np.arange(4)] = 0.3             # nothing locked
    got = _same(plan_exe, [H16 + (10,), H17 + (10,), Hp + (10,), Hfirst + (10,), Hlocked_only + (10,), Hn + (10,),
                           H17 + (10, 8), H16 + (10, 16, 200.0), _dominant(3) + (10,), (H16[0], 2, H16[2], 10), (H16[0], 1, H16[2], 10)])
    assert got == [16, 16, 15, 0, 0, 0, 8, 0, 3, 0, 0], got


def test_general_hessenberg_behind_an_accidental_zero_gives_no_plan(plan_exe):
    """A leading block that is NOT quasi-triangular: a general Hessenberg matrix (a caller's own H; an accidental zero in the active
    part) in front of the last zero sub-diagonal entry, with Ritz values that are not that block's (the library's from its last
    restart).  Its 1 x 1 / 2 x 2 diagonal blocks are not its eigenvalues; before the quasi-triangular rule the plan read them
    anyway -- on this matrix it took all 6 columns at steps = 10, with the "eigenvalues" 65.1, 54.9, 63.2, 56.8, 60 +- 1.4i of three
    2 x 2 blocks that do not exist (the block's own: 66.5, 55.4 +- 0.7i, 61.3 +- 3.3i, 60.1) -- and drove the Ritz classification, the shift exclusion and the growth test with them.  Now: 0 columns, from both
    implementations; one zero more among the sub-diagonal entries does not change that while two consecutive non-zero ones remain,
    and a proper quasi-triangular block of the same size is still taken."""
    m = 14
    rng = np.random.default_rng(5)
    H = np.triu(rng.standard_normal((m + 1, m)), -1)
    H[np.arange(1, m + 1), np.arange(m)] = 0.5
    H[:6, :6] = np.triu(rng.standard_normal((6, 6)), -1) * 3.0
    H[np.arange(6), np.arange(6)] = 60.0
    H[np.arange(1, 6), np.arange(5)] = [5.0, 4.0, 3.0, 2.0, 1.0]      # a general Hessenberg 6 x 6 block ...
    H[6, 5] = 0.0                                                       # ... behind an accidental zero
    H[7:, :6] = 0.0
    ritz = [1.0, 0.3 + 0.4j, 0.3 - 0.4j]
    Hq = H.copy()
    Hq[[2, 4], [1, 3]] = 0.0                                            # 2 x 2 blocks at 0-1, 2-3, 4-5: quasi-triangular
    ritz_q = list(np.concatenate([np.linalg.eigvals(Hq[j:j + 2, j:j + 2]) for j in (0, 2, 4)])) + [1.0, 0.3 + 0.4j, 0.3 - 0.4j]
    Hh = H.copy()
    Hh[2, 1] = 0.0                                                      # still two consecutive non-zero entries further down
    got = _same(plan_exe, [(H, m, ritz, 10), (Hq, m, ritz_q, 10), (Hh, m, ritz, 10)])
    assert got == [0, 6, 0], got
