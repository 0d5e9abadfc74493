"""`-m gpu`: the z-marching stencil product that derives its masks from the grid (k_spmv_stencil_marchg, csrc/ks_spmv_march.hpp;
the host decision: csrc/ks_stencil_geom.hpp), at the smallest grids that select it: planes of >= 64 tiles of 512 rows, >= 8 planes.

  182 x 182 x 9   nx even: the near taps +-nx are aligned 16-byte window reads
  181 x 182 x 8   nx odd (a lane's pair straddles two grid lines), P = 32 942 even, the minimum of 8 planes, two z-ranges
  182 x 182 x 9   with one entry knocked out: not a box any more, the product must fall back to the form that reads the masks

Non-symmetric coefficients (the values of tests/stencil_cases.py).  Every product is required bit for bit: the forms add the same
separately rounded products in the same slot order, so there is no tolerance anywhere in this file.  The destination is filled
with NaN before every product: a row that is never stored cannot hide behind an earlier, identical result.  The store policy of
the shifted product (KS_SHIFT_PLAIN, which the library reads once per process) is set per product through the `cacheable`
argument of the debug entry point, which is what the variable forces."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import stencil_cases as sc
from __graft_entry__ import import_package

pytestmark = pytest.mark.gpu
pkg = import_package()
ENV = ("KS_SPMV_FORMAT", "KS_MARCH_GEOM", "KS_MARCH_Z", "KS_MARCH_WINDOW", "KS_STENCIL_MARCH", "KS_MARCH_S", "KS_MARCH_ZR", "KS_SHIFT_FUSED",
       "KS_SHIFT_PLAIN", "KS_SSTEP")
FORMS = (("default", {}), ("masks", {"KS_MARCH_GEOM": "0"}), ("window", {"KS_MARCH_Z": "0"}), ("stencil2", {"KS_STENCIL_MARCH": "0"}))
SHIFTS = ((1234.56789, 2.0 ** -10), (-0.6180339887, 0.3))
GRIDS = {"182x182x9": ((182, 182, 9), None), "181x182x8": ((181, 182, 8), None), "182x182x9-knocked": ((182, 182, 9), (91, 90, 4, 4))}


def _setenv(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _matrix(name):
    """The 7-point box stencil on the grid with seven different values, optionally without the entry of slot `k` in row (x, y, z)."""
    (nx, ny, nz), knock = GRIDS[name]
    n, P = nx * ny * nz, nx * ny
    vals = sc._values(40 + len(name), 7, np.float64)
    r = np.arange(n, dtype=np.int64)
    ix, iy, iz = r % nx, (r // nx) % ny, r // P
    taps = ((-P, iz > 0), (-nx, iy > 0), (-1, ix > 0), (0, ix >= 0), (1, ix < nx - 1), (nx, iy < ny - 1), (P, iz < nz - 1))
    rows, cols, data = [], [], []
    for k, (d, ok) in enumerate(taps):
        if knock is not None and knock[3] == k:
            ok = ok & (r != knock[0] + nx * (knock[1] + ny * knock[2]))
        rows.append(r[ok]); cols.append(r[ok] + d); data.append(np.full(int(ok.sum()), vals[k]))
    A = sp.csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    x = np.random.default_rng(len(name)).standard_normal(n)
    return A, x


class Product:
    """One operator on one workspace: column 0 = x, column 1 = the (poisoned) destination."""

    def __init__(self, op, x):
        self.op = op
        self.ws = pkg.ArnoldiWorkspace(len(x), 2, op.dtype, ctx=op.ctx)
        self.ws.set_col(0, x)
        self.poison = np.full(len(x), np.nan)

    def all(self):
        """The plain product, then the shifted product for both (theta, sigma) in both store policies."""
        out = []
        self.ws.set_col(1, self.poison)
        self.ws.apply(self.op, 0, 1)
        out.append(self.ws.col(1))
        for cacheable in (False, True):
            for th, sg in SHIFTS:
                self.ws.set_col(1, self.poison)
                self.ws.apply_shifted(self.op, 0, 1, th, sg, cacheable)
                out.append(self.ws.col(1))
        return out


@pytest.mark.parametrize("name", list(GRIDS))
def test_products_bit_identical_across_forms_and_to_plain_csr(name, monkeypatch):
    A, x = _matrix(name)
    _setenv(monkeypatch, {"KS_SPMV_FORMAT": "csr"})
    rows = pkg.csr_operator(A)
    assert rows.format["layout"] == "csr"
    want = Product(rows, x).all()
    assert all(np.all(np.isfinite(y)) for y in want)
    # (the two store policies of the reference carry the same values)
    for k in range(len(SHIFTS)):
        assert np.array_equal(_bits(want[1 + k]), _bits(want[1 + len(SHIFTS) + k]))
    _setenv(monkeypatch, {})
    op = pkg.csr_operator(A, rows.ctx)
    assert op.format["layout"] == "stencil" and op.format["ndict"] == 7, op.format
    P = Product(op, x)
    for form, env in FORMS:
        _setenv(monkeypatch, env)
        got = P.all()
        for k, (y, w) in enumerate(zip(got, want)):
            bad = _bits(y) != _bits(w)
            first = int(np.flatnonzero(bad)[0]) if bad.any() else -1
            assert first < 0, (name, form, "product %d" % k, "rows that differ", int(bad.sum()), "first", first, y[first], w[first])


def test_two_restart_cycles_of_the_block_expansion_are_bit_identical(monkeypatch):
    """182 x 182 x 9, nev 4, 8 / 16, blocks of 8: H, the basis size, the locked count and the Ritz values after each of two restart
    cycles, with the masks derived and with the masks read."""
    A, _x = _matrix("182x182x9")
    n = A.shape[0]
    v1 = pkg.matrices.start_vector(n)
    _setenv(monkeypatch, {})
    op = pkg.csr_operator(A)
    assert op.format["layout"] == "stencil"
    trails = []
    for geom in ("0", "1"):
        _setenv(monkeypatch, {"KS_MARCH_GEOM": geom})
        ws = pkg.ArnoldiWorkspace(n, 16, np.float64, ctx=op.ctx)
        ws.set_sstep(8)
        ws.reinitialize(0, v1)
        ws.iterate_arnoldi(op, 1, 8)
        k, active, trail = 8, 0, []
        for _ in range(2):
            r = ws.expand_restart(op, k, active, 4, "SR", 1e-10, 8, 16)
            k, active = r["k"], min(r["nlock"], 3)
            trail.append((k, active, r["eigenvalues"].copy(), np.array(ws.H)))
        assert ws.sstep_info["blocks"] > 0, ws.sstep_info   # (otherwise this ran the step-by-step path)
        trails.append(trail)
        ws.close()
    for (k0, a0, e0, H0), (k1, a1, e1, H1) in zip(*trails):
        assert (k0, a0) == (k1, a1)
        assert np.all(np.isfinite(H0)) and np.array_equal(_bits(H0), _bits(H1))
        assert np.array_equal(_bits(e0.real), _bits(e1.real)) and np.array_equal(_bits(e0.imag), _bits(e1.imag))
