"""The geometric multigrid V-cycle of `ks_operator_multigrid` (include/kschur.h (xix), csrc/ks_mg_plan.hpp, csrc/ks_mg.hpp) in numpy,
step for step: Float64 and ComplexF64, with a shift.  Plain numpy: no device, no library.  The device differs from this model in
the fused multiply-add of its smoother step, in the order of the sums inside its level products and in how those products take
the shift.  Every function works in the precision of `real` (np.float64, or np.longdouble for the reference of the model's own
rounding error, tests/mg_cases.py: ERR).

    levels:  l = 0 ... L;  shapes[l] = (nx[, ny[, nz]]);  per axis kept or halved (ceil)
    cycle_l(b):  l == L:  coarse @ b
                 x = S(b) from x = 0;  t = (A_l - shift) x;  r_c = s P^T (b - t);  x = x + P cycle_{l+1}(r_c);  x = S(b, x)
    S:  k = degree Chebyshev steps  d = a_j d + b_j dinv o (rhs - t),  x = x + d  with t = (A_l - shift) x  (pre, step 0: t = 0, x = d)"""
import numpy as np


def dims3(shape):
    d = [int(e) for e in np.atleast_1d(shape)]
    return d + [1] * (3 - len(d))


def halved(fine, coarse):
    """Per axis: 1 where `coarse` halves the extent of `fine`, 0 where it keeps it."""
    f, c = dims3(fine), dims3(coarse)
    out = []
    for a in range(3):
        assert c[a] in (f[a], (f[a] + 1) // 2), (fine, coarse)
        out.append(0 if c[a] == f[a] else 1)
    assert any(out), (fine, coarse)
    return out


def coefficients(lam, ratio, degree, real=np.float64):
    """(a, b): the smoother's coefficients with every operation rounded once in `real`, in the order of ks_mg_plan.hpp."""
    R = real
    lam, ratio = R(lam), R(ratio)
    lo = lam / ratio
    thc, dl = (lam + lo) / R(2), (lam - lo) / R(2)
    sig = thc / dl
    rho = R(1) / sig
    a, b = [R(0)], [R(1) / thc]
    for _ in range(1, degree):
        rho_new = R(1) / (R(2) * sig - rho)
        a.append(rho_new * rho)
        b.append((R(2) * rho_new) / dl)
        rho = rho_new
    return a, b


def restrict(fine, coarse, b, t):
    """s P^T (b - t): the terms of an aggregate added to +0.0 in ascending fine row order (x fastest, then y, then z)."""
    f, c, h = dims3(fine), dims3(coarse), halved(fine, coarse)
    r = (np.asarray(b) - np.asarray(t)).reshape(f[2], f[1], f[0])
    acc = np.zeros((c[2], c[1], c[0]), dtype=r.dtype)
    for dz in range(1 + h[2]):
        for dy in range(1 + h[1]):
            for dx in range(1 + h[0]):
                part = r[dz::1 + h[2], dy::1 + h[1], dx::1 + h[0]]
                acc[:part.shape[0], :part.shape[1], :part.shape[2]] += part
    s = r.real.dtype.type(2.0) ** -sum(h)
    return (s * acc).reshape(-1)


def prolong(fine, coarse, e):
    """P e: every fine cell takes the value of its coarse cell."""
    f, c, h = dims3(fine), dims3(coarse), halved(fine, coarse)
    E = np.asarray(e).reshape(c[2], c[1], c[0])
    iz, iy, ix = (np.arange(f[2]) >> h[2]), (np.arange(f[1]) >> h[1]), (np.arange(f[0]) >> h[0])
    return E[np.ix_(iz, iy, ix)].reshape(-1)


class Diagonals:
    """A scipy sparse matrix held by its stored diagonals in the precision of `real`, so that a product in np.longdouble needs no
    dense copy (7 diagonals of a stencil instead of n^2 entries).  `D @ x` adds the terms of a row in ascending column order, which
    is the order of numpy's own np.longdouble matrix product; the zeros that one adds in between change no bit."""

    def __init__(self, matrix, real):
        dia = matrix.todia()
        self.n = dia.shape[0]
        assert dia.shape == (self.n, self.n)
        order = np.argsort(dia.offsets)
        self.offsets = [int(o) for o in dia.offsets[order]]
        self.data = np.asarray(dia.data)[order].astype(real)     # data[k, j] = A[j - offsets[k], j]

    def __matmul__(self, x):
        y = np.zeros(self.n, dtype=np.result_type(self.data.dtype, x.dtype))
        for off, d in zip(self.offsets, self.data):
            lo, hi = max(off, 0), min(self.n + off, self.n)      # the columns j of this diagonal; its rows are j - off
            y[lo - off:hi - off] += d[lo:hi] * x[lo:hi]
        return y


class Cycle:
    """M as a callable b -> M b.  `matrices[l]`: the level matrices (dense or scipy sparse, real); `inverse_diagonals[l]`,
    `bounds[l]`; `coarse`: the dense matrix applied on the last level.  In a wider precision than Float64 a sparse level matrix is
    held as `Diagonals`, a dense one as a dense copy."""

    def __init__(self, matrices, shapes, inverse_diagonals, bounds, coarse, shift=0.0, degree=2, ratio=4.0, real=np.float64):
        assert len(shapes) == len(matrices) + 1 == len(inverse_diagonals) + 1 == len(bounds) + 1
        self.real, self.degree, self.shapes = real, int(degree), [tuple(np.atleast_1d(s)) for s in shapes]
        wide = real is not np.float64
        self.A = [(Diagonals(m, real) if hasattr(m, "todia") else np.asarray(m).astype(real)) if wide else m for m in matrices]
        self.dinv = [np.asarray(d).astype(real) for d in inverse_diagonals]
        self.coarse = np.asarray(coarse).astype(real) if wide else np.asarray(coarse)
        self.shift = real(shift)
        self.coef = [coefficients(lam, ratio, self.degree, real) for lam in bounds]
        self.products = [0] * len(matrices)

    def _t(self, l, x):
        self.products[l] += 1
        y = self.A[l] @ x
        return y - self.shift * x if self.shift != 0 else y

    def _smooth(self, l, rhs, x):
        a, b = self.coef[l]
        d = None
        for j in range(self.degree):
            res = rhs if x is None else rhs - self._t(l, x)
            w = self.dinv[l] * res
            d = b[0] * w if j == 0 else a[j] * d + b[j] * w
            x = d.copy() if x is None else x + d
        return x

    def _cycle(self, l, b):
        if l == len(self.A):
            return self.coarse @ b
        x = self._smooth(l, b, None)
        rc = restrict(self.shapes[l], self.shapes[l + 1], b, self._t(l, x))
        x = x + prolong(self.shapes[l], self.shapes[l + 1], self._cycle(l + 1, rc))
        return self._smooth(l, b, x)

    def __call__(self, b):
        b = np.asarray(b)
        if self.real is not np.float64:
            b = b.astype(np.clongdouble if b.dtype.kind == "c" else np.longdouble)
        return self._cycle(0, b)
