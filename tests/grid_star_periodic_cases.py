"""Shapes, wrap values and the independent reference assembly shared by tests/test_grid_star_periodic_cpu.py and
tests/test_gpu_grid_star_periodic.py (star stencils of radius 2-4 with periodic axes for the matrix-free grid operator,
`ks_operator_grid_star_periodic`, k_grid_star_per of csrc/ks_grid.hpp).  Plain numpy / scipy: no device, no library."""
import numpy as np
import scipy.sparse as sp

import grid_star_cases as sc
from grid_star_cases import RADII, TILE, TILE_HALF, TILE_WIDE, TILE_WIDE_HALF, potential, size, taps, vector, zmin  # noqa: F401

X, Y, ZP, ALL = (True, False, False), (False, True, False), (False, False, True), (True, True, True)


def _uniq(seq):
    return list(dict.fromkeys(seq))


def _edges(t, R):
    """a periodic axis at its smallest extents (where a double wrap or a coinciding link would show) and around a tile of extent t"""
    return (2 * R + 1, 2 * R + 2, t - R, t - 1, t, t + 1, t + R, 2 * t + 1)


def _half(t, R):
    return (t - R, t - 1, t, t + 1, t + R)


def _zedges(R):
    zc = zmin(R)
    return (2 * R + 1, 2 * R + 2, zc - 1, zc, zc + 1, zc + R, 2 * zc + 1)


# (shape, periodic flags in the order of the shape), per radius
def cases_axis(R):
    """each axis in turn periodic at its edge extents while the others stay small (and open)"""
    return _uniq([((k, 3, 2), X) for k in _edges(TILE, R)] + [((5, k, 2), Y) for k in _edges(TILE, R) + _half(TILE_HALF, R)]
                 + [((4, 3, k), ZP) for k in _zedges(R)])


def cases_all(R):
    """all axes periodic: the smallest torus; tiles and z-ranges crossed; a single partial tile along x / along y (the images sit
    in owned slots and halo cells at once)"""
    m = 2 * R + 1
    return [(s, ALL) for s in ((m, m, m), (35, 34, 17), (33, 9, 9), (31, 9, 9), (9, 31, 9))]


def cases_mixed(R):
    return [((1025, 1, 9), (True, False, True)), ((33, 34, 9), Y), ((33, 34, 9), (True, False, True))]


def cases_2d(R):
    m = 2 * R + 1
    return [(s, (True, True)) for s in ((m, m), (33, 65), (257, m))]


def cases_1d(R):
    return _uniq([((k,), (True,)) for k in (2 * R + 1, TILE_WIDE - R, TILE_WIDE - 1, TILE_WIDE, TILE_WIDE + 1, TILE_WIDE + R, 2 * TILE_WIDE + 1)
                  + _half(TILE_WIDE_HALF, R)])


GROUPS = {"1d": cases_1d, "2d": cases_2d, "axis": cases_axis, "all": cases_all, "mixed": cases_mixed}
# one shape per dimensionality that exercises tile edges, all axes periodic, and the 3-D one with x alone
EDGE_CASES = [((2 * TILE_WIDE + 1,), (True,)), ((65, 33), (True, True)), ((33, 34, 9), ALL)]
EDGE_CASES_X = EDGE_CASES + [((33, 34, 9), X)]


def case_id(case):
    shape, per = case
    return "x".join(map(str, shape)) + "-" + "".join("xyz"[a] for a in range(len(shape)) if per[a])


def wrap(ndim, R, dtype):
    """2 ndim R distinct values in the order of the taps without the centre: the boundary-crossing link of distance d along axis a
    (x = 0) in direction s has the value +(17 + 3 a + [s > 0]) / 32 / 2^(d - 1) -- exact in binary, distinct for every slot, and
    positive where every off-diagonal value of sc.taps is negative (the centre 6.5 is larger than any of them)."""
    cplx = np.dtype(dtype).kind == "c"
    w = np.zeros(2 * ndim * R, dtype=dtype)
    c = ndim * R
    for a in range(ndim):
        for d in range(1, R + 1):
            for s in (-1, 1):
                val = (17 + 3 * a + (1 if s > 0 else 0)) / 32.0 / 2 ** (d - 1)
                if cplx:
                    val = val - 1j * s * (a + 1) * 0.09375 / 2 ** (d - 1)
                w[c - a * R - d if s < 0 else c + a * R + d - 1] = val
    return w


def taps_as_wrap(t, ndim, R):
    """the taps without the centre: what wrap = None means"""
    return np.delete(t, ndim * R)


def kron_matrix(shape, per, R, t, w=None, v=None):
    """The definition of the operator, assembled independently of the library: Kronecker sums of the 1-D off-diagonal parts with
    diagonals at +-1 ... +-R and, on a periodic axis of extent m, the R (R + 1) / 2 corner entries per side -- [i, i + d - m] holds
    the wrap value of +d for i + d >= m, [i, i - d + m] that of -d for i < d; w = None: the taps.  The patterns are disjoint for
    m >= 2 R + 1, so every stored value is a tap, a wrap value or the diagonal sum (one numpy addition) unchanged."""
    ndim = len(shape)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype, np.float64 if w is None else w.dtype)
    ext = list(shape) + [1] * (3 - ndim)
    pr = list(per) + [False] * (3 - ndim)
    c = ndim * R
    w = taps_as_wrap(t, ndim, R) if w is None else w
    n = size(shape)
    eye = [sp.identity(m, dtype=dt, format="csr") for m in ext]

    def off(a):
        m = ext[a]
        A = sp.lil_matrix((m, m), dtype=dt)
        if a >= ndim:
            return A.tocsr()
        if pr[a]:
            assert m >= 2 * R + 1
        for d in range(1, R + 1):
            lo, hi = t[c - a * R - d], t[c + a * R + d]
            for i in range(m):
                if i - d >= 0:
                    A[i, i - d] = lo
                elif pr[a]:
                    assert A[i, i - d + m] == 0
                    A[i, i - d + m] = w[c - a * R - d]
                if i + d < m:
                    A[i, i + d] = hi
                elif pr[a]:
                    assert A[i, i + d - m] == 0
                    A[i, i + d - m] = w[c + a * R + d - 1]
        return A.tocsr()

    A = sp.kron(eye[2], sp.kron(eye[1], off(0)))
    A = A + sp.kron(eye[2], sp.kron(off(1), eye[0]))
    A = A + sp.kron(off(2), sp.kron(eye[1], eye[0]))
    d = np.full(n, t[c], dtype=dt) if v is None else np.add(t[c].astype(dt), np.asarray(v, dtype=dt).ravel())
    A = (A + sp.diags(d, 0, shape=(n, n), dtype=dt)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def nnz(shape, per, R):
    """n + sum over the axes a of (periodic ? 2 R n : sum over d = 1 ... R of 2 max(m_a - d, 0) n / m_a)"""
    n = size(shape)
    return n + sum(2 * R * n if p else sum(2 * max(m - d, 0) * (n // m) for d in range(1, R + 1)) for m, p in zip(shape, per))


def neighbours(shape, per, r, R):
    """Rows whose stencil reads point r (r itself included): the points at the distances 1 ... R along every axis by index
    arithmetic, wrap neighbours included."""
    ext = list(shape) + [1] * (3 - len(shape))
    pr = list(per) + [False] * (3 - len(shape))
    idx = [r % ext[0], (r // ext[0]) % ext[1], r // (ext[0] * ext[1])]
    out = {r}
    for a in range(3):
        for d in range(1, R + 1):
            for s in (-1, 1):
                j = list(idx)
                j[a] += s * d
                if pr[a]:
                    j[a] %= ext[a]
                if 0 <= j[a] < ext[a]:
                    out.add(j[0] + ext[0] * (j[1] + ext[1] * j[2]))
    return out


assert sc.RADII == (2, 3, 4)
