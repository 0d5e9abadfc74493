"""Shapes, wrap values and the independent reference assembly shared by tests/test_grid_periodic_cpu.py and
tests/test_gpu_grid_periodic.py (the matrix-free grid operator with periodic axes, `ks_operator_grid_periodic`, csrc/ks_grid.hpp).
Plain numpy / scipy: no device, no library."""
import itertools

import numpy as np
import scipy.sparse as sp

import grid_cases as gc

T, TW, Z = gc.TILE, gc.TILE_WIDE, gc.ZMIN
X, Y, ZP, ALL = (True, False, False), (False, True, False), (False, False, True), (True, True, True)


def _edges(t):
    return (3, t - 1, t, t + 1, 2 * t + 1)


# (shape, periodic flags in the order of the shape).  With t the tile extent of k_grid along an axis (32 along x and y, 1024 along x
# where ny == 1, z-ranges of 8 planes): each axis in turn periodic at 3, t - 1, t, t + 1, 2 t + 1 while the others stay <= 5 ...
CASES_AXIS = ([((k, 3, 2), X) for k in _edges(T)] + [((5, k, 2), Y) for k in _edges(T)] + [((4, 3, k), ZP) for k in _edges(Z)])
# ... all three axes periodic: the smallest grid; odd nx with two z-ranges; two tiles along x and y, three z-ranges; a single partial
# tile along x (the +x wrap neighbour is the LDS slot of an owned point), and along y
CASES_ALL = [(s, ALL) for s in ((3, 3, 3), (33, 5, 9), (35, 34, 17), (31, 3, 3), (5, 31, 3))]
CASES_2D = [(s, (True, True)) for s in ((3, 3), (33, 65), (257, 3))]
CASES_1D = [((k,), (True,)) for k in (3, TW - 1, TW, TW + 1, 2 * TW + 1)]
# the wide tile with planes; one axis / two axes of a grid with partial tiles along x and y
CASES_MIXED = [((1025, 1, 9), (True, False, True)), ((33, 34, 9), Y), ((33, 34, 9), (True, False, True))]
GROUPS = {"1d": CASES_1D, "2d": CASES_2D, "axis": CASES_AXIS, "all": CASES_ALL, "mixed": CASES_MIXED}
# one shape per dimensionality that exercises tile edges, all axes periodic, and the 3-D one with x alone
EDGE_CASES = [((2 * TW + 1,), (True,)), ((65, 33), (True, True)), ((33, 34, 9), ALL)]
EDGE_CASES_X = EDGE_CASES + [((33, 34, 9), X)]


def case_id(case):
    shape, per = case
    return "x".join(map(str, shape)) + "-" + "".join("xyz"[a] for a in range(len(shape)) if per[a])


def masks(ndim):
    return list(itertools.product((False, True), repeat=ndim))


def wrap(ndim, dtype):
    """2 ndim values in the order of the taps without the centre, distinct from one another and from every value of gc.taps."""
    full = np.array([-1.5, -0.375, -1.625, -0.5625, -1.875, -2.125])
    w = full[3 - ndim : 3 + ndim].astype(dtype)
    if np.dtype(dtype).kind == "c":
        w = w + 1j * np.array([0.3125, -0.4375, 0.1875, 0.6875, -0.28125, 0.09375])[3 - ndim : 3 + ndim]
    return w


def nnz(shape, per):
    n = gc.size(shape)
    return n + sum(2 * n if p else 2 * (m - 1) * (n // m) for m, p in zip(shape, per))


def kron_matrix(shape, per, t, w=None, v=None):
    """The definition of the periodic operator, assembled independently of the library: gc.kron_matrix with two corner entries
    in each 1-D off-diagonal part of a periodic axis -- [0, m - 1] holds the wrap value of the - direction (point 0's - neighbour is
    point m - 1), [m - 1, 0] that of the + direction; w = None: the taps.  The parts have disjoint patterns (extents >= 3 on periodic
    axes), so every stored value is a tap, a wrap value or the diagonal sum unchanged.  (Non-zero taps, wrap values and diagonals.)"""
    ndim = len(shape)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype, np.float64 if w is None else w.dtype)
    ext = list(shape) + [1] * (3 - ndim)
    pr = list(per) + [False] * (3 - ndim)
    t7 = np.zeros(7, dtype=dt)
    t7[3 - ndim : 4 + ndim] = t
    w6 = np.zeros(6, dtype=dt)
    w6[3 - ndim : 3 + ndim] = np.delete(t, ndim) if w is None else w
    n = gc.size(shape)
    eye = [sp.identity(m, dtype=dt, format="csr") for m in ext]

    def off(m, lo, hi, periodic, wlo, whi):
        D = sp.diags([np.full(max(m - 1, 0), lo, dtype=dt), np.full(max(m - 1, 0), hi, dtype=dt)], [-1, 1], shape=(m, m), format="lil", dtype=dt)
        if periodic:
            assert m >= 3
            D[0, m - 1] = wlo
            D[m - 1, 0] = whi
        return D.tocsr()

    A = sp.kron(eye[2], sp.kron(eye[1], off(ext[0], t7[2], t7[4], pr[0], w6[2], w6[3])))
    A = A + sp.kron(eye[2], sp.kron(off(ext[1], t7[1], t7[5], pr[1], w6[1], w6[4]), eye[0]))
    A = A + sp.kron(off(ext[2], t7[0], t7[6], pr[2], w6[0], w6[5]), sp.kron(eye[1], eye[0]))
    d = np.full(n, t7[3], dtype=dt) if v is None else np.add(t7[3], np.asarray(v, dtype=dt).ravel())
    A = (A + sp.diags(d, 0, shape=(n, n), dtype=dt)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def neighbours(shape, per, r):
    """Rows whose stencil reads point r (r itself included): the neighbours by index arithmetic, wrap neighbours included."""
    ext = list(shape) + [1] * (3 - len(shape))
    pr = list(per) + [False] * (3 - len(shape))
    idx = [r % ext[0], (r // ext[0]) % ext[1], r // (ext[0] * ext[1])]
    out = {r}
    for a in range(3):
        for d in (-1, 1):
            j = list(idx)
            j[a] += d
            if pr[a]:
                j[a] %= ext[a]
            if 0 <= j[a] < ext[a]:
                out.add(j[0] + ext[0] * (j[1] + ext[1] * j[2]))
    return out
