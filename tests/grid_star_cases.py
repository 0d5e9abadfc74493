"""Shapes, coefficients and the independent reference assembly shared by tests/test_grid_star_cpu.py and
tests/test_gpu_grid_star.py (star stencils of radius 2-4 for the matrix-free grid operator, k_grid_star of csrc/ks_grid.hpp).
Plain numpy / scipy: no device, no library."""
import numpy as np
import scipy.sparse as sp

from grid_cases import harmonic, potential, size, vector  # noqa: F401  (shared with the radius-1 tests)

RADII = (2, 3, 4)
# launch shape of k_grid_star: in-plane tiles of 32 x 32 points (1024 x 1 where ny == 1), z-ranges of >= 8 R planes; ComplexF64 at
# R >= 3 takes half tiles, 32 x 16 and 512 x 1
TILE, TILE_WIDE, TILE_HALF, TILE_WIDE_HALF = 32, 1024, 16, 512


def zmin(R):
    return 8 * R


def _edges(t, R):
    return (1, 2, R, R + 1, 2 * R, 2 * R + 1, t - 1, t, t + 1, t + R, 2 * t + 1)


def _half(t, R):
    """the extents at which a half tile of extent t ends (2 t - 1 ... 2 t + R and 4 t + 1 are edges of the whole tile already)"""
    return (t - 1, t, t + 1, t + R)


def _zedges(R):
    zc = zmin(R)
    return (1, 2, R, R + 1, zc - 1, zc, zc + 1, 2 * zc + 1)


def _uniq(seq):
    return list(dict.fromkeys(seq))


def shapes_3d(R):
    """each axis in turn at its edge extents while the other two stay <= 5, the wide tile of ny == 1 with planes, and the shapes
    where every axis has all its taps and tiles and z-ranges are crossed"""
    return _uniq([(k, 3, 2) for k in _edges(TILE, R)] + [(5, k, 2) for k in _edges(TILE, R) + _half(TILE_HALF, R)]
                 + [(4, 3, k) for k in _zedges(R)]
                 + [(k, 1, 2) for k in (TILE_WIDE - 1, TILE_WIDE, TILE_WIDE + 1, TILE_WIDE + R, 2 * TILE_WIDE + 1) + _half(TILE_WIDE_HALF, R)]
                 + [(35, 34, 17), (33, 9, 9), (1025, 1, 9)])


def shapes_2d(R):
    return _uniq([(k, 3) for k in _edges(TILE, R)] + [(5, k) for k in _edges(TILE, R) + _half(TILE_HALF, R)] + [(65, 33)])


def shapes_1d(R):
    return _uniq([(k,) for k in _edges(TILE_WIDE, R) + _half(TILE_WIDE_HALF, R)])


# one shape per dimensionality that exercises tile edges and has every tap (shifted product, non-finite x)
EDGE_SHAPES = [(2 * TILE_WIDE + 1,), (65, 33), (33, 34, 9)]


def taps(ndim, R, dtype, symmetric=False):
    """2 ndim R + 1 distinct values in ascending column order, non-symmetric unless asked otherwise: the link of distance d along
    axis a (x = 0) in direction s has the value -(8 + 3 a + [s > 0]) / 8 / 2^(d - 1), exact in binary and distinct for every slot."""
    cplx = np.dtype(dtype).kind == "c"
    t = np.zeros(2 * ndim * R + 1, dtype=dtype)
    c = ndim * R
    t[c] = 6.5 + (0.75j if cplx and not symmetric else 0)
    for a in range(ndim):
        for d in range(1, R + 1):
            for s in (-1, 1):
                up = 1 if s > 0 and not symmetric else 0
                val = -(8 + 3 * a + up) / 8.0 / 2 ** (d - 1)
                if cplx and not symmetric:
                    val = val + 1j * s * (a + 1) * 0.0625 / d
                t[c + s * (a * R + d)] = val
    return t


def kron_matrix(shape, R, t, v=None):
    """The definition of the operator, assembled independently of the library: Kronecker sums of the 1-D off-diagonal parts with
    diagonals at +-1 ... +-R (an axis shorter than d + 1 has none at distance d) plus diags(centre + potential).  The parts have
    disjoint patterns, so every stored value is a tap (or the diagonal sum, one numpy addition) unchanged."""
    ndim = len(shape)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype)
    ext = list(shape) + [1] * (3 - ndim)
    c = ndim * R
    n = size(shape)
    eye = [sp.identity(m, dtype=dt, format="csr") for m in ext]

    def off(a):
        m = ext[a]
        A = sp.csr_matrix((m, m), dtype=dt)
        if a >= ndim:
            return A
        for d in range(1, R + 1):
            if m > d:
                A = A + sp.diags([np.full(m - d, t[c - a * R - d], dtype=dt), np.full(m - d, t[c + a * R + d], dtype=dt)], [-d, d],
                                 shape=(m, m), format="csr", dtype=dt)
        return A

    A = sp.kron(eye[2], sp.kron(eye[1], off(0)))
    A = A + sp.kron(eye[2], sp.kron(off(1), eye[0]))
    A = A + sp.kron(off(2), sp.kron(eye[1], eye[0]))
    d = np.full(n, t[c], dtype=dt) if v is None else np.add(t[c].astype(dt), np.asarray(v, dtype=dt).ravel())
    A = (A + sp.diags(d, 0, shape=(n, n), dtype=dt)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def nnz(shape, R):
    """n + sum over the axes a and d = 1 ... R of 2 max(m_a - d, 0) n / m_a"""
    n = size(shape)
    return n + sum(2 * max(m - d, 0) * (n // m) for m in shape for d in range(1, R + 1))


def neighbours(shape, r, radius):
    """Rows whose stencil reads point r (r itself included): the in-grid points at the distances 1 ... radius along every axis."""
    ext = list(shape) + [1] * (3 - len(shape))
    nx, ny, nz = ext
    p = [r % nx, (r // nx) % ny, r // (nx * ny)]
    out = {r}
    for a in range(3):
        for d in range(1, radius + 1):
            for s in (-1, 1):
                q = list(p)
                q[a] += s * d
                if 0 <= q[a] < ext[a]:
                    out.add(q[0] + nx * (q[1] + ny * q[2]))
    return out
