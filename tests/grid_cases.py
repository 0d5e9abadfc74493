"""Shapes, coefficients and the independent reference assembly shared by tests/test_grid_operator_cpu.py and
tests/test_gpu_grid_operator.py (the matrix-free grid operator, csrc/ks_grid.hpp).  Plain numpy / scipy: no device, no library."""
import numpy as np
import scipy.sparse as sp

# launch shape of k_grid (csrc/ks_grid.hpp): in-plane tiles of 32 x 32 points (1024 x 1 where ny == 1), z-ranges of >= 8 planes
TILE, TILE_WIDE, ZMIN = 32, 1024, 8


def _edges(t):
    return (1, 2, t - 1, t, t + 1, 2 * t + 1)


# each axis in turn at 1, 2, t - 1, t, t + 1, 2 t + 1 while the other two stay <= 5
SHAPES_3D = ([(k, 3, 2) for k in _edges(TILE)] + [(5, k, 2) for k in _edges(TILE)] + [(4, 3, k) for k in _edges(ZMIN)]
             + [(k, 1, 2) for k in (TILE_WIDE - 1, TILE_WIDE, TILE_WIDE + 1, 2 * TILE_WIDE + 1)]   # the wide tile of ny == 1, with planes
             + [(33, 5, 9),      # odd nx: x-lines start at odd rows (not 16-byte aligned); n = 1485 is no multiple of 64; two z-ranges
                (35, 34, 17)])   # two tiles along x and along y, three z-ranges; n = 20230 is no multiple of 64
SHAPES_2D = [(k, k) for k in (1, 2, 63, 64, 65, 257)] + [(257, 3), (3, 257)]
SHAPES_1D = [(k,) for k in (1, 2, 63, 64, 65, 257, TILE_WIDE - 1, TILE_WIDE, TILE_WIDE + 1, 2 * TILE_WIDE + 1)]
# one shape per dimensionality that exercises tile edges (shifted product, non-finite x)
EDGE_SHAPES = [(2 * TILE_WIDE + 1,), (65, 33), (33, 34, 9)]


def size(shape):
    return int(np.prod(shape))


def taps(ndim, dtype, symmetric=False):
    """2 ndim + 1 distinct values in ascending column order, non-symmetric unless asked otherwise."""
    full = np.array([-1.75, -0.625, -1.125, 6.5, -0.875, -1.375, -2.25])
    if symmetric:
        full = np.array([-2.0, -0.75, -1.25, 6.5, -1.25, -0.75, -2.0])
    t = full[3 - ndim : 4 + ndim].astype(dtype)
    if np.dtype(dtype).kind == "c":
        t = t + 1j * np.array([0.25, -0.5, 0.125, 0.75, -0.375, 0.0625, -0.15625])[3 - ndim : 4 + ndim]
        if symmetric:
            t = t.real.astype(dtype)
    return t


def potential(shape, dtype, seed=5):
    rng = np.random.default_rng(seed + size(shape))
    v = rng.random(size(shape)) * 3.0 - 1.0
    if np.dtype(dtype).kind == "c":
        v = v + 1j * (rng.random(size(shape)) - 0.5)
    return v.astype(dtype)


def harmonic(shape):
    """V = |p - centre|^2 / 8 on the grid points, flat in row order (x fastest)."""
    ax = [np.arange(m, dtype=np.float64) - (m - 1) / 2.0 for m in shape]
    grids = np.meshgrid(*ax[::-1], indexing="ij")   # C order (z, y, x): ravel() is the row order
    return (sum(g * g for g in grids) / 8.0).ravel()


def vector(shape, dtype, seed=11):
    rng = np.random.default_rng(seed + size(shape))
    x = rng.random(size(shape)) - 0.5
    if np.dtype(dtype).kind == "c":
        x = x + 1j * (rng.random(size(shape)) - 0.5)
    return x.astype(dtype)


def kron_matrix(shape, t, v=None):
    """The definition of the operator, assembled independently of the library: Kronecker sums of the three 1-D off-diagonal parts
    plus diags(centre + potential).  The parts have disjoint patterns, so every stored value is a tap (or the diagonal sum, one
    numpy addition) unchanged.  (scipy's sparse sums drop zeros: use non-zero taps and diagonals here.)"""
    ndim = len(shape)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype)
    ext = list(shape) + [1] * (3 - ndim)
    t7 = np.zeros(7, dtype=dt)
    t7[3 - ndim : 4 + ndim] = t
    n = size(shape)
    eye = [sp.identity(m, dtype=dt, format="csr") for m in ext]

    def off(m, lo, hi):
        return sp.diags([np.full(max(m - 1, 0), lo, dtype=dt), np.full(max(m - 1, 0), hi, dtype=dt)], [-1, 1], shape=(m, m), format="csr", dtype=dt)

    A = sp.kron(eye[2], sp.kron(eye[1], off(ext[0], t7[2], t7[4])))
    A = A + sp.kron(eye[2], sp.kron(off(ext[1], t7[1], t7[5]), eye[0]))
    A = A + sp.kron(off(ext[2], t7[0], t7[6]), sp.kron(eye[1], eye[0]))
    d = np.full(n, t7[3], dtype=dt) if v is None else np.add(t7[3], np.asarray(v, dtype=dt).ravel())
    A = (A + sp.diags(d, 0, shape=(n, n), dtype=dt)).tocsr()
    A.eliminate_zeros()   # (sp.kron goes through dense blocks where a factor is small and full: their zeros are not entries)
    A.sort_indices()
    return A


def neighbours(shape, r):
    """Rows whose stencil reads point r (r itself included): the in-grid neighbours, by index arithmetic."""
    ext = list(shape) + [1] * (3 - len(shape))
    nx, ny, nz = ext
    ix, iy, iz = r % nx, (r // nx) % ny, r // (nx * ny)
    out = {r}
    for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        jx, jy, jz = ix + dx, iy + dy, iz + dz
        if 0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz:
            out.add(jx + nx * (jy + ny * jz))
    return out
