"""Coefficients and the independent reference assembly shared by tests/test_grid_var_cpu.py and tests/test_gpu_grid_var.py (the
matrix-free variable-coefficient grid operator, csrc/ks_grid_var.hpp).  Shapes, taps, potential and vector are those of
tests/grid_cases.py.  Plain numpy / scipy: no device, no library."""
import numpy as np
import scipy.sparse as sp

import grid_cases as gc

# in-plane tiles of k_grid_var (csrc/ks_grid_var.hpp): Float64 as k_grid (32 x 32, 1024 x 1 where ny == 1, gc.SHAPES_* walk their
# edges), ComplexF64 32 x 16 and 512 x 1 -- the edges t - 1, t, t + 1, 2 t + 1 of these two along their axes
TILE_Y_C64, TILE_WIDE_C64 = 16, 512
SHAPES_C64_TILE = ([(5, k, 2) for k in (TILE_Y_C64 - 1, TILE_Y_C64, TILE_Y_C64 + 1, 2 * TILE_Y_C64 + 1)]
                   + [(k, 1, 2) for k in (TILE_WIDE_C64 - 1, TILE_WIDE_C64, TILE_WIDE_C64 + 1, 2 * TILE_WIDE_C64 + 1)]
                   + [(TILE_WIDE_C64 + 1,), (2 * TILE_WIDE_C64 + 1,)])


def _ext(shape):
    return list(shape) + [1] * (3 - len(shape))


def coeff(shape):
    """The smooth field with a jump, 1 + 0.5 sin(0.7 x + 0.3 y) cos(0.5 z) + 1.5 [x > nx // 2] with x, y, z the point indices: flat
    in row order (x fastest), full mantissas, between 0.5 and 3."""
    nx, ny, nz = _ext(shape)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (1.0 + 0.5 * np.sin(0.7 * x + 0.3 * y) * np.cos(0.5 * z) + 1.5 * (x > nx // 2)).ravel()


def random_coeff(shape, seed=23):
    """A random field in [0.5, 2): neighbouring values share nothing, so a product that pairs the wrong c with an x shows."""
    rng = np.random.default_rng(seed + gc.size(shape))
    return 0.5 + 1.5 * rng.random(gc.size(shape))


def nnz(shape):
    nx, ny, nz = _ext(shape)
    return nx * ny * nz + 2 * ((nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1))


def links(shape):
    """Per slot 0 ... 6 (-z, -y, -x, centre, +x, +y, +z): (the rows that have the link, the column offset)."""
    nx, ny, nz = _ext(shape)
    idx = np.arange(nx * ny * nz)
    ix, iy, iz = idx % nx, (idx // nx) % ny, idx // (nx * ny)
    return [(iz > 0, -nx * ny), (iy > 0, -nx), (ix > 0, -1), (np.ones(idx.size, dtype=bool), 0), (ix < nx - 1, 1), (iy < ny - 1, nx),
            (iz < nz - 1, nx * ny)]


def assemble(shape, t, c, v=None):
    """The definition of the operator, assembled independently of the library: per direction the index mask and, on REAL arrays,
    h[k] * (c[r] + c[s]) -- for complex taps the real and the imaginary part separately (numpy's complex multiply may fuse) --
    and the diagonal centre + potential, one numpy addition.  Returns CSR with the row's entries in slot order."""
    ndim = len(shape)
    n = gc.size(shape)
    cplx = np.dtype(t.dtype).kind == "c" or (v is not None and np.dtype(v.dtype).kind == "c")
    t7 = np.zeros(7, dtype=np.complex128)
    t7[3 - ndim : 4 + ndim] = t
    hre, him = 0.5 * t7.real, 0.5 * t7.imag
    idx = np.arange(n)
    cols = np.zeros((n, 7), dtype=np.int64)
    vre, vim = np.zeros((n, 7)), np.zeros((n, 7))
    mask = np.zeros((n, 7), dtype=bool)
    for k, (ok, off) in enumerate(links(shape)):
        mask[:, k] = ok
        s = np.where(ok, idx + off, idx)
        cols[:, k] = s
        if k == 3:
            d = np.full(n, t7[3]) if v is None else np.add(t7[3], np.asarray(v, dtype=np.complex128).ravel())
            vre[:, k], vim[:, k] = d.real, d.imag
        else:
            m = c + c[s]
            vre[:, k], vim[:, k] = hre[k] * m, him[k] * m
    data = vre[mask]
    if cplx:      # (the two parts are stored, not combined by arithmetic)
        data = np.empty(int(mask.sum()), dtype=np.complex128)
        data.real, data.imag = vre[mask], vim[mask]
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    return sp.csr_matrix((data, cols[mask].astype(np.int32), indptr), shape=(n, n))
