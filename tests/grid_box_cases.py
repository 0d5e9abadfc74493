"""Taps and the independent reference assembly shared by tests/test_grid_box_cpu.py and tests/test_gpu_grid_box.py (the matrix-free
box-stencil grid operator, csrc/ks_grid_box.hpp).  Shapes, potential and vector are those of tests/grid_cases.py: they walk every
axis at 1, 2, t - 1, t, t + 1, 2 t + 1 of the 32 x 32 and 1024 x 1 tiles and of the 8-plane z-range, which are the tiles (in both
element types) and the z-range of k_grid_box too; (35, 34, 17) crosses tiles in x and in y, so the corner halo cell at a tile junction
is read, and spans three z-ranges.  Plain numpy / scipy: no device, no library."""
import itertools

import numpy as np
import scipy.sparse as sp

import grid_cases as gc

SHAPES_1D, SHAPES_2D, SHAPES_3D, EDGE_SHAPES = gc.SHAPES_1D, gc.SHAPES_2D, gc.SHAPES_3D, gc.EDGE_SHAPES


def _ext(shape):
    return list(shape) + [1] * (3 - len(shape))


def taps(ndim, dtype, seed=41):
    """3^ndim distinct, non-symmetric values with full mantissas, magnitudes in [0.5, 2) and mixed signs, in slot order: any
    exchange of two slots changes bits.  ComplexF64: distinct imaginary parts as well."""
    rng = np.random.default_rng(seed + ndim)
    cnt = 3 ** ndim
    t = (0.5 + 1.5 * rng.random(cnt)) * np.where(rng.random(cnt) < 0.5, -1.0, 1.0)
    if np.dtype(dtype).kind == "c":
        t = t + 1j * (0.5 + 1.5 * rng.random(cnt)) * np.where(rng.random(cnt) < 0.5, -1.0, 1.0)
    t = t.astype(dtype)
    assert np.unique(t.real).size == cnt and np.unique(np.abs(t.real)).size == cnt and np.all(t.real != 0)
    if np.dtype(dtype).kind == "c":
        assert np.unique(t.imag).size == cnt and np.all(t.imag != 0)
    return t


def nnz(shape):
    return int(np.prod([3 * m - 2 for m in shape]))


def offsets(ndim):
    """(dx, dy, dz) of the slots 0 ... 3^ndim - 1."""
    return [tuple(reversed(d)) + (0,) * (3 - ndim) for d in itertools.product((-1, 0, 1), repeat=ndim)]


def neighbours(shape, r):
    """Rows whose stencil reads point r (r itself included): the up to 27 in-grid neighbours, by index arithmetic."""
    nx, ny, nz = _ext(shape)
    ix, iy, iz = r % nx, (r // nx) % ny, r // (nx * ny)
    out = set()
    for dx, dy, dz in itertools.product((-1, 0, 1), repeat=3):
        jx, jy, jz = ix + dx, iy + dy, iz + dz
        if 0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz:
            out.add(jx + nx * (jy + ny * jz))
    return out


def assemble(shape, t, v=None):
    """The definition of the operator, assembled independently of the library: the sum over the slots of
    t[k] S_z^dz (x) S_y^dy (x) S_x^dx with the 1-D shift matrices S^d (ones on the diagonal d).  The patterns of the slots are
    disjoint, so every stored value is a tap unchanged (one multiplication by 1.0); the diagonal is centre + potential, one numpy
    addition.  (scipy's sparse sums drop zeros: use non-zero taps and diagonals here.)"""
    ndim = len(shape)
    t = np.asarray(t).reshape(-1)
    assert t.size == 3 ** ndim and np.all(t != 0)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype)
    nx, ny, nz = _ext(shape)
    n = gc.size(shape)

    def shift(m, d):
        return sp.diags([np.ones(max(m - abs(d), 0), dtype=dt)], [d], shape=(m, m), format="csr", dtype=dt)

    A = sp.csr_matrix((n, n), dtype=dt)
    centre = (3 ** ndim - 1) // 2
    for k, (dx, dy, dz) in enumerate(offsets(ndim)):
        if k == centre:
            d = np.full(n, t[k], dtype=dt) if v is None else np.add(dt.type(t[k]), np.asarray(v, dtype=dt).ravel())
            assert np.all(d != 0)
            A = A + sp.diags(d, 0, shape=(n, n), dtype=dt)
        else:
            S = sp.kron(shift(nz, dz), sp.kron(shift(ny, dy), shift(nx, dx))).tocsr()
            S.eliminate_zeros()   # (sp.kron goes through dense blocks where a factor is small and full: their zeros are not entries)
            A = A + dt.type(t[k]) * S
    A = A.tocsr()
    A.sort_indices()
    return A


def embed_star(t7, ndim):
    """The 2 ndim + 1 taps of a 3-, 5- or 7-point stencil in the 3^ndim slots of the box stencil (zeros elsewhere)."""
    t7 = np.asarray(t7)
    out = np.zeros((3,) * ndim, dtype=t7.dtype)
    c = (1,) * ndim
    out[c] = t7[ndim]
    for a in range(ndim):          # axis a (x = 0) is index ndim - 1 - a; its - link is tap ndim - 1 - a, its + link tap ndim + 1 + a
        for s, k in ((-1, ndim - 1 - a), (1, ndim + 1 + a)):
            i = list(c)
            i[ndim - 1 - a] += s
            out[tuple(i)] = t7[k]
    return out
