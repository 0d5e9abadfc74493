"""Cases, link tables and the independent reference assembly shared by tests/test_grid_box_periodic_cpu.py and
tests/test_gpu_grid_box_periodic.py (the box-stencil grid operator with periodic axes, `ks_operator_grid_box_periodic`,
k_grid_box_per of csrc/ks_grid_box.hpp).  Plain numpy / scipy: no device, no library.

The cases are the smallest shapes at which each part of the kernel can go wrong: the smallest torus; every axis alone at 3,
t - 1, t, t + 1, 2 t + 1 of the 32 x 32 tile and of the 8-plane z-range; a partial last tile, where the +x / +y / corner neighbour
of the last point is the LDS slot of an owned point beyond the grid ((31, 31, 3): the both-axes image, point (0, 0)); an exact
tile, where the corner HALO cell wraps in both axes; two tiles both ways with three z-ranges; two z-ranges (the pass over plane 0
and the one over plane nz - 1 in different work items); mixed flags; the wide tile with planes; 2-D and 1-D."""
import itertools

import numpy as np
import scipy.sparse as sp

import grid_box_cases as bc
import grid_cases as gc

T, Z = gc.TILE, gc.ZMIN
ALL3, ALL2 = (True, True, True), (True, True)
CASES_3D = ([((3, 3, 3), ALL3)]
            + [((k, 3, 2), (True, False, False)) for k in (3, T - 1, T, T + 1, 2 * T + 1)]
            + [((5, k, 2), (False, True, False)) for k in (3, T - 1, T, T + 1, 2 * T + 1)]
            + [((4, 3, k), (False, False, True)) for k in (3, Z - 1, Z, Z + 1, 2 * Z + 1)]
            + [((31, 3, 3), ALL3), ((5, 31, 3), ALL3), ((31, 31, 3), ALL3),   # partial tile: the images beyond it, the corner image
               ((32, 32, 3), ALL3),                                          # exact tile: the corner halo cell wraps in both axes
               ((35, 34, 17), ALL3),                                         # two tiles both ways, three z-ranges
               ((33, 5, 9), ALL3),                                           # two z-ranges, odd nx
               ((33, 34, 9), (False, True, False)), ((33, 34, 9), (True, False, True)),
               ((1025, 1, 9), (True, False, True))])                         # the wide tile with planes
CASES_2D = [((3, 3), ALL2), ((33, 65), ALL2), ((257, 3), ALL2)]
CASES_1D = [((k,), (True,)) for k in (3, gc.TILE_WIDE - 1, gc.TILE_WIDE, gc.TILE_WIDE + 1, 2 * gc.TILE_WIDE + 1)]
CASES = CASES_1D + CASES_2D + CASES_3D
# one case per dimensionality that exercises tile edges (non-finite x, shifted product)
EDGE_CASES = [((2 * gc.TILE_WIDE + 1,), (True,)), ((65, 33), ALL2), ((33, 34, 9), ALL3)]


def case_id(case):
    shape, flags = case
    return "x".join(str(m) for m in shape) + "-" + "".join("xyz"[a] for a, f in enumerate(flags) if f)


def _ext(shape):
    return list(shape) + [1] * (3 - len(shape))


def links(ndim, dtype, seed=97):
    """5^ndim distinct values with full mantissas, magnitudes in [2.5, 4) (the taps of grid_box_cases lie in [0.5, 2)) and mixed
    signs, flat in [e_z, e_y, e_x] order: any mix-up of two crossing classes, or of a class with a tap, changes bits."""
    rng = np.random.default_rng(seed + ndim)
    cnt = 5 ** ndim
    w = (2.5 + 1.5 * rng.random(cnt)) * np.where(rng.random(cnt) < 0.5, -1.0, 1.0)
    if np.dtype(dtype).kind == "c":
        w = w + 1j * (2.5 + 1.5 * rng.random(cnt)) * np.where(rng.random(cnt) < 0.5, -1.0, 1.0)
    w = w.astype(dtype)
    assert np.unique(w.real).size == cnt and np.unique(np.abs(w.real)).size == cnt
    return w


def classes(ndim):
    """(e_x, e_y, e_z) of the flat link indices 0 ... 5^ndim - 1 (a missing dimension: class 2)."""
    return [tuple(reversed(e)) + (2,) * (3 - ndim) for e in itertools.product(range(5), repeat=ndim)]


def read_mask(ndim, flags):
    """Which link values are read: some axis has class 0 or 4 and every such axis is periodic."""
    per = list(flags) + [False] * (3 - ndim)
    return np.array([any(c in (0, 4) for c in e) and all(per[a] for a, c in enumerate(e) if c in (0, 4)) for e in classes(ndim)])


def nnz(shape, flags):
    return int(np.prod([3 * m if f else 3 * m - 2 for m, f in zip(shape, flags)]))


def slot_of(e, ndim):
    """The tap slot of the link of classes e = (e_x, e_y, e_z): the offsets -1 / 0 / +1 for the classes 0, 1 / 2 / 3, 4."""
    d = [(-1, -1, 0, 1, 1)[c] for c in e]
    return sum((d[a] + 1) * 3 ** a for a in range(ndim))


def assemble(shape, flags, t, w=None, v=None):
    """The definition of the operator, assembled independently of the library:
    A = sum_e value(e) C_z^{e_z} (x) C_y^{e_y} (x) C_x^{e_x} with the 1-D parts C^1 / C^3 = ones on the diagonal -1 / +1,
    C^0 = a single one at [0, m - 1], C^4 = a single one at [m - 1, 0], C^2 = the identity; value(e) = the tap of the slot where no
    class is 0 or 4, the link value (w None: the tap of the slot) where the classes 0 and 4 all lie on periodic axes, and nothing
    otherwise.  For extents >= 3 on the periodic axes the patterns are disjoint, so every stored value is a tap or a link unchanged;
    the diagonal is centre + potential, one numpy addition."""
    ndim = len(shape)
    t = np.asarray(t).reshape(-1)
    dt = np.result_type(t.dtype, np.float64 if v is None else v.dtype, np.float64 if w is None else np.asarray(w).dtype)
    ext = _ext(shape)
    per = list(flags) + [False] * (3 - ndim)
    n = gc.size(shape)

    def part(m, c):
        if c == 2:
            return sp.identity(m, dtype=np.float64, format="coo")
        if c in (1, 3):
            return sp.diags([np.ones(max(m - 1, 0))], [-1 if c == 1 else 1], shape=(m, m), format="coo")
        return sp.coo_matrix(([1.0], ([0 if c == 0 else m - 1], [m - 1 if c == 0 else 0])), shape=(m, m))

    rows, cols, vals = [], [], []
    for k, e in enumerate(classes(ndim)):
        cross = [a for a in range(3) if e[a] in (0, 4)]
        if any(not per[a] for a in cross):
            continue
        S = sp.kron(part(ext[2], e[2]), sp.kron(part(ext[1], e[1]), part(ext[0], e[0]))).tocoo()
        keep = S.data != 0   # (sp.kron goes through dense blocks where a factor is small and full: their zeros are not entries)
        r, c = S.row[keep], S.col[keep]
        if e == (2, 2, 2):
            val = np.full(n, t[slot_of(e, ndim)], dtype=dt) if v is None else np.add(dt.type(t[slot_of(e, ndim)]), np.asarray(v, dtype=dt).ravel())
            val = val[r]
        else:
            one = t[slot_of(e, ndim)] if not cross or w is None else np.asarray(w).reshape(-1)[k]
            val = np.full(r.size, one, dtype=dt)
        rows.append(r), cols.append(c), vals.append(val)
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    assert np.unique(rows.astype(np.int64) * n + cols).size == rows.size   # disjoint patterns: nothing is summed
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n), dtype=dt)
    A.sort_indices()
    assert A.nnz == rows.size
    return A


def axis_links(i, m, per):
    """(offset, class) of the links of point i along an axis of extent m, in row order."""
    if per and i == 0:
        return [(0, 2), (1, 3), (-1, 0)]
    if per and i == m - 1:
        return [(1, 4), (-1, 1), (0, 2)]
    return [(d, d + 2) for d in (-1, 0, 1) if 0 <= i + d < m]


def row_by_definition(shape, flags, r):
    """[(column, (e_x, e_y, e_z))] of row r by the nested-offset definition: over dz in the order of its z index, inside dy, inside dx."""
    nx, ny, nz = _ext(shape)
    per = list(flags) + [False] * (3 - len(shape))
    ix, iy, iz = r % nx, (r // nx) % ny, r // (nx * ny)
    return [(((ix + dx) % nx) + nx * (((iy + dy) % ny) + ny * ((iz + dz) % nz)), (ex, ey, ez))
            for dz, ez in axis_links(iz, nz, per[2]) for dy, ey in axis_links(iy, ny, per[1]) for dx, ex in axis_links(ix, nx, per[0])]


def neighbours(shape, flags, r):
    """Rows whose stencil reads point r (r itself included), wrap images included, by index arithmetic."""
    nx, ny, nz = _ext(shape)
    per = list(flags) + [False] * (3 - len(shape))
    ix, iy, iz = r % nx, (r // nx) % ny, r // (nx * ny)
    out = set()
    for d in itertools.product((-1, 0, 1), repeat=3):
        j = [ix + d[0], iy + d[1], iz + d[2]]
        for a, m in enumerate((nx, ny, nz)):
            if per[a]:
                j[a] %= m
        if 0 <= j[0] < nx and 0 <= j[1] < ny and 0 <= j[2] < nz:
            out.add(j[0] + nx * (j[1] + ny * j[2]))
    return out


taps = bc.taps

# ---------------------------------------------------------------------------------------------- the whole solves
SOLVE_SHAPE = (12, 10, 9)
SOLVE_THETA = (0.7, 1.1, 1.9)
SOLVE_TENSOR = np.array([[1.0, 0.3, 0.2], [0.3, 1.5, 0.25], [0.2, 0.25, 2.0]])


def solve_potential(scale=1.0):
    """The harmonic potential of the solves, scaled so that the lowest eigenvalues of the torus are separated (on a torus the
    Laplacian alone has a degenerate shell above its constant mode; tests/test_grid_box_periodic_cpu.py checks the gaps)."""
    return scale * gc.harmonic(SOLVE_SHAPE)
