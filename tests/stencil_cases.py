"""Deterministic constant-coefficient, NON-symmetric stencil matrices for the stencil-mask layout and its marching kernels
(csrc/ks_spmv_march.hpp), in the style of layout_cases.py: shared by tests/test_stencil_cases_cpu.py (which layout and slot order
they plan to) and tests/test_gpu_shifted_product.py (products against exact references).

A family is a list of taps (column offset, value) -- on a line, or on an nx x ny x (as many planes as n needs) grid whose rows
lack the taps that leave the grid -- cut to n rows, without and with about 10 % of its entries knocked out at seeded positions:
every row stays a sub-sequence of the one slot order, so the matrix stays in the stencil layout while interior rows miss slots.

Sizes: tile = 512 rows.  k_spmv_stencil_march takes tile t through its unclamped path iff 512 t + 512 + dmax + 1 <= n (the window
form: ... + max(dmax + 1, 257)), so n = 512 * 27 + bound + e with e in {-1, 0, 1} puts tile 27 one short of, exactly at and one
past that bound; 14079 is one more odd size away from it.  28-29 tiles: 3-4 per XCD, walked by 1-4 workgroups (KS_MARCH_S)."""
import functools

import numpy as np
import scipy.sparse as sp

TILE = 512
KTILES = 27
ODD_N = 14079
KNOCK = 0.10


def _values(seed, count, dtype):
    """`count` tap values in +-[0.5, 1.5) with full mantissas (products round), complex ones for a complex dtype."""
    rng = np.random.default_rng(1000 + seed)
    v = (0.5 + rng.random(count)) * np.where(rng.random(count) < 0.5, -1.0, 1.0)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * (0.5 + rng.random(count)) * np.where(rng.random(count) < 0.5, -1.0, 1.0)
    return v.astype(dtype)


class Family:
    """name; deltas in the slot order the plan must give; grid = (nx, ny) or None (a line); kernel: what launch_march picks by
    default, and `forms`: the environment settings under which the case takes ANOTHER kernel."""

    def __init__(self, name, seed, deltas=None, grid=None, dims=3, kernel=None, forms=()):
        self.name, self.seed, self.grid, self.dims = name, seed, grid, dims
        if grid is not None:
            nx, ny = grid
            deltas = [-nx, -1, 0, 1, nx] if dims == 2 else [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
        self.deltas = list(deltas)
        self.kernel = kernel
        self.forms = dict(forms)
        self.dmax = max(0, max(self.deltas))
        self.dmin = min(0, min(self.deltas))

    @property
    def bound(self):
        """Rows behind the start of the last unclamped tile."""
        reach = self.dmax + 1
        if self.kernel.startswith("window"):
            reach = max(reach, 257)   # (its dmax starts at 256: the window reaches 256 rows past the tile)
        return TILE + reach

    def sizes(self):
        base = TILE * (KTILES - 1) + self.bound
        return [base - 1, base, base + 1, ODD_N]

    def cases(self):
        return [(n, knock) for n in self.sizes() for knock in (False, True)]


FORMS_W = {"registers": {"KS_MARCH_Z": "0", "KS_MARCH_WINDOW": "0"}}
FAMILIES = [
    Family("line3", 1, [-1, 0, 1], kernel="march<3,1>"),
    Family("grid2d-37", 2, grid=(37, 0), dims=2, kernel="march<5,2>"),
    Family("grid3d-20x15", 3, grid=(20, 15), kernel="window<0x14>", forms=FORMS_W),
    Family("grid3d-21x15", 4, grid=(21, 15), kernel="window<0x36>", forms=FORMS_W),
    Family("grid3d-300x3", 5, grid=(300, 3), kernel="march<7,3>"),
    Family("hollow", 6, [-1, 1], kernel="march<2,-1>"),
    Family("upwind", 7, [-1, 0], kernel="march<2,-1>"),
    Family("diagonal", 8, [0], kernel="march<1,-1>"),
    Family("super3", 9, [3], kernel="march<1,-1>"),
    Family("forward3", 10, [0, 1, 2], kernel="march<3,-1>"),
    Family("four", 11, [-5, -1, 0, 2], kernel="march<4,-1>"),
    Family("five-offcentre", 12, [-1, 0, 1, 2, 7], kernel="march<5,-1>"),
    Family("six-hollow", 13, [-40, -3, -1, 1, 3, 40], kernel="march<6,-1>"),
    Family("seven-offcentre", 14, [-1, 0, 1, 2, 3, 4, 5], kernel="march<7,-1>"),
    Family("eight-wide", 15, [-600, -40, -1, 0, 1, 2, 40, 600], kernel="march<8,-1>"),
    # near taps that are neither +-1 nor +-nx (all even here): the window form's catch-all, every near tap as two 8-byte reads
    Family("seven-even-near", 17, [-300, -20, -2, 0, 2, 20, 300], kernel="window<0x3e>", forms=FORMS_W),
]
# the one large grid: planes of >= 64 tiles and >= 8 of them -> the z-marching form; KS_MARCH_Z=0: the window form, ... registers
BIG = Family("grid3d-182x182x9", 16, grid=(182, 182), kernel="marchz<0x14>",
             forms={"window": {"KS_MARCH_Z": "0"}, "registers": {"KS_MARCH_Z": "0", "KS_MARCH_WINDOW": "0"}})
BIG_N = 182 * 182 * 9
BY_NAME = {f.name: f for f in FAMILIES + [BIG]}


def expected_kernel(deltas, n, env=None):
    """What CsrOp::launch_march (csrc/ks_operators.hpp) launches for a Float64 stencil with these slots on n rows."""
    env = env or {}
    flag = lambda k: int(env.get(k, "1"))  # noqa: E731
    if not flag("KS_STENCIL_MARCH"):
        return "stencil2"
    ns = len(deltas)
    kown = deltas.index(0) if 0 in deltas else -1
    if flag("KS_MARCH_WINDOW") and ns == 7 and kown == 3:
        shape = abs(deltas[0]) > 256 and abs(deltas[6]) > 256 and all(abs(d) <= 256 for d in deltas[1:6])
        odd = sum(1 << k for k in range(1, 6) if deltas[k] & 1)
        oddname = {0x14: "0x14", 0x36: "0x36"}.get(odd, "0x3e")
        P = deltas[6]
        if shape and flag("KS_MARCH_Z") and deltas[0] == -P and P % 2 == 0 and P >= 8 * 8 * 512 and (n + P - 1) // P >= 8:
            return "marchz<%s>" % oddname
        if shape:
            return "window<%s>" % oddname
    if (ns, kown) in ((7, 3), (5, 2), (3, 1)):
        return "march<%d,%d>" % (ns, kown)
    return "march<%d,-1>" % ns


@functools.lru_cache(maxsize=4)
def build(name, n, knock, dtype="float64"):
    """(A, x, removed): the n x n CSR matrix of family `name`, a start vector, and the (rows, columns) of the knocked-out entries."""
    fam = BY_NAME[name]
    dtype = np.dtype(dtype)
    vals = _values(fam.seed, len(fam.deltas), dtype)
    r = np.arange(n, dtype=np.int64)
    rows, cols, data = [], [], []
    for k, d in enumerate(fam.deltas):
        c = r + d
        ok = (c >= 0) & (c < n)
        if fam.grid is not None:
            nx, ny = fam.grid
            ix = r % nx
            if d == -1:
                ok &= ix > 0
            elif d == 1:
                ok &= ix < nx - 1
            elif fam.dims == 3 and abs(d) == nx:
                iy = (r // nx) % ny
                ok &= (iy > 0) if d < 0 else (iy < ny - 1)
        rows.append(r[ok]); cols.append(c[ok]); data.append(np.full(int(ok.sum()), vals[k], dtype=dtype))
    rows, cols, data = np.concatenate(rows), np.concatenate(cols), np.concatenate(data)
    rng = np.random.default_rng(7000 + 31 * fam.seed + n % 1000)
    removed = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    if knock:
        out = rng.random(rows.size) < KNOCK
        removed = (rows[out], cols[out])
        rows, cols, data = rows[~out], cols[~out], data[~out]
    A = sp.csr_matrix((data, (rows, cols)), shape=(n, n))
    A.sort_indices()
    x = rng.standard_normal(n)
    if dtype.kind == "c":
        x = x + 1j * rng.standard_normal(n)
    return A, x.astype(dtype), removed
