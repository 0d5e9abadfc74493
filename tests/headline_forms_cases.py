"""Data, exact references and launch-shape arithmetic shared by tests/test_headline_forms_cases_cpu.py and
tests/test_gpu_headline_forms.py (the kernel forms that only large problems select, run at small sizes through KS_GRID_CAP /
KS_FUSED_WB / KS_V_NT).  Plain numpy: no device, no library.

Every number below is a dyadic rational with so few bits that h = V^H w, w' = w - V h, c = V^H w' and w'' = w' - V c are EXACT in
Float64 whatever the order of the sums (products included, so fused multiply-adds change nothing): a kernel may split the rows over
any grid, any number of trips and any staging depth and must still return them bit for bit.  Only sum |w''|^2 is rounded.
tests/test_headline_forms_cases_cpu.py re-checks that claim for every case the device tests use."""
import functools
from fractions import Fraction

import numpy as np

DTYPES = [np.float64, np.complex128]
EPS = np.finfo(np.float64).eps
ETA = 1.0 / np.sqrt(2.0)          # DGKS threshold (src/expansion.jl:91)
KBLOCK = 256                      # threads per workgroup of the streaming kernels
PACK = 16                         # bytes per pack: 2 Float64 rows or 1 ComplexF64 row

# (n0, tail): n = n0 + tail rows, n0 = 4^k.  (16384, 77) under a grid cap of 1 and (65536, 513) under a cap of 3 are the smallest
# shapes at which one workgroup of k_axpy_dots_cs wraps its write-back ring at every (U, WB) the library instantiates.
SMALL = (16384, 77)
LARGE = (65536, 513)
# fused step (maxdim 64): every edge of NCW = ceil(j / 4) that matters, the U = 4 -> 2 switch at 41, the 40-column chunks of k_dots
J_FUSED = (1, 3, 4, 5, 8, 9, 16, 17, 39, 40, 41, 44, 45, 63, 64)
# ... on the large shape: one j per (U, WB) family and the widest
J_FUSED_LARGE = (9, 40, 41, 64)
# eager sequence (maxdim > 64): the 128-column chunk of k_axpy, the 40-column chunks of k_dots
J_EAGER = (65, 100, 128, 129)
MAXDIM_FUSED, MAXDIM_EAGER = 64, 129
# gemv_t / gemv_n_sub: the chunk edges of k_dots (40) and k_axpy (128) and the ragged 4-column granule
J_GEMV = (1, 5, 40, 41, 64, 65, 100, 128, 129)
VECTORS = ("a", "b")
FUSED_UWB = ((4, 8), (2, 8), (4, 24), (2, 48))     # (packs per lane and tile, tiles staged) of k_axpy_dots_cs


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def nrows(shape):
    return shape[0] + shape[1]


# ---------------------------------------------------------------------------------------------- launch-shape arithmetic
def leading_dimension(n):
    """Rows per column as the workspace pads them (multiples of 64; the stride rule only applies from 4 MiB columns on)."""
    return max((n + 63) // 64 * 64, 64)


def npacks(n, dtype):
    return leading_dimension(n) * np.dtype(dtype).itemsize // PACK


def block_ranges(total, nb):
    """Packs [begin, end) of each of nb workgroups (block_range, csrc/ks_kernels.hpp)."""
    per = (total + nb - 1) // nb
    return [(min(b * per, total), min(b * per + per, total)) for b in range(nb)]


def capped_grid(n, dtype, cap, packs_per_iter):
    """Upper bound on the workgroups of a streaming launch under KS_GRID_CAP=cap: min(cap, packs / (2 packs_per_iter)) -- the
    device-dependent term (resident workgroups) is far larger at these sizes."""
    return max(1, min(cap, npacks(n, dtype) // (2 * packs_per_iter)))


def fused_tiles(n, dtype, cap, U):
    """(tiles, packs in the last tile) of every workgroup of k_axpy_dots_cs<.., U, ..>: tiles of 64 U packs."""
    nb = capped_grid(n, dtype, cap, 64 * U)
    out = []
    for b, e in block_ranges(npacks(n, dtype), nb):
        cnt = e - b
        tiles = (cnt + 64 * U - 1) // (64 * U)
        out.append((tiles, cnt - (tiles - 1) * 64 * U if tiles else 0))
    return out


def ring_wrap_covered(n, dtype, cap, U, WB):
    """Some workgroup sees more than WB tiles, a tile count that is no multiple of WB, and a partial last tile."""
    return any(t > WB and t % WB != 0 and last < 64 * U for t, last in fused_tiles(n, dtype, cap, U))


def axpy_packs_per_workgroup(n, dtype, cap):
    """ppb of enqueue_steps_deferred (>= 3072 selects k_axpy<D, 8>) under KS_GRID_CAP=cap."""
    return npacks(n, dtype) // capped_grid(n, dtype, cap, 2 * KBLOCK)


# ---------------------------------------------------------------------------------------------- the basis
def _rng(*key):
    return np.random.default_rng([20240917, *key])


@functools.lru_cache(maxsize=None)
def _walsh(n0, ncols):
    """ncols Walsh functions +-2^-k on n0 = 4^k points with distinct random non-zero masks: orthonormal columns."""
    k = int(round(np.log2(n0))) // 2
    assert 4 ** k == n0 and ncols < n0
    masks = _rng(1, n0).choice(np.arange(1, n0), size=ncols, replace=False)
    i = np.arange(n0, dtype=np.int64)
    W = np.empty((n0, ncols), order="F")
    for c, m in enumerate(masks):
        x = i & int(m)
        par = np.zeros(n0, dtype=np.int64)
        while x.any():
            par ^= x & 1
            x = x >> 1
        W[:, c] = (1.0 - 2.0 * par) * 2.0 ** (-k)
    return W


@functools.lru_cache(maxsize=None)
def basis(shape, ncols, dtype):
    """n x ncols, column-major.  Walsh columns on the first n0 rows, zero on the tail; every third column + 1/4 of its left
    neighbour (V^H V != I: the second-pass correction is non-zero); ComplexF64: every other column times i."""
    n0, tail = shape
    W = _walsh(n0, ncols)
    B = W.copy(order="F")
    for c in range(2, ncols, 3):
        B[:, c] += 0.25 * W[:, c - 1]
    V = np.zeros((n0 + tail, ncols), dtype=dtype, order="F")
    V[:n0] = B
    if is_complex(dtype):
        V[:, 1::2] *= 1j
    V.setflags(write=False)
    return V


def basis_for(shape, j, dtype):
    """The basis a step at column j runs on: 64 columns on the fused path, 129 on the eager one (one array per path, so that
    the device tests upload it once)."""
    return basis(shape, MAXDIM_FUSED if j <= MAXDIM_FUSED else MAXDIM_EAGER, dtype)


@functools.lru_cache(maxsize=None)
def start_vector(shape, j, dtype, which):
    """(a) integers in [-15, 15] / 128 (+ i times another such): ||w'|| / ||w|| ~ 0.998, no second pass;
    (b) V[:, 0:j) g + r with g from [-8, 8] / 8 and r sparse (200 entries in [-3, 3] / 128, non-zero): most of w lies in the
    span of the basis, the second pass is taken.  g is +-5..8 / 8 on the columns that are orthogonal to all others (every third
    one, from column 0) and zero on the pairs coupled by the 1/4 admixture: with weight on those, the first projection leaves
    V (I - V^H V) g behind, several times the size of r, the second pass removes it, and ||w''|| <= eta ||w'|| -- which is a
    BREAKDOWN by the reference's own rule (src/expansion.jl:99), not a step.  The correction c = (I - V^H V) V^H r stays
    non-zero on every coupled column."""
    n = nrows(shape)
    cx = is_complex(dtype)
    rng = _rng(2, n, j, int(cx), ord(which))
    if which == "a":
        w = rng.integers(-15, 16, n) / 128.0
        if cx:
            w = w + 1j * (rng.integers(-15, 16, n) / 128.0)
    else:
        def nonzero(lo, hi, size):
            v = rng.integers(lo, hi, size)       # lo .. hi-1 without 0
            return np.where(v >= 0, v + 1, v)

        def weights(size):
            mag = rng.integers(5, 9, size) * rng.choice([-1.0, 1.0], size) / 8.0
            return np.where(np.arange(size) % 3 == 0, mag, 0.0)

        g = weights(j)
        r = np.zeros(n, dtype=dtype)
        at = rng.choice(n, size=200, replace=False)
        r[at] = nonzero(-3, 3, 200) / 128.0
        if cx:
            g = g + 1j * weights(j)
            r[at] += 1j * (nonzero(-3, 3, 200) / 128.0)
        w = basis_for(shape, j, dtype)[:, :j] @ g + r
    w = np.ascontiguousarray(w.astype(dtype))
    w.setflags(write=False)
    return w


# ---------------------------------------------------------------------------------------------- exact references
def _cdot(V, w, chunk=None, reverse=False):
    """V^H w summed over row chunks in a chosen order (None: one BLAS call)."""
    if chunk is None:
        return V.conj().T @ w
    starts = list(range(0, V.shape[0], chunk))
    if reverse:
        starts = starts[::-1]
    acc = np.zeros(V.shape[1], dtype=V.dtype)
    for s in starts:
        acc = acc + V[s : s + chunk].conj().T @ w[s : s + chunk]
    return acc


def _vh(V, h, chunk=None, reverse=False):
    """V h summed over column chunks in a chosen order."""
    if chunk is None:
        return V @ h
    starts = list(range(0, V.shape[1], chunk))
    if reverse:
        starts = starts[::-1]
    acc = np.zeros(V.shape[0], dtype=V.dtype)
    for s in starts:
        acc = acc + V[:, s : s + chunk] @ h[s : s + chunk]
    return acc


def projections(V, w, row_chunk=None, col_chunk=None, reverse=False):
    """(h, w', c, w'') of one DGKS step, summed in the order the arguments choose."""
    h = _cdot(V, w, row_chunk, reverse)
    w1 = w - _vh(V, h, col_chunk, reverse)
    c = _cdot(V, w1, row_chunk, reverse)
    w2 = w1 - _vh(V, c, col_chunk, reverse)
    return h, w1, c, w2


class Step:
    """What orthogonalize(j) must leave behind for (shape, j, dtype, which): the column of H above the sub-diagonal, the
    unnormalised new vector and its norm, and whether the second pass is taken (src/expansion.jl:81-96)."""

    def __init__(self, shape, j, dtype, which):
        V = basis_for(shape, j, dtype)[:, :j]
        w = start_vector(shape, j, dtype, which)
        self.w = w
        self.h, self.w1, self.c, self.w2 = projections(V, w)
        self.rnorm = float(np.sqrt(np.sum(np.abs(w) ** 2)))
        self.wnorm1 = float(np.sqrt(np.sum(np.abs(self.w1) ** 2)))
        self.reorth = self.wnorm1 < ETA * self.rnorm
        self.hcol = self.h + self.c if self.reorth else self.h
        self.vec = self.w2 if self.reorth else self.w1
        self.beta = float(np.sqrt(np.sum(np.abs(self.vec) ** 2)))
        self.ok = not (self.reorth and self.beta <= ETA * self.wnorm1)      # src/expansion.jl:99


@functools.lru_cache(maxsize=None)
def step(shape, j, dtype, which):
    return Step(shape, j, dtype, which)


@functools.lru_cache(maxsize=None)
def gemv_case(j, dtype):
    """(w, g, V[:, 0:j)^H w, w - V[:, 0:j) g) on the 129-column basis of the small shape: w = vector (a), g non-zero integers / 8."""
    V = basis(SMALL, MAXDIM_EAGER, dtype)[:, :j]
    w = start_vector(SMALL, j, dtype, "a")
    rng = _rng(3, j, int(is_complex(dtype)))
    g = rng.integers(1, 9, j) * rng.choice([-1.0, 1.0], j) / 8.0
    if is_complex(dtype):
        g = g + 1j * (rng.integers(1, 9, j) * rng.choice([-1.0, 1.0], j) / 8.0)
    g = g.astype(dtype)
    return w, g, _cdot(V, w), w - _vh(V, g)


def exact_dot(V, w, col):
    """conj(V[:, col]) . w in rational arithmetic (the anchor of the order-independence claim): every entry is an integer
    multiple of 2^-50, the sums are taken over Python integers."""
    scale = 2.0 ** 50

    def ints(x):
        y = np.asarray(x, dtype=np.float64) * scale
        assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2.0 ** 62
        return y.astype(np.int64).astype(object)

    ar, ai, br, bi = ints(np.real(V[:, col])), ints(np.imag(V[:, col])), ints(np.real(w)), ints(np.imag(w))
    re, im = (ar * br + ai * bi).sum(), (ar * bi - ai * br).sum()
    return Fraction(int(re), 2 ** 100), Fraction(int(im), 2 ** 100)


# ---------------------------------------------------------------------------------------------- rotations
ROT_C = (8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 44, 45, 64, 65, 100)
ROT_C0 = (0, 2)
ROT_MAXDIM = 103                   # 104 columns: c0 + c <= 102 fits
ROT_ROWS = {np.dtype(np.float64): 1300, np.dtype(np.complex128): 700}


def rot_widths(c):
    return sorted({1, 16, 17, c} & set(range(1, c + 1)))


def rot_trips(n, dtype):
    """(trips, the last one is partial) of the row loop of ONE workgroup (KS_GRID_CAP=1) in each rotation kernel:
    k_rotate_valu / k_rotate_fma walk the packs of the padded column 256 at a time, k_gemm_tall the n rows 256 at a time,
    k_rotate_mfma the 32-row wave tiles of the padded column 8 at a time (4 waves x 2 tiles)."""
    ld = leading_dimension(n)
    counts = {"packs": (npacks(n, dtype), KBLOCK), "rows": (n, KBLOCK), "wave_tiles": (ld // 32, 8)}
    return {k: (-(-cnt // per), cnt % per != 0) for k, (cnt, per) in counts.items()}


def small_ints(rng, dtype, *shape):
    M = rng.integers(-7, 8, shape).astype(np.float64)
    if is_complex(dtype):
        M = M + 1j * rng.integers(-7, 8, shape)
    return np.asfortranarray(M.astype(dtype))


def int_product(V, Q):
    """V Q in int64 (complex: four real products), converted back -- exact for the small integers above."""
    Vr, Vi = np.real(V).astype(np.int64), np.imag(V).astype(np.int64)
    Qr, Qi = np.real(Q).astype(np.int64), np.imag(Q).astype(np.int64)
    re, im = Vr @ Qr - Vi @ Qi, Vr @ Qi + Vi @ Qr
    if is_complex(V.dtype):
        return (re + 1j * im).astype(V.dtype)
    assert not im.any()
    return re.astype(V.dtype)
