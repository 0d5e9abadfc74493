"""The matrices of the device-layout tests, shared by tests/test_gpu_spmv_layouts.py (uploads them, checks the products)
and tests/test_csr_layout_cpu.py (asks ks_host_csr_plan which layout they get), and CASES: the fixed list of
(matrix, dtype, environment) whose layout facts are recorded in tests/golden/csr_layout_plans.json
(tools/record_csr_layout_plans.py writes it from uploaded operators).  Every generator draws from its random generator in
the order the GPU tests always did, so the matrices are the same in both files."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle.matrices import laplace3d

LAYOUT_ENV = ("KS_SPMV_FORMAT", "KS_SPMV_PTR64", "KS_SELL_SIGMA", "KS_DVI_RPT", "KS_SPMV_COLBLOCKS", "KS_SPMV_CB_RPT",
              "KS_SPMV_CB_SINGLE", "KS_SPMV_NI", "KS_SPMV_CSR_ROWGATHER")
NUM_CU = 256  # MI355X


def rnd(rng, dtype, *shape):
    a = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "c":
        a = a + 1j * rng.standard_normal(shape)
    return a.astype(dtype)


def skewed(rng, dtype, n):
    """Short random rows + empty rows + a band of 300-entry rows + rows far longer than any block capacity."""
    cplx = np.dtype(dtype).kind == "c"
    A = sp.random(n, n, density=4.0 / n, random_state=rng, format="lil", dtype=np.float64)
    for r, cnt in ((3, 4097), (n // 3, 9000), (n - 2, 9000)):
        c = rng.choice(n, cnt, replace=False)
        A[r, c] = rng.standard_normal(cnt)
    for r in range(n // 2, n // 2 + 40):
        c = rng.choice(n, 300, replace=False)
        A[r, c] = rng.standard_normal(300)
    A[10:30, :] = 0
    A = A.tocsr()
    if cplx:
        B = A.copy()
        B.data = rng.standard_normal(B.nnz)
        A = (A + 1j * B).tocsr()
    A.sort_indices()
    return A.astype(dtype)


def skewed_case(dtype):
    rng = np.random.default_rng(101)
    n = 20011
    A = skewed(rng, dtype, n)
    return A, rnd(rng, dtype, n)


def varcoef_and_ragged(dtype):
    """(A, x): 7-point stencil with variable coefficients; (R, xr): rows of 0..40 entries, a few distinct values, Inf in xr."""
    cplx = np.dtype(dtype).kind == "c"
    rng = np.random.default_rng(55)
    A = laplace3d(13, 14, 15).astype(dtype)
    A.data = A.data * (1.0 + 0.5 * rng.random(A.nnz)) + (0.1j * rng.random(A.nnz) if cplx else 0)
    x = rnd(rng, dtype, A.shape[0])
    m = 5003
    R = sp.random(m, m, density=8.0 / m, random_state=rng, format="csr", dtype=np.float64)
    R.data = np.array([1.5, -2.0, 0.25, -0.0])[rng.integers(0, 4, R.nnz)]
    R = R.tolil()
    R[100:164, :] = 0
    R[7, rng.choice(m, 40, replace=False)] = 3.0
    R = R.tocsr().astype(dtype)
    R.sort_indices()
    xr = rnd(rng, dtype, m)
    xr[rng.choice(m, 5, replace=False)] = np.inf  # a padding entry must never be multiplied
    return A, x, R, xr


def stencil19(dtype):
    """27-point-like stencil with 19 offsets on a 9 x 8 x 7 grid, random coefficients; returns (A, x, rng)."""
    cplx = np.dtype(dtype).kind == "c"
    rng = np.random.default_rng(91)
    mx, my, mz = 9, 8, 7
    n = mx * my * mz
    rows, cols, vals = [], [], []
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if abs(dx) + abs(dy) + abs(dz) <= 2]
    assert len(offs) == 19
    coef = {o: (rng.standard_normal() + (1j * rng.standard_normal() if cplx else 0)) for o in offs}
    for z in range(mz):
        for y in range(my):
            for x_ in range(mx):
                r = x_ + mx * (y + my * z)
                for (dx, dy, dz) in offs:
                    if 0 <= x_ + dx < mx and 0 <= y + dy < my and 0 <= z + dz < mz:
                        rows.append(r); cols.append(r + dx + mx * (dy + my * dz)); vals.append(coef[(dx, dy, dz)])
    A = sp.csr_matrix((np.array(vals, dtype=dtype), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A, rnd(rng, dtype, n), rng


def opposite_orders(dtype):
    """6 x 6, unsorted CSR: row 0 holds the entries (delta 1, 5.0), (delta 2, 7.0), row 2 the same two in the opposite
    order -- no single slot order embeds both rows.  Returns (ptr, idx, val)."""
    ptr = np.array([0, 2, 2, 4, 4, 4, 4], dtype=np.int64)
    idx = np.array([1, 2, 4, 3], dtype=np.int64)            # row 0: cols 1, 2;  row 2: cols 4, 3 (unsorted)
    val = np.array([5.0, 7.0, 7.0, 5.0]).astype(dtype)       # row 0: (d1,5),(d2,7); row 2: (d2,7),(d1,5)  -> cycle
    return ptr, idx, val


def banded33(dtype):
    n4 = 400
    diags = [np.full(n4 - k, 1.0 + k) for k in range(33)]
    return sp.diags(diags, list(range(33)), format="csr").astype(dtype)


def colblock_matrix(dtype):
    """Scattered columns, empty rows, rows confined to the first / last column block; returns (A, x, rng)."""
    rng = np.random.default_rng(11)
    n = 30_000
    A = sp.random(n, n, density=6.0 / n, random_state=rng, format="lil", dtype=np.float64)
    A[100:140, :] = 0                                   # empty rows
    for r in range(200, 260):                           # rows confined to the first / last column block
        A[r, :] = 0
        A[r, rng.choice(n // 8, 5, replace=False)] = rng.standard_normal(5)
        A[r + 100, :] = 0
        A[r + 100, n - 1 - rng.choice(n // 8, 5, replace=False)] = rng.standard_normal(5)
    A = A.tocsr()
    if np.dtype(dtype).kind == "c":
        B = A.copy()
        B.data = rng.standard_normal(B.nnz)
        A = (A + 1j * B).tocsr()
    A = A.astype(dtype)
    A.sort_indices()
    return A, rnd(rng, dtype, n), rng


def reversed_row(A, r=5000):
    """A with the entries of row r stored in descending column order (None if the row has fewer than two)."""
    U = A.copy()
    U.has_sorted_indices = False
    a, b = U.indptr[r], U.indptr[r + 1]
    if b - a < 2:
        return None
    U.indices[a:b] = U.indices[a:b][::-1].copy()
    U.data[a:b] = U.data[a:b][::-1].copy()
    return U


def colblock_big(rng, pkg, dtype=np.float64):
    """(H, xh, Bd): the hashed matrix of BASELINE config 3 at n = 1e6 (x = 8 MB, scattered columns), a vector, and a banded
    matrix of the same order."""
    H = pkg.matrices.hashed_nonsymmetric_csr(1_000_000, seed=7)
    xh = rnd(rng, dtype, H.shape[0])
    Bd = sp.diags([rng.standard_normal(1_000_000 - abs(k)) for k in (-3, -1, 0, 1, 3)], [-3, -1, 0, 1, 3], format="csr")
    return H, xh, Bd


def slab(A, offsets, rank):
    """Row block `rank` of the square scipy matrix A cut at `offsets`, columns LOCAL-EXTENDED as ks_operator_csr_dist takes
    them (ghost slots in global column order behind the local columns).  Returns dict(ptr, idx, val, n, nghost, nlow)."""
    r0, r1 = int(offsets[rank]), int(offsets[rank + 1])
    S = A[r0:r1].tocsr()
    S.sort_indices()
    g = S.indices.astype(np.int64)
    owned = (g >= r0) & (g < r1)
    ghosts = np.unique(g[~owned])
    idx = np.where(owned, g - r0, (r1 - r0) + np.searchsorted(ghosts, g))
    return dict(ptr=S.indptr.astype(np.int64), idx=idx.astype(np.int64), val=np.ascontiguousarray(S.data), n=r1 - r0,
                nghost=int(len(ghosts)), nlow=int((ghosts < r0).sum()), ghost_global=ghosts, offsets=offsets, rank=rank)


def _csr(A):
    A = A.tocsr()
    return dict(ptr=A.indptr.astype(np.int64), idx=A.indices.astype(np.int64), val=np.ascontiguousarray(A.data), n=A.shape[0],
                nghost=-1, nlow=0)


@functools.lru_cache(maxsize=8)
def matrix(key, dtype):
    """The matrix named `key` as dict(ptr, idx, val, n, nghost, nlow); nghost < 0: a whole square matrix on one GPU."""
    dtype = np.dtype(dtype).type
    name, _, arg = key.partition(":")
    if name == "skewed":
        return _csr(skewed_case(dtype)[0])
    if name == "varcoef":
        return _csr(varcoef_and_ragged(dtype)[0])
    if name == "ragged":
        return _csr(varcoef_and_ragged(dtype)[2])
    if name == "laplace":
        return _csr(laplace3d(*map(int, arg.split("x"))).astype(dtype))
    if name == "stencil19":
        return _csr(stencil19(dtype)[0])
    if name == "opposite":
        ptr, idx, val = opposite_orders(dtype)
        return dict(ptr=ptr, idx=idx, val=val, n=6, nghost=-1, nlow=0)
    if name == "banded33":
        return _csr(banded33(dtype))
    if name == "colblock":
        return _csr(colblock_matrix(dtype)[0])
    if name == "colblock-reversed":
        return _csr(reversed_row(colblock_matrix(dtype)[0]))
    if name in ("hashed1e6", "banded1e6"):
        from __graft_entry__ import import_package

        rng = colblock_matrix(dtype)[2]
        H, _xh, Bd = colblock_big(rng, import_package(), dtype)
        return _csr(H if name == "hashed1e6" else Bd)
    if name == "hashed":  # BASELINE config 3 at a small size
        from __graft_entry__ import import_package

        return _csr(import_package().matrices.hashed_nonsymmetric_csr(int(arg), seed=7).astype(dtype))
    if name == "slab":  # BASELINE config 5 at a small size: "GxGxG/world/rank"
        grid, world, rank = arg.split("/")
        A = laplace3d(*map(int, grid.split("x"))).astype(dtype)
        n = A.shape[0]
        offsets = np.array([n * r // int(world) for r in range(int(world) + 1)], dtype=np.int64)
        return slab(A, offsets, int(rank))
    raise KeyError(key)


def _cases():
    f64, c64 = "float64", "complex128"
    both = (f64, c64)
    out = []

    def add(key, dtypes, **env):
        for dt in dtypes:
            out.append(dict(matrix=key, dtype=dt, env={k: str(v) for k, v in env.items()}))

    # test_csr_row_blocks_long_rows_and_64bit_offsets
    for p64 in (0, 1):
        add("skewed", both, KS_SPMV_FORMAT="csr", KS_SPMV_PTR64=p64)
    # test_sliced_ellpack_is_bit_identical_and_chosen_for_uniform_rows
    add("varcoef", both)
    add("varcoef", both, KS_SPMV_FORMAT="csr")
    add("ragged", both)
    add("ragged", both, KS_SPMV_FORMAT="csr")
    for fmt, sigma in (("sell", 1), ("sell", 256), ("sellvi", 1), ("sellvi", 640)):
        add("ragged", both, KS_SPMV_FORMAT=fmt, KS_SELL_SIGMA=sigma)
    add("ragged", both, KS_SPMV_FORMAT="sellvi", KS_SELL_SIGMA=640, KS_SPMV_PTR64=1)
    # test_dvi_rows_per_thread_variants_bit_identical
    for shape in ("37x41x43", "5x3x2", "300x7x1"):
        add("laplace:" + shape, (f64,), KS_SPMV_FORMAT="csr")
        for rpt in (1, 2, 4):
            add("laplace:" + shape, (f64,), KS_SPMV_FORMAT="dvi", KS_DVI_RPT=rpt)
        add("laplace:" + shape, (f64,), KS_SPMV_FORMAT="sellvi", KS_DVI_RPT=1)
        add("laplace:" + shape, (f64,), KS_SPMV_FORMAT="stencil", KS_DVI_RPT=1)
    # test_solver_end_to_end_on_each_layout; ComplexF64 beside it: one case per layout
    add("laplace:14x15x16", both)
    for fmt in ("stencil", "dvi", "vi", "csr", "sell", "sellvi"):
        add("laplace:14x15x16", both, KS_SPMV_FORMAT=fmt)
    # test_stencil_mask_layout
    add("stencil19", both)
    add("stencil19", both, KS_SPMV_FORMAT="csr")
    add("laplace:6x5x4", both)
    add("opposite", both)
    add("opposite", both, KS_SPMV_FORMAT="stencil")  # refused: KS_ERR_ARGUMENT
    add("banded33", both)
    # test_column_blocked_csr_is_bit_identical
    for nb in (0, 2, 3, 5):
        add("colblock", both, KS_SPMV_FORMAT="csr", KS_SPMV_COLBLOCKS=nb)
    for nb in (2, 5, 8):
        for rpt in (1, 2, 4, 8, 16):
            add("colblock", both, KS_SPMV_FORMAT="csr", KS_SPMV_COLBLOCKS=nb, KS_SPMV_CB_RPT=rpt)
        add("colblock", both, KS_SPMV_FORMAT="csr", KS_SPMV_COLBLOCKS=nb, KS_SPMV_CB_SINGLE=0)
    add("colblock-reversed", both, KS_SPMV_FORMAT="csr", KS_SPMV_COLBLOCKS=2)
    add("hashed1e6", (f64,))
    add("hashed1e6", (f64,), KS_SPMV_COLBLOCKS=0)
    add("banded1e6", (f64,))
    # test_marching_forms_of_the_stencil_product_are_bit_identical
    for grid in ("182x182x9", "181x182x10", "256x128x8", "64x64x70"):
        add("laplace:" + grid, (f64,))
        add("laplace:" + grid, (f64,), KS_SPMV_FORMAT="csr")
    # the headline Laplacian at a small grid; BASELINE config 3 (hashed columns) and config 5 (Laplacian slabs) at small sizes
    add("laplace:48x48x48", (f64,))
    add("hashed:50000", both)
    add("hashed:50000", both, KS_SPMV_COLBLOCKS=4)
    for rank in (0, 1, 2):
        add("slab:24x24x24/3/%d" % rank, both)
        add("slab:24x24x24/3/%d" % rank, both, KS_SPMV_FORMAT="csr", KS_SPMV_COLBLOCKS=4)
    return out


CASES = _cases()


def case_id(c):
    return "%s|%s|%s" % (c["matrix"], c["dtype"], ",".join("%s=%s" % kv for kv in sorted(c["env"].items())))
