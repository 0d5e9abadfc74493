"""`-m "not gpu"`: what a distributed row block exchanges with its neighbours (csrc/ks_halo_plan.hpp) through ks_host_halo_plan --
the plan ks_operator_csr_dist uploads, made without a device.  The expected values come from `reference` below, written from the
definitions (loops over rows and lists), never from the library.  The peer-to-peer table and the inputs that used to be read out
of bounds also run in a stand-alone host program under the address and undefined-behaviour sanitizers (tests/halo_plan_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import ROOT, import_package
from oracle.matrices import laplace3d

pkg = import_package()
from arnoldimethod_jl_amd import dist as ksd  # noqa: E402  (registered by import_package)

_lib = pkg._lib
FACTS = ("nlow", "ghost_lo_end", "ghost_hi_begin", "nscatter")  # KS_HALO_* of include/kschur.h


def _arr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return None if a is None else a.ctypes.data


def halo_plan(ptr, idx, n, nghost, rank, neigh, send_ptr, send_idx, recv_cnt, elem=8, p2p=False, nneigh=None):
    """ks_host_halo_plan; an array given as None goes in as a null pointer.  Returns the plan, or (code, message)."""
    L = _lib.load()
    ptr, idx = _arr(ptr, np.int64), _arr(idx, np.int32)
    neigh, send_ptr, send_idx, recv_cnt = _arr(neigh, np.int32), _arr(send_ptr, np.int64), _arr(send_idx, np.int32), _arr(recv_cnt, np.int64)
    nn = nneigh if nneigh is not None else len(neigh)
    cap = 0 if send_idx is None else len(send_idx)
    facts, ghost = np.full(len(FACTS), -7, dtype=np.int64), np.full(2, -7, dtype=np.int64)
    recv_ptr, send_first, pack_ptr = (np.full(max(nn, 0) + k, -7, dtype=np.int64) for k in (1, 0, 1))
    packed = np.full(cap, -7, dtype=np.int32)
    rc = L.ks_host_halo_plan(n, nghost, len(idx), _ptr(ptr), _ptr(idx), nn, _ptr(neigh), _ptr(send_ptr), _ptr(send_idx), _ptr(recv_cnt), rank, elem,
                             _ptr(facts), _ptr(recv_ptr), _ptr(send_first), _ptr(pack_ptr), _ptr(packed), cap, _ptr(ghost) if p2p else None)
    if rc != 0:
        return rc, L.ks_last_error_string().decode()
    out = dict(zip(FACTS, (int(v) for v in facts)), recv_ptr=recv_ptr.tolist(), send_first=send_first.tolist(), pack_ptr=pack_ptr.tolist())
    out["packed"] = packed[:out["nscatter"]].tolist()
    if p2p:
        out.update(ghost_stride=int(ghost[0]), arena_bytes=int(ghost[1]))
    return out


def reference(ptr, idx, n, rank, neigh, send_ptr, send_idx, recv_cnt):
    """The definitions, one loop each."""
    nlow, not_lower_seen, ascending = 0, False, True
    for p, q in enumerate(neigh):
        if q < rank:
            ascending = ascending and not not_lower_seen
            nlow += int(recv_cnt[p])
        else:
            not_lower_seen = True   # (a self exchange counts as not lower)
    touching = [r for r in range(n) if any(c >= n for c in idx[ptr[r]:ptr[r + 1]])]
    if touching:
        gaps = [(0, touching[0])] + [(a + 1, b) for a, b in zip(touching, touching[1:])]
        best = gaps[0]
        for g in gaps[1:]:
            if g[1] - g[0] > best[1] - best[0]:   # the first gap strictly longer than every earlier one
                best = g
        if n - (touching[-1] + 1) > best[1] - best[0]:
            best = (touching[-1] + 1, n)
    else:
        best = (0, n)
    recv_ptr, send_first, pack_ptr, packed = [0], [], [0], []
    for p in range(len(neigh)):
        recv_ptr.append(recv_ptr[-1] + int(recv_cnt[p]))
        lst = [int(v) for v in send_idx[send_ptr[p]:send_ptr[p + 1]]]
        if lst and all(lst[k] == lst[k - 1] + 1 for k in range(1, len(lst))):
            send_first.append(lst[0])
        else:
            send_first.append(-1)
            packed += lst
        pack_ptr.append(len(packed))
    return dict(nlow=nlow if ascending else -1, ghost_lo_end=best[0], ghost_hi_begin=best[1], nscatter=len(packed), recv_ptr=recv_ptr,
                send_first=send_first, pack_ptr=pack_ptr, packed=packed)


def check(ptr, idx, n, nghost, rank, neigh, send_ptr, send_idx, recv_cnt):
    got = halo_plan(ptr, idx, n, nghost, rank, neigh, send_ptr, send_idx, recv_cnt)
    assert got == reference(ptr, idx, n, rank, neigh, send_ptr, send_idx, recv_cnt)
    return got


def diag_block(n, touching, nghost):
    """n rows with their diagonal; the rows in `touching` also read ghost column n + (row mod nghost)."""
    ptr, idx = [0], []
    for r in range(n):
        idx.append(r)
        if r in touching:
            idx.append(n + r % nghost)
        ptr.append(len(idx))
    return np.array(ptr), np.array(idx)


# ---------------------------------------------------------------------------------------------- plans
def test_slab_laplacian_over_three_ranks():
    """5 x 5 x 15 in slabs of five planes: every send list is one plane (in place, nothing packed), the interior is what lies between
    a slab's first and last plane, and the ghost slots of the lower neighbour come first."""
    m, world = 5, 3
    offs = ksd.partition_rows(m * m * 3 * m, world, granule=m * m)
    assert offs.tolist() == [0, 125, 250, 375]
    blocks = [pkg.matrices.laplace3d_csr(m, m, 3 * m, int(offs[r]), int(offs[r + 1]), index_dtype=np.int64) for r in range(world)]
    needs = []
    for r in range(world):
        ix = blocks[r][1]
        g = np.unique(ix[(ix < offs[r]) | (ix >= offs[r + 1])])
        owner = np.searchsorted(offs, g, side="right") - 1
        needs.append([g[owner == q] for q in range(world)])
    want = [dict(nlow=0, ghost_lo_end=0, ghost_hi_begin=100), dict(nlow=25, ghost_lo_end=25, ghost_hi_begin=100), dict(nlow=25, ghost_lo_end=25, ghost_hi_begin=125)]
    for r in range(world):
        pl = ksd.build_halo_plan(blocks[r][1], offs, r, exchange=lambda need: needs)
        got = check(blocks[r][0], pl.colidx_local, pl.n_local, pl.nghost, r, pl.neigh, pl.send_ptr, pl.send_idx, pl.recv_cnt)
        assert {k: got[k] for k in want[r]} == want[r]
        assert all(f >= 0 for f in got["send_first"]) and got["nscatter"] == 0 and got["packed"] == []
    assert got["nlow"] == pl.nghost == 25


@pytest.mark.parametrize("pattern", ["contiguous", "scattered"])
def test_self_exchanges_of_the_single_rank_collective_test(pattern):
    """The two plans of test_gpu_parity.py::test_collective_path_single_rank (6 x 7 x 8, a periodic closure through ghosts this very
    rank fills): all rows in order go out as ONE in-place run, the list of odd rows is packed whole."""
    A = laplace3d(6, 7, 8).tocsr()
    n = A.shape[0]
    extra = (np.arange(n) + n // 2) % n if pattern == "contiguous" else ((np.arange(n) * 7 + 3) % n) | 1
    ghosts = np.unique(extra)
    ptr, idx = [0], []
    for i in range(n):
        idx += A.indices[A.indptr[i]:A.indptr[i + 1]].tolist() + [n + int(np.searchsorted(ghosts, extra[i]))]
        ptr.append(len(idx))
    got = check(np.array(ptr), np.array(idx), n, len(ghosts), 0, [0], [0, len(ghosts)], ghosts, [len(ghosts)])
    assert got["nlow"] == 0 and got["ghost_lo_end"] == got["ghost_hi_begin"]   # (a self exchange is not lower; every row reads a ghost)
    if pattern == "contiguous":
        assert got["send_first"] == [0] and got["nscatter"] == 0 and got["pack_ptr"] == [0, 0]
    else:
        assert got["send_first"] == [-1] and got["nscatter"] == len(ghosts) and got["packed"] == ghosts.tolist() and got["pack_ptr"] == [0, len(ghosts)]


def test_mixed_plan_entry_by_entry():
    """A consecutive list, a scattered one, and a neighbour that is sent nothing but fills three ghost slots."""
    ptr, idx = diag_block(12, {0, 11}, 6)
    got = check(ptr, idx, 12, 6, 1, [0, 2, 3], [0, 3, 6, 6], [3, 4, 5, 1, 7, 8], [2, 1, 3])
    assert got == dict(nlow=2, ghost_lo_end=1, ghost_hi_begin=11, nscatter=3, recv_ptr=[0, 2, 3, 6], send_first=[3, -1, -1], pack_ptr=[0, 0, 3, 3],
                       packed=[1, 7, 8])


def test_lower_neighbour_after_a_higher_one():
    ptr, idx = diag_block(12, {0, 11}, 6)
    assert check(ptr, idx, 12, 6, 1, [2, 0], [0, 1, 2], [4, 5], [4, 2])["nlow"] == -1
    assert check(ptr, idx, 12, 6, 1, [1, 0], [0, 1, 2], [4, 5], [4, 2])["nlow"] == -1   # (a self exchange is not lower either)
    assert check(ptr, idx, 12, 6, 1, [0, 2], [0, 1, 2], [4, 5], [4, 2])["nlow"] == 4


def test_no_neighbours():
    ptr, idx = diag_block(11, set(), 1)
    got = halo_plan(ptr, idx, 11, 0, 0, None, None, None, None, nneigh=0)
    assert got == dict(nlow=0, ghost_lo_end=0, ghost_hi_begin=11, nscatter=0, recv_ptr=[0], send_first=[], pack_ptr=[0], packed=[])


@pytest.mark.parametrize("touching, want", [((), (0, 11)), ((0,), (1, 11)), ((10,), (0, 10)), ((0, 5, 10), (1, 5)), (tuple(range(11)), None),
                                            ((3, 4), (5, 11)), ((2, 8), (3, 8)), ((4, 6), (0, 4))])
def test_interior_interval_of_eleven_rows(touching, want):
    """The edge cases of the interval: no touching row, the first, the last, two gaps of four (the first wins), every row (empty); and
    a trailing gap that is strictly longer, a middle gap that is, a trailing gap of the same length as the leading one (the leading
    one stays)."""
    ptr, idx = diag_block(11, set(touching), 2)
    got = check(ptr, idx, 11, 2, 0, [1], [0, 0], [], [2])
    if want is None:
        assert got["ghost_lo_end"] == got["ghost_hi_begin"]
    else:
        assert (got["ghost_lo_end"], got["ghost_hi_begin"]) == want


@pytest.mark.parametrize("elem", [8, 16])
@pytest.mark.parametrize("nghost", [0, 1, 32, 33])
def test_ghost_stride_and_arena_bytes(nghost, elem):
    """Peer-to-peer transport: the two ghost slots lie round_up(max(nghost, 1), 32) elements apart and take
    round_up(2 stride elem, 256) bytes of the shared arena."""
    ptr, idx = diag_block(11, set(), 1)
    got = halo_plan(ptr, idx, 11, nghost, 0, [1], [0, 0], [], [nghost], elem=elem, p2p=True)
    stride = -(-max(nghost, 1) // 32) * 32
    assert got["ghost_stride"] == stride == {0: 32, 1: 32, 32: 32, 33: 64}[nghost]
    assert got["arena_bytes"] == -(-2 * stride * elem // 256) * 256


# ---------------------------------------------------------------------------------------------- refusals
GOOD = dict(rank=1, nneigh=2, neigh=[0, 2], send_ptr=[0, 3, 6], send_idx=[3, 4, 5, 1, 7, 8], recv_cnt=[2, 4])
ERRORS = [
    ("recv_cnt", [7, -1], "negative receive count"),
    ("recv_cnt", [2, 3], "recv counts do not add up to nghost"),
    ("send_idx", [3, 4, 5, 1, 7, 12], "send index out of range"),
    ("send_idx", [3, 4, 5, -1, 7, 8], "send index out of range"),
    # inputs that used to be read out of bounds
    ("nneigh", -1, "negative neighbour count"),
    ("neigh", None, "null halo plan array"),
    ("send_ptr", None, "null halo plan array"),
    ("recv_cnt", None, "null halo plan array"),
    ("send_idx", None, "null send index array"),
    ("send_ptr", [2, 3, 6], "send pointer does not start at 0"),
    ("send_ptr", [0, 4, 3], "send pointer is not monotone"),
    # the row block itself: the checks ks_operator_csr_dist makes on its CSR arrays
    ("ptr", None, "null argument"),
    ("ptr", [1] + list(range(2, 13)) + [14], "row pointer does not match nnz"),
    ("ptr", [0, 3, 2] + list(range(3, 12)) + [14], "pointer array is not monotone within [0, nnz]"),
    ("idx", [0, 18] + list(range(1, 12)) + [17], "local-extended column index out of range"),
    ("n", 2 ** 31 - 1, "local-extended column range must fit int32"),
    ("elem", 4, "element size must be 8 or 16"),
]


@pytest.mark.parametrize("field, value, message", ERRORS, ids=[f"{f}-{m.replace(' ', '_')}" for f, _, m in ERRORS])
def test_one_faulty_argument(field, value, message):
    ptr, idx = diag_block(12, {0, 11}, 6)
    args = dict(GOOD, ptr=ptr, idx=idx, n=12, nghost=6)
    assert isinstance(halo_plan(**args), dict)
    args[field] = value
    assert halo_plan(**args) == (_lib.KS_ERR_ARGUMENT, message)


def test_seventeen_neighbours_only_refused_for_the_peer_to_peer_transport():
    ptr, idx = diag_block(12, set(), 1)
    args = dict(ptr=ptr, idx=idx, n=12, nghost=0, rank=0, neigh=list(range(1, 18)), send_ptr=[0] * 18, send_idx=[], recv_cnt=[0] * 17)
    assert halo_plan(**args)["send_first"] == [-1] * 17
    assert halo_plan(**args, p2p=True) == (_lib.KS_ERR_ARGUMENT, "peer-to-peer halo supports at most 16 neighbours per rank")


# ---------------------------------------------------------------------------------------------- the header on its own
def _host_compiler():
    for cand in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        cc = shutil.which(cand)
        if cc:
            return cc
    return None


def test_plan_header_alone_under_the_sanitizers(tmp_path):
    """csrc/ks_halo_plan.hpp with a plain host compiler (no HIP), address and undefined-behaviour sanitizers on: the mixed plan, the
    malformed inputs (each array on the heap at its exact size), the peer-to-peer table of two and three ranks with its "plans
    disagree" message, the neighbour limit and the "bad neighbour rank" check, which need a rank count ks_host_halo_plan is not given."""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++, c++, clang++) found")
    exe = str(tmp_path / "halo_plan_check")
    src = os.path.join(ROOT, "tests", "halo_plan_check.cpp")
    # (GCC links the sanitizer runtimes as shared libraries unless told otherwise, and a shared ASan runtime refuses to start behind
    # any other preloaded library; clang links them statically)
    gnu = "clang" not in subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    b = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                       + (["-static-libasan", "-static-libubsan"] if gnu else []) + [src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HALO_PLAN_CHECK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
