#!/usr/bin/env python
"""Uploads every case of tests/layout_cases.py on the GPU and writes what ks_operator_format reports (layout, ndict,
bytes_per_nnz; an upload that is refused records its error code) as JSON -- tests/golden/csr_layout_plans.json is the output
of this script.  With --check FILE it compares against an existing record instead and exits 1 on any difference.

    python tools/record_csr_layout_plans.py OUT.json
    python tools/record_csr_layout_plans.py --check tests/golden/csr_layout_plans.json"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from __graft_entry__ import import_package  # noqa: E402
import layout_cases as lc  # noqa: E402

pkg = import_package()
_lib = pkg._lib


def upload(ctx, M, dtype, ctxs):
    """ks_operator_csr / ks_operator_csr_dist on the arrays of layout_cases.matrix(); returns (rc, handle)."""
    L = _lib.load()
    code = _lib.KS_C64 if np.dtype(dtype).kind == "c" else _lib.KS_F64
    h = C.c_void_p()
    val = np.ascontiguousarray(M["val"], dtype=dtype)
    if M["nghost"] < 0:
        rc = L.ks_operator_csr(ctx._h, M["n"], M["n"], len(val), M["ptr"].ctypes.data, M["idx"].ctypes.data, val.ctypes.data,
                               _lib.KS_CSR, 0, _lib.KS_I64, code, C.byref(h))
        return rc, h, ctx
    # a row block of a distributed operator: one context per (rank, world) with a host transport that is never called
    offsets, rank = M["offsets"], M["rank"]
    world = len(offsets) - 1
    if (rank, world) not in ctxs:
        ctxs[(rank, world)] = pkg.Context(0, rank=rank, nranks=world, hostcomm=(lambda buf: None, lambda peers, send, recv: None))
    dctx = ctxs[(rank, world)]
    gg = M["ghost_global"]
    owner = np.searchsorted(offsets, gg, side="right") - 1
    r0, r1 = int(offsets[rank]), int(offsets[rank + 1])
    neigh, send_ptr, send_idx, recv_cnt = [], [0], [], []
    for q in range(world):
        if q == rank:
            continue
        other = lc.matrix(_key_of_rank(M, q), dtype)["ghost_global"]
        mine = other[(other >= r0) & (other < r1)] - r0
        cnt = int((owner == q).sum())
        if len(mine) or cnt:
            neigh.append(q)
            send_idx.append(mine.astype(np.int32))
            send_ptr.append(send_ptr[-1] + len(mine))
            recv_cnt.append(cnt)
    neigh = np.asarray(neigh, dtype=np.int32)
    send_ptr = np.asarray(send_ptr, dtype=np.int64)
    send_idx = np.concatenate(send_idx).astype(np.int32) if send_idx else np.zeros(0, dtype=np.int32)
    recv_cnt = np.asarray(recv_cnt, dtype=np.int64)
    col = M["idx"].astype(np.int32)
    rc = L.ks_operator_csr_dist(dctx._h, M["n"], M["nghost"], len(val), M["ptr"].ctypes.data, col.ctypes.data, val.ctypes.data, code,
                                len(neigh), neigh.ctypes.data, send_ptr.ctypes.data, send_idx.ctypes.data, recv_cnt.ctypes.data, C.byref(h))
    return rc, h, dctx


def _key_of_rank(M, q):
    return M["key"].rsplit("/", 1)[0] + "/%d" % q


def record():
    out = {}
    ctx = pkg.default_context()
    ctxs = {}
    for c in lc.CASES:
        for k in lc.LAYOUT_ENV:
            os.environ.pop(k, None)
        os.environ.update(c["env"])
        M = dict(lc.matrix(c["matrix"], c["dtype"]), key=c["matrix"])
        rc, h, octx = upload(ctx, M, np.dtype(c["dtype"]), ctxs)
        if rc != 0:
            out[lc.case_id(c)] = {"error": rc}
            continue
        op = pkg.Operator(octx, h, (M["n"], M["n"]), np.dtype(c["dtype"]))
        out[lc.case_id(c)] = op.format
        op.close()
        print(lc.case_id(c), out[lc.case_id(c)], flush=True)
    return out


if __name__ == "__main__":
    got = record()
    if sys.argv[1] == "--check":
        want = json.load(open(sys.argv[2]))
        bad = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
        for k in bad:
            print("DIFFERS", k, want.get(k), got.get(k))
        print("csr layout record: %d cases, %d differ" % (len(want), len(bad)))
        sys.exit(1 if bad else 0)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d cases" % len(got))
