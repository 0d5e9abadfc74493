"""Host-side mirror of the reference's public interface for the accelerated path:

    partialschur(A; v1, nev, which, tol, mindim, maxdim, restarts)      src/run.jl:100-129
    partialschur!(A, arnoldi; start_from, initialize, ...)               src/run.jl:152-179
    partialeigen(P)                                                      src/eigvals.jl:92-95
    ArnoldiWorkspace(n, k) / (v1, k)                                     src/ArnoldiMethod.jl:41-93
    PartialSchur, History, targets LM/LR/SR/LI/SI                        src/ArnoldiMethod.jl:130-137,
                                                                         src/run.jl:217-222, src/targets.jl

Same names, argument meaning and error behaviour (ArgumentError / DimensionMismatch) so that the
parity tests read like the reference's own tests.  Julia is not available in the build image, so
this Python layer (ctypes over the C ABI of include/kschur.h) stands in for the Julia glue that is
shipped, untested, in julia/KrylovSchurHIP.jl.  All n-sized arithmetic happens in libkschur_hip.so
on the GPU; this file only validates arguments and moves small host arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import ArgumentError, DimensionMismatch, check

EPS = float(np.finfo(np.float64).eps)
DEFAULT_SEED = 20240917


# ------------------------------------------------------------------ targets (src/targets.jl:7-32)
class Target:
    name = "LM"

    def __repr__(self):
        return f"{self.name}()"


class LM(Target):
    name = "LM"


class LR(Target):
    name = "LR"


class SR(Target):
    name = "SR"


class LI(Target):
    name = "LI"


class SI(Target):
    name = "SI"


def _which_code(which) -> int:
    """_symbol_to_target, src/run.jl:181-185."""
    if isinstance(which, Target):
        return _lib.WHICH[which.name]
    if isinstance(which, type) and issubclass(which, Target):
        return _lib.WHICH[which.name]
    if isinstance(which, str):
        s = which.lstrip(":")
        if s in _lib.WHICH:
            return _lib.WHICH[s]
    raise ArgumentError(f"Unknown target: {which}")


def vtype(A):
    """src/run.jl:9-12."""
    dt = np.dtype(getattr(A, "dtype", np.float64))
    return np.complex128 if dt.kind == "c" else np.float64


def _dtype_code(dt) -> int:
    return _lib.KS_C64 if np.dtype(dt).kind == "c" else _lib.KS_F64


# ------------------------------------------------------------------ context
class Context:
    """One GPU (+ optionally one rank of a multi-GPU job: RCCL communicator or peer-to-peer regions)."""

    def __init__(self, device: int = 0, rank: int = 0, nranks: int = 1, unique_id: bytes | None = None, p2p: bool = False,
                 hostcomm=None):
        """`hostcomm = (allreduce(buf: np.ndarray) -> None, exchange(peers, sendbufs, recvbufs) -> None)` selects the
        host-staged transport (ks_ctx_create_hostcomm): numpy views of the pinned staging buffers are handed to the
        two callables, which must sum `buf` in place over all ranks / fill `recvbufs[i]` from rank `peers[i]`."""
        L = _lib.load()
        h = C.c_void_p()
        self._keep = ()
        if hostcomm is not None:
            allreduce, exchange = hostcomm
            errs = []

            def _ar(_user, buf, count):
                try:
                    allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                    return 0
                except Exception as e:  # noqa: BLE001 - must not propagate through C
                    errs.append(e)
                    return 1

            def _ex(_user, npeers, peers, sbufs, sbytes, rbufs, rbytes):
                try:
                    pl = [int(peers[i]) for i in range(npeers)]
                    sb = [np.ctypeslib.as_array(C.cast(sbufs[i], C.POINTER(C.c_uint8)), shape=(int(sbytes[i]),)) if sbytes[i] else np.zeros(0, np.uint8)
                          for i in range(npeers)]
                    rb = [np.ctypeslib.as_array(C.cast(rbufs[i], C.POINTER(C.c_uint8)), shape=(int(rbytes[i]),)) if rbytes[i] else np.zeros(0, np.uint8)
                          for i in range(npeers)]
                    exchange(pl, sb, rb)
                    return 0
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
                    return 1

            cb1, cb2 = _lib.HOST_ALLREDUCE_FN(_ar), _lib.HOST_EXCHANGE_FN(_ex)
            self._keep = (cb1, cb2, errs)
            self.comm_errors = errs
            check(L.ks_ctx_create_hostcomm(device, rank, nranks, cb1, cb2, None, C.byref(h)))
        elif p2p:
            check(L.ks_ctx_create_p2p(device, rank, nranks, C.byref(h)))
        elif nranks > 1 or unique_id is not None:
            assert unique_id is not None and len(unique_id) == 128
            buf = C.create_string_buffer(unique_id, 128)
            check(L.ks_ctx_create_dist(device, rank, nranks, buf, C.byref(h)))
        else:
            check(L.ks_ctx_create(device, C.byref(h)))
        self._h = h
        self.device, self.rank, self.nranks = device, rank, nranks

    # peer-to-peer transport: export this rank's region handle / map everybody else's (include/kschur.h)
    def p2p_handle(self) -> bytes:
        buf = C.create_string_buffer(64)
        check(_lib.load().ks_ctx_p2p_handle(self._h, buf))
        return buf.raw

    def p2p_attach(self, handles: list[bytes]):
        assert len(handles) == self.nranks and all(len(x) == 64 for x in handles)
        buf = C.create_string_buffer(b"".join(handles), 64 * self.nranks)
        check(_lib.load().ks_ctx_p2p_attach(self._h, buf))

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(_lib.load().ks_comm_unique_id(buf))
        return buf.raw

    def synchronize(self):
        check(_lib.load().ks_ctx_synchronize(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        check(_lib.load().ks_ctx_stream(self._h, C.byref(s)))
        return s.value or 0

    # per-kernel-class HIP-event timing (bench.py)
    PROFILE_CLASSES = ("spmv", "dots", "axpy", "scale", "rotate", "fin", "fused")

    def profile_enable(self, on: bool = True):
        check(_lib.load().ks_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        check(_lib.load().ks_profile_reset(self._h))

    def profile_get(self) -> dict:
        n = len(self.PROFILE_CLASSES)
        ms, by, cnt = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
        check(_lib.load().ks_profile_get(self._h, n, ms.ctypes.data, by.ctypes.data, cnt.ctypes.data))
        return {k: dict(ms=float(ms[i]), bytes=float(by[i]), count=int(cnt[i])) for i, k in enumerate(self.PROFILE_CLASSES)}

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().ks_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ------------------------------------------------------------------ operators
class Operator:
    """Anything with mul!(y, A, x), eltype, size (src/run.jl:21-22)."""

    def __init__(self, ctx, handle, shape, dtype, keep=()):
        self.ctx, self._h, self.shape, self.dtype, self._keep = ctx, handle, shape, np.dtype(dtype), keep

    @property
    def format(self) -> dict:
        """Device layout of a stored matrix: bytes streamed per non-zero and dictionary size (0 = plain CSR)."""
        b, d, lay = C.c_double(), C.c_int(), C.c_int()
        check(_lib.load().ks_operator_format(self._h, C.byref(b), C.byref(d), C.byref(lay)))
        return dict(bytes_per_nnz=b.value, ndict=d.value, layout=_lib.LAYOUTS.get(lay.value, "?"))

    @property
    def chebyshev_info(self) -> dict:
        """Degree and intermediate vectors of a `chebyshev_operator` (0 / 0 for any other operator), and the Clenshaw steps this
        operator has run since its creation by the path they took: `fused_steps` in the product's own launch, `generic_steps` as
        the product plus one streaming pass (`ks_operator_chebyshev_info`)."""
        d, t, f, g = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        check(_lib.load().ks_operator_chebyshev_info(self._h, C.byref(d), C.byref(t), C.byref(f), C.byref(g)))
        return dict(degree=d.value, temporaries=t.value, fused_steps=f.value, generic_steps=g.value)

    @property
    def cg_info(self) -> dict:
        """Counters of a `cg_operator` since its creation (`ks_operator_cg_info`; ArgumentError for any other operator): solves,
        iterations of all of them, iterations and the recurrence's relative residual sqrt(rho' / rho0) of the last solve, and the
        largest such residual of any solve."""
        a, it, last = C.c_int64(), C.c_int64(), C.c_int()
        rel, worst = C.c_double(), C.c_double()
        check(_lib.load().ks_operator_cg_info(self._h, C.byref(a), C.byref(it), C.byref(last), C.byref(rel), C.byref(worst)))
        return dict(applications=a.value, iterations=it.value, last_iterations=last.value, last_relres=rel.value, worst_relres=worst.value)

    @property
    def pcg_info(self) -> dict:
        """Counters of a `pcg_operator` since its creation (`ks_operator_pcg_info`; ArgumentError for any other operator): the
        fields of `cg_info`, `preconditioner_applications` (generic path: launches of M, those behind the end of a solve inside a
        chunk included; Jacobi path: one per solve and one per iteration) and `path`, "jacobi" or "generic"."""
        a, it, last, pa, path = C.c_int64(), C.c_int64(), C.c_int(), C.c_int64(), C.c_int()
        rel, worst = C.c_double(), C.c_double()
        check(_lib.load().ks_operator_pcg_info(self._h, C.byref(a), C.byref(it), C.byref(last), C.byref(rel), C.byref(worst), C.byref(pa),
                                               C.byref(path)))
        return dict(applications=a.value, iterations=it.value, last_iterations=last.value, last_relres=rel.value, worst_relres=worst.value,
                    preconditioner_applications=pa.value, path="jacobi" if path.value == _lib.KS_PCG_PATH_JACOBI else "generic")

    @property
    def multigrid_info(self) -> dict:
        """Counters of a `multigrid_operator` since its creation (`ks_operator_multigrid_info`; ArgumentError for any other
        operator): `levels`, the `rows` of every level, `applications`, `level_products` (per smoothed level the products with its
        operator: 2 degree per application) and `coarse_applications`."""
        n, a = C.c_int(), C.c_int64()
        rows, prod = np.zeros(16, dtype=np.int64), np.zeros(16, dtype=np.int64)
        check(_lib.load().ks_operator_multigrid_info(self._h, C.byref(n), rows.ctypes.data, C.byref(a), prod.ctypes.data))
        nl = n.value
        return dict(levels=nl, rows=tuple(int(r) for r in rows[:nl]), applications=a.value,
                    level_products=tuple(int(p) for p in prod[:nl - 1]), coarse_applications=int(prod[nl - 1]))

    @property
    def minres_info(self) -> dict:
        """Counters of a `minres_operator` since its creation (`ks_operator_minres_info`; ArgumentError for any other operator):
        solves, iterations of all of them, iterations and the recurrence's relative residual |phibar| / ||b|| of the last solve, and
        the largest such residual of any solve."""
        a, it, last = C.c_int64(), C.c_int64(), C.c_int()
        rel, worst = C.c_double(), C.c_double()
        check(_lib.load().ks_operator_minres_info(self._h, C.byref(a), C.byref(it), C.byref(last), C.byref(rel), C.byref(worst)))
        return dict(applications=a.value, iterations=it.value, last_iterations=last.value, last_relres=rel.value, worst_relres=worst.value)

    @property
    def bicgstab_info(self) -> dict:
        """Counters of a `bicgstab_operator` since its creation (`ks_operator_bicgstab_info`; ArgumentError for any other operator):
        solves, iterations of all of them (four products each), iterations and the recurrence's relative residual ||r0|| / ||b|| of
        the last solve, and the largest such residual of any solve."""
        a, it, last = C.c_int64(), C.c_int64(), C.c_int()
        rel, worst = C.c_double(), C.c_double()
        check(_lib.load().ks_operator_bicgstab_info(self._h, C.byref(a), C.byref(it), C.byref(last), C.byref(rel), C.byref(worst)))
        return dict(applications=a.value, iterations=it.value, last_iterations=last.value, last_relres=rel.value, worst_relres=worst.value)

    def close(self):
        # never touch a handle whose context is already gone (interpreter shutdown order is arbitrary)
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            _lib.load().ks_operator_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_op(rc: int, op):
    """`check(rc)` for calls that may run a Python operator callback: an exception raised inside the callback
    cannot cross the C ABI (the callback returns 1 -> KS_ERR_OPERATOR); re-raise THAT exception here instead
    of the generic library error, chained to it."""
    errs = getattr(op, "errors", None)
    if errs:
        e = errs.pop(0)
        del errs[:]
        try:
            check(rc)
        except Exception as lib_err:  # noqa: BLE001
            raise e from lib_err
        raise e
    check(rc)


def csr_operator(A, ctx: Context | None = None) -> Operator:
    """Device CSR operand from a scipy.sparse matrix (CSR or CSC; CSC is what Julia hands over) or a
    dense ndarray.  Integer/bool matrices are promoted like `vtype` does (test/partial_schur.jl:41-45)."""
    import scipy.sparse as sp

    ctx = ctx or default_context()
    L = _lib.load()
    shp = A.shape
    if len(shp) != 2 or shp[0] != shp[1]:
        raise DimensionMismatch(f"matrix is not square: dimensions are {tuple(shp)}")
    dt = vtype(A)
    if sp.issparse(A):
        if A.format == "csc":
            M, layout = A, _lib.KS_CSC
        else:
            M, layout = A.tocsr(), _lib.KS_CSR
    else:
        M, layout = sp.csr_matrix(np.asarray(A)), _lib.KS_CSR
    ptr = np.ascontiguousarray(M.indptr)
    idx = np.ascontiguousarray(M.indices)
    if ptr.dtype != idx.dtype:
        ptr = ptr.astype(np.int64)
        idx = idx.astype(np.int64)
    itype = _lib.KS_I64 if ptr.dtype == np.int64 else _lib.KS_I32
    if ptr.dtype not in (np.int32, np.int64):
        ptr, idx, itype = ptr.astype(np.int64), idx.astype(np.int64), _lib.KS_I64
    val = np.ascontiguousarray(M.data.astype(dt))
    h = C.c_void_p()
    check(
        L.ks_operator_csr(
            ctx._h, shp[0], shp[1], M.nnz, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data if M.nnz else None,
            layout, 0, itype, _dtype_code(dt), C.byref(h),
        )
    )
    return Operator(ctx, h, tuple(shp), dt)


def lu_operator(L, U, perm_in=None, perm_out=None, scale=None, ctx: Context | None = None) -> Operator:
    """y = P_out U^-1 L^-1 P_in (scale o x) with both sparse triangular solves on the device (`ks_operator_lu`): the
    `ldiv!(y, F, x)` of the LinearMap a user of the reference wraps around a host factorisation
    (docs/src/index.md:246-249).  `L`, `U`: scipy.sparse triangular factors (any format; converted to CSR here),
    `perm_in[i]` = the entry of x that becomes row i of the triangular system, `perm_out[i]` = the entry of y that
    receives solution entry i.  See `splu_operator` for the SuperLU convention."""
    import scipy.sparse as sp

    ctx = ctx or default_context()
    lib = _lib.load()
    n = L.shape[0]
    if L.shape != (n, n) or U.shape != (n, n):
        raise DimensionMismatch(f"factors are not square of one size: {L.shape}, {U.shape}")
    dt = np.dtype(np.complex128 if (L.dtype.kind == "c" or U.dtype.kind == "c") else np.float64)
    arrs = []
    for M in (L, U):
        M = sp.csr_matrix(M)
        M.sort_indices()
        arrs += [np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32),
                 np.ascontiguousarray(M.data, dtype=dt)]
    pin = None if perm_in is None else np.ascontiguousarray(perm_in, dtype=np.int32)
    pout = None if perm_out is None else np.ascontiguousarray(perm_out, dtype=np.int32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    for a, name in ((pin, "perm_in"), (pout, "perm_out"), (sc, "scale")):
        if a is not None and a.shape != (n,):
            raise DimensionMismatch(f"{name} must have {n} entries")
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
    h = C.c_void_p()
    check(lib.ks_operator_lu(ctx._h, n, _dtype_code(dt), arrs[0].ctypes.data, ptr(arrs[1]), ptr(arrs[2]), arrs[3].ctypes.data,
                             ptr(arrs[4]), ptr(arrs[5]), ptr(pin), ptr(pout), ptr(sc), C.byref(h)))
    op = Operator(ctx, h, (n, n), dt)
    v = [C.c_int64() for _ in range(4)]
    check(lib.ks_operator_lu_info(h, *[C.byref(x) for x in v]))
    op.lu_info = dict(nnz_l=v[0].value, nnz_u=v[1].value, levels_l=v[2].value, levels_u=v[3].value)
    for upper, tag in ((0, "l"), (1, "u")):
        w = [C.c_int64() for _ in range(3)]
        g = C.c_int()
        check(lib.ks_operator_lu_layout(h, upper, C.byref(w[0]), C.byref(w[1]), C.byref(w[2]), C.byref(g)))
        op.lu_info.update({f"rows_{tag}": w[0].value, f"run_rows_{tag}": w[1].value, f"top_rows_{tag}": w[2].value, f"groups_{tag}": g.value})
    return op


def splu_operator(lu, ctx: Context | None = None) -> Operator:
    """The device operator x -> A^-1 x from a `scipy.sparse.linalg.splu` factorisation (`Pr A Pc = L U`:
    z[perm_r] = x, L U w = z, y = w[perm_c])."""
    n = lu.shape[0]
    inv_r = np.empty(n, dtype=np.int32)
    inv_r[lu.perm_r] = np.arange(n, dtype=np.int32)
    inv_c = np.empty(n, dtype=np.int32)
    inv_c[lu.perm_c] = np.arange(n, dtype=np.int32)
    return lu_operator(lu.L, lu.U, perm_in=inv_r, perm_out=inv_c, ctx=ctx)


def _tridiag_args(dl, d, du, sigma):
    cplx = any(np.asarray(a).dtype.kind == "c" for a in (dl, d, du)) or isinstance(sigma, (complex, np.complexfloating))
    dt = np.dtype(np.complex128 if cplx else np.float64)
    arrs = [np.ascontiguousarray(a, dtype=dt) for a in (dl, d, du)]
    n = arrs[1].shape[0] if arrs[1].ndim == 1 else -1
    if n < 0 or arrs[0].shape != (max(n - 1, 0),) or arrs[2].shape != (max(n - 1, 0),):
        raise DimensionMismatch(f"d must be a vector of n entries, dl and du of n - 1: {[a.shape for a in arrs]}")
    sg = complex(sigma)
    return dt, n, arrs, sg.real, sg.imag


def tridiagonal_solve_operator(dl, d, du, sigma=0.0, ctx: Context | None = None, block_rows: int = 0) -> Operator:
    """y = (T - sigma I)^-1 x for the tridiagonal T with sub-/main/super-diagonals dl (n-1), d (n), du (n-1): the
    `ldiv!(y, F, x)` of the reference's shift-invert recipe (docs/src/index.md:234-259) on a 1-D operator, as a LIBRARY
    operator (`ks_operator_tridiag_solve`): factored once on the host at upload (recursive separator elimination, pivoted LU
    per block of `block_rows` rows, 0 = 64), applied by the library's own kernels with every vector resident in HBM.  The
    eigenvalues of T closest to sigma are sigma + 1/theta for the largest-magnitude theta.  `operator.tridiag_info`: levels,
    rows per level, blocks the planner shortened, largest block growth, backward error of the check solve."""
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, n, arrs, sre, sim = _tridiag_args(dl, d, du, sigma)
    ptr = lambda a: None if a.size == 0 else a.ctypes.data  # noqa: E731
    h = C.c_void_p()
    check(lib.ks_operator_tridiag_solve(ctx._h, n, _dtype_code(dt), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), sre, sim, int(block_rows), C.byref(h)))
    op = Operator(ctx, h, (n, n), dt)
    lv, sh, gr, res = C.c_int(), C.c_int64(), C.c_double(), C.c_double()
    rows = np.zeros(8, dtype=np.int64)
    check(lib.ks_operator_tridiag_info(h, C.byref(lv), rows.ctypes.data, C.byref(sh), C.byref(gr), C.byref(res)))
    op.tridiag_info = dict(levels=lv.value, level_rows=[int(r) for r in rows[: lv.value]], shortened_blocks=sh.value, max_growth=gr.value,
                           residual=res.value)
    return op


def host_tridiagonal_solve(dl, d, du, b, sigma=0.0, block_rows: int = 0):
    """The host path of `tridiagonal_solve_operator` (`ks_host_tridiag_solve` / `ks_host_tridiag_info`, no device): plan, factors
    and the apply that walks the arrays the device kernels read.  `b`: (n,) or (n, nrhs).  Returns (x, info) with info as
    `operator.tridiag_info`."""
    lib = _lib.load()
    dt, n, arrs, sre, sim = _tridiag_args(dl, d, du, sigma)
    B = np.asarray(b, dtype=dt)
    cols = np.asfortranarray(B.reshape(n, -1))
    X = np.zeros_like(cols, order="F")
    ptr = lambda a: None if a.size == 0 else a.ctypes.data  # noqa: E731
    lv, sh, gr, res = C.c_int(), C.c_int64(), C.c_double(), C.c_double()
    rows = np.zeros(8, dtype=np.int64)
    check(lib.ks_host_tridiag_solve(n, _dtype_code(dt), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), sre, sim, int(block_rows), cols.shape[1],
                                    ptr(cols), max(n, 1), ptr(X), max(n, 1), C.byref(lv), C.byref(gr), C.byref(res)))
    check(lib.ks_host_tridiag_info(n, _dtype_code(dt), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), sre, sim, int(block_rows), C.byref(lv),
                                   rows.ctypes.data, C.byref(sh), C.byref(gr), C.byref(res)))
    info = dict(levels=lv.value, level_rows=[int(r) for r in rows[: lv.value]], shortened_blocks=sh.value, max_growth=gr.value, residual=res.value)
    return X.reshape(B.shape), info


def _pencil_args(kdl, kd, kdu, mdl, md, mdu, sigma):
    """The six diagonals of a tridiagonal pencil (K, M) promoted to one element type like `_tridiag_args` promotes three, and
    T = K - sigma M formed here, in numpy: the library does no arithmetic on its inputs."""
    both = (kdl, kd, kdu, mdl, md, mdu)
    cplx = any(np.asarray(a).dtype.kind == "c" for a in both) or isinstance(sigma, (complex, np.complexfloating))
    dt = np.dtype(np.complex128 if cplx else np.float64)
    arrs = [np.ascontiguousarray(a, dtype=dt) for a in both]
    n = arrs[1].shape[0] if arrs[1].ndim == 1 else -1
    want = [(max(n - 1, 0),), (n,), (max(n - 1, 0),)] * 2
    if n < 0 or [a.shape for a in arrs] != want:
        raise DimensionMismatch(f"the diagonals of K and of M must have n entries, their off-diagonals n - 1: {[a.shape for a in arrs]}")
    sg = dt.type(sigma)
    K, M = arrs[:3], arrs[3:]
    return dt, n, [np.ascontiguousarray(k - sg * m) for k, m in zip(K, M)], M


def tridiagonal_pencil_operator(kdl, kd, kdu, mdl, md, mdu, sigma=0.0, ctx: Context | None = None, block_rows: int = 0) -> Operator:
    """y = (K - sigma M)^-1 M x for tridiagonal K and M (sub-/main/super-diagonals of n-1, n, n-1 entries each): the operator
    `x -> (A - sigma B) \\ (B x)` of the reference's shift-and-invert recipe for generalized problems A x = B x lambda
    (docs/src/index.md:273-287) on a 1-D pencil -- FEM stiffness and consistent mass --, as ONE library operator
    (`ks_operator_tridiag_pencil`): T = K - sigma M is formed here and factored once like `tridiagonal_solve_operator(T, 0)`
    factors it, and level 0 of the elimination forms M x while it stages its right-hand side: no launch and no vector for
    the multiplication.  The eigenvalues of the pencil closest to sigma are sigma + 1/theta.  `operator.tridiag_info` as for
    `tridiagonal_solve_operator`."""
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, n, T, M = _pencil_args(kdl, kd, kdu, mdl, md, mdu, sigma)
    ptr = lambda a: None if a.size == 0 else a.ctypes.data  # noqa: E731
    h = C.c_void_p()
    check(lib.ks_operator_tridiag_pencil(ctx._h, n, _dtype_code(dt), ptr(T[0]), ptr(T[1]), ptr(T[2]), ptr(M[0]), ptr(M[1]), ptr(M[2]),
                                         int(block_rows), C.byref(h)))
    op = Operator(ctx, h, (n, n), dt)
    lv, sh, gr, res = C.c_int(), C.c_int64(), C.c_double(), C.c_double()
    rows = np.zeros(8, dtype=np.int64)
    check(lib.ks_operator_tridiag_info(h, C.byref(lv), rows.ctypes.data, C.byref(sh), C.byref(gr), C.byref(res)))
    op.tridiag_info = dict(levels=lv.value, level_rows=[int(r) for r in rows[: lv.value]], shortened_blocks=sh.value, max_growth=gr.value,
                           residual=res.value)
    return op


def host_tridiagonal_pencil_solve(kdl, kd, kdu, mdl, md, mdu, b, sigma=0.0, block_rows: int = 0):
    """The host path of `tridiagonal_pencil_operator` (no device): the same T = K - sigma M, t = M b in the order of the device
    kernel (md x[r], then mdl x[r-1], then mdu x[r+1]), and `host_tridiagonal_solve(T, t, sigma=0)`.  `b`: (n,) or (n, nrhs).
    Returns (x, info) with info as `operator.tridiag_info`."""
    dt, n, T, M = _pencil_args(kdl, kd, kdu, mdl, md, mdu, sigma)
    B = np.asarray(b, dtype=dt)
    cols = B.reshape(n, -1)
    t = M[1][:, None] * cols
    if n > 1:
        t[1:] += M[0][:, None] * cols[:-1]
        t[:-1] += M[2][:, None] * cols[1:]
    return host_tridiagonal_solve(T[0], T[1], T[2], t.reshape(B.shape), sigma=0.0, block_rows=block_rows)


class _FactorErrors:
    """The `errors` lists of a product's callback factors seen as one list: what `_check_op` looks at, pops from and clears."""

    def __init__(self, lists):
        self._lists = lists

    def __len__(self):
        return sum(len(x) for x in self._lists)

    def pop(self, i=0):
        for x in self._lists:
            if len(x):
                return x.pop(i)
        raise IndexError("pop from empty list")

    def __delitem__(self, _):
        for x in self._lists:
            del x[:]


def product_operator(*factors, ctx: Context | None = None) -> Operator:
    """y = factors[0] factors[1] ... factors[-1] x, in mathematical order (the last factor is applied to x first), with every
    intermediate vector resident in HBM (`ks_operator_product`): the composed LinearMaps of the reference's recipes for
    generalized problems (docs/src/index.md:273-287, 325-336; `extras.generalized_shift_invert`, `extras.b_orthonormal_operator`).
    2 to 8 `Operator`s of one size, element type and context; a factor may appear more than once.  The product keeps its factors
    alive (`.factors`); closing it leaves them usable.  An exception raised inside a Python callback factor surfaces as that
    exception from the call that applied the product."""
    ctx = ctx or (factors[0].ctx if factors and isinstance(factors[0], Operator) else default_context())
    lib = _lib.load()
    hs = (C.c_void_p * max(len(factors), 1))(*[getattr(f, "_h", None) for f in factors])
    h = C.c_void_p()
    check(lib.ks_operator_product(ctx._h, len(factors), hs, C.byref(h)))
    n, dt = factors[0].shape[0], factors[0].dtype
    op = Operator(ctx, h, (n, n), dt, keep=tuple(factors))
    op.factors = tuple(factors)
    errs = [f.errors for f in factors if getattr(f, "errors", None) is not None]
    if errs:
        op.errors = _FactorErrors(errs)
    return op


def _chebyshev_args(degree, center, halfwidth, coeffs):
    g = np.asarray(coeffs)
    if g.ndim != 1 or g.dtype.kind not in "fiu":
        raise ArgumentError(f"coeffs must be a 1-D sequence of real numbers (gamma_0 ... gamma_degree), got shape {g.shape}, dtype {g.dtype}")
    g = np.ascontiguousarray(g, dtype=np.float64)
    if degree is None:
        degree = g.size - 1
    elif g.size != int(degree) + 1:
        raise DimensionMismatch(f"a filter of degree {degree} takes {int(degree) + 1} coefficients, got {g.size}")
    return int(degree), float(center), float(halfwidth), g


def host_chebyshev_plan(degree, center, halfwidth, coeffs):
    """(steps, temporaries) of the Clenshaw schedule `chebyshev_operator` runs (`ks_host_chebyshev_plan`; no device needed): one
    dict per operator step `out = sigma (A in - center in) - w + gamma x0` with the slots `in`, `out`, `w` (-1 = x0 as `in` / y as
    `out`, -2 = none, 0..2 = the filter's intermediate vectors) and the scalars `sigma`, `gamma`."""
    degree, center, halfwidth, g = _chebyshev_args(degree, center, halfwidth, coeffs)
    steps = (_lib.ks_cheb_step * max(degree, 1))()
    nt = C.c_int()
    check(_lib.load().ks_host_chebyshev_plan(degree, center, halfwidth, g.ctypes.data, C.cast(steps, C.c_void_p), C.byref(nt)))
    return [{"in": s.in_, "out": s.out, "w": s.w, "sigma": s.sigma, "gamma": s.gamma} for s in steps[:degree]], nt.value


def chebyshev_operator(A: Operator, center, halfwidth, coeffs, ctx: Context | None = None) -> Operator:
    """y = p(A) x with p(A) = sum_k coeffs[k] T_k((A - center) / halfwidth), every vector resident in HBM (`ks_operator_chebyshev`):
    the spectral transformation for operators that cannot be factored.  `partialschur(F, which="LR")` finds the eigenvalues of A
    that p maps highest -- `extras.chebyshev_window` / `extras.chebyshev_damping` make (center, halfwidth, coeffs) for an interior
    window or a clustered low end; [center - halfwidth, center + halfwidth] must contain A's spectrum
    (`extras.grid_spectrum_bounds`).  degree = len(coeffs) - 1 products per application; the grid operators can fuse each Clenshaw
    step into their product (the default where that measured faster; KS_CHEB_FUSED=1 / 0 forces), every other operator adds one
    streaming pass per step (`.chebyshev_info` counts both).  The filter
    keeps A alive (`.base`); closing it leaves A usable.  An exception raised inside a Python callback A surfaces as that
    exception from the call that applied the filter."""
    if not isinstance(A, Operator):
        raise ArgumentError(f"chebyshev_operator takes an Operator (as_operator(A) makes one), got {type(A).__name__}")
    ctx = ctx or A.ctx
    degree, center, halfwidth, g = _chebyshev_args(None, center, halfwidth, coeffs)
    h = C.c_void_p()
    check(_lib.load().ks_operator_chebyshev(ctx._h, A._h, degree, center, halfwidth, g.ctypes.data, C.byref(h)))
    op = Operator(ctx, h, A.shape, A.dtype, keep=(A,))
    op.base = A
    if getattr(A, "errors", None) is not None:
        op.errors = A.errors
    return op


def host_cg_step(rho, pq, rho_new, stop):
    """(alpha, beta, done, fail) of one conjugate-gradient iteration as `cg_operator`'s kernels decide it (`ks_host_cg_step`; no
    device needed): from rho = ||r||^2, pq = Re p^H (A - shift) p, rho_new = ||r - alpha q||^2 and stop = tol^2 ||b||^2.  `fail`
    (pq not finite or <= 0, alpha or rho_new not finite) gives alpha = beta = 0; `done` is rho_new <= stop and gives beta = 0."""
    a, b, d, f = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    check(_lib.load().ks_host_cg_step(float(rho), float(pq), float(rho_new), float(stop), C.byref(a), C.byref(b), C.byref(d), C.byref(f)))
    return a.value, b.value, bool(d.value), bool(f.value)


def cg_operator(A: Operator, shift=0.0, tol=1e-13, maxit=1000, check_every=0, ctx: Context | None = None) -> Operator:
    """y ~ (A - shift I)^-1 x by conjugate gradients, every vector resident in HBM and every scalar of the recurrence on the device
    (`ks_operator_cg`): the inner iterative solver for operators that have nothing to factor -- the mass matrix of matrix-free
    finite elements (`extras.generalized_cg_operator`), any Hermitian operator with `shift` below its spectrum.  A - shift I must be
    Hermitian positive definite (Float64 or ComplexF64; `shift` is real).  The solve stops when the recurrence's residual is below
    `tol` ||x||; `maxit` bounds the iterations, the host looks at the device's record every `check_every` iterations (0: the
    library default, 8) -- neither the result nor the iteration count depends on it, and equal inputs give equal bits.  For an
    ill-conditioned operator (a coefficient jump, an anisotropic grid) `pcg_operator` is this solve with a preconditioner.

    The solve is linear in x only up to tol * cond(A - shift I), and the Arnoldi relation of an outer `partialschur` on this
    operator inherits that: choose `tol` at least 100 times tighter than the outer tolerance.

    Refused (ArgumentError): an A of another context, one that cannot be enqueued ahead (a host callback, another `cg_operator`, a
    product or filter of one), a context of several ranks, tol outside (0, 1), maxit < 1, check_every < 0, a shift that is not
    finite.  At apply time "not positive definite" and "did not converge" raise HipError; the operator stays usable.  `.cg_info`
    counts solves and iterations.  The operator keeps A alive (`.base`); closing it leaves A usable."""
    if not isinstance(A, Operator):
        raise ArgumentError(f"cg_operator takes an Operator (as_operator(A) makes one), got {type(A).__name__}")
    ctx = ctx or A.ctx
    h = C.c_void_p()
    check(_lib.load().ks_operator_cg(ctx._h, A._h, float(shift), float(tol), int(maxit), int(check_every), C.byref(h)))
    op = Operator(ctx, h, A.shape, A.dtype, keep=(A,))
    op.base = A
    return op


PCG_FAIL = {0: None, 1: "right-hand side", 2: "curvature", 3: "preconditioner", 4: "residual"}   # the reason codes of ks_host_pcg_step


def host_pcg_step(tau, pq, rho_new, stop, tau_new):
    """(alpha, beta, done, fail) of one preconditioned conjugate-gradient iteration as `pcg_operator`'s kernels decide it
    (`ks_host_pcg_step`; no device needed): from tau = Re r^H M r, pq = Re p^H (A - shift) p, rho_new = ||r - alpha q||^2,
    stop = tol^2 ||b||^2 and tau_new = Re r^H M r after the step.  `fail` is 0 or a reason code (`PCG_FAIL`): 2, pq not finite or <= 0
    or alpha not finite, and 4, rho_new not finite, give alpha = beta = 0; `done` is rho_new <= stop and gives beta = 0 without a look
    at tau_new; otherwise 3, tau_new not finite or <= 0 or beta not finite, gives beta = 0 and leaves alpha."""
    a, b, d, f = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    check(_lib.load().ks_host_pcg_step(float(tau), float(pq), float(rho_new), float(stop), float(tau_new), C.byref(a), C.byref(b), C.byref(d),
                                       C.byref(f)))
    return a.value, b.value, bool(d.value), f.value


def diagonal_operator(d, dtype=None, ctx: Context | None = None) -> Operator:
    """y = d o x for a real vector d of n finite entries, on Float64 (the default) or ComplexF64 vectors (`ks_operator_diagonal`):
    a lumped mass matrix or its inverse (M^-1 K as `product_operator(diagonal_operator(1 / m), K)`), a scaling, the Jacobi
    preconditioner of `pcg_operator` (`extras.jacobi_preconditioner`).  One streaming kernel, 24 bytes per row in Float64; usable
    wherever an operator is.  Negative entries and zeros are allowed: it is an operator, not only a preconditioner."""
    ctx = ctx or default_context()
    v = np.asarray(d)
    if v.ndim != 1 or v.dtype.kind not in "fiu":
        raise ArgumentError(f"d must be a 1-D sequence of real numbers, got shape {v.shape}, dtype {v.dtype}")
    v = np.ascontiguousarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        raise ArgumentError(f"d must be finite (entry {int(np.flatnonzero(~np.isfinite(v))[0])} is not)")
    dt = np.dtype(np.float64 if dtype is None else dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise ArgumentError(f"element type must be float64 or complex128, not {dt}")
    h = C.c_void_p()
    check(_lib.load().ks_operator_diagonal(ctx._h, v.size, _dtype_code(dt), v.ctypes.data if v.size else None, C.byref(h)))
    op = Operator(ctx, h, (v.size, v.size), dt)
    op.diagonal = v
    return op


def pcg_operator(A: Operator, M: Operator, shift=0.0, tol=1e-13, maxit=1000, check_every=0, ctx: Context | None = None) -> Operator:
    """y ~ (A - shift I)^-1 x by PRECONDITIONED conjugate gradients with the device operator M ~ (A - shift I)^-1, every vector
    resident in HBM and every scalar of the recurrence on the device (`ks_operator_pcg`): `cg_operator` for the operators it cannot
    reach -- a coefficient jump (`extras.jacobi_preconditioner`: 72 iterations where plain conjugate gradients take 519), an
    anisotropic grid (`extras.line_preconditioner`: 16 against 94), a large grid (`extras.grid_multigrid_preconditioner`, a
    `multigrid_operator`: 16 against Jacobi's 72, and a count that hardly grows with the grid), the caller's incomplete factors
    (`lu_operator`).  A - shift I and M
    must be Hermitian positive definite and M the same linear map in every iteration; build M for A - shift I, not for A.  The
    stopping test, `tol`, `maxit` and `check_every` are `cg_operator`'s (the 2-norm of the recurrence's residual below `tol` ||x||),
    and so is the advice on an outer `partialschur`.  A `diagonal_operator` as M is fused into the solver's own kernels (three
    launches per iteration, no extra vector; KS_PCG_FUSED=0 runs it like any other M, with the same bits).  A
    `chebyshev_operator` of A as M works but does not reduce the number of products.

    Refused (ArgumentError): what `cg_operator` refuses, an M that is not an Operator, of another context, element type or size, or one
    that cannot be enqueued ahead (a host callback, a `cg_operator` or one of its siblings: that would need flexible conjugate
    gradients).  At apply time "not positive definite", "the preconditioner is not positive definite" and "did not converge" raise
    HipError; the operator stays usable.  `.pcg_info` counts solves, iterations and applications of M.  The operator keeps A and M
    alive (`.base`, `.preconditioner`); closing it leaves them usable."""
    for what, op in (("an Operator (as_operator(A) makes one)", A), ("an Operator as preconditioner", M)):
        if not isinstance(op, Operator):
            raise ArgumentError(f"pcg_operator takes {what}, got {type(op).__name__}")
    ctx = ctx or A.ctx
    h = C.c_void_p()
    check(_lib.load().ks_operator_pcg(ctx._h, A._h, M._h, float(shift), float(tol), int(maxit), int(check_every), C.byref(h)))
    op = Operator(ctx, h, A.shape, A.dtype, keep=(A, M))
    op.base, op.preconditioner = A, M
    return op


def _mg_dims(shapes):
    """int64[nlevels, 3]: one row of extents (x, y, z; unused axes 1) per level."""
    try:
        rows = [[int(e) for e in np.atleast_1d(np.asarray(s)).ravel()] for s in shapes]
    except (TypeError, ValueError) as e:
        raise ArgumentError(f"shapes must hold 1 to 3 integer extents per level: {shapes!r}") from e
    if not rows or any(not 1 <= len(r) <= 3 for r in rows):
        raise ArgumentError(f"shapes must hold 1 to 3 integer extents per level: {shapes!r}")
    return np.ascontiguousarray([r + [1] * (3 - len(r)) for r in rows], dtype=np.int64)


def _mg_levels(dims, inverse_diagonals, bounds):
    """(array of pointers or None, the arrays it points to, float64 bounds) for the smoothed levels of a dims chain."""
    nsmooth = dims.shape[0] - 1
    lam = np.ascontiguousarray(np.atleast_1d(np.asarray(bounds, dtype=np.float64)).ravel())
    if lam.size != nsmooth:
        raise DimensionMismatch(f"{nsmooth} smoothed levels take {nsmooth} bounds, got {lam.size}")
    if inverse_diagonals is None:
        return None, [], lam
    if len(inverse_diagonals) != nsmooth:
        raise DimensionMismatch(f"{nsmooth} smoothed levels take {nsmooth} inverse diagonals, got {len(inverse_diagonals)}")
    ds = []
    for l, d in enumerate(inverse_diagonals):
        v = np.asarray(d)
        if v.ndim != 1 or v.dtype.kind not in "fiu":
            raise ArgumentError(f"the inverse diagonal of level {l} must be a 1-D sequence of real numbers, got shape {v.shape}, dtype {v.dtype}")
        if v.size != int(np.prod(dims[l])):
            raise DimensionMismatch(f"the inverse diagonal of level {l} has {v.size} entries, its grid {tuple(int(e) for e in dims[l])} has {int(np.prod(dims[l]))}")
        ds.append(np.ascontiguousarray(v, dtype=np.float64))
    ptrs = (C.c_void_p * max(nsmooth, 1))(*[d.ctypes.data for d in ds])
    return ptrs, ds, lam


def host_multigrid_plan(shapes, bounds, degree=2, ratio=4.0, inverse_diagonals=None) -> dict:
    """The host plan of `multigrid_operator` (`ks_host_multigrid_plan`; no device needed) for the grids `shapes` (finest first) and one
    bound per smoothed level: `rows` per level, and per smoothed level the restriction `scale` and the Chebyshev smoother's
    coefficients `a[l][j]`, `b[l][j]` of step j (d = a d + b dinv o (rhs - t), x += d).  Refuses what the operator refuses."""
    dims = _mg_dims(shapes)
    nsmooth = dims.shape[0] - 1
    ptrs, _keep, lam = _mg_levels(dims, inverse_diagonals, bounds)
    k = max(int(degree), 1)
    a, b = np.zeros((max(nsmooth, 1), k)), np.zeros((max(nsmooth, 1), k))
    scale, rows = np.zeros(max(nsmooth, 1)), np.zeros(nsmooth + 1, dtype=np.int64)
    check(_lib.load().ks_host_multigrid_plan(nsmooth, dims.ctypes.data, ptrs, lam.ctypes.data if lam.size else None, int(degree), float(ratio),
                                             a.ctypes.data, b.ctypes.data, scale.ctypes.data, rows.ctypes.data))
    return dict(rows=tuple(int(r) for r in rows), scale=scale[:nsmooth].copy(), a=a[:nsmooth].copy(), b=b[:nsmooth].copy())


def _mg_transfer_args(fine_shape, coarse_shape, *vectors):
    dims = _mg_dims([fine_shape, coarse_shape])
    dt = np.result_type(*[np.asarray(v).dtype for v in vectors])
    dt = np.dtype(np.complex128 if dt.kind == "c" else np.float64)
    return dims, dt, [np.ascontiguousarray(v, dtype=dt).ravel() for v in vectors]


def host_multigrid_restrict(fine_shape, coarse_shape, b, t):
    """r_c = s P^T (b - t) between two consecutive grids as `multigrid_operator`'s kernel forms it (`ks_host_multigrid_restrict`; no
    device needed): per coarse cell the terms fl(b[i] - t[i]) of its aggregate added to +0.0 in ascending fine row order, times
    s = 2^-(halved axes).  Float64 or ComplexF64."""
    dims, dt, (bv, tv) = _mg_transfer_args(fine_shape, coarse_shape, b, t)
    nf, nc = int(np.prod(dims[0])), int(np.prod(dims[1]))
    if bv.size != nf or tv.size != nf:
        raise DimensionMismatch(f"the fine grid {tuple(int(e) for e in dims[0])} has {nf} rows, b has {bv.size} and t {tv.size}")
    rc = np.zeros(nc, dtype=dt)
    check(_lib.load().ks_host_multigrid_restrict(_dtype_code(dt), dims[0].ctypes.data, dims[1].ctypes.data, bv.ctypes.data, tv.ctypes.data, rc.ctypes.data))
    return rc


def host_multigrid_prolong_add(fine_shape, coarse_shape, e, x):
    """x + P e between two consecutive grids (`ks_host_multigrid_prolong_add`; no device needed): every fine cell takes the value of
    its coarse cell.  Returns a new vector."""
    dims, dt, (ev, xv) = _mg_transfer_args(fine_shape, coarse_shape, e, x)
    nf, nc = int(np.prod(dims[0])), int(np.prod(dims[1]))
    if ev.size != nc or xv.size != nf:
        raise DimensionMismatch(f"the grids have {nf} and {nc} rows, x has {xv.size} and e {ev.size}")
    out = xv.copy()
    check(_lib.load().ks_host_multigrid_prolong_add(_dtype_code(dt), dims[0].ctypes.data, dims[1].ctypes.data, ev.ctypes.data, out.ctypes.data))
    return out


def multigrid_operator(operators, shapes, inverse_diagonals, bounds, coarse: Operator, shift=0.0, degree=2, ratio=4.0,
                       ctx: Context | None = None) -> Operator:
    """y = M x with M ~ (A - shift I)^-1: ONE symmetric geometric multigrid V-cycle on the grids `shapes` (finest first, len(operators)
    + 1 of them; `ks_operator_multigrid`, csrc/ks_mg.hpp) -- a fixed Hermitian positive definite map that can be enqueued ahead, so
    `pcg_operator(A, M, shift=shift)` takes it as its preconditioner, and usable wherever an operator is.  `operators[l]` is the
    device operator of level l (any that can be enqueued ahead), `inverse_diagonals[l]` the real, positive 1 / (diag(A_l) - shift),
    `bounds[l]` an upper bound on the spectrum of D_l^-1 (A_l - shift), `coarse` the operator applied on the last grid (its inverse).
    Each smoothed level runs `degree` Chebyshev steps on [bound / ratio, bound] before and after the coarse correction; consecutive
    grids keep or halve (ceil) each extent, the transfers are piecewise constant.  `extras.grid_multigrid_preconditioner` builds all
    of it for -div(c grad) + V.  With no smoothed level M is `coarse`.  The cycle keeps its operators alive (`.levels`, `.coarse`);
    closing it leaves them usable.  `.multigrid_info` counts applications and products per level."""
    operators = list(operators)
    for what, op in [(f"an Operator for level {l}", A) for l, A in enumerate(operators)] + [("an Operator as coarse", coarse)]:
        if not isinstance(op, Operator):
            raise ArgumentError(f"multigrid_operator takes {what}, got {type(op).__name__}")
    dims = _mg_dims(shapes)
    nsmooth = len(operators)
    if dims.shape[0] != nsmooth + 1:
        raise DimensionMismatch(f"{nsmooth} level operators and a coarse one take {nsmooth + 1} shapes, got {dims.shape[0]}")
    if inverse_diagonals is None:
        raise ArgumentError("multigrid_operator takes one inverse diagonal per smoothed level")
    ptrs, keep, lam = _mg_levels(dims, list(inverse_diagonals), bounds)
    ctx = ctx or coarse.ctx
    hs = (C.c_void_p * max(nsmooth, 1))(*[A._h for A in operators])
    h = C.c_void_p()
    check(_lib.load().ks_operator_multigrid(ctx._h, nsmooth, hs, dims.ctypes.data, ptrs, lam.ctypes.data if lam.size else None, coarse._h,
                                            float(shift), int(degree), float(ratio), C.byref(h)))
    n = int(np.prod(dims[0]))
    op = Operator(ctx, h, (n, n), coarse.dtype, keep=tuple(operators) + (coarse,))
    op.levels, op.coarse = tuple(operators), coarse
    del keep
    return op


def host_minres_step(alpha, beta, beta_new, c, s, c_prev, s_prev, phibar, stop):
    """(eps, delta, gamma, c', s', phi, phibar', done, fail) of one MINRES iteration as `minres_operator`'s kernels decide it
    (`ks_host_minres_step`; no device needed): the column (beta, alpha, beta_new) of the Lanczos matrix through the two previous
    rotations (c_prev, s_prev), (c, s), the rotation (c', s') that annihilates beta_new with gamma = hypot(gbar, beta_new), the step
    length phi = c' phibar and the new residual norm phibar' = -s' phibar.  `fail` (alpha, beta_new or gamma not finite, gamma == 0)
    zeroes every output but gamma; `done` is |phibar'| <= stop."""
    out = (C.c_double * 7)()
    d, f = C.c_int(), C.c_int()
    args = [float(t) for t in (alpha, beta, beta_new, c, s, c_prev, s_prev, phibar, stop)]
    check(_lib.load().ks_host_minres_step(*args, C.cast(out, C.c_void_p), C.byref(d), C.byref(f)))
    return tuple(out) + (bool(d.value), bool(f.value))


def minres_operator(A: Operator, shift=0.0, tol=1e-13, maxit=10000, check_every=0, ctx: Context | None = None) -> Operator:
    """y ~ (A - shift I)^-1 x by MINRES, every vector resident in HBM and every scalar of the recurrence on the device
    (`ks_operator_minres`): shift-invert for operators that have nothing to factor, with `shift` ANYWHERE on the real axis that is
    not an eigenvalue -- inside the spectrum too, where `cg_operator` stops at its first negative curvature.
    `partialschur(minres_operator(A, shift=sigma), which="LM")` finds the eigenvalues of A nearest sigma
    (`extras.interior_eigenvalues(mu, sigma)` maps them back).  A must be Hermitian (Float64 or ComplexF64; `shift` is real); an A
    that is not Hermitian is NOT detected -- the three-term recurrence then solves some other problem without a complaint.  The
    solve stops when the recurrence's residual norm is below `tol` ||x||; `maxit` bounds the iterations (their number grows with
    the spectrum's width over the distance from `shift` to the nearest eigenvalue), the host looks at the device's record every
    `check_every` iterations (0: the library default, 8) -- neither the result nor the iteration count depends on it, and equal
    inputs give equal bits.

    The solve is linear in x only up to tol * cond(A - shift I), and the Arnoldi relation of an outer `partialschur` on this
    operator inherits that: choose `tol` at least 100 times tighter than the outer tolerance.

    Refused (ArgumentError): an A of another context, one that cannot be enqueued ahead (a host callback, a `cg_operator`, another
    `minres_operator`, a product or filter of one), a context of several ranks, tol outside (0, 1), maxit < 1, check_every < 0, a
    shift that is not finite.  At apply time "not finite" (the right-hand side), "singular" (the shift is an eigenvalue) and "did
    not converge" raise HipError; the operator stays usable.  `.minres_info` counts solves and iterations.  The operator keeps A
    alive (`.base`); closing it leaves A usable."""
    if not isinstance(A, Operator):
        raise ArgumentError(f"minres_operator takes an Operator (as_operator(A) makes one), got {type(A).__name__}")
    ctx = ctx or A.ctx
    h = C.c_void_p()
    check(_lib.load().ks_operator_minres(ctx._h, A._h, float(shift), float(tol), int(maxit), int(check_every), C.byref(h)))
    op = Operator(ctx, h, A.shape, A.dtype, keep=(A,))
    op.base = A
    return op


def _scalar_pair(z):
    z = complex(z)
    return (C.c_double * 2)(z.real, z.imag)


def host_bicgstab_coef(rho0, rho1, alpha, gamma, complex_scalars=None):
    """(beta, alpha', fail) of one BiCG coefficient step as `bicgstab_operator`'s kernels decide it (`ks_host_bicgstab_coef`; no
    device needed): beta = alpha rho1 / rho0, alpha' = rho1 / gamma.  fail 1: rho0 zero or not finite, or beta not finite (both
    outputs 0); fail 2: gamma zero or not finite, or alpha' not finite (alpha' = 0).  Complex arithmetic when any argument is complex
    (or `complex_scalars` says so): the outputs are then complex, else floats."""
    args = (rho0, rho1, alpha, gamma)
    cplx = any(isinstance(t, (complex, np.complexfloating)) for t in args) if complex_scalars is None else bool(complex_scalars)
    beta, anew, f = (C.c_double * 2)(), (C.c_double * 2)(), C.c_int()
    pairs = [_scalar_pair(t) for t in args]
    check(_lib.load().ks_host_bicgstab_coef(int(cplx), *[C.cast(t, C.c_void_p) for t in pairs], C.cast(beta, C.c_void_p), C.cast(anew, C.c_void_p),
                                            C.byref(f)))
    if cplx:
        return complex(beta[0], beta[1]), complex(anew[0], anew[1]), f.value
    return beta[0], anew[0], f.value


def host_bicgstab_mr(g11, g22, g12, h1, h2, complex_scalars=None):
    """(g1, g2, det, fail) of the two-dimensional minimal-residual step of `bicgstab_operator` (`ks_host_bicgstab_mr`; no device
    needed): the Hermitian system [g11 g12; conj(g12) g22] g = h by Cramer's rule with det = fma(g11, g22, -|g12|^2).  fail: det
    zero or not finite, or a quotient not finite (g = 0).  Complex arithmetic when g12, h1 or h2 is complex."""
    args = (g12, h1, h2)
    cplx = any(isinstance(t, (complex, np.complexfloating)) for t in args) if complex_scalars is None else bool(complex_scalars)
    g1, g2, det, f = (C.c_double * 2)(), (C.c_double * 2)(), C.c_double(), C.c_int()
    pairs = [_scalar_pair(t) for t in args]
    check(_lib.load().ks_host_bicgstab_mr(int(cplx), float(g11), float(g22), *[C.cast(t, C.c_void_p) for t in pairs], C.cast(g1, C.c_void_p),
                                          C.cast(g2, C.c_void_p), C.byref(det), C.byref(f)))
    if cplx:
        return complex(g1[0], g1[1]), complex(g2[0], g2[1]), det.value, f.value
    return g1[0], g2[0], det.value, f.value


def bicgstab_operator(A: Operator, shift=0.0, tol=1e-13, maxit=10000, check_every=0, ctx: Context | None = None) -> Operator:
    """y ~ (A - shift I)^-1 x by BiCGStab(2), every vector resident in HBM and every scalar of the recurrence on the device
    (`ks_operator_bicgstab`): shift-invert for operators that are NOT Hermitian and have nothing to factor -- a grid stencil with a
    convection term, a `product_operator` chain, a Bloch cell with a complex shift -- where `cg_operator` and `minres_operator` need a
    Hermitian A.  `partialschur(bicgstab_operator(A, shift=sigma), which="LM")` finds the eigenvalues of A nearest sigma
    (`extras.interior_eigenvalues(mu, sigma)` maps them back).  Float64 with a real `shift`, or ComplexF64 with a complex one.  An
    iteration is two BiCG steps and a two-dimensional minimal-residual step, four products; the solve stops when the recurrence's
    residual norm is below `tol` ||x||, tested after each BiCG step and after the minimal-residual step.  `maxit` bounds the
    iterations, the host looks at the device's record every `check_every` iterations (0: the library default, 8) -- neither the
    result nor the iteration count depends on it, and equal inputs give equal bits.

    No preconditioner and no residual replacement: on a shift deep inside a complex spectrum the solve needs hundreds of iterations
    and the true residual drifts above the recurrence's (README).  The solve is linear in x only up to tol * cond(A - shift I):
    choose `tol` at least 100 times tighter than the outer tolerance.

    Refused (ArgumentError): an imaginary shift on a Float64 operator (build the operator in ComplexF64), an A of another context,
    one that cannot be enqueued ahead (a host callback, a `cg_operator`, `minres_operator` or another `bicgstab_operator`, a product
    or filter of one), a context of several ranks, tol outside (0, 1), maxit < 1, check_every < 0, a shift that is not finite.  At
    apply time "not finite" (the right-hand side), "breakdown" (rho, gamma or det G zero or not finite: the shift is an eigenvalue)
    and "did not converge" raise HipError; the operator stays usable.  `.bicgstab_info` counts solves and iterations.  The operator
    keeps A alive (`.base`); closing it leaves A usable."""
    if not isinstance(A, Operator):
        raise ArgumentError(f"bicgstab_operator takes an Operator (as_operator(A) makes one), got {type(A).__name__}")
    ctx = ctx or A.ctx
    h = C.c_void_p()
    z = complex(shift)
    check(_lib.load().ks_operator_bicgstab(ctx._h, A._h, z.real, z.imag, float(tol), int(maxit), int(check_every), C.byref(h)))
    op = Operator(ctx, h, A.shape, A.dtype, keep=(A,))
    op.base = A
    return op


def _grid_radius(radius, periodic, wrap):
    """The radius of a grid operator's star stencil as an int: an integer in 1...4, above 1 only with open boundaries."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 4:
        raise ArgumentError(f"radius must be an integer in 1...4 (the distance of the farthest neighbour along an axis), got {radius!r}")
    if int(radius) > 1 and (periodic is not None or wrap is not None):
        raise ArgumentError(f"periodic / wrap are supported for radius 1 only here, got radius = {int(radius)}: "
                            "grid_star_operator / host_grid_star_matrix take periodic axes at every radius")
    return int(radius)


def _grid_args(shape, taps, potential, dtype, radius=1, box=False):
    """(dtype, dims, taps, potential or None) of a grid operator.  The element type is promoted like `_tridiag_args` promotes
    (ComplexF64 as soon as the taps or the potential are complex) unless `dtype` pins it; a pinned Float64 refuses imaginary parts.
    `box`: the 3^ndim taps of a box stencil, flat or as an array of shape (3,) * ndim in C order."""
    try:
        dims = np.atleast_1d(np.asarray(shape, dtype=np.int64))
    except (TypeError, ValueError, OverflowError) as e:
        raise ArgumentError(f"shape must hold 1 to 3 integer extents: {shape!r}") from e
    if dims.ndim != 1 or not 1 <= dims.size <= 3:
        raise ArgumentError(f"a grid has 1, 2 or 3 dimensions (ndim), shape = {shape!r}")
    ndim = int(dims.size)
    t, v = np.asarray(taps), None if potential is None else np.asarray(potential)
    cplx = t.dtype.kind == "c" or (v is not None and v.dtype.kind == "c")
    dt = np.dtype(np.complex128 if cplx else np.float64) if dtype is None else np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise ArgumentError(f"element type must be float64 or complex128, not {dt}")
    if dt.kind == "f" and cplx and (np.any(t.imag != 0) or (v is not None and np.any(v.imag != 0))):
        raise ArgumentError("taps or potential have an imaginary part but the element type is Float64 (KS_F64)")
    if box:
        if t.shape == (3,) * ndim:
            t = t.reshape(-1)
        if t.shape != (3 ** ndim,):
            raise DimensionMismatch(f"the box stencil of a {ndim}-D grid takes {3 ** ndim} taps in ascending column order, flat or of shape "
                                    f"{(3,) * ndim} ([dz, dy, dx]), got shape {t.shape}")
    elif t.shape != (2 * ndim * radius + 1,):
        of = "" if radius == 1 else f" of radius {radius}"
        raise DimensionMismatch(f"a {ndim}-D grid{of} takes {2 * ndim * radius + 1} taps in ascending column order, got shape {t.shape}")
    t = np.ascontiguousarray(t.real if dt.kind == "f" else t, dtype=dt)
    if v is not None:
        n = math.prod(int(d) for d in dims)
        # (an extent < 1 is the library's refusal to make: it checks the extents before it reads the potential)
        if np.all(dims >= 1) and v.shape != (n,) and v.shape != tuple(int(d) for d in dims[::-1]):
            raise DimensionMismatch(f"potential must have shape {tuple(int(d) for d in dims[::-1])} (C order, x fastest) or ({n},), got {v.shape}")
        v = np.ascontiguousarray((v.real if dt.kind == "f" else v).reshape(-1), dtype=dt)
    return dt, np.ascontiguousarray(dims), t, v


def _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap, radius=1):
    """(dtype, taps, potential, flags, wrap or None) of a grid operator with periodic axes: `periodic` a bool or one bool per axis,
    `wrap` 2 ndim radius values in the order of the taps without the centre.  A complex `wrap` promotes the element type like
    complex taps do; a pinned Float64 refuses an imaginary part."""
    ndim = int(dims.size)
    if periodic is None:
        periodic = False
    if isinstance(periodic, (bool, np.bool_)):
        flags = np.full(ndim, int(bool(periodic)), dtype=np.int32)
    else:
        try:
            seq = list(periodic)
        except TypeError as e:
            raise ArgumentError(f"periodic must be a bool or a sequence of {ndim} bools: {periodic!r}") from e
        if len(seq) != ndim or not all(isinstance(p, (bool, np.bool_)) for p in seq):
            raise DimensionMismatch(f"periodic takes one bool per axis in the order of shape ({ndim}), got {periodic!r}")
        flags = np.array([int(bool(p)) for p in seq], dtype=np.int32)
    w = None
    if wrap is not None:
        w = np.asarray(wrap)
        if w.shape != (2 * ndim * radius,):
            of = "" if radius == 1 else f" of radius {radius}"
            raise DimensionMismatch(f"a {ndim}-D grid{of} takes {2 * ndim * radius} wrap values in the order of the taps without the centre, "
                                    f"got shape {w.shape}")
        if w.dtype.kind == "c" and dt.kind == "f":
            if dtype is None:   # promote, like complex taps do
                dt = np.dtype(np.complex128)
                t = t.astype(dt)
                v = None if v is None else v.astype(dt)
            elif np.any(w.imag != 0):
                raise ArgumentError("wrap has an imaginary part but the element type is Float64 (KS_F64)")
        w = np.ascontiguousarray(w.real if dt.kind == "f" else w, dtype=dt)
    return dt, t, v, flags, w


def _grid_operator(ctx, h, dims, dt, t, v, extra_bytes=0, **info) -> Operator:
    """The Operator of a grid operator's handle with its `grid_info`: shape, taps, has_potential, bytes_per_row and what `info` adds."""
    n = math.prod(int(d) for d in dims)
    op = Operator(ctx, h, (n, n), dt)
    op.grid_info = dict(shape=tuple(int(d) for d in dims), taps=t.copy(), has_potential=v is not None,
                        bytes_per_row=dt.itemsize * (3 if v is not None else 2) + extra_bytes, **info)
    return op


def _grid_nnz(dims, radius=1, flags=()):
    """(n, nnz) of a grid matrix: the diagonal, the links of distance 1...radius and, per line of a periodic axis, the 2 d links of
    distance d that cross the boundary.  (0, 0) for a shape that the library refuses (so do extents below 2 radius + 1 on a periodic
    axis: the count is then never used)."""
    ext = [int(d) for d in dims]
    n = math.prod(ext)
    if not (all(1 <= e < 2 ** 31 for e in ext) and n < 2 ** 31 - 1):
        return 0, 0
    nnz = n + sum(2 * max(e - d, 0) * (n // e) for e in ext for d in range(1, radius + 1))
    return n, nnz + sum(2 * min(d, e) * (n // e) for e, f in zip(ext, flags) if f for d in range(1, radius + 1))


def _host_grid_csr(entry, n, nnz, dt, *args):
    """The scipy.sparse.csr_matrix one of the `ks_host_grid_*` entries fills: `args` are its arguments in front of the arrays."""
    import scipy.sparse as sp

    got = C.c_int64()
    rowptr, colidx, val = np.zeros(n + 1, dtype=np.int64), np.zeros(max(nnz, 1), dtype=np.int32), np.zeros(max(nnz, 1), dtype=dt)
    check(entry(*args, rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, nnz, C.byref(got)))
    assert got.value == nnz == rowptr[-1]
    return sp.csr_matrix((val[:nnz], colidx[:nnz], rowptr), shape=(n, n))


def grid_operator(shape, taps, potential=None, dtype=None, ctx: Context | None = None, periodic=None, wrap=None, radius=1) -> Operator:
    """Matrix-free operator of a constant-coefficient 3-, 5- or 7-point stencil plus a per-point diagonal term on a grid
    (`ks_operator_grid`): mul!(y, A, x), src/expansion.jl:121, for A = -Laplacian + V(x) and its kin with nothing stored per
    non-zero -- 24 bytes per row and product in Float64 (16 without a potential) where a stored matrix with a varying diagonal
    streams about 100.

    `shape` = (nx,), (nx, ny) or (nx, ny, nz), x fastest: row r = ix + nx (iy + ny iz).  `taps`: 2 ndim + 1 values in ascending
    column order, [-z, -y, -x, centre, +x, +y, +z] in 3-D; a tap whose neighbour lies outside the grid is absent (no wrap-around).
    `potential`: None, or n values added to the centre tap -- flat in row order, or an array of shape (nz, ny, nx) / (ny, nx) in C
    order (so that `potential.ravel()` is the row order).  The operator is exactly the matrix `host_grid_matrix` returns, and its
    products have the bits `csr_operator` of that matrix gives.  `operator.grid_info`: shape, taps, has_potential, bytes_per_row,
    periodic, wrap.

    `periodic` (`ks_operator_grid_periodic`): True, or one bool per axis in the order of `shape` -- on such an axis (extent >= 3)
    the first and the last point of a line are neighbours.  `wrap`: 2 ndim values in the order of the taps without the centre
    ([-z, -y, -x, +x, +y, +z] in 3-D), the entries of the links that cross the boundary; None = the taps (plain periodicity),
    `extras.bloch_wrap(taps, theta)` = Bloch phases, `-taps` = antiperiodic.  The traffic per row is unchanged.

    `radius` (`ks_operator_grid_star`): an integer R in 1...4, a star stencil with neighbours at the distances 1...R along every
    axis -- central differences of order 2 R (`extras.fd_laplacian_taps(ndim, 2 * R)`).  `taps` then holds 2 ndim R + 1 values in
    ascending column order, [-R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z] in
    3-D; boundaries are open (R > 1 together with `periodic` or `wrap` is refused).  The traffic per row is still unchanged, where
    the stored matrix streams about 12 bytes per non-zero.  The radius is never inferred from the length of `taps`."""
    radius = _grid_radius(radius, periodic, wrap)
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, radius)
    h = C.c_void_p()
    flags, w = np.zeros(dims.size, dtype=np.int32), None
    if radius > 1:
        check(lib.ks_operator_grid_star(ctx._h, int(dims.size), dims.ctypes.data, radius, _dtype_code(dt), t.ctypes.data,
                                        None if v is None else v.ctypes.data, C.byref(h)))
    elif periodic is None and wrap is None:
        check(lib.ks_operator_grid(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data, None if v is None else v.ctypes.data,
                                   C.byref(h)))
    else:
        dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap)
        check(lib.ks_operator_grid_periodic(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data,
                                            None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data,
                                            C.byref(h)))
    return _grid_operator(ctx, h, dims, dt, t, v, periodic=tuple(bool(f) for f in flags), wrap=None if w is None else w.copy(), radius=radius)


def host_grid_matrix(shape, taps, potential=None, dtype=None, periodic=None, wrap=None, radius=1):
    """The matrix that defines `grid_operator(shape, taps, potential)` as a scipy.sparse.csr_matrix (`ks_host_grid_matrix`: the host
    path, no device): ascending columns, the diagonal entry centre + potential[r] stored even where it is zero.  `periodic`, `wrap`:
    as for `grid_operator` (`ks_host_grid_matrix_periodic`); `radius`: as for `grid_operator` (`ks_host_grid_matrix_star`)."""
    radius = _grid_radius(radius, periodic, wrap)
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, radius)
    head = (int(dims.size), dims.ctypes.data)
    if radius > 1:
        n, nnz = _grid_nnz(dims, radius)
        return _host_grid_csr(lib.ks_host_grid_matrix_star, n, nnz, dt, *head, radius, _dtype_code(dt), t.ctypes.data,
                              None if v is None else v.ctypes.data)
    if periodic is None and wrap is None:
        n, nnz = _grid_nnz(dims)
        return _host_grid_csr(lib.ks_host_grid_matrix, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data, None if v is None else v.ctypes.data)
    dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap)
    n, nnz = _grid_nnz(dims, 1, flags)
    return _host_grid_csr(lib.ks_host_grid_matrix_periodic, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data,
                          None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data)


def grid_star_operator(shape, taps, radius, potential=None, dtype=None, ctx: Context | None = None, periodic=None, wrap=None) -> Operator:
    """Matrix-free operator of a star stencil of radius 1...4 plus a per-point diagonal term on a grid whose axes may be PERIODIC
    (`ks_operator_grid_star_periodic`): mul!(y, A, x), src/expansion.jl:121, for central differences of order 2 R on a crystal cell or
    a supercell -- a band structure at a k-point with an 8th-order Laplacian -- with nothing stored per non-zero: 24 bytes per row
    and product in Float64 (16 without a potential) at every radius.

    `shape`, `taps`, `radius`, `potential`, `dtype`: as for `grid_operator(..., radius=radius)`; the radius is never inferred from
    the length of `taps`.  `periodic`: True, or one bool per axis in the order of `shape`; a periodic axis needs an extent of at
    least 2 radius + 1, an axis that does not wrap is truncated.  `wrap`: 2 ndim radius values in the order of the taps without the
    centre ([-R z ... -1 z, -R y ... -1 y, -R x ... -1 x, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z] in 3-D), the entry of the link
    of that direction and distance where it crosses the cell boundary; None = the taps (plain periodicity),
    `extras.bloch_wrap(taps, theta, radius=radius)` = Bloch phases.  A complex `wrap` promotes the element type like complex taps do.

    The operator is exactly the matrix `host_grid_star_matrix` returns, and its products have the bits `csr_operator` of that matrix
    gives.  With no periodic axis it is `grid_operator(..., radius=radius)`, with `radius=1` `grid_operator(..., periodic=, wrap=)`.
    `operator.grid_info`: shape, taps, has_potential, bytes_per_row, periodic, wrap, radius."""
    radius = _grid_radius(radius, None, None)
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, radius)
    dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap, radius)
    h = C.c_void_p()
    check(lib.ks_operator_grid_star_periodic(ctx._h, int(dims.size), dims.ctypes.data, radius, _dtype_code(dt), t.ctypes.data,
                                             None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data,
                                             C.byref(h)))
    return _grid_operator(ctx, h, dims, dt, t, v, periodic=tuple(bool(f) for f in flags), wrap=None if w is None else w.copy(), radius=radius)


def host_grid_star_matrix(shape, taps, radius, potential=None, dtype=None, periodic=None, wrap=None):
    """The matrix that defines `grid_star_operator(shape, taps, radius, potential, periodic=, wrap=)` as a scipy.sparse.csr_matrix
    (`ks_host_grid_matrix_star_periodic`: the host path, no device): ascending columns, on a fully periodic grid 6 radius + 1 entries
    per row, the diagonal entry centre + potential[r] stored even where it is zero."""
    radius = _grid_radius(radius, None, None)
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, radius)
    dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap, radius)
    n, nnz = _grid_nnz(dims, radius, flags)
    return _host_grid_csr(lib.ks_host_grid_matrix_star_periodic, n, nnz, dt, int(dims.size), dims.ctypes.data, radius, _dtype_code(dt),
                          t.ctypes.data, None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data)


def _grid_coeff(dims, coeff):
    """The cell-centred coefficient of a variable-coefficient grid operator as n contiguous Float64 values in row order."""
    c = np.asarray(coeff)
    if c.dtype.kind == "c":
        raise ArgumentError("coeff must be real (one Float64 per grid point, also for ComplexF64 operators)")
    n = math.prod(int(d) for d in dims)
    # (an extent < 1 is the library's refusal to make, as for the potential)
    if np.all(dims >= 1) and c.shape != (n,) and c.shape != tuple(int(d) for d in dims[::-1]):
        raise DimensionMismatch(f"coeff must have shape {tuple(int(d) for d in dims[::-1])} (C order, x fastest) or ({n},), got {c.shape}")
    try:
        return np.ascontiguousarray(c.reshape(-1), dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ArgumentError(f"coeff must hold real numbers: {e}") from e


def grid_variable_operator(shape, taps, coeff, potential=None, dtype=None, ctx: Context | None = None, periodic=None, wrap=None) -> Operator:
    """Matrix-free operator of a 3-, 5- or 7-point stencil with a VARIABLE, cell-centred coefficient plus a per-point diagonal
    term on a grid (`ks_operator_grid_var`): mul!(y, A, x), src/expansion.jl:121, for A = -div(c(x) grad) + V(x) and its kin --
    heterogeneous diffusion, a position-dependent effective mass, div (1 / eps) grad -- with nothing stored per non-zero: 32 bytes
    per row and product in Float64 (24 without a potential) where the stored matrix streams about 100.

    `shape`, `taps`, `potential`, `dtype`: as for `grid_operator` (radius 1).  `coeff`: n real values, one per
    grid point -- flat in row order, or an array of shape (nz, ny, nx) / (ny, nx) in C order; always Float64, also for ComplexF64
    operators.  The entry of the link from row r to its in-grid neighbour s in direction k is fl(0.5 taps[k] * fl(c[r] + c[s]));
    the diagonal entry is centre + potential[r].  The operator is exactly the matrix `host_grid_variable_matrix` returns, and its
    products have the bits `csr_operator` of that matrix gives; with c == 1 it is `grid_operator(shape, taps, potential)`.

    The diffusion operator -div(c grad) + V:  `taps, diagonal = extras.diffusion_terms(shape, coeff, spacing, V, boundary)`, then
    `grid_variable_operator(shape, taps, coeff, potential=diagonal)`.

    `periodic`, `wrap` (`ks_operator_grid_var_periodic`): as for `grid_operator` -- photonic and phononic crystals, a superlattice
    with a position-dependent mass, diffusion on a torus.  A link that crosses the boundary of a periodic axis (extent >= 3) carries
    fl(0.5 wrap[k] * fl(c[r] + c[s])) with s the wrap image at the other end of the line; a row is summed in the 13-slot order of
    the periodic `grid_operator`.  A complex `wrap` promotes the element type to ComplexF64 (`coeff` stays real); the traffic per row
    is unchanged.  A band structure at the k-point theta:  `taps, diagonal = extras.diffusion_terms(shape, coeff, spacing, V,
    periodic=True)`, then `grid_variable_operator(shape, taps, coeff, diagonal, periodic=True, wrap=extras.bloch_wrap(taps, theta))`
    -- exactly Hermitian.

    `operator.grid_info`: shape, taps, has_potential, variable=True, bytes_per_row, and with `periodic` or `wrap` given also
    periodic, wrap (as for `grid_operator`)."""
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype)
    c = _grid_coeff(dims, coeff)
    h = C.c_void_p()
    if periodic is None and wrap is None:
        check(lib.ks_operator_grid_var(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data, c.ctypes.data,
                                       None if v is None else v.ctypes.data, C.byref(h)))
        return _grid_operator(ctx, h, dims, dt, t, v, extra_bytes=8, variable=True)
    dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap)
    check(lib.ks_operator_grid_var_periodic(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data, c.ctypes.data,
                                            None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data,
                                            C.byref(h)))
    return _grid_operator(ctx, h, dims, dt, t, v, extra_bytes=8, variable=True, periodic=tuple(bool(f) for f in flags),
                          wrap=None if w is None else w.copy())


def host_grid_variable_matrix(shape, taps, coeff, potential=None, dtype=None, periodic=None, wrap=None):
    """The matrix that defines `grid_variable_operator(shape, taps, coeff, potential)` as a scipy.sparse.csr_matrix
    (`ks_host_grid_var_matrix`: the host path, no device): ascending columns, off-diagonal entries fl(0.5 taps[k] * fl(c[r] + c[s])),
    the diagonal entry centre + potential[r] stored even where it is zero.  `periodic`, `wrap`: as for `grid_variable_operator`
    (`ks_host_grid_var_matrix_periodic`)."""
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype)
    c = _grid_coeff(dims, coeff)
    head = (int(dims.size), dims.ctypes.data)
    if periodic is None and wrap is None:
        n, nnz = _grid_nnz(dims)
        return _host_grid_csr(lib.ks_host_grid_var_matrix, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data, c.ctypes.data,
                              None if v is None else v.ctypes.data)
    dt, t, v, flags, w = _grid_wrap_args(dims, t, v, dt, dtype, periodic, wrap)
    n, nnz = _grid_nnz(dims, 1, flags)
    return _host_grid_csr(lib.ks_host_grid_var_matrix_periodic, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data, c.ctypes.data,
                          None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data)


def _grid_box_nnz(dims, flags=None):
    """(n, nnz) of a box-stencil grid matrix, nnz = prod_a (periodic_a ? 3 m_a : 3 m_a - 2); (0, 0) for a shape that the library
    refuses (so do extents below 3 on a periodic axis: the count is then never used)."""
    n, _ = _grid_nnz(dims)
    flags = [0] * len(dims) if flags is None else flags
    return n, (math.prod(3 * int(d) - (0 if f else 2) for d, f in zip(dims, flags)) if n else 0)


def _grid_box_links_args(dims, t, v, dt, dtype, periodic, links):
    """(dtype, taps, potential, flags, links or None) of a box-stencil grid operator with periodic axes: `periodic` as for
    `_grid_wrap_args`, `links` 5^ndim values, flat or of shape (5,) * ndim in [e_z, e_y, e_x] order.  A complex `links` promotes the
    element type like a complex `wrap` does; a pinned Float64 refuses an imaginary part."""
    ndim = int(dims.size)
    dt, t, v, flags, _ = _grid_wrap_args(dims, t, v, dt, dtype, periodic, None)
    w = None
    if links is not None:
        w = np.asarray(links)
        if w.shape == (5,) * ndim:
            w = w.reshape(-1)
        if w.shape != (5 ** ndim,):
            raise DimensionMismatch(f"the box stencil of a {ndim}-D grid takes {5 ** ndim} link values by class, flat or of shape "
                                    f"{(5,) * ndim} ([e_z, e_y, e_x]), got shape {w.shape}")
        if w.dtype.kind == "c" and dt.kind == "f":
            if dtype is None:   # promote, like complex taps do
                dt = np.dtype(np.complex128)
                t = t.astype(dt)
                v = None if v is None else v.astype(dt)
            else:
                # (entries that are never read may hold anything: the classes that are read decide)
                read = _grid_box_links_read(ndim, flags)
                if np.any(w.imag[read] != 0):
                    raise ArgumentError("links has an imaginary part but the element type is Float64 (KS_F64)")
        w = np.ascontiguousarray(w.real if dt.kind == "f" else w, dtype=dt)
    return dt, t, v, flags, w


def _grid_box_links_read(ndim, flags) -> np.ndarray:
    """Which of the 5^ndim link values the library reads (flat, bool): some axis has class 0 or 4, and every such axis is periodic."""
    e = np.indices((5,) * ndim).reshape(ndim, -1)[::-1]   # e[a]: the class along axis a (x first) of every flat index
    cross = (e == 0) | (e == 4)
    per = np.asarray(flags, dtype=bool)[:, None]
    return cross.any(axis=0) & ~(cross & ~per).any(axis=0)


def grid_box_operator(shape, taps, potential=None, dtype=None, ctx: Context | None = None, periodic=None, links=None) -> Operator:
    """Matrix-free operator of a constant-coefficient 3-, 9- or 27-point BOX stencil plus a per-point diagonal term on a grid
    (`ks_operator_grid_box`): mul!(y, A, x), src/expansion.jl:121, for stencils that link a point to its diagonal neighbours too --
    the mixed derivatives of -div(D grad) + V with a full constant tensor D (`extras.tensor_laplacian_taps`), compact (Mehrstellen)
    Laplacians, stiffness and mass matrices of multilinear (Q1) finite elements on a uniform grid (`extras.q1_fem_taps`) -- with
    nothing stored per non-zero: 24 bytes per row and product in Float64 (16 without a potential) where the stored matrix streams
    about 330.

    `shape`, `potential`, `dtype`: as for `grid_operator` (open boundaries).  `taps`: 3^ndim values in ascending column order --
    flat, slot k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) in 3-D, k = 3 (dy + 1) + (dx + 1) in 2-D, k = dx + 1 in 1-D, or an array of
    shape (3,) * ndim in C order ([dz, dy, dx], so that `taps.ravel()` is the slot order).  Row r has the entry taps[k] at column
    r + dx + nx (dy + ny dz) for every slot whose neighbour lies inside the grid (stored even where the tap is zero); the diagonal
    entry is centre + potential[r].  The operator is exactly the matrix `host_grid_box_matrix` returns, and its products have the
    bits `csr_operator` of that matrix gives.  A variable coefficient and a radius above 1 are not offered.

    `periodic` (`ks_operator_grid_box_periodic`): True, or one bool per axis in the order of `shape`, as for `grid_operator` (extent
    >= 3 on such an axis) -- a crystal in a non-orthogonal cell, Q1 elements or a compact Laplacian on a torus.  A diagonal link can
    cross two or three cell faces at once, so the entries of the crossing links are given per CLASS: `links` holds 5^ndim values,
    flat or of shape (5,) * ndim in [e_z, e_y, e_x] order, the class e along an axis being 0 = offset -1 across the boundary,
    1 = offset -1, 2 = offset 0, 3 = offset +1, 4 = offset +1 across the boundary.  Only entries with a class 0 or 4, all on periodic
    axes, are read (the others may hold anything, NaN included); None = the tap of the link's slot (a plain torus),
    `extras.box_bloch_links(taps, theta)` = Bloch phases, `-extras.box_bloch_links(taps, np.zeros(ndim)).real` = antiperiodic.  At the
    first point of a periodic axis a row takes the offsets in the order (0, +1, -1), at the last in the order (+1, -1, 0): ascending
    columns.  A complex `links` promotes the element type; the traffic per row is unchanged.

    `operator.grid_info`: shape, taps (flat), has_potential, box=True, bytes_per_row, and with `periodic` or `links` given also
    periodic, links (flat, or None)."""
    ctx = ctx or default_context()
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, box=True)
    h = C.c_void_p()
    if periodic is None and links is None:
        check(lib.ks_operator_grid_box(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data,
                                       None if v is None else v.ctypes.data, C.byref(h)))
        return _grid_operator(ctx, h, dims, dt, t, v, box=True)
    dt, t, v, flags, w = _grid_box_links_args(dims, t, v, dt, dtype, periodic, links)
    check(lib.ks_operator_grid_box_periodic(ctx._h, int(dims.size), dims.ctypes.data, _dtype_code(dt), t.ctypes.data,
                                            None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data,
                                            C.byref(h)))
    return _grid_operator(ctx, h, dims, dt, t, v, box=True, periodic=tuple(bool(f) for f in flags), links=None if w is None else w.copy())


def host_grid_box_matrix(shape, taps, potential=None, dtype=None, periodic=None, links=None):
    """The matrix that defines `grid_box_operator(shape, taps, potential)` as a scipy.sparse.csr_matrix (`ks_host_grid_box_matrix`:
    the host path, no device): ascending columns, nnz = prod_a (3 m_a - 2), an entry stored even where its tap is zero, the diagonal
    entry centre + potential[r].  In 1-D it is the matrix of `host_grid_matrix`.  `periodic`, `links`: as for `grid_box_operator`
    (`ks_host_grid_box_matrix_periodic`), nnz = prod_a (periodic_a ? 3 m_a : 3 m_a - 2)."""
    lib = _lib.load()
    dt, dims, t, v = _grid_args(shape, taps, potential, dtype, box=True)
    head = (int(dims.size), dims.ctypes.data)
    if periodic is None and links is None:
        n, nnz = _grid_box_nnz(dims)
        return _host_grid_csr(lib.ks_host_grid_box_matrix, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data,
                              None if v is None else v.ctypes.data)
    dt, t, v, flags, w = _grid_box_links_args(dims, t, v, dt, dtype, periodic, links)
    n, nnz = _grid_box_nnz(dims, flags)
    return _host_grid_csr(lib.ks_host_grid_box_matrix_periodic, n, nnz, dt, *head, _dtype_code(dt), t.ctypes.data,
                          None if v is None else v.ctypes.data, flags.ctypes.data, None if w is None else w.ctypes.data)


def host_operator(fn, n: int, dtype=np.float64, ctx: Context | None = None) -> Operator:
    """Opaque host operator: `fn(y, x)` fills y = A*x on numpy views (a LinearMap wrapping ldiv!,
    docs/src/index.md:246-249).  Columns are staged over PCIe by the library."""
    ctx = ctx or default_context()
    L = _lib.load()
    dt = np.dtype(vtype(np.empty(0, dtype=dtype)))
    err = []

    def _cb(_user, xp, yp):
        try:
            x = np.ctypeslib.as_array(C.cast(xp, C.POINTER(C.c_double)), shape=(n * (2 if dt.kind == "c" else 1),)).view(dt)
            y = np.ctypeslib.as_array(C.cast(yp, C.POINTER(C.c_double)), shape=(n * (2 if dt.kind == "c" else 1),)).view(dt)
            fn(y, x)
            return 0
        except Exception as e:  # noqa: BLE001 - must not propagate through C
            err.append(e)
            return 1

    cb = _lib.HOST_APPLY_FN(_cb)
    h = C.c_void_p()
    check(L.ks_operator_host_callback(ctx._h, n, _dtype_code(dt), cb, None, C.byref(h)))
    op = Operator(ctx, h, (n, n), dt, keep=(cb, err))
    op.errors = err
    return op


class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can wrap a raw device pointer without copying."""

    def __init__(self, ptr: int, n: int, dt: np.dtype):
        self.__cuda_array_interface__ = {
            "shape": (n,), "typestr": "<c16" if dt.kind == "c" else "<f8", "data": (ptr, False), "version": 2, "strides": None,
        }


def device_operator(fn, n: int, dtype=np.float64, ctx: Context | None = None) -> Operator:
    """Opaque DEVICE operator: `fn(y, x)` receives two torch tensors that alias columns of V in HBM and must
    enqueue y = A*x on the current torch stream (which is the library's stream while `fn` runs).  This is the
    device-resident form of the `mul!(y, A, x)` seam (src/expansion.jl:121): e.g. a dense matrix via
    `torch.mv`, a matrix-free stencil, a preconditioned solve.  torch is only plumbing here."""
    import torch

    ctx = ctx or default_context()
    L = _lib.load()
    dt = np.dtype(vtype(np.empty(0, dtype=dtype)))
    err = []

    def _cb(_user, xp, yp, stream):
        try:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=torch.device("cuda", ctx.device))):
                x = torch.as_tensor(_DevArray(xp, n, dt), device=torch.device("cuda", ctx.device))
                y = torch.as_tensor(_DevArray(yp, n, dt), device=torch.device("cuda", ctx.device))
                fn(y, x)
            return 0
        except Exception as e:  # noqa: BLE001 - must not propagate through C
            err.append(e)
            return 1

    cb = _lib.DEVICE_APPLY_FN(_cb)
    h = C.c_void_p()
    check(L.ks_operator_device_callback(ctx._h, n, _dtype_code(dt), cb, None, C.byref(h)))
    op = Operator(ctx, h, (n, n), dt, keep=(cb, err))
    op.errors = err
    return op


def dense_operator(A, ctx: Context | None = None) -> Operator:
    """mul!(y, A::Matrix, x): the dense matrix lives row-major in HBM (ks_operator_dense)."""
    ctx = ctx or default_context()
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise DimensionMismatch(f"matrix is not square: dimensions are {A.shape}")
    dt = vtype(A)
    col_major = A.flags.f_contiguous and not A.flags.c_contiguous
    M = np.asfortranarray(A, dtype=dt) if col_major else np.ascontiguousarray(A, dtype=dt)
    h = C.c_void_p()
    check(_lib.load().ks_operator_dense(ctx._h, A.shape[0], M.ctypes.data, A.shape[0], 1 if col_major else 0, _dtype_code(dt), C.byref(h)))
    return Operator(ctx, h, A.shape, dt)


def as_operator(A, ctx: Context | None = None) -> Operator:
    import scipy.sparse as sp

    if isinstance(A, Operator):
        return A
    if isinstance(A, np.ndarray):
        # a mostly-zero array is cheaper as CSR (12 B per stored entry vs 8 B per entry of the dense stream)
        if A.ndim == 2 and A.size and np.count_nonzero(A) > 0.5 * A.size:
            return dense_operator(A, ctx)
        return csr_operator(A, ctx)
    if sp.issparse(A):
        return csr_operator(A, ctx)
    if all(hasattr(A, k) for k in ("L", "U", "perm_r", "perm_c", "solve")):
        return splu_operator(A, ctx)  # a scipy SuperLU factorisation: the operator is x -> A^-1 x, applied on the device
    shp = getattr(A, "shape", None)
    if shp is None or len(shp) != 2 or shp[0] != shp[1]:
        raise DimensionMismatch(f"matrix is not square: dimensions are {shp}")
    if hasattr(A, "mul_"):
        return host_operator(lambda y, x: A.mul_(y, x), shp[0], getattr(A, "dtype", np.float64), ctx)
    if hasattr(A, "matvec"):
        def f(y, x):
            y[:] = A.matvec(x)
        return host_operator(f, shp[0], getattr(A, "dtype", np.float64), ctx)
    raise TypeError("operator must be a scipy.sparse matrix, an ndarray, an Operator, or implement mul_/matvec")


# ------------------------------------------------------------------ workspace (src/ArnoldiMethod.jl:41-93)
class ArnoldiWorkspace:
    """V (n x (k+1), in HBM), H ((k+1) x k, host, zero-initialised), Q (k x k, host).

    ArnoldiWorkspace(n, k [, dtype])  or  ArnoldiWorkspace(v1, k)  (the array type follows v1).

    Deviation from the reference, on purpose: `ArnoldiWorkspace(v1, k)` (src/ArnoldiMethod.jl:71-79) only takes the ARRAY
    TYPE from `v1` and `partialschur!` then starts from `rand!` (src/run.jl:177); here the workspace remembers `v1` and
    `partialschur_(A, ws)` with `initialize=True, start_from=1` starts from it -- the tests need reproducible start
    vectors and Python has no array-type dispatch to express the original meaning.  Pass `ArnoldiWorkspace(n, k)` to get
    the reference's random start (counter-based RNG, `set_seed`)."""

    def __init__(self, n_or_v1, krylov_dimension: int, dtype=np.float64, ctx: Context | None = None,
                 n_global: int | None = None, row_begin: int = 0):
        self.ctx = ctx or default_context()
        L = _lib.load()
        self._v1 = None
        if isinstance(n_or_v1, (int, np.integer)):
            n = int(n_or_v1)
        else:
            v1 = np.asarray(n_or_v1)
            n = v1.shape[0]
            dtype = vtype(v1)
            self._v1 = np.ascontiguousarray(v1.astype(dtype))
        self.dtype = np.dtype(vtype(np.empty(0, dtype=dtype)))
        ng = n if n_global is None else int(n_global)
        if not krylov_dimension <= ng:
            raise ArgumentError("Krylov dimension should be less than matrix order.")
        h = C.c_void_p()
        check(L.ks_workspace_create(self.ctx._h, n, ng, row_begin, krylov_dimension, _dtype_code(self.dtype), C.byref(h)))
        self._h = h
        self.n, self.n_global, self.maxdim = n, ng, krylov_dimension
        self.H = self._host_matrix(L.ks_workspace_H, krylov_dimension + 1, krylov_dimension)
        self.Q = self._host_matrix(L.ks_workspace_Q, krylov_dimension, krylov_dimension)

    def _host_matrix(self, getter, rows, cols):
        p, ld = C.c_void_p(), C.c_int()
        check(getter(self._h, C.byref(p), C.byref(ld)))
        nd = 2 if self.dtype.kind == "c" else 1
        flat = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(ld.value * cols * nd,))
        return flat.view(self.dtype).reshape((ld.value, cols), order="F")[:rows, :]

    # --- the verbs the reference applies to V ---
    def set_seed(self, seed: int):
        check(_lib.load().ks_workspace_set_seed(self._h, seed))

    def col(self, j: int) -> np.ndarray:
        out = np.empty(self.n, dtype=self.dtype)
        check(_lib.load().ks_col_download(self._h, j, out.ctypes.data))
        return out

    def cols(self, j0: int, ncols: int) -> np.ndarray:
        out = np.empty((self.n, ncols), dtype=self.dtype, order="F")
        if ncols and self.n:
            check(_lib.load().ks_cols_download(self._h, j0, ncols, out.ctypes.data, self.n))
        return out

    def set_col(self, j: int, v):
        v = np.ascontiguousarray(np.asarray(v, dtype=self.dtype))
        if v.shape != (self.n,):
            raise ArgumentError("v1 should have the same dimension as A")
        check(_lib.load().ks_col_upload(self._h, j, v.ctypes.data))

    def set_cols(self, j0: int, M):
        M = np.asfortranarray(np.asarray(M, dtype=self.dtype))
        check(_lib.load().ks_cols_upload(self._h, j0, M.shape[1], M.ctypes.data, M.shape[0]))

    @property
    def V(self) -> np.ndarray:
        """Host copy of the whole basis (tests / small problems only)."""
        return self.cols(0, self.maxdim + 1)

    def fill_uniform(self, j: int, seed: int):
        check(_lib.load().ks_col_fill_uniform(self._h, j, seed))

    def norm(self, j: int) -> float:
        out = C.c_double()
        check(_lib.load().ks_col_norm(self._h, j, C.byref(out)))
        return out.value

    def div(self, j: int, s: float):
        check(_lib.load().ks_col_div(self._h, j, s))

    def copy_col(self, dst: int, src: int):
        check(_lib.load().ks_col_copy(self._h, dst, src))

    def apply(self, A: Operator, jsrc: int, jdst: int):
        _check_op(_lib.load().ks_apply(A._h, self._h, jsrc, jdst), A)

    def apply_shifted(self, A: Operator, jsrc: int, jdst: int, theta, sigma: float, cacheable: bool = False):
        """Column jdst = sigma (A column jsrc - theta column jsrc): one Newton step of the s-step expansion (diagnostics)."""
        theta = complex(theta)
        _check_op(_lib.load().ks_debug_apply_shifted(A._h, self._h, jsrc, jdst, theta.real, theta.imag, float(sigma), int(bool(cacheable))), A)

    def apply_clenshaw(self, A: Operator, jsrc: int, jdst: int, jw: int | None, jx0: int | None, theta, sigma: float, gamma: float,
                       cacheable: bool = False):
        """Column jdst = sigma (A column jsrc - theta column jsrc) - column jw + gamma column jx0: one Clenshaw step of a
        Chebyshev filter (diagnostics).  jw / jx0 = None: no such term."""
        theta = complex(theta)
        _check_op(_lib.load().ks_debug_apply_clenshaw(A._h, self._h, jsrc, jdst, -1 if jw is None else jw, -1 if jx0 is None else jx0,
                                                      theta.real, theta.imag, float(sigma), float(gamma), int(bool(cacheable))), A)

    def gemv_t(self, j: int, jv: int) -> np.ndarray:
        h = np.empty(j, dtype=self.dtype)
        check(_lib.load().ks_gemv_t(self._h, j, jv, h.ctypes.data))
        return h

    def gemv_n_sub(self, j: int, jv: int, h):
        h = np.ascontiguousarray(np.asarray(h, dtype=self.dtype))
        check(_lib.load().ks_gemv_n_sub(self._h, j, jv, h.ctypes.data))

    def rotate(self, c0: int, Qblock):
        Qb = np.asfortranarray(np.asarray(Qblock, dtype=self.dtype))
        c, r = Qb.shape
        check(_lib.load().ks_rotate(self._h, c0, c, r, Qb.ctypes.data, c))

    def basis_times(self, c: int, Y) -> np.ndarray:
        Y = np.asarray(Y)
        ydt = np.complex128 if (Y.dtype.kind == "c" or self.dtype.kind == "c") else np.float64
        Yf = np.asfortranarray(Y.astype(ydt))
        out = np.empty((self.n, Yf.shape[1]), dtype=ydt, order="F")
        check(_lib.load().ks_basis_times(self._h, c, Yf.shape[1], Yf.ctypes.data, Yf.shape[0], _dtype_code(ydt), out.ctypes.data, self.n))
        return out

    def basis_times_device(self, c: int, Y) -> "DeviceVectors":
        """`basis_times` with the product left in HBM (`ks_basis_times_device`): no copy of the vectors to the host."""
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.shape[0] != c or Y.shape[1] < 1:
            raise DimensionMismatch(f"coefficients must be ({c}, r) with r >= 1, got {Y.shape}")
        ydt = np.complex128 if (Y.dtype.kind == "c" or self.dtype.kind == "c") else np.float64
        Yf = np.asfortranarray(Y.astype(ydt))
        out = DeviceVectors(self.n, Yf.shape[1], ydt, self.ctx)
        check(_lib.load().ks_basis_times_device(self._h, c, Yf.shape[1], Yf.ctypes.data, Yf.shape[0], _dtype_code(ydt), out._h))
        return out

    def orthogonalize(self, j: int) -> bool:
        ok = C.c_int()
        check(_lib.load().ks_orthogonalize(self._h, j, C.byref(ok)))
        return bool(ok.value)

    def reinitialize(self, j: int = 0, v1=None) -> bool:
        ok = C.c_int()
        p = None
        if v1 is not None:
            v1 = np.ascontiguousarray(np.asarray(v1, dtype=self.dtype))
            p = v1.ctypes.data
        check(_lib.load().ks_reinitialize(self._h, j, p, C.byref(ok)))
        return bool(ok.value)

    def iterate_arnoldi(self, A: Operator, frm: int, to: int):
        st = _lib.ks_expand_stats()
        _check_op(_lib.load().ks_iterate_arnoldi(A._h, self._h, frm, to, C.byref(st)), A)
        return dict(steps=st.steps, reorth=st.reorth, breakdowns=st.breakdowns, explicit_steps=st.explicit_steps)

    def restart(self, active: int, nev: int, which="LM", tol=None, mindim=None, maxdim=None):
        """One Krylov-Schur restart (src/run.jl:278-365): host Schur / grouping / restore, then the
        basis rotation on the device.  `active` is 0-based.  Returns dict(k, nlock, purge, ...)."""
        maxdim = self.maxdim if maxdim is None else maxdim
        mindim = min(max(10, nev), self.n_global) if mindim is None else mindim
        tol = math.sqrt(EPS) if tol is None else tol
        p = _lib.ks_params(nev, _which_code(which), float(tol), mindim, maxdim, 1, 1, 0, 0)
        k, nlock, purge = C.c_int(), C.c_int(), C.c_int()
        lams, rs, groups = np.zeros(2 * maxdim), np.zeros(maxdim), np.zeros(maxdim, dtype=np.int32)
        check(_lib.load().ks_restart(self._h, C.byref(p), active, C.byref(k), C.byref(nlock), C.byref(purge),
                                     lams.ctypes.data, rs.ctypes.data, groups.ctypes.data))
        return dict(k=k.value, nlock=nlock.value, purge=purge.value, eigenvalues=lams[0::2] + 1j * lams[1::2],
                    residuals=rs, groups=groups)

    def expand_restart(self, A: Operator, k: int, active: int, nev: int, which="LM", tol=None, mindim=None, maxdim=None):
        """One whole cycle of `_partialschur`'s loop (src/run.jl:272-365): iterate_arnoldi!(k+1 : maxdim) and the restart in
        ONE library call (what `partialschur` does internally; bit-identical to iterate_arnoldi + restart).  With the explicit
        second pass (`passes == 3`) the early part of the restart's host work overlaps the tail of the expansion; with the
        implicit second pass (default) H is final only when the batch ends.  `k` = basis size the previous restart
        left.  Returns restart()'s dict plus steps / reorth / breakdowns and seconds = (expansion, host, rotation enqueue)."""
        maxdim = self.maxdim if maxdim is None else maxdim
        mindim = min(max(10, nev), self.n_global) if mindim is None else mindim
        tol = math.sqrt(EPS) if tol is None else tol
        p = _lib.ks_params(nev, _which_code(which), float(tol), mindim, maxdim, 1, 1, 0, 0)
        ko, nlock, purge = C.c_int(), C.c_int(), C.c_int()
        lams, rs, groups = np.zeros(2 * maxdim), np.zeros(maxdim), np.zeros(maxdim, dtype=np.int32)
        st = _lib.ks_expand_stats()
        sec = np.zeros(3)
        _check_op(_lib.load().ks_expand_restart(A._h, self._h, C.byref(p), active, k, C.byref(ko), C.byref(nlock), C.byref(purge),
                                                lams.ctypes.data, rs.ctypes.data, groups.ctypes.data, C.byref(st), sec.ctypes.data), A)
        return dict(k=ko.value, nlock=nlock.value, purge=purge.value, eigenvalues=lams[0::2] + 1j * lams[1::2], residuals=rs,
                    groups=groups, steps=st.steps, reorth=st.reorth, breakdowns=st.breakdowns, explicit_steps=st.explicit_steps,
                    seconds=tuple(sec))

    def residual_norms(self, A: Operator, ncols: int):
        r, o = C.c_double(), C.c_double()
        _check_op(_lib.load().ks_residual_norms(A._h, self._h, ncols, C.byref(r), C.byref(o)), A)
        return r.value, o.value

    def arnoldi_relation(self, A: Operator, k: int):
        r, o = C.c_double(), C.c_double()
        _check_op(_lib.load().ks_arnoldi_relation(A._h, self._h, k, C.byref(r), C.byref(o)), A)
        return r.value, o.value

    @property
    def passes(self) -> int:
        """Reads of the basis per fused expansion step: 2 (implicit second pass, default) or 3 (KS_PASSES=3)."""
        k = C.c_int()
        check(_lib.load().ks_workspace_passes(self._h, C.byref(k)))
        return k.value

    def set_passes(self, passes: int, max_ratio: float = float("nan")):
        """Per-workspace switch: 2 = implicit second DGKS pass, 3 = explicit; `max_ratio` = largest ||c|| / beta the
        implicit form carries before a step is redone explicitly (NaN keeps the current value, <= 0 removes the limit)."""
        check(_lib.load().ks_workspace_set_passes(self._h, int(passes), float(max_ratio)))

    def set_sstep(self, s: int, pivot_min: float = float("nan"), gram_dev_max: float = float("nan")):
        """s-step (block) expansion: s >= 2 takes the steps of an expansion in blocks of up to s (two reads of the basis per
        BLOCK instead of per step; include/kschur.h, ks_workspace_set_sstep); 0 switches it off.  `pivot_min`: smallest
        Cholesky pivot ratio, `gram_dev_max`: largest deviation of the written block's Gram matrix from I a block may have
        before it is abandoned and redone step by step (NaN keeps the value)."""
        check(_lib.load().ks_workspace_set_sstep(self._h, int(s), float(pivot_min), float(gram_dev_max)))

    @property
    def sstep_info(self) -> dict:
        """Block size in force, blocks completed / abandoned since creation, and of the last batch: smallest pivot ratios of
        the two Gram-Schmidt stages and the largest entry of |Gram matrix of the written block - I|."""
        s, b, a = C.c_int(), C.c_int(), C.c_int()
        d = (C.c_double * 3)()
        check(_lib.load().ks_workspace_sstep_info(self._h, C.byref(s), C.byref(b), C.byref(a), d))
        fr, sa, sd = C.c_int(), C.c_int(), C.c_int()
        check(_lib.load().ks_workspace_fused_rotations(self._h, C.byref(fr), C.byref(sa), C.byref(sd)))
        sr = C.c_int()
        check(_lib.load().ks_workspace_split_rotations(self._h, C.byref(sr)))
        db, dc = C.c_int(), C.c_int()
        check(_lib.load().ks_workspace_deflated_blocks(self._h, C.byref(db), C.byref(dc)))
        return dict(s=s.value, blocks=b.value, abandoned=a.value, pivot_stage1=d[0], pivot_stage2=d[1], gram_dev=d[2], fused_rotations=fr.value,
                    split_rotations=sr.value, chains_adopted=sa.value, chains_dropped=sd.value, deflated_blocks=db.value, deflated_columns=dc.value)

    @property
    def relation_info(self) -> dict:
        """Restarts that cut through a 2 x 2 block of the real Schur form (ks_workspace_relation_info): count and the largest
        dropped entry relative to ||H||_F.  After the first one the s-step expansion stays off for the run.  `probes`: relation
        measurements taken on factorisations a caller vouched for (ks_workspace_relation_probes)."""
        b, w = C.c_int(), C.c_double()
        check(_lib.load().ks_workspace_relation_info(self._h, C.byref(b), C.byref(w)))
        pr = C.c_int()
        check(_lib.load().ks_workspace_relation_probes(self._h, C.byref(pr)))
        return dict(breaks=b.value, worst_leak=w.value, probes=pr.value)

    def assert_arnoldi(self, k: int):
        """The caller vouches that columns 0..k are orthonormal and satisfy, with the H now in `self.H`, the Arnoldi
        relation of k steps (a restart the host language ran itself): re-enables the implicit second pass."""
        check(_lib.load().ks_workspace_assert_arnoldi(self._h, int(k)))

    @property
    def provenance(self) -> int:
        """Steps of the factorisation the library trusts as its own (-1: none) -- see ks_workspace_assert_arnoldi."""
        k = C.c_int()
        check(_lib.load().ks_workspace_provenance(self._h, C.byref(k)))
        return k.value

    @property
    def placement(self) -> dict:
        """Outcome of the placement search at creation: candidates timed, calibration ms of the kept / slowest one."""
        k, b, w, r = C.c_int(), C.c_double(), C.c_double(), C.c_int()
        check(_lib.load().ks_workspace_placement(self._h, C.byref(k), C.byref(b), C.byref(w), C.byref(r)))
        return dict(candidates=k.value, kept_ms=b.value, slowest_ms=w.value, refused=r.value)

    def guard_intact(self) -> bool:
        """KS_GUARD=1 debugging: True unless a kernel wrote outside the basis."""
        ok = C.c_int()
        check(_lib.load().ks_workspace_check_guard(self._h, C.byref(ok)))
        return bool(ok.value)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            _lib.load().ks_workspace_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sstep_partition(dtype, k0: int, count: int, smax: int) -> list:
    """Block sizes the s-step expansion uses for `count` steps on top of `k0` existing columns (ks_sstep_partition: the
    library's own blk_partition, csrc/ks_block.hpp -- the sizes depend on which kernel forms are switched on; [] = not
    block-capable).  For byte accounting in benchmarks: a block of s steps on k columns reads 8 n (k + s) + 8 n (k + s) and
    writes 8 n s bytes (x2 for ComplexF64) next to its s operator products."""
    if k0 < 1 or count < 1 or smax < 1:
        return []
    cap = 64
    out = (C.c_int * cap)()
    nb = C.c_int(0)
    check(_lib.load().ks_sstep_partition(_dtype_code(dtype), int(k0), int(count), int(smax), out, cap, C.byref(nb)))
    return [int(out[i]) for i in range(min(nb.value, cap))]


# ------------------------------------------------------------------ results
class PartialSchur:
    """src/ArnoldiMethod.jl:130-137.  `Q` stays in HBM (a view of the workspace's V, src/run.jl:375,389)
    and is downloaded on first access; `R` is a view of the workspace's host H."""

    def __init__(self, ws: ArnoldiWorkspace, nconv: int, eigenvalues: np.ndarray):
        self.workspace = ws
        self.nconverged = nconv
        self.R = ws.H[:nconv, :nconv]
        self.eigenvalues = eigenvalues
        self._Q = None

    @property
    def Q(self) -> np.ndarray:
        if self._Q is None:
            self._Q = self.workspace.cols(0, self.nconverged)
        return self._Q

    def __repr__(self):  # src/show.jl:23-33
        return (
            f"PartialSchur decomposition ({'ComplexF64' if self.workspace.dtype.kind == 'c' else 'Float64'}) "
            f"of dimension {self.nconverged}\neigenvalues:\n{self.eigenvalues!r}"
        )


@dataclass
class History:
    """src/run.jl:217-222 (+ timing diagnostics of the device path)."""

    mvproducts: int
    nconverged: int
    converged: bool
    nev: int
    restarts: int = 0
    reorth: int = 0
    breakdowns: int = 0
    explicit_steps: int = 0  # steps the implicit second DGKS pass handed back to the explicit form
    seconds_expand: float = 0.0
    seconds_host: float = 0.0
    seconds_rotate: float = 0.0

    def __str__(self):  # src/show.jl:3-21
        head = "Converged" if self.converged else "Not converged"
        return f"{head}: {self.nconverged} of {self.nev} eigenvalues in {self.mvproducts} matrix-vector products"


# ------------------------------------------------------------------ drivers
def _run(op: Operator, ws: ArnoldiWorkspace, nev, which, tol, mindim, maxdim, restarts, start_from, initialize, v1):
    L = _lib.load()
    p = _lib.ks_params(nev, _which_code(which), float(tol), mindim, maxdim, restarts, start_from, 1 if initialize else 0, 0)
    h = _lib.ks_history()
    eig = np.zeros(2 * max(maxdim, 1))
    v1p = None
    if v1 is not None:
        v1 = np.ascontiguousarray(np.asarray(v1, dtype=ws.dtype))
        v1p = v1.ctypes.data
    _check_op(L.ks_partialschur(op._h, ws._h, C.byref(p), v1p, eig.ctypes.data, C.byref(h)), op)
    lam = (eig[0::2] + 1j * eig[1::2])[: h.nconverged].copy()
    hist = History(h.mvproducts, h.nconverged, bool(h.converged), h.nev, h.restarts, h.reorth, h.breakdowns, h.explicit_steps,
                   h.seconds_expand, h.seconds_host, h.seconds_rotate)
    return PartialSchur(ws, h.nconverged, lam), hist


def partialschur(A, v1=None, nev=None, which="LM", tol=None, mindim=None, maxdim=None, restarts=200,
                 seed=DEFAULT_SEED, ctx: Context | None = None):
    """partialschur(A; v1, nev, which, tol, mindim, maxdim, restarts) -> (PartialSchur, History)

    src/run.jl:100-129.  A: scipy.sparse matrix / ndarray (uploaded as device CSR), an `Operator`, or
    any object with `mul_(y, x)` / `matvec(x)` (host-callback operator)."""
    shp = getattr(A, "shape", None)
    if shp is None or len(shp) != 2 or shp[0] != shp[1]:
        raise DimensionMismatch(f"matrix is not square: dimensions are {tuple(shp) if shp else shp}")
    n = shp[0]
    if nev is None:
        nev = min(6, n)
    if tol is None:
        tol = math.sqrt(EPS)
    if mindim is None:
        mindim = min(max(10, nev), n)
    if maxdim is None:
        maxdim = min(max(20, 2 * nev), n)
    if nev < 1:
        raise ArgumentError("nev cannot be less than 1")
    if not (nev <= mindim <= maxdim <= n):
        raise ArgumentError(f"nev ≤ mindim ≤ maxdim ≤ size(A, 1) does not hold, got {nev} ≤ {mindim} ≤ {maxdim} ≤ {n}")
    _which_code(which)
    if v1 is not None and len(v1) != n:
        raise ArgumentError("v1 should have the same dimension as A")
    v1_complex = v1 is not None and np.asarray(v1).dtype.kind == "c"
    if v1_complex and not isinstance(A, Operator) and np.dtype(getattr(A, "dtype", np.float64)).kind != "c" and hasattr(A, "astype"):
        # ArnoldiWorkspace(v1, maxdim) takes the element type of v1 (src/ArnoldiMethod.jl:71-79): a real matrix
        # with a complex start vector runs in complex arithmetic
        A = A.astype(np.complex128)
    op = as_operator(A, ctx)
    dtype = np.complex128 if (op.dtype.kind == "c" or v1_complex) else np.float64
    if np.dtype(dtype) != op.dtype:
        raise ArgumentError("a complex start vector needs a complex operator")
    ws = ArnoldiWorkspace(n, maxdim, dtype, ctx=op.ctx)
    ws.set_seed(seed)
    return _run(op, ws, nev, which, tol, mindim, maxdim, restarts, 1, True, v1)


def partialschur_(A, arnoldi: ArnoldiWorkspace, start_from=1, initialize=None, nev=None, which="LM", tol=None,
                  mindim=None, maxdim=None, restarts=200):
    """`partialschur!(A, arnoldi; start_from, initialize, ...)`, src/run.jl:152-179."""
    shp = getattr(A, "shape", None)
    if shp is None or len(shp) != 2 or shp[0] != shp[1]:
        raise DimensionMismatch(f"matrix is not square: dimensions are {tuple(shp) if shp else shp}")
    s = shp[0]
    ncolsV = arnoldi.maxdim + 1
    if initialize is None:
        initialize = start_from == 1
    if nev is None:
        nev = min(6, s)
    if tol is None:
        tol = math.sqrt(EPS)
    if mindim is None:
        mindim = min(max(10, nev), s, ncolsV - 1)
    if maxdim is None:
        maxdim = min(max(20, 2 * nev), s, ncolsV - 1)
    if nev < 1:
        raise ArgumentError("nev cannot be less than 1")
    if not (nev <= mindim <= maxdim <= s):
        raise ArgumentError(f"nev ≤ mindim ≤ maxdim ≤ size(A, 1) does not hold, got {nev} ≤ {mindim} ≤ {maxdim} ≤ {s}")
    if not maxdim < ncolsV:
        raise ArgumentError("maxdim should be strictly less than size(arnoldi.V, 2)")
    if not (1 <= start_from <= maxdim):
        raise ArgumentError("start_from should be between 1 and maxdim")
    _which_code(which)
    op = as_operator(A, arnoldi.ctx)
    v1 = arnoldi._v1 if (initialize and start_from == 1) else None
    return _run(op, arnoldi, nev, which, tol, mindim, maxdim, restarts, start_from, initialize, v1)


def partialeigen(P: PartialSchur, device: bool = False):
    """partialeigen(P) -> (eigenvalues, eigenvectors), src/eigvals.jl:92-95: LAPACK `eigen(R)` on the
    host (nev x nev) and the tall-skinny product Q*vecs on the device.  `device=True` leaves the eigenvectors in HBM and
    returns them as `DeviceVectors` (`ks_basis_times_device`) for `residuals` / `gram` / `DeviceVectors.apply`."""
    import scipy.linalg as sla

    k = P.nconverged
    if k == 0:
        if device:
            raise ArgumentError("no converged eigenvalues: there are no vectors to keep on the device")
        return np.zeros(0, dtype=np.complex128), np.zeros((P.workspace.n, 0), dtype=np.complex128)
    vals, vecs = sla.eig(np.array(P.R))
    if P.workspace.dtype.kind == "f" and np.all(vals.imag == 0):
        vecs = vecs.real
    if device:
        return vals, P.workspace.basis_times_device(k, vecs)
    return vals, P.workspace.basis_times(k, vecs)


# ------------------------------------------------------------------ device-resident vectors
class DeviceVectors:
    """n x r vectors in HBM (`ks_vectors`, include/kschur.h): operators are applied to them column by column and their residuals
    and Gram matrices come back as a few small numbers, so the recipes of the reference's "Bringing problems to standard form"
    stay on the device through "translate back" (docs/src/index.md:347) and the checks against the ORIGINAL matrices
    (docs/src/index.md:258, 302, 350-351).  1 <= r <= 64."""

    def __init__(self, n: int, ncols: int, dtype=np.float64, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.dtype = np.dtype(vtype(np.empty(0, dtype=dtype)))
        self.shape = (int(n), int(ncols))
        h = C.c_void_p()
        check(_lib.load().ks_vectors_create(self.ctx._h, int(n), int(ncols), _dtype_code(self.dtype), C.byref(h)))
        self._h = h

    @classmethod
    def from_host(cls, M, ctx: Context | None = None) -> "DeviceVectors":
        M = np.asarray(M)
        if M.ndim != 2:
            raise DimensionMismatch(f"vectors must be a matrix (n, r), got shape {M.shape}")
        X = cls(M.shape[0], M.shape[1], vtype(M), ctx)
        Mf = np.asfortranarray(M.astype(X.dtype))
        if Mf.shape[0]:
            check(_lib.load().ks_vectors_upload(X._h, 0, Mf.shape[1], Mf.ctypes.data, Mf.shape[0]))
        return X

    def download(self) -> np.ndarray:
        n, r = self.shape
        out = np.empty((n, r), dtype=self.dtype, order="F")
        if n:
            check(_lib.load().ks_vectors_download(self._h, 0, r, out.ctypes.data, n))
        return out

    @property
    def ld(self) -> int:
        """Leading dimension in elements (a multiple of 64; rows n .. ld-1 of every column are zero)."""
        ld = C.c_int64()
        check(_lib.load().ks_vectors_dims(self._h, None, None, None, C.byref(ld)))
        return ld.value

    def col_ptr(self, j: int) -> int:
        """Device address of column j (`ld` elements, the first n of them the column)."""
        p = C.c_void_p()
        check(_lib.load().ks_vectors_col_ptr(self._h, int(j), C.byref(p)))
        return p.value or 0

    def apply(self, op: Operator) -> "DeviceVectors":
        """op applied to every column, as new vectors; a Float64 operator on ComplexF64 vectors acts on the real and the imaginary
        part.  An exception raised inside a Python callback operator surfaces as that exception."""
        _check_apply(op, self)
        out = DeviceVectors(self.shape[0], self.shape[1], self.dtype, self.ctx)
        _check_op(_lib.load().ks_vectors_apply(op._h, self._h, out._h), op)
        return out

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            _lib.load().ks_vectors_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_apply(op, X):
    """The argument checks of `DeviceVectors.apply` / `residuals`, before any device call."""
    if not isinstance(op, Operator):
        raise ArgumentError(f"expected an Operator, got {type(op).__name__}")
    if not isinstance(X, DeviceVectors):
        raise ArgumentError(f"expected DeviceVectors, got {type(X).__name__}")
    if op.shape[0] != X.shape[0]:
        raise DimensionMismatch(f"the operator has {op.shape[0]} rows, the vectors have {X.shape[0]}")
    if op.ctx is not X.ctx:
        raise ArgumentError("the operator and the vectors live on different contexts")
    if op.dtype.kind == "c" and X.dtype.kind != "c":
        raise ArgumentError("a ComplexF64 operator needs ComplexF64 vectors")


def _check_pair(X, Y, same_cols: bool):
    for V in (X, Y):
        if not isinstance(V, DeviceVectors):
            raise ArgumentError(f"expected DeviceVectors, got {type(V).__name__}")
    if X.shape[0] != Y.shape[0] or (same_cols and X.shape[1] != Y.shape[1]):
        raise DimensionMismatch(f"the vectors have shapes {X.shape} and {Y.shape}")
    if X.dtype != Y.dtype:
        raise ArgumentError(f"the vectors have element types {X.dtype} and {Y.dtype}")
    if X.ctx is not Y.ctx:
        raise ArgumentError("the vectors live on different contexts")


def residual_coefficients(lam_or_C, r: int, dtype) -> np.ndarray:
    """The r x r coefficient block of `residuals` in the vectors' element type: a 1-D `lam` (r eigenvalues) becomes diag(lam), a 2-D
    block (R of a Schur decomposition, or a block-diagonal matrix whose real 2 x 2 blocks carry conjugate pairs) is taken as it
    is.  Complex coefficients with Float64 vectors are an ArgumentError (use the complex vectors of `partialeigen`)."""
    dt = np.dtype(vtype(np.empty(0, dtype=dtype)))
    Cm = np.asarray(lam_or_C)
    if Cm.ndim == 1:
        if Cm.shape[0] != r:
            raise DimensionMismatch(f"{Cm.shape[0]} eigenvalues for {r} vectors")
        Cm = np.diag(Cm)
    elif Cm.ndim != 2 or Cm.shape != (r, r):
        raise DimensionMismatch(f"the coefficient block must be ({r}, {r}), got {Cm.shape}")
    if Cm.dtype.kind == "c" and dt.kind != "c":
        raise ArgumentError("complex coefficients need ComplexF64 vectors")
    return np.asfortranarray(Cm.astype(dt))


def residuals(A: Operator, X: DeviceVectors, lam_or_C, B: Operator | None = None):
    """(resid, bnorm) with resid[i] = ||A X[:, i] - sum_j (B X)[:, j] C[j, i]||_2 and bnorm[i] = ||(B X)[:, i]||_2, evaluated on the
    device against the ORIGINAL `A` (and `B`; None: the identity): `lam_or_C` is a vector of eigenvalues (A x = x lambda,
    A x = B x lambda, docs/src/index.md:258, 302) or a square block such as R (A Q = B Q R).  Only 2 r numbers cross PCIe."""
    _check_apply(A, X)
    if B is not None:
        _check_apply(B, X)
    Cm = residual_coefficients(lam_or_C, X.shape[1], X.dtype)
    AX = X.apply(A)
    BX = X if B is None else X.apply(B)
    r = X.shape[1]
    resid, bnorm = np.zeros(r), np.zeros(r)
    check(_lib.load().ks_vectors_residuals(AX._h, BX._h, Cm.ctypes.data, r, resid.ctypes.data_as(C.POINTER(C.c_double)),
                                           bnorm.ctypes.data_as(C.POINTER(C.c_double))))
    AX.close()
    if BX is not X:
        BX.close()
    return resid, bnorm


def vector_residuals(AX: DeviceVectors, BX: DeviceVectors, lam_or_C):
    """`residuals` for products that already exist: (||AX[:, i] - sum_j BX[:, j] C[j, i]||_2, ||BX[:, i]||_2); BX may be AX."""
    _check_pair(AX, BX, True)
    Cm = residual_coefficients(lam_or_C, AX.shape[1], AX.dtype)
    r = AX.shape[1]
    resid, bnorm = np.zeros(r), np.zeros(r)
    check(_lib.load().ks_vectors_residuals(AX._h, BX._h, Cm.ctypes.data, r, resid.ctypes.data_as(C.POINTER(C.c_double)),
                                           bnorm.ctypes.data_as(C.POINTER(C.c_double))))
    return resid, bnorm


def gram(X: DeviceVectors, Y: DeviceVectors) -> np.ndarray:
    """X^H Y (r_x x r_y) computed on the device: Q* B Q - I and Q* A Q - R of docs/src/index.md:350-351 from Q and Q.apply(...)."""
    _check_pair(X, Y, False)
    G = np.zeros((X.shape[1], Y.shape[1]), dtype=X.dtype, order="F")
    check(_lib.load().ks_vectors_gram(X._h, Y._h, G.ctypes.data, X.shape[1]))
    return G


def schur_vectors(P: PartialSchur) -> DeviceVectors:
    """A device copy of the Schur vectors Q of `P` (the basis times the identity): `schur_vectors(P).apply(back.operator)` is the
    back-transformation of `extras.b_orthonormal_operator` without the host."""
    k = P.nconverged
    if k == 0:
        raise ArgumentError("no converged eigenvalues: there are no vectors to keep on the device")
    return P.workspace.basis_times_device(k, np.eye(k, dtype=P.workspace.dtype))
