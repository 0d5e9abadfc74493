"""Ready-made DEVICE operators built on the opaque-operator seam (`ks_operator_device_callback`, include/kschur.h;
`mul!(y, A, x)` with a user-supplied `A`, src/expansion.jl:121).  These are USER-side operators -- the counterpart of
the `LinearMap` a Julia user wraps around `ldiv!(factorize(A - sigma*I))` (docs/src/index.md:246-249, 273-287) -- not
part of the library's hot path: they exist so that BASELINE config 4 (ComplexF64 shift-invert) can run with every
vector resident in HBM instead of crossing PCIe twice per product.

    TridiagonalShiftInvert(dl, d, du, sigma)   y = (T - sigma I)^{-1} x  with rocSPARSE's pivoting tridiagonal solver
                                               (rocsparse_[dz]gtsv), on the library's stream.  torch is only plumbing
                                               (device buffers for the three diagonals and the solver's work space).
    sparse_shift_invert(A, sigma)              y = (A - sigma I)^{-1} x for a general sparse A: SuperLU factorisation on
                                               the host (scipy), both triangular solves of every product on the device
                                               through the LIBRARY's own operator `ks_operator_lu` (hand-written
                                               synchronisation-free solve, csrc/ks_sptrsv.hpp) -- no vendor call, no torch.

    generalized_shift_invert(A, B, sigma)      y = (A - sigma B)^{-1} B x for the pencil A x = B x lambda: the two operators
                                               above composed on the device (`api.product_operator`).
    b_orthonormal_operator(A, L)               y = L^{-1} A L^{-*} x for B = L L*: B-orthonormal Schur vectors of A.

The LIBRARY's own tridiagonal shift-invert -- factored once at upload, applied by its own kernels, no rocSPARSE and no torch --
is `api.tridiagonal_solve_operator(dl, d, du, sigma)` (`ks_operator_tridiag_solve`, csrc/ks_tridiag.hpp).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import api


def _rocsparse():
    for path in ("/opt/rocm/lib/librocsparse.so", "librocsparse.so"):
        try:
            return C.CDLL(path)
        except OSError:
            continue
    raise ImportError("librocsparse.so not found (the tridiagonal shift-invert operator needs rocSPARSE)")


class TridiagonalShiftInvert:
    """Builds `api.Operator` for y = (T - sigma I)^{-1} x, T tridiagonal with sub-/main/super-diagonals dl (n-1), d (n),
    du (n-1).  The eigenvalues lambda of T closest to sigma are sigma + 1/theta for the largest-magnitude theta."""

    def __init__(self, dl, d, du, sigma=0.0, ctx: api.Context | None = None):
        import torch

        self.ctx = ctx or api.default_context()
        cplx = any(np.asarray(a).dtype.kind == "c" for a in (dl, d, du)) or isinstance(sigma, complex)
        self.dtype = np.complex128 if cplx else np.float64
        n = len(d)
        self.n = n
        dev = torch.device("cuda", self.ctx.device)
        L = np.zeros(n, dtype=self.dtype)
        L[1:] = dl                                    # rocSPARSE convention: dl[0] = 0, du[n-1] = 0, all of length n
        U = np.zeros(n, dtype=self.dtype)
        U[:-1] = du
        D = np.asarray(d, dtype=self.dtype) - sigma
        self._dl, self._d, self._du = (torch.as_tensor(a, device=dev) for a in (L, D, U))
        self._lib = _rocsparse()
        self._h = C.c_void_p()
        self._check(self._lib.rocsparse_create_handle(C.byref(self._h)))
        self._check(self._lib.rocsparse_set_stream(self._h, C.c_void_p(self.ctx.stream)))
        pre = "z" if cplx else "d"
        self._solve = getattr(self._lib, f"rocsparse_{pre}gtsv")
        size = C.c_size_t(0)
        probe = torch.zeros(n, dtype=torch.complex128 if cplx else torch.float64, device=dev)
        self._check(getattr(self._lib, f"rocsparse_{pre}gtsv_buffer_size")(
            self._h, C.c_int(n), C.c_int(1), C.c_void_p(self._dl.data_ptr()), C.c_void_p(self._d.data_ptr()),
            C.c_void_p(self._du.data_ptr()), C.c_void_p(probe.data_ptr()), C.c_int(n), C.byref(size)))
        self._buf = torch.empty(max(int(size.value), 16), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def apply(y, x):          # called with two tensors aliasing columns of V, on the library's stream
            y.copy_(x)
            self._check(self._solve(self._h, C.c_int(n), C.c_int(1), C.c_void_p(self._dl.data_ptr()), C.c_void_p(self._d.data_ptr()),
                                    C.c_void_p(self._du.data_ptr()), C.c_void_p(y.data_ptr()), C.c_int(n), C.c_void_p(self._buf.data_ptr())))

        self.operator = api.device_operator(apply, n, self.dtype, self.ctx)
        self.operator._owner = self      # the diagonals and the rocSPARSE handle live as long as the operator

    @staticmethod
    def _check(rc):
        if rc != 0:
            raise RuntimeError(f"rocSPARSE returned status {rc}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rocsparse_destroy_handle(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sparse_shift_invert(A, sigma=0.0, ctx: api.Context | None = None, symmetric_pattern: bool | None = None,
                        residual_limit: float = 1e-10, **splu_kw) -> api.Operator:
    """`api.Operator` for y = (A - sigma I)^{-1} x, A scipy.sparse.  The factorisation runs once on the host
    (`scipy.sparse.linalg.splu`, i.e. SuperLU -- the role SuiteSparse plays behind `factorize` in
    docs/src/index.md:246-249); its triangular factors live in HBM and are applied on the device.  The cost of a product
    is the length of the factors' dependency chains (`operator.lu_info`), so the ordering matters: for matrices with a
    symmetric non-zero pattern (`symmetric_pattern`, detected if None) minimum degree on A + A' with diagonal pivots gives
    far shorter chains and less fill than SuperLU's default column ordering -- kept only if one residual check of the
    factors passes (`residual_limit`), otherwise replaced by the partially pivoted default.  `operator.factor_residual`
    reports the residual of the factors in use."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    n = A.shape[0]
    cplx = A.dtype.kind == "c" or isinstance(sigma, complex)
    M = (sp.csc_matrix(A, dtype=np.complex128 if cplx else np.float64) - sigma * sp.identity(n, format="csc")).tocsc()
    if symmetric_pattern is None:
        P = M.copy()
        P.data[:] = 1.0
        symmetric_pattern = (P != P.T).nnz == 0
    unpivoted = bool(symmetric_pattern and not splu_kw)
    if unpivoted:
        splu_kw = dict(permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    lu = spla.splu(M, **splu_kw)
    if unpivoted:
        # Diagonal-only pivoting is not backward stable: A - sigma I is indefinite and nearly singular exactly when sigma
        # lies inside the spectrum (the use case), and element growth / tiny pivots then go unnoticed.  One solve against
        # a known right-hand side decides: above `residual_limit` the factors are discarded and the default,
        # partially pivoted factorisation (what `lu` / `factorize` of the reference workflow do) is used instead.
        rel = _relative_residual(M, lu)
        if not (rel <= residual_limit):
            import warnings

            warnings.warn(f"sparse_shift_invert: the diagonally pivoted factorisation has relative residual {rel:.1e} "
                          f"(> {residual_limit:.0e}); refactorising with partial pivoting", RuntimeWarning, stacklevel=2)
            lu = spla.splu(M)
    op = api.splu_operator(lu, ctx)
    op.factor_residual = _relative_residual(M, lu)
    return op


def _relative_residual(M, lu) -> float:
    """|| M y - b || / (||M||_1 ||y|| + ||b||) for one deterministic right-hand side (host solve of the same factors)."""
    import scipy.sparse.linalg as spla

    n = M.shape[0]
    b = np.cos(0.7 * np.arange(n) + 0.3).astype(M.dtype)
    y = lu.solve(b)
    if not np.all(np.isfinite(y)):
        return float("inf")
    return float(np.linalg.norm(M @ y - b) / (spla.norm(M, 1) * np.linalg.norm(y) + np.linalg.norm(b)))


def generalized_shift_invert(A, B, sigma=0.0, ctx: api.Context | None = None, **kw) -> api.Operator:
    """`api.Operator` for y = (A - sigma B)^{-1} (B x), A and B scipy.sparse: the `ShiftAndInvert` LinearMap of the reference's
    recipe for generalized problems A x = B x lambda (docs/src/index.md:273-287: `mul!(temp, B, x); ldiv!(y, A_lu, temp)`),
    with the product, both triangular solves and the vector between them on the device: `sparse_shift_invert(A - sigma B, 0)`
    (keywords are passed on to it) composed with `csr_operator(B)` by `api.product_operator`.  The eigenvalues of the pencil
    closest to sigma are sigma + 1/theta for the largest-magnitude theta."""
    import scipy.sparse as sp

    cplx = A.dtype.kind == "c" or B.dtype.kind == "c" or isinstance(sigma, (complex, np.complexfloating))
    dt = np.complex128 if cplx else np.float64
    A, B = sp.csc_matrix(A, dtype=dt), sp.csr_matrix(B, dtype=dt)
    if A.shape != B.shape:
        raise api.DimensionMismatch(f"A and B must have one size: {A.shape}, {B.shape}")
    ctx = ctx or api.default_context()
    solve = sparse_shift_invert((A - dt(sigma) * B.tocsc()).tocsc(), 0.0, ctx, **kw)
    op = api.product_operator(solve, api.csr_operator(B, ctx), ctx=ctx)
    op.factor_residual = solve.factor_residual
    return op


def generalized_cg_operator(A: api.Operator, B: api.Operator, **cg) -> api.Operator:
    """`api.Operator` for y = B^{-1} (A x) with A and B device operators and B Hermitian positive definite: the reference's recipe
    for generalized problems A x = B x lambda (docs/src/index.md:273-287) where B has nothing to factor -- the consistent mass
    matrix of matrix-free finite elements (`q1_fem_taps`).  `api.product_operator(api.cg_operator(B, **cg), A)`: the solve is
    conjugate gradients on the device (keywords are passed on to `api.cg_operator`), the eigenvalues of the operator are the
    pencil's, so `partialschur(..., which="SR")` finds the lowest ones directly.  B^{-1} A is not symmetric: verify with
    `residuals(A, X, lambda, B)`.  `.solve` is the conjugate-gradient factor (`.solve.cg_info` counts its iterations).  The inner
    `tol` should be at least 100 times tighter than the outer one (`api.cg_operator`)."""
    solve = api.cg_operator(B, **cg)
    op = api.product_operator(solve, A, ctx=solve.ctx)
    op.solve = solve
    return op


def jacobi_preconditioner(diagonal, shift=0.0, dtype=None, ctx: api.Context | None = None) -> api.Operator:
    """`api.diagonal_operator(1 / (diagonal - shift))`: the Jacobi preconditioner of `api.pcg_operator(A, M, shift=shift)` from the
    matrix diagonal of A (the second value of `diffusion_terms`, `centre + potential` of a grid operator) -- what a coefficient jump
    needs: the iteration count then follows the jump no longer.  The entries are checked here, without a device: ArgumentError
    unless every `diagonal - shift` is positive and finite (a Hermitian positive definite A - shift I has a positive diagonal).
    `dtype`: the element type of A, Float64 (the default) or ComplexF64; the entries stay real."""
    d = np.asarray(diagonal)
    if d.dtype.kind == "c":
        if np.any(d.imag != 0):
            raise api.ArgumentError("jacobi_preconditioner: the diagonal of a Hermitian operator is real")
        d = d.real
    if d.ndim != 1 or d.dtype.kind not in "fiu":
        raise api.ArgumentError(f"jacobi_preconditioner: diagonal must be a 1-D sequence of real numbers, got shape {d.shape}, dtype {d.dtype}")
    s = float(shift)
    if not np.isfinite(s):
        raise api.ArgumentError("jacobi_preconditioner: shift is not finite")
    t = np.asarray(d, dtype=np.float64) - s
    bad = np.flatnonzero(~(np.isfinite(t) & (t > 0)))
    if bad.size:
        raise api.ArgumentError(f"jacobi_preconditioner: diagonal - shift must be positive and finite, entry {int(bad[0])} is {t[bad[0]]!r} "
                                f"({bad.size} such entries): A - shift I is not positive definite")
    return api.diagonal_operator(1.0 / t, dtype=dtype, ctx=ctx)


def grid_line_terms(shape, taps, potential=None, coeff=None, shift=0.0):
    """(dl, d, du): the three central diagonals of the 3-, 5- or 7-point `api.grid_operator(shape, taps, potential)` -- with `coeff`,
    of `api.grid_variable_operator(shape, taps, coeff, potential)` -- minus `shift` on the main one, as `tridiagonal_solve_operator`
    takes them: the x-lines of the grid, one tridiagonal block per line.  n - 1, n and n - 1 values with n = prod(shape) and the
    element type of the operator; `dl[r - 1]` and `du[r]` are zero where an x-line ends (ix = nx - 1), so the blocks do not touch.
    The matrix is never formed, and the entries are the bits of `api.host_grid_matrix` / `api.host_grid_variable_matrix` on those
    diagonals: the taps -x and +x (with `coeff`: fl(0.5 tap * fl(c[r] + c[s]))), and fl(centre + potential[r]) - shift.

    The links that wrap a PERIODIC x axis are left out (they lie far from the diagonal): for such an operator the result is still a
    valid preconditioner, the open-line part of it."""
    dt, dims, t, v = api._grid_args(shape, taps, potential, None)
    if np.any(dims < 1):
        raise api.ArgumentError(f"every extent must be at least 1, shape = {shape!r}")
    ndim, nx = int(dims.size), int(dims[0])
    n = int(np.prod(dims))
    s = float(shift)
    if not np.isfinite(s):
        raise api.ArgumentError("grid_line_terms: shift is not finite")
    d = np.full(n, t[ndim], dtype=dt) if v is None else t[ndim] + v
    d = d - s
    inner = (np.arange(n - 1) % nx) != nx - 1       # row r has its +x neighbour r + 1 inside the line
    if coeff is None:
        lo, up = np.full(n - 1, t[ndim - 1], dtype=dt), np.full(n - 1, t[ndim + 1], dtype=dt)
    else:
        c = api._grid_coeff(dims, coeff)
        pair = c[:-1] + c[1:]
        lo, up = (0.5 * t[ndim - 1]) * pair, (0.5 * t[ndim + 1]) * pair
    zero = np.zeros(n - 1, dtype=dt)
    return np.where(inner, lo, zero), d, np.where(inner, up, zero)


def line_preconditioner(shape, taps, potential=None, coeff=None, shift=0.0, ctx: api.Context | None = None) -> api.Operator:
    """`api.tridiagonal_solve_operator(*grid_line_terms(shape, taps, potential, coeff, shift))`: the x-line preconditioner of
    `api.pcg_operator(A, M, shift=shift)` for a grid operator whose x links dominate (an anisotropic grid, hx << hy, hz): every
    x-line is solved exactly, 5 launches per application, and the iteration count no longer follows the anisotropy.  The lines
    must be positive definite (they are where A - shift I is); put the strong axis first in `shape`."""
    return api.tridiagonal_solve_operator(*grid_line_terms(shape, taps, potential, coeff, shift), ctx=ctx)


def _aggregate_mean(values, dims, halved):
    """The arithmetic mean of a flat cell array (x fastest) over the aggregates of `multigrid_operator`: cells 2 I and 2 I + 1 along
    every halved axis, the last cell of an odd extent alone (the true count)."""
    a = np.asarray(values, dtype=np.float64).reshape(dims[2], dims[1], dims[0])
    for axis, h in zip((2, 1, 0), halved):        # array axis 2 is x
        if not h:
            continue
        m = a.shape[axis]
        even, odd = np.take(a, range(0, m, 2), axis=axis), np.take(a, range(1, m, 2), axis=axis)
        total = even.copy()
        idx = [slice(None)] * 3
        idx[axis] = slice(0, odd.shape[axis])
        total[tuple(idx)] += odd
        count = np.full(even.shape[axis], 2.0)
        if m % 2:
            count[-1] = 1.0
        shape = [1, 1, 1]
        shape[axis] = count.size
        a = total / count.reshape(shape)
    return np.ascontiguousarray(a.reshape(-1))


def multigrid_hierarchy(shape, coeff, spacing=1.0, potential=None, boundary="dirichlet", shift=0.0, coarsest_rows=512):
    """The grids of a geometric multigrid cycle for -div(c grad) + V - shift (`grid_multigrid_preconditioner`,
    `api.multigrid_operator`): a list with one dict per level, finest first, holding `shape`, `spacing` (per axis), `coeff`,
    `potential` (None without V), and what `diffusion_terms` makes of them -- `taps`, `diagonal` -- with `inverse_diagonal` =
    1 / (diagonal - shift) and `bound`, an upper bound on the spectrum of D^-1 (A - shift).  Every axis with an extent of at least
    2 is halved (ceil) from level to level until a level has at most `coarsest_rows` rows.  c and V of a coarse cell are the
    arithmetic means over its aggregate (cells 2 I and 2 I + 1 per halved axis; the single cell of an odd tail counts once), the
    spacing doubles on halved axes, and the coarse operator is `diffusion_terms` of those again: rediscretised, not the Galerkin
    product.  `bound` is Gershgorin's: max_r (d_r - shift + sum |e|) / (d_r - shift), the off-diagonal sum taken from
    `diffusion_terms(..., boundary="neumann")` without V.  ArgumentError if some d_r - shift <= 0 (A - shift I is then not positive
    definite).  Open boundaries only.  Plain numpy, no device."""
    s = float(shift)
    if not np.isfinite(s):
        raise api.ArgumentError("multigrid_hierarchy: shift is not finite")
    if isinstance(coarsest_rows, (bool, np.bool_)) or not isinstance(coarsest_rows, (int, np.integer)) or int(coarsest_rows) < 1:
        raise api.ArgumentError(f"multigrid_hierarchy: coarsest_rows must be a positive integer, got {coarsest_rows!r}")
    try:
        dims = [int(e) for e in np.atleast_1d(np.asarray(shape)).ravel()]
    except (TypeError, ValueError) as e:
        raise api.ArgumentError(f"shape must hold 1 to 3 integer extents: {shape!r}") from e
    if not 1 <= len(dims) <= 3 or any(d < 1 for d in dims):
        raise api.ArgumentError(f"a grid has 1, 2 or 3 dimensions of extent at least 1, shape = {shape!r}")
    ndim = len(dims)
    h = _box_spacing(ndim, spacing)
    c = api._grid_coeff(np.asarray(dims, dtype=np.int64), coeff)
    v = None
    if potential is not None:
        v = np.asarray(potential)
        if v.dtype.kind == "c":
            raise api.ArgumentError("multigrid_hierarchy: the potential of a Hermitian operator is real")
        v = np.ascontiguousarray(v.reshape(-1), dtype=np.float64)
        if v.size != c.size:
            raise api.DimensionMismatch(f"potential must have {c.size} entries, got {v.size}")
    levels = []
    while True:
        taps, diag = diffusion_terms(tuple(dims), c, h, v, boundary)
        _, off = diffusion_terms(tuple(dims), c, h, None, "neumann")     # the sum of |e| over the links of each row
        t = diag - s
        bad = np.flatnonzero(~(np.isfinite(t) & (t > 0)))
        if bad.size:
            raise api.ArgumentError(f"multigrid_hierarchy: level {len(levels)}: diagonal - shift must be positive and finite, entry "
                                    f"{int(bad[0])} is {t[bad[0]]!r}: A - shift I is not positive definite")
        levels.append(dict(shape=tuple(dims), spacing=h.copy(), coeff=c, potential=v, taps=taps, diagonal=diag, inverse_diagonal=1.0 / t,
                           bound=float(np.max((t + off) / t))))
        halved = [1 if d >= 2 else 0 for d in dims]
        if c.size <= int(coarsest_rows) or not any(halved):
            return levels
        full = dims + [1] * (3 - ndim)
        hv = halved + [0] * (3 - ndim)
        c = _aggregate_mean(c, full, hv)
        v = None if v is None else _aggregate_mean(v, full, hv)
        dims = [(d + 1) // 2 if k else d for d, k in zip(dims, halved)]
        h = np.where(np.asarray(halved, dtype=bool), 2.0 * h, h)


def grid_multigrid_preconditioner(shape, coeff, spacing=1.0, potential=None, boundary="dirichlet", shift=0.0, coarsest_rows=512,
                                  degree=2, ratio=4.0, dtype=None, ctx: api.Context | None = None) -> api.Operator:
    """The geometric multigrid preconditioner of `api.pcg_operator(A, M, shift=shift)` for A = -div(c grad) + V as
    `diffusion_terms` / `api.grid_variable_operator` assemble it: `api.multigrid_operator` on the grids of `multigrid_hierarchy`,
    with an `api.grid_variable_operator` per level and, on the coarsest, `api.dense_operator` of the symmetrised inverse of
    `host_grid_variable_matrix(...) - shift I`.  Where Jacobi's iteration count doubles with the grid extent, this one's grows by a
    few iterations; one application costs 2 `degree` products on the finest grid and about a seventh of that again below it.
    `dtype`: the element type of A, Float64 (the default) or ComplexF64.  Open boundaries only.  The hierarchy stays readable as
    `.hierarchy`; the cycle keeps its level operators alive."""
    ctx = ctx or api.default_context()
    dt = np.dtype(np.float64 if dtype is None else dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.complex128)):
        raise api.ArgumentError(f"element type must be float64 or complex128, not {dt}")
    H = multigrid_hierarchy(shape, coeff, spacing, potential, boundary, shift, coarsest_rows)
    ops = [api.grid_variable_operator(L["shape"], L["taps"], L["coeff"], L["diagonal"], dtype=dt, ctx=ctx) for L in H[:-1]]
    last = H[-1]
    Ac = api.host_grid_variable_matrix(last["shape"], last["taps"], last["coeff"], last["diagonal"]).toarray().real
    inv = np.linalg.inv(Ac - float(shift) * np.eye(Ac.shape[0]))
    coarse = api.dense_operator((0.5 * (inv + inv.T)).astype(dt), ctx)
    M = api.multigrid_operator(ops, [L["shape"] for L in H], [L["inverse_diagonal"] for L in H[:-1]], [L["bound"] for L in H[:-1]], coarse,
                               shift=shift, degree=degree, ratio=ratio, ctx=ctx)
    M.hierarchy = H
    return M


def interior_eigenvalues(mu, shift):
    """lambda = shift + 1 / mu: the eigenvalues of A from the eigenvalues mu = 1 / (lambda - shift) of a shift-invert operator
    (`api.minres_operator(A, shift=...)`, `api.cg_operator`, `api.bicgstab_operator`, `sparse_shift_invert`) -- the
    back-transformation of the reference's recipe (docs/src/index.md:234-259).  The largest |mu| are the eigenvalues nearest
    `shift`.  Real input stays real; a complex mu (the pairs of an operator that is not Hermitian) or a complex shift gives complex
    eigenvalues."""
    mu = np.asarray(mu)
    return shift + 1.0 / mu


def b_orthonormal_operator(A, L, ctx: api.Context | None = None):
    """The reference's recipe for B-orthonormal Schur vectors (docs/src/index.md:306-352), B = L L* with a sparse
    lower-triangular L (its Cholesky factor): returns `(operator, back)` with operator = C = L^{-1} A L^{-*} -- three device
    factors composed by `api.product_operator`: `lu_operator(L, I)`, `csr_operator(A)`, `lu_operator(I, L*)` -- and
    `back(Y) = L^{-*} Y` on the host (`back.operator`: the device factor L^{-*} itself, for vectors that stay in HBM:
    `api.schur_vectors(P).apply(back.operator)`).  A partial Schur decomposition C Y = Y R then gives Q = back(Y) with Q* A Q = R and
    Q* B Q = I.

    The ORDER of the two solves follows the derivation on that page, A Q = B Q R  =>  L^{-1} A Q = L* Q R  =>  (L^{-1} A L^{-*}) Y
    = Y R with Y = L* Q.  The page's formula writes L^{-*} A L^{-1} and its code applies L^{-1} first; that coincides with the
    derivation only where L commutes with A or, as in its example, B is diagonal (L = L*): with a bidiagonal L it leaves
    ||Q* A Q - R|| = 0.8."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    n = A.shape[0]
    cplx = A.dtype.kind == "c" or L.dtype.kind == "c"
    dt = np.complex128 if cplx else np.float64
    L = sp.csr_matrix(L, dtype=dt)
    LH = L.conj().T.tocsr()
    I = sp.identity(n, dtype=dt, format="csr")
    ctx = ctx or api.default_context()
    op = api.product_operator(api.lu_operator(L, I, ctx=ctx), api.csr_operator(sp.csr_matrix(A, dtype=dt), ctx), api.lu_operator(I, LH, ctx=ctx), ctx=ctx)

    def back(Y):
        return spla.spsolve_triangular(LH, np.asarray(Y, dtype=dt), lower=False)

    # the same back-transformation on the device: Q = api.schur_vectors(P).apply(back.operator)
    back.operator = op.factors[2]
    return op, back


def bloch_wrap(taps, theta, radius=1) -> np.ndarray:
    """The `wrap` array of `api.grid_operator(..., periodic=..., wrap=...)` for Bloch boundary conditions: the link that leaves the
    cell in the + direction of axis a carries t_{+a} e^{+i theta_a}, the one in the - direction t_{-a} e^{-i theta_a} (a band
    structure at the k-point theta_a = k_a L_a).  `taps`: the 2 ndim + 1 taps in ascending column order; `theta`: one phase per axis
    in the order of the shape (x[, y[, z]]).  Returns 2 ndim complex values in the order of the taps without the centre.  With
    symmetric real taps (or t_{-a} = conj(t_{+a})) the operator is Hermitian.

    The same array serves `api.grid_variable_operator`: a crystal with a variable coefficient (div (1 / eps) grad, a
    position-dependent mass) at the k-point theta is

        taps, diagonal = diffusion_terms(shape, coeff, spacing, V, periodic=True)
        op = api.grid_variable_operator(shape, taps, coeff, diagonal, periodic=True, wrap=bloch_wrap(taps, theta))

    -- exactly Hermitian for a real `coeff`; the diagonal does not depend on theta (|hw| = |h|).

    `radius` = R (never inferred from the length of `taps`): the 2 ndim R + 1 taps of a star stencil, for
    `api.grid_star_operator(shape, taps, R, ..., periodic=True, wrap=bloch_wrap(taps, theta, radius=R))`.  Returns 2 ndim R values
    in the order of the taps without the centre: every +-d link of axis a carries t e^{+-i theta_a}, the same phase at every
    distance d, because a link crosses the cell boundary at most once."""
    t = np.asarray(taps)
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 4:
        raise api.ArgumentError(f"radius must be an integer in 1...4, got {radius!r}")
    R = int(radius)
    if t.ndim != 1 or t.size not in (2 * R + 1, 4 * R + 1, 6 * R + 1):
        raise api.DimensionMismatch(f"taps must hold {2 * R + 1}, {4 * R + 1} or {6 * R + 1} values"
                                    f"{'' if R == 1 else f' at radius {R}'}, got shape {t.shape}")
    ndim = (t.size - 1) // (2 * R)
    if th.shape != (ndim,):
        raise api.DimensionMismatch(f"theta takes one phase per axis ({ndim}), got shape {th.shape}")
    w = np.empty(2 * ndim * R, dtype=np.complex128)
    c = ndim * R
    for a in range(ndim):
        for d in range(1, R + 1):
            w[c - a * R - d] = t[c - a * R - d] * np.exp(-1j * th[a])
            w[c + a * R + d - 1] = t[c + a * R + d] * np.exp(1j * th[a])
    return w


# 1-D weights of -d^2/dx^2 by central differences, centre first then the distances 1, 2, ...: (numerator, denominator)
_FD_WEIGHTS = {
    2: ((2, 1), (-1, 1)),
    4: ((5, 2), (-4, 3), (1, 12)),
    6: ((49, 18), (-3, 2), (3, 20), (-1, 90)),
    8: ((205, 72), (-8, 5), (1, 5), (-8, 315), (1, 560)),
}


def fd_laplacian_taps(ndim, order, spacing=1.0, scale=1.0) -> np.ndarray:
    """The taps of `scale * (-Laplacian)` by central differences of `order` 2, 4, 6 or 8 for `api.grid_operator(shape, taps, ...,
    radius=order // 2)`: 2 ndim R + 1 Float64 values in ascending column order, [-R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre,
    +1 x ... +R x, +1 y ... +R y, +1 z ... +R z] in 3-D.  `spacing`: the grid spacing h, a scalar or one value per axis in the order
    of the shape (x[, y[, z]]).  The weight of distance d along axis a is scale * w_d / h_a^2 with the rational w_d rounded once;
    the centre is the sum over the axes."""
    if isinstance(ndim, (bool, np.bool_)) or not isinstance(ndim, (int, np.integer)) or not 1 <= int(ndim) <= 3:
        raise api.ArgumentError(f"a grid has 1, 2 or 3 dimensions (ndim), got {ndim!r}")
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or int(order) not in _FD_WEIGHTS:
        raise api.ArgumentError(f"order must be 2, 4, 6 or 8, got {order!r}")
    ndim, order = int(ndim), int(order)
    h = np.asarray(spacing, dtype=np.float64)
    if h.ndim == 0:
        h = np.full(ndim, float(h))
    if h.shape != (ndim,):
        raise api.DimensionMismatch(f"spacing takes a scalar or one value per axis ({ndim}), got shape {h.shape}")
    if not np.all(np.isfinite(h)) or np.any(h <= 0):
        raise api.ArgumentError(f"spacing must be positive and finite, got {spacing!r}")
    R = order // 2
    w = [num / den for num, den in _FD_WEIGHTS[order]]
    t = np.zeros(2 * ndim * R + 1, dtype=np.float64)
    c = ndim * R
    for a in range(ndim):
        f = float(scale) / (h[a] * h[a])
        t[c] += f * w[0]
        for d in range(1, R + 1):
            # axis a: its -d link is entry c - a R - d, its +d link entry c + a R + d
            t[c - a * R - d] = t[c + a * R + d] = f * w[d]
    return t


def diffusion_terms(shape, coeff, spacing=1.0, potential=None, boundary="dirichlet", periodic=None):
    """(taps, diagonal) of the diffusion operator -div(c grad) + V on a grid with the cell-centred coefficient `coeff`, for
    `api.grid_variable_operator`:

        taps, diagonal = diffusion_terms(shape, coeff, spacing, V, boundary)
        op = api.grid_variable_operator(shape, taps, coeff, potential=diagonal)

    `taps`: -1 / h_a^2 on the two links of axis a, centre 0 (`spacing`: the grid spacing h, a scalar or one value per axis in the
    order of the shape, as in `fd_laplacian_taps`), so that the link from r to s carries e = fl(0.5 t_k * fl(c[r] + c[s])), minus the
    arithmetic mean of the two coefficients over h^2.  `diagonal[r] = (0.0 - e_1 - e_2 ...) + V[r]`, the e_k of the row in slot order
    (-z, -y, -x, +x, +y, +z), flat in row order.  A direction whose neighbour lies outside the grid: `boundary="dirichlet"` takes
    c[s] := c[r] (a ghost cell with the boundary cell's coefficient and the value 0: with c == 1 and spacing 1 exactly the
    [-1 ... 2 ndim ... -1] Laplacian), `"neumann"` leaves the term out (no flux: the row sums vanish up to rounding).

    `periodic`: True, or one bool per axis in the order of the shape, for `api.grid_variable_operator(..., periodic=periodic)`: on
    such an axis (extent >= 3) the neighbour beyond the edge is the wrap image at the other end of the line, its c[s] enters the
    link's e, and e is subtracted in the diagonal like that of an interior link (on a torus the row sums vanish up to rounding);
    `boundary` applies to the remaining open axes.  The diagonal does not depend on a Bloch phase (|hw| = |h|): for a k-point pass
    `wrap=bloch_wrap(taps, theta)` to the operator and keep this diagonal.  Plain numpy, no device."""
    if boundary not in ("dirichlet", "neumann"):
        raise api.ArgumentError(f"boundary must be 'dirichlet' or 'neumann', got {boundary!r}")
    try:
        ndim = int(np.atleast_1d(np.asarray(shape)).size)
    except (TypeError, ValueError) as e:
        raise api.ArgumentError(f"shape must hold 1 to 3 integer extents: {shape!r}") from e
    if not 1 <= ndim <= 3:
        raise api.ArgumentError(f"a grid has 1, 2 or 3 dimensions (ndim), shape = {shape!r}")
    taps = fd_laplacian_taps(ndim, 2, spacing)
    taps[ndim] = 0.0
    _dt, dims, _t, v = api._grid_args(shape, taps, potential, None)
    if np.any(dims < 1):
        raise api.ArgumentError(f"every extent must be at least 1, shape = {shape!r}")
    c = api._grid_coeff(dims, coeff)
    per = [bool(f) for f in api._grid_wrap_args(dims, _t, v, _dt, None, periodic, None)[3]]
    for a in range(ndim):
        if per[a] and dims[a] < 3:   # (the library's wording: ks_operator_grid_periodic)
            raise api.ArgumentError(f"diffusion_terms: periodic axis {a} ({'xyz'[a]}) has extent {int(dims[a])} (a periodic axis needs at "
                                    "least 3 points: at 2 the two neighbours coincide, at 1 the link is a self-link)")
    ext = [int(d) for d in dims] + [1] * (3 - ndim)
    nx, ny, nz = ext
    idx = np.arange(nx * ny * nz)
    pos = (idx % nx, (idx // nx) % ny, idx // (nx * ny))
    stride = (1, nx, nx * ny)
    d = np.zeros(idx.size, dtype=np.float64)
    # slot order: -z, -y, -x, then +x, +y, +z; axis a has its - link at tap ndim - 1 - a and its + link at tap ndim + 1 + a
    for sign, axes in ((-1, range(ndim - 1, -1, -1)), (1, range(ndim))):
        for a in axes:
            has = pos[a] > 0 if sign < 0 else pos[a] < ext[a] - 1
            cs = c.copy()
            cs[has] = c[idx[has] + sign * stride[a]]
            if per[a]:   # the wrap image: the other end of the line
                cs[~has] = c[idx[~has] - sign * (ext[a] - 1) * stride[a]]
                has = np.ones_like(has)
            e = (0.5 * taps[ndim + sign * (1 + a)]) * (c + cs)
            if boundary == "neumann":
                e = np.where(has, e, 0.0)
            d = d - e
    return taps, (d if v is None else d + v)


def _box_spacing(ndim, spacing):
    """One positive, finite grid spacing per axis in the order of the shape (x[, y[, z]])."""
    h = np.asarray(spacing, dtype=np.float64)
    if h.ndim == 0:
        h = np.full(ndim, float(h))
    if h.shape != (ndim,):
        raise api.DimensionMismatch(f"spacing takes a scalar or one value per axis ({ndim}), got shape {h.shape}")
    if not np.all(np.isfinite(h)) or np.any(h <= 0):
        raise api.ArgumentError(f"spacing must be positive and finite, got {spacing!r}")
    return h


def tensor_laplacian_taps(D, spacing=1.0, scale=1.0) -> np.ndarray:
    """The taps of `scale * (-div(D grad))` for a constant symmetric ndim x ndim tensor `D` (axes in the order of the shape:
    x[, y[, z]]) for `api.grid_box_operator`: 3^ndim Float64 values in slot order, slot 9 (dz + 1) + 3 (dy + 1) + (dx + 1) in 3-D.
    The two axis neighbours of axis a carry -D_aa / h_a^2 and the centre sum_a 2 D_aa / h_a^2 (second central differences; with a
    diagonal D these are the taps of `fd_laplacian_taps(ndim, 2)` axis by axis); the mixed term -2 D_ab d_a d_b by central
    differences lives on the four in-plane corners of the axes a < b: the corner (s_a, s_b), s = -1 or +1, carries
    -s_a s_b D_ab / (2 h_a h_b).  Every other slot is 0.  `spacing`: the grid spacing h, a scalar or one value per axis.  The matrix
    of these taps is symmetric; it is positive definite for a positive definite D whose mixed terms are small enough against the
    diagonal ones for the corner entries not to outweigh the axis entries."""
    try:
        d = np.atleast_2d(np.asarray(D, dtype=np.float64))
    except (TypeError, ValueError) as e:
        raise api.ArgumentError(f"D must be a real ndim x ndim tensor: {e}") from e
    if d.ndim != 2 or d.shape[0] != d.shape[1] or not 1 <= d.shape[0] <= 3:
        raise api.DimensionMismatch(f"D must be an ndim x ndim tensor with ndim = 1, 2 or 3, got shape {d.shape}")
    if not np.all(np.isfinite(d)):
        raise api.ArgumentError("D must be finite")
    if not np.array_equal(d, d.T):
        raise api.ArgumentError("D must be symmetric")
    ndim = d.shape[0]
    h = _box_spacing(ndim, spacing)
    t = np.zeros((3,) * ndim, dtype=np.float64)   # [dz, dy, dx]: axis a is index ndim - 1 - a
    centre = (1,) * ndim

    def slot(steps):
        """the index of the neighbour at the given {axis: step}"""
        i = list(centre)
        for a, s in steps.items():
            i[ndim - 1 - a] += s
        return tuple(i)

    for a in range(ndim):
        f = float(scale) * d[a, a] / (h[a] * h[a])
        t[centre] += f * 2.0
        t[slot({a: -1})] = t[slot({a: 1})] = f * -1.0
    for a in range(ndim):
        for b in range(a + 1, ndim):
            f = float(scale) * d[a, b] / (2.0 * h[a] * h[b])
            if f == 0.0:   # (no mixed term: the corners stay +0.0)
                continue
            for sa in (-1, 1):
                for sb in (-1, 1):
                    t[slot({a: sa, b: sb})] = -sa * sb * f
    return t.ravel()


def box_bloch_links(taps, theta) -> np.ndarray:
    """The `links` array of `api.grid_box_operator(..., periodic=..., links=...)` for Bloch boundary conditions (a band structure
    at the k-point theta_a = k_a L_a): 5^ndim complex values, flat in [e_z, e_y, e_x] order,

        links[e] = taps[slot(e)] * exp(i sum_a theta_a c_a),   c_a = -1 / 0 / +1 for the class e_a = 0 / 1, 2, 3 / 4,

    slot(e) being the slot of the link's offsets (-1 for the classes 0 and 1, 0 for 2, +1 for 3 and 4): a link that leaves the cell
    through two or three faces carries the product of their phases, in the sign convention of `bloch_wrap`.  `taps`: the 3^ndim taps,
    flat or of shape (3,) * ndim; `theta`: one phase per axis in the order of the shape (x[, y[, z]]).  The phase of a face is
    computed once, the one of the opposite face is its conjugate, and conjugation commutes with every rounding of a complex product:
    links[mirror(e)] == conj(links[e]) holds exactly, mirror: e_a -> 4 - e_a, whenever taps[-k] == conj(taps[k]) -- the operator is
    then exactly Hermitian.  In 1-D [links[0], links[4]] is `bloch_wrap(taps, theta)` bit for bit.  The entries without a class 0
    or 4 are the taps themselves (the library does not read them).

    An antiperiodic cell (the sign -1 on every link that crosses):  `links = -box_bloch_links(taps, np.zeros(ndim)).real`."""
    t = np.asarray(taps)
    ndim = {3: 1, 9: 2, 27: 3}.get(t.size)
    if ndim is None or t.shape not in ((3 ** ndim,), (3,) * ndim):
        raise api.DimensionMismatch(f"taps must hold 3, 9 or 27 values, flat or of shape (3,) * ndim, got shape {t.shape}")
    t = t.reshape((3,) * ndim)
    th = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if th.shape != (ndim,):
        raise api.DimensionMismatch(f"theta takes one phase per axis ({ndim}), got shape {th.shape}")
    plus = [np.exp(1j * th[a]) for a in range(ndim)]   # the + face of axis a; its - face: the conjugate
    out = np.empty((5,) * ndim, dtype=np.complex128)
    for e in np.ndindex(*out.shape):   # e = (e_z, e_y, e_x): axis a is index ndim - 1 - a
        phase = None
        for a in range(ndim):
            ea = e[ndim - 1 - a]
            if ea in (0, 4):
                f = plus[a] if ea == 4 else np.conj(plus[a])
                phase = f if phase is None else phase * f
        tap = t[tuple(0 if c < 2 else 2 if c > 2 else 1 for c in e)]
        out[e] = tap if phase is None else tap * phase
    return out.reshape(-1)


def q1_fem_taps(ndim, spacing=1.0):
    """(stiffness_taps, mass_taps) of multilinear (Q1) finite elements on a uniform grid for `api.grid_box_operator`, each 3^ndim
    Float64 values in slot order: the tensor products of the 1-D element matrices K_a = [-1, 2, -1] / h_a and
    M_a = h_a [1, 4, 1] / 6,  M = prod_a M_a  and  K = sum_a K_a (x) prod_{b != a} M_b.  With the open truncation of the grid
    operator these are the stiffness and the consistent mass matrix of the interior nodes under homogeneous Dirichlet conditions
    (the boundary nodes lie one spacing outside the grid); the generalized problem K x = lambda M x runs in HBM with
    `product_operator` and `residuals(K, X, lambda, M)`."""
    if isinstance(ndim, (bool, np.bool_)) or not isinstance(ndim, (int, np.integer)) or not 1 <= int(ndim) <= 3:
        raise api.ArgumentError(f"a grid has 1, 2 or 3 dimensions (ndim), got {ndim!r}")
    ndim = int(ndim)
    h = _box_spacing(ndim, spacing)
    k1 = [np.array([-1.0, 2.0, -1.0]) / h[a] for a in range(ndim)]
    m1 = [h[a] * np.array([1.0, 4.0, 1.0]) / 6.0 for a in range(ndim)]

    def outer(parts):
        """the tensor product with axis ndim - 1 slowest: [dz, dy, dx]"""
        out = parts[ndim - 1]
        for a in range(ndim - 2, -1, -1):
            out = np.multiply.outer(out, parts[a])
        return out

    mass = outer(m1)
    stiff = sum(outer([k1[b] if b == a else m1[b] for b in range(ndim)]) for a in range(ndim))
    return np.ascontiguousarray(stiff).ravel(), np.ascontiguousarray(mass).ravel()


# ------------------------------------------------------------------ Chebyshev polynomial filters (api.chebyshev_operator)
def _cheb_interval(bounds):
    try:
        a, b = (float(v) for v in bounds)
    except (TypeError, ValueError) as e:
        raise api.ArgumentError(f"bounds must be a pair (a, b) that contains the spectrum, got {bounds!r}") from e
    if not (np.isfinite(a) and np.isfinite(b) and a < b):
        raise api.ArgumentError(f"bounds must be finite with a < b, got ({a}, {b})")
    return a, b, 0.5 * (a + b), 0.5 * (b - a)


def _cheb_degree(degree):
    if isinstance(degree, (bool, np.bool_)) or not isinstance(degree, (int, np.integer)) or not 1 <= int(degree) <= 256:
        raise api.ArgumentError(f"degree must be an integer in 1...256, got {degree!r}")
    return int(degree)


def jackson_factors(degree) -> np.ndarray:
    """g_0 ... g_degree of the Jackson kernel for an expansion with degree + 1 terms: with N = degree + 1,
    g_k = ((N - k + 1) cos(pi k / (N + 1)) + sin(pi k / (N + 1)) cot(pi / (N + 1))) / (N + 1).  The kernel is positive: the damped
    expansion of a function with values in [0, 1] stays in [0, 1]."""
    m = _cheb_degree(degree)
    N = m + 1
    k = np.arange(N, dtype=np.float64)
    q = np.pi / (N + 1)
    return ((N - k + 1) * np.cos(q * k) + np.sin(q * k) / np.tan(q)) / (N + 1)


def chebyshev_window(lo, hi, bounds, degree, damping="jackson"):
    """(center, halfwidth, coeffs) for `api.chebyshev_operator`: the Chebyshev expansion of the indicator of [lo, hi] on
    bounds = (a, b), damped with the Jackson kernel (`damping="jackson"`; None: the truncated series, which overshoots).  With
    c = (a + b) / 2, e = (b - a) / 2, t1 = acos((lo - c) / e), t2 = acos((hi - c) / e):
        gamma_0 = (t1 - t2) / pi,   gamma_k = 2 (sin k t1 - sin k t2) / (k pi),
    each multiplied by its Jackson factor.  The eigenvalues of A inside the window become the LARGEST of p(A): solve with
    which="LR", then recover A's eigenvalues from the Schur vectors (README).  The filter is unbounded outside `bounds`: they must
    contain A's spectrum (`grid_spectrum_bounds`)."""
    a, b, c, e = _cheb_interval(bounds)
    m = _cheb_degree(degree)
    lo, hi = float(lo), float(hi)
    if not a <= lo < hi <= b:
        raise api.ArgumentError(f"the window must lie inside the bounds: need a <= lo < hi <= b, got [{lo}, {hi}] in [{a}, {b}]")
    if damping not in ("jackson", None):
        raise api.ArgumentError(f'damping must be "jackson" or None, got {damping!r}')
    t1 = np.arccos(min(1.0, max(-1.0, (lo - c) / e)))
    t2 = np.arccos(min(1.0, max(-1.0, (hi - c) / e)))
    k = np.arange(1, m + 1, dtype=np.float64)
    g = np.empty(m + 1)
    g[0] = (t1 - t2) / np.pi
    g[1:] = 2.0 * (np.sin(k * t1) - np.sin(k * t2)) / (k * np.pi)
    if damping == "jackson":
        g *= jackson_factors(m)
    return c, e, g


def _cheb_t(m, t):
    """T_m(t) by the three-term recurrence in extended precision (no cancellation for |t| >= 1, where T_m grows)."""
    t = np.longdouble(t)
    p, q = np.longdouble(1.0), t
    if m == 0:
        return p
    for _ in range(m - 1):
        p, q = q, 2 * t * q - p
    return q


def chebyshev_damping(bounds, below, degree):
    """(center, halfwidth, coeffs) for `api.chebyshev_operator`: p(t) = T_m((t - c) / e) / T_m((below - c) / e) on bounds = (a, b)
    -- |p| <= 1 / |T_m((below - c) / e)| on [a, b], p(below) = 1, and p grows as fast as a polynomial of degree m can outside the
    interval.  `below` lies at or beyond an end of `bounds`; only the top coefficient is non-zero.  With bounds = the part of the
    spectrum to damp and `below` at the wanted end, the wanted eigenvalues are the largest of p(A) (which="LR"); bounds = the
    whole spectrum and below = a separates a clustered low end: p rises to 1 towards a."""
    a, b, c, e = _cheb_interval(bounds)
    m = _cheb_degree(degree)
    below = float(below)
    if not np.isfinite(below) or a < below < b:
        raise api.ArgumentError(f"`below` must be finite and lie at or beyond an end of the bounds, got {below} in ({a}, {b})")
    top = _cheb_t(m, (np.longdouble(below) - np.longdouble(c)) / np.longdouble(e))
    g = np.zeros(m + 1)
    g[m] = float(np.longdouble(1.0) / top)
    if not np.isfinite(g[m]) or g[m] == 0.0:
        raise api.ArgumentError(f"T_{m} at `below` = {below} is out of range: lower the degree or move `below` closer to the bounds")
    return c, e, g


def chebyshev_eval(center, halfwidth, coeffs, t):
    """p(t) = sum_k coeffs[k] T_k((t - center) / halfwidth) by Clenshaw's recurrence, elementwise: where the filter maps an
    eigenvalue t of A."""
    g = np.asarray(coeffs, dtype=np.float64)
    s = (np.asarray(t, dtype=np.float64) - center) / halfwidth
    b1 = np.zeros_like(s)
    b2 = np.zeros_like(s)
    for k in range(g.size - 1, 0, -1):
        b1, b2 = g[k] + 2.0 * s * b1 - b2, b1
    return g[0] + s * b1 - b2


def grid_spectrum_bounds(taps, potential=None, radius=1):
    """(a, b): the Gershgorin interval of a Hermitian constant-coefficient star operator (`api.grid_operator`,
    `api.grid_star_operator`; 2 ndim radius + 1 taps with a real centre, a real potential): every eigenvalue lies in
    [centre + min V - s, centre + max V + s] with s the sum of the moduli of the off-centre taps (a boundary row has fewer links,
    its disc lies inside).  Safe bounds for `chebyshev_window` / `chebyshev_damping`; periodic axes with wrap values of the taps'
    moduli (Bloch phases) have the same interval."""
    t = np.asarray(taps)
    if t.ndim != 1 or t.size % 2 != 1 or t.size < 3:
        raise api.ArgumentError(f"taps must hold 2 ndim radius + 1 values, got shape {t.shape}")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 4 \
            or (t.size - 1) % (2 * int(radius)) or not 1 <= (t.size - 1) // (2 * int(radius)) <= 3:
        raise api.ArgumentError(f"{t.size} taps do not belong to a star stencil of radius {radius!r} in 1, 2 or 3 dimensions")
    centre = t[t.size // 2]
    v = np.zeros(1) if potential is None else np.asarray(potential).ravel()
    if np.imag(centre) != 0 or np.any(np.imag(v) != 0):
        raise api.ArgumentError("Gershgorin bounds on the real line need a Hermitian operator: the centre tap and the potential must be real")
    if v.size == 0 or not (np.all(np.isfinite(v.real)) and np.all(np.isfinite(t))):
        raise api.ArgumentError("taps and potential must be finite (and the potential non-empty)")
    s = float(np.sum(np.abs(t)) - abs(centre))
    d = float(np.real(centre))
    return d + float(v.real.min()) - s, d + float(v.real.max()) + s
