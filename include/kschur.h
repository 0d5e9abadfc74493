/*
 * kschur.h -- C ABI of libkschur_hip.so: the MI355X (gfx950) implementation of the
 * Krylov-Schur Arnoldi hot path of ArnoldiMethod.jl.
 *
 * This header is the drop-in boundary.  Every entry point names the reference
 * interface it replaces as  <file>:<line>  relative to the reference tree
 * (JuliaLinearAlgebra/ArnoldiMethod.jl v0.4.0).  The Julia-side binding a maintainer
 * would add is shown in INTEGRATION.md (one `ccall` per function below).
 *
 * Conventions
 *   - plain C: opaque handles, plain pointers and sizes, no C++/torch types;
 *   - every function returns an int status (KS_OK == 0); no exceptions cross the ABI;
 *     ks_last_error_string() describes the last failure on the calling thread;
 *   - matrices are COLUMN-MAJOR like Julia's `Matrix`; indices in THIS header are 0-based
 *     (column j here is column j+1 of the reference);
 *   - dtype: KS_F64 = Float64, KS_C64 = ComplexF64 (interleaved re,im); host pointers typed
 *     `void*` point at elements of the handle's dtype;
 *   - host pointers are borrowed for the duration of a call only (GC.@preserve suffices);
 *   - one host thread drives one context; calls are stream-ordered on the device and
 *     synchronous with respect to any host value they return;
 *   - multi-GPU: one process per GPU, rows of A and V are block-partitioned across ranks,
 *     the global sums inside the Gram-Schmidt steps are RCCL all-reduces, H/Q stay
 *     replicated on every host.
 */
#ifndef KSCHUR_H
#define KSCHUR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_VERSION_MAJOR 0
#define KS_VERSION_MINOR 1

/* ---- status codes -------------------------------------------------------------------- */
enum {
  KS_OK = 0,
  KS_ERR_ARGUMENT = 1,  /* Julia ArgumentError     (src/run.jl:111-116,123-124,165-174,185) */
  KS_ERR_DIMENSION = 2, /* Julia DimensionMismatch (checksquare, src/run.jl:110)            */
  KS_ERR_HIP = 3,       /* HIP runtime failure                                              */
  KS_ERR_RCCL = 4,      /* RCCL failure                                                     */
  KS_ERR_QR = 5,        /* "QR algorithm did not converge" (src/schurfact.jl:406)           */
  KS_ERR_INTERNAL = 6,
  KS_ERR_NO_DEVICE = 7, /* no gfx950 device visible: the product path has NO CPU fallback   */
  KS_ERR_OPERATOR = 8,  /* user operator callback reported failure                          */
  KS_ERR_COMM = 9       /* a peer did not show up within KS_P2P_TIMEOUT_S (peer-to-peer mode) */
};

enum { KS_F64 = 0, KS_C64 = 1 };                 /* element type of A, V, H, Q              */
enum { KS_I32 = 0, KS_I64 = 1 };                 /* index type of an uploaded sparse matrix */
enum { KS_CSR = 0, KS_CSC = 1 };                 /* layout of an uploaded sparse matrix     */
/* Targets, src/targets.jl:7-32 and _symbol_to_target, src/run.jl:181-185 */
enum { KS_LM = 0, KS_LR = 1, KS_SR = 2, KS_LI = 3, KS_SI = 4 };

typedef struct ks_ctx ks_ctx;             /* device + stream (+ RCCL communicator)           */
typedef struct ks_operator ks_operator;   /* anything with mul!(y, A, x)  (src/run.jl:21-22) */
typedef struct ks_workspace ks_workspace; /* ArnoldiWorkspace (src/ArnoldiMethod.jl:41-93)   */

const char* ks_last_error_string(void);
int ks_version(int* major, int* minor);

/* ---- context ------------------------------------------------------------------------- */
/* Single-GPU context on HIP device `device`. */
int ks_ctx_create(int device, ks_ctx** out);
/* Multi-GPU context: rank `rank` of `nranks`, one process per GPU.  `unique_id` is the 128-byte
 * RCCL id produced by ks_comm_unique_id() on rank 0 and broadcast by the host language
 * (torch.distributed / MPI / Distributed.jl).  No reference equivalent: the reference is a
 * single process. */
int ks_comm_unique_id(void* out128);
int ks_ctx_create_dist(int device, int rank, int nranks, const void* unique_id128, ks_ctx** out);
/* Multi-GPU context on the peer-to-peer transport (csrc/ks_p2p.hpp): the per-step reductions and the
 * ghost exchange of the SpMV run as remote stores into IPC-shared, uncached regions over xGMI instead of
 * RCCL calls (same results; sums are formed in rank order on every rank).  Protocol: every rank calls
 * ks_ctx_create_p2p, exports its 64-byte region handle with ks_ctx_p2p_handle, the host language
 * all-gathers the handles, and every rank passes the nranks x 64 bytes (rank order) to ks_ctx_p2p_attach.
 * Needs HSA_ENABLE_IPC_MODE_LEGACY=0 on this image.  ks_ctx_create_dist with KS_TRANSPORT=p2p does the
 * same through one RCCL all-gather.  In this mode ks_operator_csr_dist is a collective call.
 * KS_P2P_CAP (2048 doubles per reduction), KS_P2P_ARENA_MB (64), KS_P2P_TIMEOUT_S (30) tune the region. */
int ks_ctx_create_p2p(int device, int rank, int nranks, ks_ctx** out);
int ks_ctx_p2p_handle(ks_ctx* ctx, void* out64);
int ks_ctx_p2p_attach(ks_ctx* ctx, const void* handles);
/* Multi-GPU context on a HOST-STAGED transport: the library runs exactly the launch structure of the RCCL
 * transport (reduce-only kernels -> all-reduce -> post kernels, src/expansion.jl:84,88,93,96 sharded by rows;
 * pack kernel -> neighbour exchange -> SpMV on the ghost buffer, src/expansion.jl:121), but every exchange is
 * copied to pinned host memory and handed to two caller-supplied functions, e.g. MPI_Allreduce /
 * MPI_Sendrecv or torch.distributed on gloo:
 *   allreduce(user, buf, count)            in-place sum over all ranks of `count` doubles; every rank must
 *                                          obtain the bit-identical result (the DGKS branches depend on it)
 *   exchange(user, npeers, peers, sendbufs, send_bytes, recvbufs, recv_bytes)
 *                                          one grouped neighbour exchange (send i -> peers[i], receive from it)
 * Both return 0 on success; anything else surfaces as KS_ERR_COMM.  No arithmetic happens on the host.  This is how
 * the code around every RCCL call site is exercised with several real ranks on a one-GPU box (RCCL refuses two
 * ranks per device), and a transport of last resort where RCCL is unavailable.  No reference equivalent. */
typedef int (*ks_host_allreduce_fn)(void* user, double* buf, int count);
typedef int (*ks_host_exchange_fn)(void* user, int npeers, const int32_t* peers, const void* const* sendbufs,
                                   const int64_t* send_bytes, void* const* recvbufs, const int64_t* recv_bytes);
int ks_ctx_create_hostcomm(int device, int rank, int nranks, ks_host_allreduce_fn allreduce,
                           ks_host_exchange_fn exchange, void* user, ks_ctx** out);
int ks_ctx_destroy(ks_ctx* ctx);
int ks_ctx_synchronize(ks_ctx* ctx);
int ks_ctx_rank(const ks_ctx* ctx, int* rank, int* nranks);
/* Raw hipStream_t of the context (so a caller can time with hipEvents on the right stream). */
int ks_ctx_stream(ks_ctx* ctx, void** hip_stream);

/* ---- operator seam:  mul!(y, A, x), eltype(A), size(A)   (src/expansion.jl:121) ------- */
/* (i) device-resident CSR operand.  Accepts CSR or CSC (Julia's SparseMatrixCSC: colptr /
 * rowval / nzval, 1-based Int64 -> layout=KS_CSC, index_base=1, index_type=KS_I64) and
 * converts once to int32 0-based CSR in HBM.  `nrows_local` x `ncols` is this rank's row block
 * (single GPU: the whole square matrix).  Replaces SparseArrays' `mul!` for
 * `SparseMatrixCSC` (stdlib; call site src/expansion.jl:121). */
int ks_operator_csr(ks_ctx* ctx, int64_t nrows_local, int64_t ncols, int64_t nnz,
                    const void* ptr, const void* idx, const void* val, int layout, int index_base,
                    int index_type, int dtype, ks_operator** out);
/* Distributed CSR: this rank owns global rows [row_begin, row_begin+nrows_local); column indices
 * are already LOCAL-EXTENDED: 0..nrows_local-1 address owned entries of x, nrows_local+g
 * addresses ghost slot g.  Ghost slots are filled before every product by the halo plan:
 * for each neighbour p: send x[send_idx[send_ptr[p] .. send_ptr[p+1])] to rank neigh[p] and
 * receive recv_cnt[p] values into consecutive ghost slots (in neighbour order). */
int ks_operator_csr_dist(ks_ctx* ctx, int64_t nrows_local, int64_t nghost, int64_t nnz,
                         const int64_t* rowptr, const int32_t* colidx, const void* val, int dtype,
                         int nneigh, const int32_t* neigh, const int64_t* send_ptr,
                         const int32_t* send_idx, const int64_t* recv_cnt, ks_operator** out);
/* (i') dense matrix (mul!(y, A::Matrix, x)): n x n elements of `dtype`, leading dimension `ld` elements,
 * KS_COL_MAJOR (Julia / Fortran) or KS_ROW_MAJOR (C / numpy).  Kept row-major in HBM; y = A*x streams it
 * once per product (8 or 16 bytes per entry).  Single-GPU contexts only. */
#define KS_ROW_MAJOR 0
#define KS_COL_MAJOR 1
int ks_operator_dense(ks_ctx* ctx, int64_t n, const void* a, int64_t ld, int layout, int dtype,
                      ks_operator** out);
/* (ii) opaque host operator (e.g. a LinearMap wrapping ldiv! with a host LU,
 * docs/src/index.md:246-249): `apply(user, x_host, y_host)` computes y = A*x on n_local
 * elements of `dtype`; return nonzero to signal failure.  The library stages the two columns
 * over PCIe. */
typedef int (*ks_host_apply_fn)(void* user, const void* x_host, void* y_host);
int ks_operator_host_callback(ks_ctx* ctx, int64_t n_local, int dtype, ks_host_apply_fn apply,
                              void* user, ks_operator** out);
/* (iii) opaque device operator: `apply(user, x_dev, y_dev, hip_stream)` must enqueue y = A*x on
 * the given stream (x_dev/y_dev are device pointers to n_local elements). */
typedef int (*ks_device_apply_fn)(void* user, const void* x_dev, void* y_dev, void* hip_stream);
int ks_operator_device_callback(ks_ctx* ctx, int64_t n_local, int dtype, ks_device_apply_fn apply,
                                void* user, ks_operator** out);
/* (iv) shift-invert from the caller's triangular factors:  y = P_out U^-1 L^-1 P_in (s o x), both sparse triangular
 * solves on the device, every vector resident in HBM.  Replaces the host `ldiv!(y, F, x)` inside the LinearMap a user of
 * the reference wraps around F = lu(A - sigma I) / factorize(A)  (docs/src/index.md:246-249, 273-287); the
 * factorisation itself stays the caller's, on the host, as there.
 *   L, U       n x n CSR, int64 row offsets, int32 0-based columns, values of `dtype`; L lower triangular (diagonal
 *              entries optional: unit where absent), U upper triangular with every diagonal entry, both non-singular
 *   perm_in    row i of the triangular system takes x[perm_in[i]]      (NULL: identity)
 *   scale      ... multiplied by the real scale[perm_in[i]]            (NULL: none; UMFPACK's row scaling `Rs`)
 *   perm_out   y[perm_out[i]] = entry i of U^-1 L^-1 (...)             (NULL: identity)
 * SuiteSparse UMFPACK (Julia `F = lu(A)`: (Rs .* A)[p, q] = L U): perm_in = p-1, scale = Rs, perm_out = q-1, factors
 * transposed from CSC.  SuperLU (scipy `splu`: Pr A Pc = L U): perm_in = inverse(perm_r), perm_out = inverse(perm_c).
 * One or two launches per factor (synchronisation-free solves: a row's wavefront waits for the entries it needs; independent
 * parts of the factor run on separate XCDs, dense triangles of narrow dependency levels are inverted at upload while their
 * inverses stay tame -- KS_LU_RUN_COND).  The cost is dependency chains and memory round trips, not bytes:
 * ks_operator_lu_info / ks_operator_lu_layout report levels, fill and the device layout -- choose a fill-reducing ordering
 * with a short, bushy elimination tree.  Products are deterministic (bit-identical when repeated).  A wait that exceeds
 * KS_LU_TIMEOUT_S (20) ends the kernel and surfaces ONCE as KS_ERR_OPERATOR at the next synchronisation point of the
 * context (the vectors of that product are garbage).  Single-GPU contexts only. */
int ks_operator_lu(ks_ctx* ctx, int64_t n, int dtype, const int64_t* l_rowptr, const int32_t* l_colind, const void* l_val,
                   const int64_t* u_rowptr, const int32_t* u_colind, const void* u_val, const int32_t* perm_in,
                   const int32_t* perm_out, const double* scale, ks_operator** out);
/* strictly triangular stored entries and dependency-chain lengths ("levels") of the two factors */
int ks_operator_lu_info(const ks_operator* op, int64_t* nnz_l, int64_t* nnz_u, int64_t* levels_l, int64_t* levels_u);
/* how one factor (upper = 0 / 1) is laid out for the device: rows of the system the kernel solves (n + one more per row
 * of an inverted dense run), rows in such runs, rows of the part next to the root of the elimination tree that runs on one
 * XCD, and the number of independent groups the rest was split into (0: one launch for everything) */
int ks_operator_lu_layout(const ks_operator* op, int upper, int64_t* rows, int64_t* run_rows, int64_t* top_rows, int* ngroups);
/* (v) tridiagonal shift-invert, factored once:  y = (T - sigma I)^-1 x  for tridiagonal T -- the `ldiv!(y, F, x)` of the
 * LinearMap the reference's shift-invert recipe wraps around F = factorize(A - sigma I)  (docs/src/index.md:234-259), for a 1-D
 * operator.  Recursive separator elimination: the rows are split into blocks of at most `block_rows` rows with one separator row
 * between neighbours; per block a partially pivoted LU and its two spikes are computed ON THE HOST at upload, the separators'
 * Schur system (tridiagonal again) becomes the next level, and a level of at most 2 block_rows rows is solved outright.  A
 * product is one launch per level down, one per level back up (5 at n = 5e5), every vector resident in HBM; no vendor library.
 *   dl, du      n - 1 entries (sub- / super-diagonal), d: n entries, all of `dtype`;  sigma_im must be 0 for KS_F64
 *   block_rows  0: default (64), otherwise 2...64.  A block is accepted only while max|M_p^-1 [e_first e_last]| ||M_p|| <= 1e6;
 *               the planner shortens blocks (with backtracking) where the default split would give a singular or badly
 *               conditioned block, and reports how many in ks_operator_tridiag_info
 * KS_ERR_ARGUMENT: non-finite input, no admissible partition (the message names level and row), an exactly zero pivot in the
 * direct solve, a check solve (b_i = cos(0.7 i + 0.3)) whose normwise backward error exceeds 1e-10, more than 8 levels, a
 * multi-rank context.  Products are deterministic (bit-identical when repeated). */
int ks_operator_tridiag_solve(ks_ctx* ctx, int64_t n, int dtype, const void* dl, const void* d, const void* du, double sigma_re,
                              double sigma_im, int block_rows, ks_operator** out);
/* what the planner of ks_operator_tridiag_solve made of the matrix (docs/src/index.md:234-259: the factorisation behind the
 * LinearMap): number of levels, rows of each (level_rows: 8 entries, zero beyond `levels`), blocks shorter than the default split,
 * the largest accepted block growth and the backward error of the check solve.  KS_ERR_ARGUMENT on any other kind of operator. */
int ks_operator_tridiag_info(const ks_operator* op, int* levels, int64_t* level_rows /* cap 8 */, int64_t* shortened_blocks,
                             double* max_growth, double* residual);
/* (vi) the tridiagonal pencil, fused:  y = T^-1 M x  for tridiagonal T (factored) and M (multiplied) -- the operator
 * x -> (A - sigma B)^-1 (B x) of the reference's shift-and-invert recipe for generalized problems A x = B x lambda
 * (docs/src/index.md:273-287) for a 1-D pencil; the CALLER forms T = K - sigma M, the library does no arithmetic on its inputs.
 * T is planned and factored exactly as ks_operator_tridiag_solve plans (dl, d, du) with shift 0 -- same refusals, same report
 * through ks_operator_tridiag_info -- and level 0 of the elimination forms its right-hand side
 * md[r] x[r] + mdl[r-1] x[r-1] + mdu[r] x[r+1] (in this order) while it stages it: no launch and no vector for M x.
 *   mdl, mdu   n - 1 entries, md: n entries, all of `dtype` and finite;  x and y of a product must be distinct
 * An M whose three diagonals are each one value (the consistent mass of a uniform mesh) is passed to the kernel by value: the
 * product then streams exactly the bytes of the plain solve, otherwise 3 n sizeof(dtype) more.
 * Eigenvalues of the pencil nearest sigma: sigma + 1/theta.  Single-GPU contexts only; deterministic like (v). */
int ks_operator_tridiag_pencil(ks_ctx* ctx, int64_t n, int dtype, const void* dl, const void* d, const void* du, const void* mdl,
                               const void* md, const void* mdu, int block_rows, ks_operator** out);
/* (vii) product of operators:  y = ops[0] ops[1] ... ops[nops-1] x  in mathematical order (ops[nops-1] is applied to x first,
 * ops[0] writes y), every intermediate vector resident in HBM -- the composed LinearMaps of the reference's recipes for
 * generalized problems: x -> (A - sigma B)^-1 (B x), docs/src/index.md:273-287, and x -> L^-1 A L^-* x for B = L L*,
 * docs/src/index.md:325-336.  2 <= nops <= 8; every factor non-null, made on `ctx`, of one n_local and one dtype
 * (KS_ERR_ARGUMENT otherwise, the message names the factor); single-GPU contexts only.  The factors are BORROWED: the product
 * never destroys them, the caller keeps them alive as long as the product is applied, and destroying the product leaves them
 * usable; a factor may appear more than once.  The product owns at most two intermediate vectors; x is never written.  An
 * error of a factor (a callback returning non-zero) comes out of the call that applied the product, unchanged.  The product is
 * enqueued ahead only if every factor can be; ks_operator_size reports the sum of the factors' nnz, ks_operator_format layout -1. */
int ks_operator_product(ks_ctx* ctx, int nops, ks_operator* const* ops, ks_operator** out);
/* (viii) matrix-free grid operator: a constant-coefficient 3-, 5- or 7-point stencil plus a per-point diagonal term (a potential
 * -Laplacian + V(x), a reaction or mass term) -- mul!(y, A, x), src/expansion.jl:121, with nothing stored per non-zero: the grid
 * shape gives the boundary rows by index arithmetic, the taps travel in the kernel arguments, the only per-row datum is the
 * diagonal entry.  A product moves x, the diagonal and y once: 24 bytes per row in Float64 (16 without a potential), twice that
 * in ComplexF64.  DEFINITION -- the operator is the matrix ks_host_grid_matrix returns:
 *   grid        nx x ny x nz points, x fastest: row r = ix + nx (iy + ny iz), n = nx ny nz; dims holds ndim extents
 *               (nx[, ny[, nz]]), for ndim 1 or 2 the missing extents are 1
 *   taps        2 ndim + 1 values of `dtype` in ascending column order: [-z, -y, -x, centre, +x, +y, +z] in 3-D,
 *               [-y, -x, centre, +x, +y] in 2-D, [-x, centre, +x] in 1-D
 *   boundaries  a tap whose neighbour lies outside the grid is absent (Dirichlet truncation, no wrap-around: the last point of
 *               an x-line and the first of the next are not neighbours)
 *   diagonal    entry of row r: centre + potential[r] -- one addition, rounded once, componentwise for ComplexF64 -- stored even
 *               when the sum is zero; potential == NULL: centre
 *   product     every product is rounded on its own and added to +0.0 in ascending column order: y has the bits every stored
 *               layout gives, i.e. the product is bit-identical to ks_operator_csr applied to the matrix of
 *               ks_host_grid_matrix, and a whole solve is interchangeable between the two
 * KS_ERR_ARGUMENT (the message names the cause): ndim outside 1...3, an extent < 1, more than 2^31 - 2 points (n and the plane
 * stride must fit the 32-bit row index of the stored matrix), a non-finite tap or potential entry, a multi-rank context.
 * ks_operator_size reports n and the number of in-grid taps, ks_operator_format 0 / 0 / -1.  The operator is enqueued ahead like a
 * stored matrix; products are deterministic; x is never written, rows >= n of y are never written; x and y of a product must be
 * distinct.  The Newton step of the s-step expansion is one launch of the same kernel (KS_SHIFT_FUSED=0: the product and a pass). */
int ks_operator_grid(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                     const void* taps /* 2*ndim+1 values of dtype */, const void* potential /* n values of dtype, or NULL */,
                     ks_operator** out);
/* (ix) ... with periodic axes: crystal Hamiltonians, band structures at a k-point (Bloch phases on the links that cross the cell
 * boundary), lattice models on a torus -- mul!(y, A, x), src/expansion.jl:121, still with nothing stored per non-zero and the same
 * compulsory traffic.  Everything of (viii) holds, with these additions.  DEFINITION -- the operator is the matrix
 * ks_host_grid_matrix_periodic returns:
 *   periodic    ndim flags in the order of dims (x[, y[, z]]); NULL: no axis wraps.  On a periodic axis of extent m the point at
 *               index 0 has a - neighbour at index m - 1 and the point at m - 1 a + neighbour at 0; an axis that is not periodic
 *               is truncated as in (viii)
 *   wrap        2 ndim values of `dtype` in the order of the taps with the centre left out ([-z, -y, -x, +x, +y, +z] in 3-D): the
 *               entry of the link that crosses the boundary in that direction.  NULL: the taps themselves (plain periodicity).
 *               Bloch: wrap[+-x] = t e^{+-i theta_x}; antiperiodic: wrap = -taps.  Values of axes that do not wrap are neither
 *               read nor checked
 *   row         columns ascending: a row is a sub-sequence of 13 slots, each present or absent by index arithmetic,
 *                 +z wrap (iz = nz-1) | -z | +y wrap (iy = ny-1) | -y | +x wrap (ix = nx-1) | -x | centre |
 *                 +x | -x wrap (ix = 0) | +y | -y wrap (iy = 0) | +z | -z wrap (iz = 0)
 *               -- a wrap link stands (and is summed) at another place than the interior link of its direction
 *   product     every product rounded on its own and added to +0.0 in this order: bit-identical to ks_operator_csr of the matrix
 * KS_ERR_ARGUMENT in addition (the message names the cause and the axis or index): a periodic axis of extent < 3 (at 2 the two
 * neighbours coincide, at 1 the link is a self-link: the matrix would need duplicate or merged entries), a non-finite wrap value
 * of a periodic axis.  ks_operator_size reports nnz = n (1 + 2 #periodic axes) + 2 sum over the open axes a of (m_a - 1) n / m_a.
 * With no periodic axis the operator is that of ks_operator_grid. */
int ks_operator_grid_periodic(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                              const void* taps /* 2*ndim+1 values of dtype */, const void* potential /* n values of dtype, or NULL */,
                              const int* periodic /* ndim flags, or NULL */, const void* wrap /* 2*ndim values of dtype, or NULL */,
                              ks_operator** out);
/* (x) ... with a STAR stencil of radius 1...4: central differences of order 2, 4, 6, 8 (extras.fd_laplacian_taps), the stencils of
 * real-space Schroedinger and electronic-structure codes -- mul!(y, A, x), src/expansion.jl:121, still with nothing stored per
 * non-zero and the same compulsory traffic (24 / 16 bytes per row in Float64), where the stored matrix of a 3-D radius-4 star streams
 * about 300.  Everything of (viii) holds, with these additions.  DEFINITION -- the operator is the matrix ks_host_grid_matrix_star
 * returns:
 *   radius      R, 1 <= R <= 4: neighbours at the distances 1...R along every axis
 *   taps        2 ndim R + 1 values of `dtype` in ascending column order: in 3-D
 *                 [-R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z]
 *               (2-D and 1-D: without the z, the z and y groups); for R = 1 the layout of (viii)
 *   boundaries  open: a tap whose neighbour i_a + d lies outside [0, m_a) is absent, no wrap-around; an axis shorter than R + 1
 *               never has its outer taps
 *   row         a sub-sequence of these 6 R + 1 slots; nnz = n + sum over the axes a and d = 1...R of 2 max(m_a - d, 0) n / m_a
 *   product     every product rounded on its own and added to +0.0 in this order: bit-identical to ks_operator_csr of the matrix.
 *               An absent tap -- outside the grid, or beyond the radius -- is not multiplied at all
 * KS_ERR_ARGUMENT in addition: radius outside 1...4 (the message names radius); "tap k is not finite" counts k in this layout.
 * Boundaries are open here; periodic axes: (x-b).  With radius == 1 the operator is that of ks_operator_grid: same matrix, same
 * kernel. */
int ks_operator_grid_star(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int radius, int dtype,
                          const void* taps /* 2*ndim*radius+1 values of dtype */,
                          const void* potential /* n values of dtype, or NULL */, ks_operator** out);
/* (x-b) ... the STAR stencil with periodic axes: crystals and supercells with central differences of order 4, 6, 8, a band structure
 * at a k-point with an 8th-order Laplacian -- mul!(y, A, x), src/expansion.jl:121, still with nothing stored per non-zero and the
 * same compulsory traffic.  Everything of (viii) and (x) holds, with these additions.  DEFINITION -- the operator is the matrix
 * ks_host_grid_matrix_star_periodic returns:
 *   periodic    as in (ix): ndim flags in the order of dims, NULL: no axis wraps.  On a periodic axis of extent m the point at
 *               index i has its +d neighbour at i + d - m where i + d >= m and its -d neighbour at i - d + m where i < d; an axis
 *               that does not wrap is truncated as in (x) and may have any extent >= 1
 *   extent      of a periodic axis: at least 2 R + 1 (below that two links of a row coincide or a link is a self-link)
 *   wrap        2 ndim R values of `dtype` in the order of the taps with the centre left out: in 3-D
 *                 [-R z ... -1 z, -R y ... -1 y, -R x ... -1 x, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z]
 *               -- the entry of the link of that direction and distance where it crosses the cell boundary.  NULL: the taps
 *               themselves (plain periodicity).  Bloch: wrap[+-d a] = t e^{+-i theta_a}, the same phase at every distance (a link
 *               crosses the boundary at most once; extras.bloch_wrap(taps, theta, radius)).  Values of axes that do not wrap are
 *               neither read nor checked
 *   row         columns ascending.  Before the centre the axes come in the order z, y, x, each with two groups: (1) its +d links
 *               that wrap (i_a + d >= m_a), d ascending, column r + (d - m_a) stride_a, value wrap[+d a]; (2) its interior -d
 *               links, d = R ... 1, value tap[-d a].  Then the centre.  After it the axes come in the order x, y, z, each with two
 *               groups: (1) its interior +d links, d = 1 ... R; (2) its -d links that wrap (i_a - d < 0), d = R ... 1, column
 *               r + (m_a - d) stride_a, value wrap[-d a].  With m_a >= 2 R + 1 this is the ascending column order; a row of a fully
 *               periodic grid has exactly 6 R + 1 entries (2 ndim R + 1).  As in (ix) a wrap link stands (and is summed) at another
 *               place than the interior link of its direction
 *   product     every product rounded on its own and added to +0.0 in this order: bit-identical to ks_operator_csr of the matrix
 *   nnz         n + sum over the axes a of (periodic ? 2 R n : sum over d = 1...R of 2 max(m_a - d, 0) n / m_a): what
 *               ks_operator_size reports
 * With tap[-d a] = conj(tap[+d a]) and wrap[-d a] = conj(wrap[+d a]) the matrix is exactly Hermitian.  KS_ERR_ARGUMENT in addition:
 * a periodic axis of extent < 2 R + 1 (the message names the axis, the extent, the radius and the word "periodic"), a non-finite
 * wrap value of a periodic axis ("wrap value k is not finite", k its index in `wrap`).  REDUCTIONS -- with no periodic axis the
 * operator is that of ks_operator_grid_star (same object, same kernel launch), with radius == 1 that of ks_operator_grid_periodic. */
int ks_operator_grid_star_periodic(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int radius, int dtype,
                                   const void* taps /* 2*ndim*radius+1 values of dtype */,
                                   const void* potential /* n values of dtype, or NULL */,
                                   const int* periodic /* ndim flags, or NULL */,
                                   const void* wrap /* 2*ndim*radius values of dtype, or NULL */, ks_operator** out);
/* (xi) ... with a VARIABLE coefficient: A = -div(c(x) grad) + V(x) -- heterogeneous diffusion, a position-dependent effective mass,
 * div (1 / eps) grad in photonics, variable-density acoustics -- mul!(y, A, x), src/expansion.jl:121, still with nothing stored per
 * non-zero although the off-diagonal entries vary from link to link: the coefficient is cell-centred, one Float64 per grid point, and
 * the link entries are formed in registers.  A product moves x, c, the diagonal and y once: 32 bytes per row in Float64 (24 without a
 * potential), 56 / 40 in ComplexF64, where the stored matrix streams about 100.  Grid, row numbering, dims, ndim, dtype, taps and
 * potential as in (viii), with these additions.  DEFINITION -- the operator is the matrix ks_host_grid_var_matrix returns:
 *   coeff       n Float64 values, one per grid point in row order; always REAL, also for KS_C64; finite, no sign requirement
 *   half taps   h_k = 0.5 t_k for the six off-diagonal slots, computed once on the host (componentwise for ComplexF64)
 *   entry       of the link from row r to its in-grid neighbour s in direction k:  A[r, s] = fl(h_k * fl(c[r] + c[s]))  -- one
 *               Float64 addition, rounded, then one multiplication, rounded; ComplexF64: the two real multiplications
 *               (h_k.re * m, h_k.im * m).  A link whose neighbour lies outside the grid is absent, as in (viii)
 *   diagonal    centre + potential[r] as in (viii), stored even where it is zero; potential == NULL: centre.  A diffusion operator
 *               passes centre 0 and its whole diagonal as the potential (extras.diffusion_terms)
 *   row         the 7 slots -z, -y, -x, centre, +x, +y, +z; nnz as in (viii)
 *   product     every product A[r, s] x[s] rounded on its own and added to +0.0 in slot order, an absent link not multiplied at all:
 *               bit-identical to ks_operator_csr of the matrix.  With c == 1 the matrix is bit for bit that of ks_host_grid_matrix
 *               (0.5 t * 2 is exact)
 * KS_ERR_ARGUMENT as in (viii), and in addition: coeff == NULL, "coefficient entry k is not finite".  ks_operator_size reports n and
 * nnz, ks_operator_format 0 / 0 / -1.  The Newton step of the s-step expansion is one launch of the same kernel, as in (viii). */
int ks_operator_grid_var(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                         const void* taps /* 2*ndim+1 values of dtype */, const double* coeff /* n values */,
                         const void* potential /* n values of dtype, or NULL */, ks_operator** out);
/* (xi-b) ... with a variable coefficient AND periodic axes: photonic and phononic crystals (div (1 / eps) grad at a k-point), a
 * superlattice with a position-dependent mass, heterogeneous diffusion on a torus -- mul!(y, A, x), src/expansion.jl:121, still with
 * nothing stored per non-zero and the traffic of (xi).  Everything of (xi) and of (ix) holds, combined as follows.  DEFINITION -- the
 * operator is the matrix ks_host_grid_var_matrix_periodic returns:
 *   periodic    as in (ix): ndim flags in the order of dims, NULL: no axis wraps; a periodic axis needs extent >= 3
 *   wrap        as in (ix): 2 ndim values of `dtype` in the order of the taps without the centre, NULL: the taps themselves; values
 *               of periodic axes must be finite, values of open axes are neither read nor checked
 *   half wrap   hw_k = 0.5 wrap_k, computed once on the host like the half taps (componentwise for ComplexF64)
 *   entry       an interior link in slot k: fl(h_k * fl(c[r] + c[s])) as in (xi); a link that crosses the boundary in direction k,
 *               s being the wrap image at the other end of the line:  A[r, s] = fl(hw_k * fl(c[r] + c[s]))  (ComplexF64: the two real
 *               multiplications)
 *   diagonal    centre + potential[r], as in (viii)
 *   row         a sub-sequence of the 13 slots of (ix), in that order; nnz as in (ix)
 *   product     every product A[r, s] x[s] rounded on its own and added to +0.0 in slot order: bit-identical to ks_operator_csr of
 *               the matrix
 * With no periodic axis the operator is that of ks_operator_grid_var (same matrix, same kernel).  With c == 1 the matrix is bit for bit
 * that of ks_host_grid_matrix_periodic (0.5 w * 2 is exact).  With real c, taps with t_{-a} = conj(t_{+a}) and Bloch wrap values
 * t_{+-a} e^{+-i theta_a} the matrix is exactly Hermitian: c[r] + c[s] commutes and the two parts are rounded separately.
 * KS_ERR_ARGUMENT: the refusals of (xi), then those of (ix); the message names the cause and the axis or index.  ks_operator_size
 * reports the periodic nnz; the bytes of a product are those of (xi).  Single-GPU contexts only; the Newton step of the s-step
 * expansion is one launch of the same kernel, as in (viii). */
int ks_operator_grid_var_periodic(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                                  const void* taps /* 2*ndim+1 values of dtype */, const double* coeff /* n values */,
                                  const void* potential /* n values of dtype, or NULL */, const int* periodic /* ndim flags, or NULL */,
                                  const void* wrap /* 2*ndim values of dtype, or NULL */, ks_operator** out);
/* (xii) ... with the DIAGONAL neighbours: the 3-, 9- or 27-point BOX stencil, a link to every neighbour at distance one in the maximum
 * norm -- the mixed derivatives of -div(D grad) + V with a full constant tensor D (anisotropic media, effective-mass tensors, a lattice
 * in sheared coordinates), compact (Mehrstellen) Laplacians, stiffness and mass matrices of multilinear (Q1) finite elements on a uniform
 * grid -- mul!(y, A, x), src/expansion.jl:121, still with nothing stored per non-zero: 24 bytes per row in Float64 (16 without a
 * potential), twice that in ComplexF64, where the stored matrix streams about 330.  Grid, row numbering, dims, ndim, dtype and potential
 * as in (viii), open boundaries.  DEFINITION -- the operator is the matrix ks_host_grid_box_matrix returns:
 *   taps        3^ndim values of dtype in ascending column order: slot k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1) in 3-D,
 *               k = 3 (dy + 1) + (dx + 1) in 2-D, k = dx + 1 in 1-D, with dx, dy, dz in -1, 0, 1; the centre is slot (3^ndim - 1) / 2
 *   row         r = ix + nx (iy + ny iz) has the entry taps[k] at column r + dx + nx (dy + ny dz) for every slot whose neighbour
 *               (ix + dx, iy + dy, iz + dz) lies inside the grid (nothing wraps), stored even where the tap is zero; slot order is
 *               ascending column order, the columns being lexicographic in (jz, jy, jx);  nnz = prod_a (3 m_a - 2)
 *   diagonal    centre + potential[r] as in (viii), stored even where it is zero; potential == NULL: centre
 *   product     every product A[r, s] x[s] rounded on its own and added to +0.0 in slot order, an absent slot not multiplied at all:
 *               bit-identical to ks_operator_csr of the matrix.  In 1-D the matrix is that of ks_host_grid_matrix with the same taps
 * KS_ERR_ARGUMENT as in (viii) ("tap k is not finite" for every one of the 3^ndim).  ks_operator_size reports n and nnz,
 * ks_operator_format 0 / 0 / -1.  The Newton step of the s-step expansion is one launch of the same kernel, as in (viii).  Periodic
 * axes: (xii-b).  A variable coefficient and a radius above 1 are not offered for this stencil. */
int ks_operator_grid_box(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                         const void* taps /* 3^ndim values of dtype */, const void* potential /* n values of dtype, or NULL */,
                         ks_operator** out);
/* (xii-b) ... the box stencil with PERIODIC axes: a crystal in a non-orthogonal cell (-div(D grad) + V with the constant tensor D of the
 * sheared lattice, on a torus with Bloch phases), Q1 finite elements and compact Laplacians on a periodic cell -- mul!(y, A, x),
 * src/expansion.jl:121, still with nothing stored per non-zero and the traffic of (xii).  Everything of (xii) holds, with the following
 * additions.  A diagonal link can cross two or three cell faces at once, so the entries of the crossing links are given per CLASS.
 * DEFINITION -- the operator is the matrix ks_host_grid_box_matrix_periodic returns:
 *   periodic    as in (ix): ndim flags in the order of dims, NULL: no axis wraps; a periodic axis needs extent >= 3 (the refusal and
 *               the message of (ix))
 *   links       5^ndim values of dtype.  Along an axis the class e of a link is 0 = offset -1 across the boundary, 1 = offset -1,
 *               2 = offset 0, 3 = offset +1, 4 = offset +1 across the boundary; the flat index is 25 e_z + 5 e_y + e_x in 3-D,
 *               5 e_y + e_x in 2-D, e_x in 1-D.  An entry is READ, and checked for finiteness, only if at least one axis has class 0
 *               or 4 and every axis with class 0 or 4 is periodic; every other entry is neither read nor checked (the taps hold the
 *               all-interior entries).  NULL: every crossing link carries the tap of its slot (a plain torus)
 *   entry       the link from r to the neighbour (ix + dx, iy + dy, iz + dz), taken modulo the extent on periodic axes: taps[slot] if it
 *               crosses no boundary, otherwise links[e] with e_a = 0 or 4 on the axes it crosses and d_a + 2 on the others; a link
 *               that would leave the grid along a non-periodic axis is absent
 *   diagonal    centre + potential[r], as in (viii)
 *   row         along an axis of extent m the present offsets at index i come in the order (-1, 0, +1) in the interior; (0, +1) at
 *               i = 0 and (-1, 0) at i = m - 1 of an open axis; (0, +1, -1) at i = 0 and (+1, -1, 0) at i = m - 1 of a periodic axis.
 *               A row runs over dz in that order, inside that over dy, inside that over dx: ascending column order, the columns being
 *               lexicographic in (jz, jy, jx);  nnz = prod_a (periodic_a ? 3 m_a : 3 m_a - 2)
 *   product     every product A[r, s] x[s] rounded on its own and added to +0.0 in this row order: bit-identical to ks_operator_csr of
 *               the matrix
 * With no periodic axis the operator is that of ks_operator_grid_box (same matrix, same kernel).  In 1-D the matrix is that of
 * ks_host_grid_matrix_periodic with wrap = [links[0], links[4]].  With taps[-k] = conj(taps[k]) and links[mirror(e)] = conj(links[e]),
 * mirror: e_a -> 4 - e_a (Bloch phases), the matrix is Hermitian.
 * KS_ERR_ARGUMENT: the refusals of (xii), then those of (ix) for the flags and extents, then "link value k is not finite" with k the flat
 * index.  ks_operator_size reports the periodic nnz, ks_operator_format 0 / 0 / -1.  Single-GPU contexts only; the Newton step of the
 * s-step expansion is one launch of the same kernel, as in (viii). */
int ks_operator_grid_box_periodic(ks_ctx* ctx, int ndim, const int64_t* dims /* ndim entries: nx[, ny[, nz]] */, int dtype,
                                  const void* taps /* 3^ndim values of dtype */, const void* potential /* n values of dtype, or NULL */,
                                  const int* periodic /* ndim flags, or NULL */, const void* links /* 5^ndim values of dtype, or NULL */,
                                  ks_operator** out);
/* (xiii) Chebyshev polynomial filter:  y = p(A) x,  p(A) = sum_{k=0..degree} coeffs[k] T_k((A - center) / halfwidth) -- the spectral
 * transformation for operators that cannot be factored (a 216^3 grid operator): run the eigensolver on p(A), whose LARGEST
 * eigenvalues are the ones the coefficients select (an interior window, a clustered low end), and read A's eigenvalues off the
 * Schur vectors (README).  Clenshaw's recurrence in `degree` operator steps
 *     out = sigma (A in - center in) - w + gamma x          evaluated as ((t - w) + gamma x), t the Newton step of (viii),
 * by the schedule ks_host_chebyshev_plan returns: `degree` products and, where A fuses the step into its product's store (the
 * grid operators, (viii) - (xii-b): 40 instead of 64 bytes per row in Float64 with a potential), no other pass over the vectors;
 * every other operator runs the product and ONE streaming pass per step.  The fused step is the default where it measured
 * faster (the 7-point operator, and the radius-2 star and the box operator with open boundaries); KS_CHEB_FUSED=1 / 0 (read per step) forces
 * the fused / the generic path for every grid operator.  A is BORROWED like a product's factors: the caller keeps it alive, destroying the filter
 * leaves it usable.  Size, dtype and whether the filter can be enqueued ahead come from A; KS_F64 and KS_C64 operators are
 * accepted, center, halfwidth and the coefficients are real.  1 <= degree <= 256, halfwidth > 0 and finite, center and every
 * coefficient finite (KS_ERR_ARGUMENT otherwise, the message names the offending index); A made on `ctx`; single-GPU contexts
 * only.  The filter owns min(degree - 1, 3) intermediate vectors; x is never written.  p is unbounded outside
 * [center - halfwidth, center + halfwidth]: the interval must contain A's spectrum.  The Newton step of the s-step expansion on
 * the filter is its product and a streaming pass. */
int ks_operator_chebyshev(ks_ctx* ctx, ks_operator* A, int degree, double center, double halfwidth,
                          const double* coeffs /* degree + 1 */, ks_operator** out);
/* degree and intermediate vectors of a filter (0 / 0 for any other operator), and the Clenshaw steps `op` has run since its
 * creation by the path they took: fused into the product's launch / product plus streaming pass.  A filter counts the steps of
 * its own applications; any other operator the steps run on it (through a filter or through ks_debug_apply_clenshaw). */
int ks_operator_chebyshev_info(const ks_operator* op, int* degree, int* temporaries, int64_t* fused_steps, int64_t* generic_steps);
/* (xiv) Conjugate-gradient solve:  y ~ (A - shift I)^-1 x  for a Hermitian positive definite A - shift I, with nothing but products of
 * A -- the inner iterative solver of the reference's "LinearMap around a solve" (docs/src/index.md:234-259, and :273-287 for the
 * pencil) for operators that have nothing to factor: M^-1 K of matrix-free finite elements (ks_operator_product of this operator on M
 * and K), (A - shift)^-1 with the shift below the spectrum.  Every vector stays in HBM and every scalar of the recurrence on the
 * device:
 *     y = 0, r = p = x, rho = rho0 = ||x||^2                         (rho0 == 0: y = 0, 0 iterations)
 *     q = (A - shift) p;  pq = Re p^H q;  alpha = rho / pq;  r -= alpha q;  rho' = ||r||^2;  y += alpha p;
 *     done if rho' <= tol^2 rho0, else beta = rho' / rho, p = r + beta p, rho = rho'
 * with the scalar step of ks_host_cg_step.  The product is the Newton step of (viii) with sigma = 1 (fused into the product by every
 * stored-matrix and grid layout), A's plain product when shift == 0; the rest of an iteration is three kernels that move 16 + 24 + 40
 * bytes per row in Float64; KS_C64 runs the same kernels on the real view.  The host enqueues `check_every` iterations (0: the
 * library default, 8), then reads a device record and goes on until done, a failure or maxit: y and the iteration count do not
 * depend on check_every, and equal inputs give equal bits.  A is BORROWED like a product's factors.  The solve is linear in x only
 * up to tol * cond(A - shift): an outer eigensolver's Arnoldi relation inherits that, choose tol at least 100 times tighter than
 * the outer tolerance.
 * KS_ERR_ARGUMENT: A made on another context; A that cannot be enqueued ahead (a host callback, another solve of this kind, a
 * product or filter of one); a context of several ranks ("single-GPU contexts only"); tol not in (0, 1); maxit < 1;
 * check_every < 0; shift not finite.  The operator itself is applied one step per batch, like a host callback.
 * KS_ERR_OPERATOR at apply time, the operator staying usable: "not positive definite: p^H (A - theta) p = ... at iteration k" (pq not
 * finite or <= 0), "did not converge: relative residual ... after maxit iterations".  ks_operator_size reports A's nnz,
 * ks_operator_format 0 / 0 / -1. */
int ks_operator_cg(ks_ctx* ctx, ks_operator* A, double shift, double tol, int maxit, int check_every /* 0: library default, 8 */,
                   ks_operator** out);
/* Counters of a conjugate-gradient operator (xiv; the inner solver of docs/src/index.md:234-259) since its creation: solves, iterations of all of them, iterations and the recurrence's
 * relative residual sqrt(rho' / rho0) of the last solve, and the largest such residual of any solve (failed ones included).
 * KS_ERR_ARGUMENT for any other operator. */
int ks_operator_cg_info(const ks_operator* op, int64_t* applications, int64_t* iterations, int* last_iterations, double* last_relres,
                        double* worst_relres);
/* (xv) MINRES solve:  y ~ (A - shift I)^-1 x  for a Hermitian A and any real shift that is not an eigenvalue -- inside the spectrum
 * too, where (xiv) stops at its first negative curvature: shift-invert (docs/src/index.md:234-259) for operators that have nothing
 * to factor.  A sibling of (xiv) at every layer: the same products, record protocol, chunked host loop and determinism, around a
 * three-term Lanczos recurrence and a running QR of its tridiagonal matrix:
 *     y = 0, beta1 = ||x||, v = x / beta1, v_ = w_ = w__ = 0, beta = 0, (c, s) = (c_, s_) = (1, 0), phibar = beta1
 *     q = (A - shift) v;  alpha = Re v^H q;  r = q - beta v_ - alpha v;  beta' = ||r||;
 *     (eps, delta, gamma, c', s', phi, phibar') = ks_host_minres_step(alpha, beta, beta', c, s, c_, s_, phibar, tol beta1);
 *     w = (v - eps w__ - delta w_) / gamma;  y += phi w;  done if |phibar'| <= tol beta1, else v_ <- v, v <- r / beta', ...
 * |phibar| is the residual norm of the recurrence; it never increases.  Beside the product an iteration is three kernels that move
 * 16 + 32 + 64 bytes per row in Float64; KS_C64 runs the same kernels on the real view.  A that is not Hermitian is NOT detected.
 * Arguments, refusals (KS_ERR_ARGUMENT) and check_every as for ks_operator_cg; A is BORROWED; choose tol at least 100 times tighter
 * than an outer eigensolver's tolerance.
 * KS_ERR_OPERATOR at apply time, the operator staying usable: "the right-hand side is not finite", "singular: gamma = ... at
 * iteration k" (gamma zero or not finite: the shift is an eigenvalue, or the product is not finite), "did not converge: relative
 * residual ... after maxit iterations". */
int ks_operator_minres(ks_ctx* ctx, ks_operator* A, double shift, double tol, int maxit, int check_every /* 0: library default, 8 */,
                       ks_operator** out);
/* Counters of a MINRES operator (xv) since its creation: solves, iterations of all of them, iterations and the recurrence's relative
 * residual |phibar| / beta1 of the last solve, and the largest such residual of any solve (failed ones included).  KS_ERR_ARGUMENT
 * for any other operator. */
int ks_operator_minres_info(const ks_operator* op, int64_t* applications, int64_t* iterations, int* last_iterations, double* last_relres,
                            double* worst_relres);
/* (xvi) BiCGStab(2) solve:  y ~ (A - shift I)^-1 x  for ANY operator A that can be enqueued ahead -- not Hermitian (a convection
 * term), or with a complex shift: shift-invert (docs/src/index.md:234-259) for general operators that have nothing to factor, where
 * (xiv) and (xv) need a Hermitian A.  KS_F64 with a real shift (shift_im must be 0), or KS_C64 with a complex one.  A sibling of
 * (xiv) and (xv) at every layer: the same products, record protocol, chunked host loop and determinism, around two BiCG steps and
 * a two-dimensional minimal-residual step per iteration (four products); <a, c> = a^H c, rt = x is read only:
 *     y = 0, r0 = x, u0 = 0, rho0 = 1, alpha = 0, omega = 1, beta1 = ||x||
 *     rho0 <- -omega rho0
 *     rho1 = <rt, r0>; beta = alpha rho1 / rho0; rho0 <- rho1; u0 <- r0 - beta u0; u1 = (A - shift) u0; gamma = <rt, u1>;
 *       alpha = rho0 / gamma; r0 -= alpha u1; y += alpha u0;                          done if ||r0|| <= tol beta1   (stage 1)
 *     r1 = (A - shift) r0; rho1 = <rt, r1>; beta = alpha rho1 / rho0; rho0 <- rho1; u0 <- r0 - beta u0; u1 <- r1 - beta u1;
 *       u2 = (A - shift) u1; gamma = <rt, u2>; alpha = rho0 / gamma; r0 -= alpha u1; r1 -= alpha u2; y += alpha u0;
 *                                                                                      done if ||r0|| <= tol beta1   (stage 2)
 *     r2 = (A - shift) r1; G = [<r1,r1> <r1,r2>; <r2,r1> <r2,r2>], h = [<r1,r0>; <r2,r0>], G g = h;
 *       y += g1 r0 + g2 r1; r0 -= g1 r1 + g2 r2; u0 -= g1 u1 + g2 u2; omega = g2;     done if ||r0|| <= tol beta1   (stage 3)
 * (ks_host_bicgstab_coef and ks_host_bicgstab_mr are the scalar steps).  Beside the products an iteration is nine streaming kernels
 * that move 352 bytes per row in Float64 (88 per product), templates on the scalar type: the scalars of KS_C64 are complex.
 * Arguments, refusals (KS_ERR_ARGUMENT) and check_every as for ks_operator_cg, and: an imaginary shift on a KS_F64 operator (build
 * the operator in KS_C64).  A is BORROWED; the operator owns six vectors.  No preconditioner; the residual is the recurrence's, which
 * drifts from the true one on hard shifts (deep inside a complex spectrum); choose tol at least 100 times tighter than an outer
 * eigensolver's tolerance.
 * KS_ERR_OPERATOR at apply time, the operator staying usable: "the right-hand side is not finite", "breakdown: rho | gamma | det G =
 * ... in stage s at iteration k" (zero or not finite: the shift is an eigenvalue, the shadow residual has lost the Krylov space, or
 * the product is not finite), "did not converge: relative residual ... after maxit iterations". */
int ks_operator_bicgstab(ks_ctx* ctx, ks_operator* A, double shift_re, double shift_im, double tol, int maxit,
                         int check_every /* 0: library default, 8 */, ks_operator** out);
/* Counters of a BiCGStab(2) operator (xvi) since its creation: solves, iterations of all of them (one iteration = four products; one
 * that ended in stage 1 or 2 counts), iterations and the recurrence's relative residual ||r0|| / beta1 of the last solve, and the
 * largest such residual of any solve (failed ones included).  KS_ERR_ARGUMENT for any other operator. */
int ks_operator_bicgstab_info(const ks_operator* op, int64_t* applications, int64_t* iterations, int* last_iterations, double* last_relres,
                              double* worst_relres);
/* (xvii) Preconditioned conjugate-gradient solve:  y ~ (A - shift I)^-1 x  for a Hermitian positive definite A - shift I, with a
 * Hermitian positive definite device operator M ~ (A - shift I)^-1 as preconditioner -- (xiv) for the operators it cannot reach: a
 * coefficient jump (M = the inverse diagonal, ks_operator_diagonal), an anisotropic grid (M = a line solve, (v)), incomplete factors
 * (ks_operator_lu).  A sibling of (xiv) at every layer: the same products, record protocol, chunked host loop and determinism:
 *     y = 0, r = x, rho0 = ||x||^2;  z = M r;  tau = Re r^H z;  p = z                 (rho0 == 0: y = 0, 0 iterations)
 *     q = (A - shift) p;  pq = Re p^H q;  alpha = tau / pq;  r -= alpha q;  rho' = ||r||^2;  y += alpha p;
 *     done if rho' <= tol^2 rho0  (the stopping test of (xiv): the 2-norm of the recurrence's residual, not its M-norm),
 *     else z = M r;  tau' = Re r^H z;  beta = tau' / tau;  p = z + beta p;  tau = tau'
 * with the scalar steps of ks_host_pcg_step.  Two paths, chosen at creation, that give the same bits:
 *   KS_PCG_PATH_GENERIC  M is any operator: beside the product and M's own launches an iteration is four kernels that move
 *                        16 + 24 + 16 + 40 bytes per row in Float64; the solver owns r, p, q and z.
 *   KS_PCG_PATH_JACOBI   M was made by ks_operator_diagonal: z = d o r is formed in registers, three kernels that move 16 + 32 + 48
 *                        bytes per row (96 against the 80 of (xiv)), no z vector.  KS_PCG_FUSED=0 forces the generic path.
 * KS_C64 runs the same kernels on the real view.  A and M are BORROWED.  M must be the SAME linear map in every iteration: a solve of
 * (xiv) - (xvii) as M would need flexible conjugate gradients and is refused.  A polynomial of A as M (ks_operator_chebyshev) works
 * but does not save products.  tol, maxit and check_every as for (xiv).
 * KS_ERR_ARGUMENT: what (xiv) refuses, and M null, made on another context, of another element type or size, or one that cannot be
 * enqueued ahead.
 * KS_ERR_OPERATOR at apply time, the operator staying usable: "the right-hand side is not finite", "not positive definite: p^H (A -
 * theta) p = ... at iteration k", "the preconditioner is not positive definite: r^H M r = ... at iteration k" (not finite or <= 0;
 * k = 0 is the start), "the residual is not finite at iteration k", "did not converge: relative residual ... after maxit iterations". */
enum { KS_PCG_PATH_GENERIC = 0, KS_PCG_PATH_JACOBI = 1 };
int ks_operator_pcg(ks_ctx* ctx, ks_operator* A, ks_operator* M, double shift, double tol, int maxit,
                    int check_every /* 0: library default, 8 */, ks_operator** out);
/* Counters of a preconditioned conjugate-gradient operator (xvii) since its creation: those of ks_operator_cg_info, the applications
 * of M (generic path: M's launches, those behind the end of a solve inside a chunk included; Jacobi path: the times d o r was formed,
 * one per solve and one per iteration) and the path, KS_PCG_PATH_*.  KS_ERR_ARGUMENT for any other operator. */
int ks_operator_pcg_info(const ks_operator* op, int64_t* applications, int64_t* iterations, int* last_iterations, double* last_relres,
                         double* worst_relres, int64_t* preconditioner_applications, int* path);
/* (xviii) Diagonal operator:  y = d o x  with n real, finite entries d (negative ones and zeros allowed) on KS_F64 or KS_C64 vectors:
 * a lumped mass matrix or its inverse, a scaling, the Jacobi preconditioner of (xvii).  One streaming kernel that moves 24 bytes per
 * row in Float64; it can be enqueued ahead and is usable wherever an operator is (products, ks_vectors_apply).  d is copied.  The
 * Newton and Clenshaw steps on it are its product and a streaming pass. */
int ks_operator_diagonal(ks_ctx* ctx, int64_t n, int dtype, const double* d, ks_operator** out);
/* (xix) Geometric multigrid V-cycle:  y = M x  with M ~ (A_0 - shift I)^-1, ONE symmetric V-cycle on a chain of grids -- a fixed linear
 * map, Hermitian positive definite by construction (below), that can be enqueued ahead: the preconditioner of (xvii) whose iteration
 * count does not grow in proportion to the grid extent (generic path, unchanged), and usable wherever an operator is.  KS_F64 or
 * KS_C64 vectors, real level data.  The cycle is generic in its level operators (any device operators that can be enqueued ahead,
 * BORROWED like a product's factors) and geometric in its transfers.  THE DEFINITION, rounding step by rounding step (fl = one
 * rounding to a double; the numpy model tests/mg_model.py implements the same, without the fused multiply-adds):
 *   LEVELS  l = 0 ... L = nsmooth,  dims[3 l ...] = (nx, ny, nz) of level l, x fastest, unused axes 1, row r = ix + nx (iy + ny iz).
 *     Per axis dims[l+1][a] is dims[l][a] (kept) or ceil(dims[l][a] / 2) (halved); at least one axis is halved per level.
 *   AGGREGATES  coarse cell I holds the fine cells 2 I and 2 I + 1 along each halved axis; with an odd extent the last coarse cell
 *     holds a single fine cell.
 *   PROLONGATION  P copies the coarse value to its aggregate:  x[i] = fl(x[i] + e[I(i)]).
 *   RESTRICTION  R = s P^T with s = 2^-(number of halved axes):  r_c[I] = s * sum fl(b[i] - t[i]) over the aggregate, the terms added
 *     to +0.0 one by one in ascending fine row order (x fastest, then y, then z); the product by s is exact.  b - t is formed inside the
 *     restriction kernel, t = (A_l - shift) x from the level operator's Newton step (shift == 0: its product).
 *   SMOOTHER on l < L:  k = degree steps of the Chebyshev iteration for B = D_l^-1 (A_l - shift) on [lambda_l / ratio, lambda_l], with
 *     dinv = inv_diag[l] (real, finite, positive) and lambda_l = lambda_max[l] an upper bound on the spectrum of B:
 *       lo = fl(lambda / ratio);  thc = fl(fl(lambda + lo) / 2);  del = fl(fl(lambda - lo) / 2);  sig = fl(thc / del);  rho_0 = fl(1 / sig);
 *       a_0 = 0,  b_0 = fl(1 / thc);   rho_j = fl(1 / fl(fl(2 sig) - rho_{j-1})),  a_j = fl(rho_j rho_{j-1}),  b_j = fl(fl(2 rho_j) / del);
 *       step 0:  d = fl(b_0 fl(dinv fl(rhs - t)));                   x = fl(x + d)
 *       step j:  d = fma(a_j, d, fl(b_j fl(dinv fl(rhs - t))));      x = fl(x + d)         with t = (A_l - shift) x before each step.
 *     PRE-smoothing starts from x = 0: its step 0 takes rhs for rhs - t and sets x = d, so it costs k - 1 products.  POST-smoothing takes
 *     k products and applies the same polynomial in B, which makes it the adjoint of the pre-smoother in the D-inner product: the cycle
 *     is symmetric.  The residual polynomial is below 1 in magnitude on (0, lambda_l]: with a true upper bound and a positive definite
 *     coarse operator the cycle is positive definite.
 *   LEVEL L  `coarse` is applied once:  x_L = coarse b_L.
 *   CYCLE  x = S(b);  r_c = R(b - (A - shift) x);  x += P cycle_{l+1}(r_c);  x = S(b, x):  2 k products per smoothed level.
 * Kernels (csrc/ks_mg.hpp), bytes per row in Float64: a smoother step reads rhs, t, dinv, d, x and writes d, x (56); the restriction
 * reads b and t and writes one coarse value per aggregate (16 + 1 in 3-D); the prolongation reads and writes x and loads one coarse
 * value for the two fine x-cells.  No device-side decision and no host read inside the cycle; in_scale and the DevState of a batch
 * are passed through to the level operators.  apply needs x != y.  nsmooth = 0 is allowed: M is then `coarse`.
 * KS_ERR_ARGUMENT (the message names the level and the entry): a context of several ranks; a null operator, one made on another
 * context, of another element type than `coarse`, or one that cannot be enqueued ahead; a size that is not the product of its level's
 * dims; a dims chain that breaks the rule above or a level of 2^31 rows or more; more than 16 levels; degree < 1; ratio <= 1 or not
 * finite; a lambda_max that is not finite or <= 0; an inv_diag entry that is not finite or <= 0; a shift that is not finite. */
int ks_operator_multigrid(ks_ctx* ctx, int nsmooth, ks_operator* const* A /* nsmooth */, const int64_t* dims /* 3 (nsmooth + 1) */,
                          const double* const* inv_diag /* nsmooth pointers to rows(l) values, copied */, const double* lambda_max /* nsmooth */,
                          ks_operator* coarse, double shift, int degree, double ratio, ks_operator** out);
/* Counters of a multigrid operator (xix): the number of levels nsmooth + 1, the rows of every level, the applications since creation
 * and, per level, the products with A_l since creation (2 degree per application; the entry of the last level counts the applications
 * of `coarse`).  rows and products have room for 16 entries.  Any output pointer may be NULL.  KS_ERR_ARGUMENT for any other operator. */
int ks_operator_multigrid_info(const ks_operator* op, int* levels, int64_t* rows, int64_t* applications, int64_t* products);
int ks_operator_destroy(ks_operator* op);
int ks_operator_size(const ks_operator* op, int64_t* n_local, int64_t* nnz, int* dtype);
/* Device layout chosen for a stored matrix at upload (mul!(y, A, x), src/expansion.jl:121; all layouts give bit-identical y):
 *   KS_LAYOUT_STENCIL  one BIT per dictionary slot and row: matrices whose (column - row, value) dictionary has <= 32 entries
 *                      and whose rows are sub-sequences of one ordering of them (constant-coefficient stencils with
 *                      truncated boundary rows); the dictionary travels in the kernel arguments
 *   KS_LAYOUT_DVI      one byte per non-zero into a <= 256-entry dictionary of (column - row, value) pairs (stencils)
 *   KS_LAYOUT_SELL     sliced ELLPACK, 64-row slices stored column-major (lane = row: coalesced loads and, for banded
 *                      matrices, coalesced gathers); taken when slicing pads the matrix by <= 15 % (uniform row lengths)
 *   KS_LAYOUT_CSR_CB   column-blocked CSR row blocks: matrices with scattered columns whose x does not fit one XCD's L2 (config 3)
 *                      are split into column blocks, one launch each, the row sums continued across the launches in CSR order
 *   KS_LAYOUT_CSR      row blocks of <= 256 rows / <= 4096 non-zeros streamed non-zero-parallel through LDS; a longer
 *                      row is a block of its own (ragged and skewed matrices)
 *   ..._VI             the same storage orders with ONE 32-bit word per non-zero (dictionary index << 24 | column):
 *                      matrices with <= 256 distinct stored values and < 2^24 columns
 * KS_SPMV_FORMAT = stencil | dvi | sell | sellvi | csr | vi pins one; KS_SELL_SIGMA sorts rows by length inside windows.
 * Non-zero offsets are 32-bit, 64-bit once nnz >= 2^31 (KS_SPMV_PTR64=1 forces them).
 * *bytes_per_nnz = what the SpMV streams per stored non-zero (padding included: 12 / 20 for plain CSR Float64 /
 * ComplexF64, 4 value-indexed, 1 delta-value-indexed), *ndict the dictionary size, *layout one of the codes below
 * (0 / 0 / -1 for dense and callback operators). */
enum { KS_LAYOUT_CSR = 0, KS_LAYOUT_CSR_VI = 1, KS_LAYOUT_DVI = 2, KS_LAYOUT_SELL = 3, KS_LAYOUT_SELL_VI = 4, KS_LAYOUT_STENCIL = 5, KS_LAYOUT_CSR_CB = 6 };
int ks_operator_format(const ks_operator* op, double* bytes_per_nnz, int* ndict, int* layout);
/* y = A*x on raw device pointers (bench / tests; the solver uses ks_apply below). */
int ks_operator_apply_raw(ks_operator* op, const void* x_dev, void* y_dev);

/* ---- workspace: ArnoldiWorkspace{T}(V, H, V_tmp, Q)  (src/ArnoldiMethod.jl:41-93) ------ */
/* V: n_local x (maxdim+1) in HBM (column-major, leading dimension padded, pad rows zero);
 * H: (maxdim+1) x maxdim on the host, zero-initialised (src/ArnoldiMethod.jl:66,76);
 * Q: maxdim x maxdim on the host.  V_tmp of the reference is not materialised: the restart
 * rotation runs in place (scratch is allocated only for shapes the in-place kernel does not
 * cover).  `n_global` is the order of A (== n_local on one GPU); `row_begin` this rank's
 * first global row (feeds the counter-based RNG so random vectors are partition-independent). */
int ks_workspace_create(ks_ctx* ctx, int64_t n_local, int64_t n_global, int64_t row_begin,
                        int maxdim, int dtype, ks_workspace** out);
int ks_workspace_destroy(ks_workspace* ws);
/* What the placement search of ks_workspace_create did: candidates timed (0: basis too small or
 * KS_PLACE_TRIALS=1, search skipped), the calibration time of the kept / the slowest candidate, and how many
 * allocations the device refused.  Round 6: ON by default (up to 10 candidates, ending with the first one in the fast cluster) for
 * a Float64 workspace of at least KS_PLACE_MIN_MB (1024) MB on one GPU that runs the block expansion -- the second pass of a large
 * block is 12 % faster on some allocations of the basis than on others (bimodal, decided by the physical pages; profiles/
 * r06_bupdate_lottery.txt); off otherwise (KS_PLACE_TRIALS >= 2 forces it).  The search holds its candidates while it runs: never
 * more than KS_PLACE_MAX_X (default 10) times the basis size at once, never more than half of the free device memory, at most
 * KS_PLACE_BUDGET_MS (1500) milliseconds; every loser is freed before ks_workspace_create returns. */
int ks_workspace_placement(const ks_workspace* ws, int* candidates, double* best_ms, double* worst_ms, int* refused);
/* How many times the fused expansion reads the basis per step on this workspace: 2 = implicit second pass (default:
 * the DGKS second projection, src/expansion.jl:93-94, is carried in a small triangular factor instead of being applied
 * to the n-vector), 3 = the second projection is applied to the vector as the reference does (KS_PASSES=3 at creation). */
int ks_workspace_passes(const ks_workspace* ws, int* passes);
/* Per-workspace switch for the above (instead of the KS_PASSES environment variable read at creation): passes = 2 or 3.
 * `max_ratio`: the largest ||c|| / beta (second-pass correction against what is left of the vector,
 * src/expansion.jl:93-96) the implicit form carries; a step whose correction is larger -- a genuine one, as opposed to
 * the rounding-level corrections the DGKS test asks for at every step of a diagonally dominant operator -- is redone
 * with the correction applied to the vector (counted in ks_expand_stats.explicit_steps / ks_history.explicit_steps).
 * Default 1e-3 (KS_IMPLICIT_MAX_RATIO at creation); <= 0 removes the limit; NaN keeps the current value. */
int ks_workspace_set_passes(ks_workspace* ws, int passes, double max_ratio);
/* S-STEP (block) EXPANSION -- a faster form of iterate_arnoldi!(A, arnoldi, from:to), src/expansion.jl:116-133, for
 * device-resident operators on one GPU.  s >= 2: the steps of a range are taken in blocks of up to s (instantiated sizes:
 * 1-20 for Float64, 1-10 for ComplexF64; beyond 5 on the FP64 matrix instruction, whose kernels take the block size at run
 * time -- ks_sstep_partition says how a range of steps is cut into blocks): s operator products build a Newton basis (shifts = Leja-ordered Ritz values
 * of the previous restart, so the first expansion of a run still goes step by step), then TWO passes over the basis
 * orthogonalise the whole block (block classical Gram-Schmidt with Pythagorean inner products, applied twice, both times
 * carried in the triangular factor of the implicit second pass) and the s Hessenberg columns follow from the basis
 * recurrence -- per block what the default expansion does per step.  Same Krylov space, hence the same H, V and Ritz values
 * up to rounding (H to ~1e-12 relative on the reference's test matrices, tests/test_sstep_model.py); the DGKS decisions of
 * src/expansion.jl:91 are not taken (the second projection is always applied).  A block whose Gram matrix has a Cholesky
 * pivot below pivot_min times its diagonal entry (breakdown, src/expansion.jl:99-102, or an ill-conditioned basis) is
 * abandoned before anything is committed and its steps are redone one at a time, which takes the reference's decisions.
 * Like the implicit second pass it needs the library's provenance of the factorisation; otherwise, and for host-callback
 * operators and maxdim > 64 the expansion runs step by step.  Default s = 20 (KS_SSTEP at creation; blocks of up to 20 on
 * up to 24 existing columns, up to 16 on up to 28, up to 12 on up to 48, up to 8 on up to 64; ComplexF64: up to 10 on up to 32 columns,
 * up to 8 on up to 48, single steps beyond); s = 0 / 1: off --
 * every step then takes the reference's DGKS decisions.  A block is also abandoned when the Gram matrix of what its first
 * stage wrote differs from I by more than
 * gram_dev_max in any entry (~ eps cond^2 of the Newton basis; the recovered H carries errors ~ eps cond): default 1e-8
 * keeps H at the per-step path's accuracy.  After an abandoned block the library lowers the block size for the following
 * expansions (s -> s/2 -> 2 -> off) and probes a larger one again after 16 clean batches: spectra the shifts cover badly
 * (a complex disc, with real shifts) simply run with small blocks.  pivot_min / gram_dev_max: NaN keeps the current value
 * (defaults 1e-6 / 1e-8; KS_SSTEP_PIVOT_MIN / KS_SSTEP_GDEV_MAX at creation).
 * ks_workspace_sstep_info: *s = block size in force; blocks completed / abandoned since creation; diag3 = of the last
 * batch { smallest pivot ratio of the first stage, of the second stage, largest |entry| of (Gram matrix of the written
 * block - I) }. */
int ks_workspace_set_sstep(ks_workspace* ws, int s, double pivot_min, double gram_dev_max);
int ks_workspace_sstep_info(const ks_workspace* ws, int* s, int* blocks, int* abandoned, double* diag3);
/* How iterate_arnoldi!(A, arnoldi, from:to) (src/expansion.jl:116-133) is cut into blocks: `count` steps on top of k0 existing
 * columns with block sizes <= smax, for dtype KS_F64 / KS_C64 -- the sizes the library itself would use (they depend on which
 * kernel forms KS_BLK_MFMA left on), for byte accounting in benchmarks.  Writes at most cap sizes to out and returns how many
 * blocks there are in *nblocks (0: the range cannot run in blocks).  The sizes may cover only a PREFIX of the range: where the
 * kernels stop (ComplexF64 beyond 48 columns) the remaining steps run one at a time. */
int ks_sstep_partition(int dtype, int k0, int count, int smax, int* out, int cap, int* nblocks);
/* Restarts of the library's drivers (ks_partialschur, ks_expand_restart, ks_restart) whose selection cut through a 2 x 2 block
 * of the real Schur form: the members of a complex pair are not neighbours in the target's order (imaginary-part targets on a
 * real matrix; src/run.jl:298-339 keeps pairs together only when they are), the truncation of src/run.jl:363-365 then drops the
 * block's sub-diagonal entry and the Arnoldi relation of the kept columns is off by that much from there on -- in the reference
 * as well.  The per-step expansion is indifferent to it; the s-step expansion (which leans on the relation of the earlier
 * columns) is switched off for the rest of the run when the dropped entry exceeds 1e-12 ||H||_F.  *breaks = such restarts
 * since creation, *worst_leak = largest dropped entry / ||H||_F.
 * Counted here as well: a relation that DRIFTS under the block expansion (a non-normal operator with a large cluster at the
 * wanted end: each block expresses A q_j through the relation of the earlier columns, and there an error of it grows from cycle
 * to cycle).  Block runs of the library's drivers measure the relation of the last kept column every first or second restart
 * cycle (one operator product + a row sample behind the speculative chain; ks_workspace_relation_probes counts them); above
 * max(1e-10, 30 tol) ||H||_F the blocks go off for the rest of the run. */
int ks_workspace_relation_info(const ks_workspace* ws, int* breaks, double* worst_leak);
/* A caller that runs the restart itself (the reference's _partialschur on a device basis, src/run.jl:298-365) and then vouches
 * for the result (ks_workspace_assert_arnoldi) is not seen by the guard above.  For such a factorisation the library MEASURES
 * the relation before blocks lean on it: the residual of the last kept column, A v_c - V H[:, c] (one operator product into a
 * dead column + a strided row sample), at the start of the ks_iterate_arnoldi that follows; more than 1e-11 ||H||_F (a measured residual carries the rounding of
 * the column's history, up to ~1e-12 behind large blocks; a cut block shows at 1e-9 .. 1e-5) counts as a
 * break exactly like a leaking restart of the library's own drivers (blocks off for the run).  *probes = measurements taken
 * since creation. */
int ks_workspace_relation_probes(const ks_workspace* ws, int* probes);
/* Restart rotations (src/run.jl:363-365) that ran fused with the first pass of the block expansion that followed them
 * (k_brotdots_mfma: the rotation of a library-run restart stays pending until the next expansion is enqueued; any other reader of
 * the basis flushes it through the ordinary rotation kernel first; KS_ROT_DEFER=0 at workspace creation switches the deferral
 * off), and what became of the speculative Newton chains (the first products of the next expansion, enqueued behind the previous
 * one so that the device works while the host runs the restart step, src/run.jl:278-360; KS_SPEC_CHAIN=0 switches them off):
 * *spec_adopted = chains the next expansion took over, *spec_dropped = chains that were void by then (the restart did not leave
 * its rotation pending, or something else touched the basis in between).  Any pointer may be null. */
int ks_workspace_fused_rotations(const ks_workspace* ws, int* count, int* spec_adopted, int* spec_dropped);
/* Memory: the fused rotation and the speculative chain keep the Newton chain of a block in scratch columns of their own -- 20
 * (Float64) / 10 (ComplexF64) columns of the workspace's leading dimension, allocated at the first restart that leaves its rotation
 * pending (1.6 GB at n = 1e7 next to a 3.3-GB basis of 41 columns); the drift watch keeps one more column, KS_TRUE_START=1 (off by
 * default) another one, the in-chain deflation 131 KB of partial sums.  When the device has no
 * room for them the library falls back to the paths that need none (rotation at once, no speculation, no watch) instead of failing:
 * a workspace that fits the device without these features runs with them switched off. */
/* Pending restart rotations (src/run.jl:363-365) for whose shape or element type there is no fused kernel (ComplexF64; Float64
 * shapes outside the instantiated ones): the ordinary rotation kernel runs when the next expansion is enqueued and BOTH passes of
 * its first block read the Newton chain from scratch columns -- what this buys is that the speculative chain (above) can run
 * behind the previous expansion for these shapes too.  *count = such rotations since creation. */
int ks_workspace_split_rotations(const ks_workspace* ws, int* count);
/* In-chain deflation of the block expansion (round 6).  The reference orthogonalises every new Krylov vector at once
 * (src/expansion.jl:69-109); a block of s steps does so only at its end.  Where LOCKED Schur vectors (src/run.jl:330) belong to
 * eigenvalues that dominate the rest of the spectrum (:LM problems with outliers: test/partial_schur.jl:122-138) the Newton chain in
 * between is projected against those columns step by step -- two small launches per product -- and no shift is placed at their
 * eigenvalues; without it such problems abandon their blocks and run step by step.  Taken: the leading locked columns whose
 * eigenvalue exceeds the largest other Ritz value by a factor r > KS_DEFLATE_RATIO (1.5) with r^(steps of the block - 1) > 1e3, at
 * most 16; several ranks all-reduce the dot products (one more small collective per product); KS_CHAIN_DEFLATE=0 at
 * workspace creation switches it off.  *blocks = blocks whose chain was deflated since creation, *columns = columns the last block
 * batch deflated against.  Any pointer may be null. */
int ks_workspace_deflated_blocks(const ks_workspace* ws, int* blocks, int* columns);
/* Diagnostics (tools/blk_bench.py): average duration of `reps` back-to-back launches of one streaming kernel of the s-step
 * expansion at basis size k and block size s (which = 0: first pass, 1: second pass), timed with HIP events on the
 * library's stream; *grid = workgroups launched.  dbg: probe flags of the kernels (1: second pass without its stores).
 * Overwrites columns k .. k+s-1 and drops the provenance of the factorisation. */
int ks_debug_blk_time(ks_workspace* ws, int k, int s, int which, int reps, int dbg, double* ms_per_launch, int* grid);
/* PROVENANCE.  The implicit second pass reads the columns < from of the host H and relies on the Arnoldi relation
 * A V[:, 0:from-1) = V[:, 0:from) H[0:from, 0:from-1) holding for them -- the reference's iterate_arnoldi! reads
 * neither.  The library therefore takes the implicit form only for a factorisation it produced itself: after
 * ks_reinitialize(ws, 0, ...) and any sequence of ks_iterate_arnoldi / ks_restart / ks_expand_restart, inside
 * ks_partialschur, and only while the host H still equals, bit for bit, what the library last left there.  Any verb
 * that writes to V (ks_col_upload, ks_col_div, ks_gemv_n_sub, ks_rotate, ks_col_copy, ks_apply, ks_orthogonalize,
 * ks_col_fill_uniform, handing out ks_workspace_col_ptr) or a changed / caller-built H makes ks_iterate_arnoldi run the
 * explicit three-pass form instead (same results as the reference's op sequence, never wrong, about 1.5x slower).
 * A host language that runs the restart itself (the reference's own `_partialschur` on a HipBasis: Schur step on its
 * own H, then ks_rotate + ks_col_copy, src/run.jl:278-365) vouches for the result with
 *     ks_workspace_assert_arnoldi(ws, k)   -- "columns 0..k are orthonormal and, with the H now in ks_workspace_H,
 *                                              satisfy the Arnoldi relation of k steps"
 * k = -1 WITHDRAWS whatever the library trusted (a binding that saw the caller write into V through a path the library
 * does not watch).  *k of ks_workspace_provenance: steps the library trusts (-1: none). */
int ks_workspace_assert_arnoldi(ks_workspace* ws, int k);
int ks_workspace_provenance(const ks_workspace* ws, int* k);
/* Debugging aid: with KS_GUARD=1 in the environment a workspace puts 1 MiB canary zones on both sides of the
 * basis; *intact = 0 if any kernel wrote outside V (always 1 without KS_GUARD). */
int ks_workspace_check_guard(ks_workspace* ws, int* intact);
int ks_workspace_dims(const ks_workspace* ws, int64_t* n_local, int* maxdim, int* dtype, int64_t* ldv);
/* Host arrays (valid until the workspace is destroyed); ldh = maxdim+1, ldq = maxdim. */
int ks_workspace_H(ks_workspace* ws, void** H, int* ldh);
int ks_workspace_Q(ks_workspace* ws, void** Q, int* ldq);
/* Device pointer of column j of V (for device-side consumers; PartialSchur.Q is a view of V,
 * src/run.jl:375,389).  The pointer may be written through: handing it out ends the library's provenance (above). */
int ks_workspace_col_ptr(ks_workspace* ws, int j, void** dev_ptr);
int ks_workspace_set_seed(ks_workspace* ws, uint64_t seed);

/* ---- the verbs the reference applies to V (array-type seam) ------ */
/* copyto!(view(V,:,j+1), v1)   src/run.jl:126   (n_local elements from host) */
int ks_col_upload(ks_workspace* ws, int j, const void* host);
/* Array(view(V,:,j+1))   (result views, src/run.jl:375,389; eigvals.jl:94) */
int ks_col_download(ks_workspace* ws, int j, void* host);
/* V[:, j0:j0+ncols) -> host matrix with leading dimension ldhost */
int ks_cols_download(ks_workspace* ws, int j0, int ncols, void* host, int64_t ldhost);
int ks_cols_upload(ks_workspace* ws, int j0, int ncols, const void* host, int64_t ldhost);
/* rand!(view(V,:,j+1))   src/expansion.jl:15,21  -- counter-based uniform [0,1) */
int ks_col_fill_uniform(ks_workspace* ws, int j, uint64_t seed);
/* norm(view(V,:,j+1))   src/expansion.jl:24,41,48,81,88,96  (global 2-norm) */
int ks_col_norm(ks_workspace* ws, int j, double* out);
/* v ./= s   src/expansion.jl:28,56,106 */
int ks_col_div(ks_workspace* ws, int j, double s);
/* copyto!(view(V,:,dst+1), view(V,:,src+1))   src/run.jl:365 */
int ks_col_copy(ks_workspace* ws, int dst, int src);
/* mul!(view(V,:,jdst+1), A, view(V,:,jsrc+1))   src/expansion.jl:121 */
int ks_apply(ks_operator* A, ks_workspace* ws, int jsrc, int jdst);
/* Diagnostics (tests/test_gpu_shifted_product.py): one Newton step of the s-step expansion,
 *     view(V,:,jdst+1) = sigma (A view(V,:,jsrc+1) - theta view(V,:,jsrc+1)),
 * the shifted form of mul! at src/expansion.jl:121, through the very call the expansion makes inside a block (fused into the
 * product's store by every stored-matrix layout, the product and one streaming pass for every other operator).  theta =
 * (theta_re, theta_im), theta_im must be 0 for KS_F64; cacheable_store != 0 takes the cacheable store of the fused kernels
 * (what blocks of ten and more steps use), 0 the streaming one.  Drops the provenance of the factorisation like ks_apply. */
int ks_debug_apply_shifted(ks_operator* A, ks_workspace* ws, int jsrc, int jdst, double theta_re, double theta_im, double sigma,
                           int cacheable_store);
/* Diagnostics (tests/test_gpu_chebyshev.py): one Clenshaw step of a Chebyshev filter (xiii),
 *     view(V,:,jdst+1) = sigma (A view(V,:,jsrc+1) - theta view(V,:,jsrc+1)) - view(V,:,jw+1) + gamma view(V,:,jx0+1),
 * through the very call the filter makes per step.  jw = -1 / jx0 = -1: no such term; jdst differs from jsrc, jw and jx0.
 * theta and cacheable_store as for ks_debug_apply_shifted.  Drops the provenance of the factorisation like ks_apply. */
int ks_debug_apply_clenshaw(ks_operator* A, ks_workspace* ws, int jsrc, int jdst, int jw, int jx0, double theta_re, double theta_im,
                            double sigma, double gamma, int cacheable_store);
/* mul!(h, view(V,:,1:j)', view(V,:,jv+1))   src/expansion.jl:37,46,84,93   (h: j host values) */
int ks_gemv_t(ks_workspace* ws, int j, int jv, void* h_host);
/* mul!(view(V,:,jv+1), view(V,:,1:j), h, -1, 1)   src/expansion.jl:38,47,85,94 */
int ks_gemv_n_sub(ks_workspace* ws, int j, int jv, const void* h_host);
/* V[:, c0:c0+r) <- V[:, c0:c0+c) * Q[0:c, 0:r)  with Q a HOST matrix, leading dimension ldq
 * (mul! into V_tmp + copyto! back, src/run.jl:363-364 and :382-383, done in place). */
int ks_rotate(ks_workspace* ws, int c0, int c, int r, const void* Q_host, int ldq);
/* out(n_local x r, host or device scratch) = V[:, 0:c) * Y[0:c, 0:r), Y complex or real host
 * matrix: the tall-skinny product of partialeigen (P.Q * vecs, src/eigvals.jl:94).  Output is
 * written to host memory `out_host` with leading dimension ldout, dtype `ydtype`. */
int ks_basis_times(ks_workspace* ws, int c, int r, const void* Y_host, int ldy, int ydtype,
                   void* out_host, int64_t ldout);

/* ---- fused hot path ---------------------------------------------------------------------- */
/* orthogonalize!(arnoldi, j)   src/expansion.jl:69-109
 * DGKS classical Gram-Schmidt of column j against columns 0..j-1 with all decisions taken on
 * globally reduced norms; writes H[0:j, j-1] and H[j, j-1] into the workspace's host H.
 * *ok = 0 on breakdown (reference returns false). */
int ks_orthogonalize(ks_workspace* ws, int j, int* ok);
/* reinitialize!(arnoldi, j, populate!)   src/expansion.jl:12-59
 * v1_host == NULL -> rand!; otherwise copyto!(v, v1).  Does not touch H. */
int ks_reinitialize(ks_workspace* ws, int j, const void* v1_host, int* ok);
/* iterate_arnoldi!(A, arnoldi, from:to)   src/expansion.jl:116-133  (from/to as in the
 * reference: step j builds 0-based column j from column j-1).  The whole range is enqueued
 * asynchronously (operator apply + fused DGKS per step, decisions on-device) and the host
 * synchronises once at the end to fetch the new columns of H.  Like the reference it needs nothing from columns < from
 * of H: the implicit second pass (ks_workspace_passes == 2), which does read them, is only taken while the library's
 * provenance of the factorisation is intact (see ks_workspace_assert_arnoldi); otherwise the explicit form runs.
 * `reorth`: the DGKS test of the implicit form is taken against max(||A v||, ||y'|| / beta) (the norm of the vector the
 * projection was really applied to; equal to the reference's rnorm, src/expansion.jl:81, unless the previous column
 * carries a correction): it can ask for the second pass where the reference would not, never the other way round. */
typedef struct ks_expand_stats {
  int32_t steps;          /* operator applications performed                                    */
  int32_t reorth;         /* steps whose DGKS test requested the second pass (src/expansion.jl:91) */
  int32_t breakdowns;     /* steps that ended in reinitialize! (src/expansion.jl:127-129)        */
  int32_t explicit_steps; /* steps the implicit second pass handed back to the explicit form (ks_workspace_set_passes) */
} ks_expand_stats;
int ks_iterate_arnoldi(ks_operator* A, ks_workspace* ws, int from, int to, ks_expand_stats* stats);

/* ---- driver:  partialschur / partialschur!   (src/run.jl:100-179, _partialschur :224-392) - */
typedef struct ks_params {
  int32_t nev;        /* default min(6, n)                       src/run.jl:103 */
  int32_t which;      /* KS_LM ...                               src/run.jl:104 */
  double tol;         /* default sqrt(eps)                       src/run.jl:105 */
  int32_t mindim;     /* default min(max(10, nev), n)            src/run.jl:106 */
  int32_t maxdim;     /* default min(max(20, 2nev), n)           src/run.jl:107 */
  int32_t restarts;   /* default 200                             src/run.jl:108 */
  int32_t start_from; /* 1-based as in partialschur!; 1 = fresh  src/run.jl:155 */
  int32_t initialize; /* 1: reinitialize!(arnoldi, start_from-1) src/run.jl:156,177 */
  int32_t reserved;
} ks_params;
typedef struct ks_history { /* src/run.jl:217-222 (+ diagnostics) */
  int32_t mvproducts;
  int32_t nconverged;
  int32_t converged;
  int32_t nev;
  int32_t restarts;   /* outer iterations performed */
  int32_t reorth;     /* DGKS second passes taken   */
  int32_t breakdowns;
  int32_t explicit_steps; /* steps redone with the explicit second pass (ks_workspace_set_passes) */
  double seconds_expand; /* wall time spent waiting for the device in iterate_arnoldi  */
  double seconds_host;   /* wall time in the host Schur / reorder / restore            */
  double seconds_rotate; /* wall time enqueueing+waiting for rotations (mostly async)  */
} ks_history;
/* Fill `p` with the reference defaults for an order-n problem (src/run.jl:103-108). */
int ks_params_default(int64_t n, ks_params* p);
/* partialschur!(A, arnoldi; ...) on a caller-owned workspace.  `v1_host` (may be NULL) is the
 * start vector of partialschur(A; v1) (src/run.jl:122-127), used only when initialize != 0 and
 * start_from == 1.  On return: V[:, 0:nconverged) = Schur vectors, H[0:nconv,0:nconv) = R,
 * eigenvalues[0:nconv) (interleaved complex doubles, src/run.jl:386-389). */
int ks_partialschur(ks_operator* A, ks_workspace* ws, const ks_params* p, const void* v1_host,
                    double* eigenvalues_c64, ks_history* history);

/* One Krylov-Schur restart on the workspace: Schur form of the active block of H, Ritz values and
 * residual estimates, lock/retain/purge grouping, three-way partition, restore_arnoldi! (all on the
 * host, src/run.jl:278-360), then the change of basis V[:, purge:k) <- V[:, purge:maxdim) Q[...] and
 * V[:, k] <- V[:, maxdim] on the device (src/run.jl:363-365).  `active` is 0-based (first non-locked
 * column).  With ks_iterate_arnoldi this lets a host language run `_partialschur`'s loop itself:
 *     ks_iterate_arnoldi(A, ws, k+1, maxdim) ; ks_restart(ws, p, active, &k, &nlock, ...) ; active = nlock
 * Out (optional): eigenvalues / residual estimates / groups of this restart (maxdim entries each). */
int ks_restart(ks_workspace* ws, const ks_params* p, int active, int* k, int* nlock, int* purge,
               double* lams_c64, double* rs, int32_t* groups);

/* One whole cycle of `_partialschur`'s loop (src/run.jl:272-365) in one call: the expansion k_in+1 .. maxdim followed by
 * the restart -- what ks_partialschur does internally.  With the explicit second pass (ks_workspace_passes == 3) the part
 * of the restart's host work that does not need H[maxdim+1, maxdim] (Schur form, Ritz values, unit residuals, ordering:
 * src/run.jl:278-289) runs on the host WHILE the device finishes the last expansion step; with the implicit second pass
 * (default) H is final only when the batch ends and the host step follows it.  Results are bit-identical to
 * ks_iterate_arnoldi + ks_restart either way.  `k_in` is the
 * basis size the previous restart left (mindim after the initial expansion).  seconds[3] (optional): wall time of the
 * expansion (including whatever of the early host part the device did not hide), of the remaining host part, of
 * enqueueing the rotation. */
int ks_expand_restart(ks_operator* A, ks_workspace* ws, const ks_params* p, int active, int k_in, int* k, int* nlock,
                      int* purge, double* eigenvalues_c64, double* residuals, int32_t* groups, ks_expand_stats* stats,
                      double* seconds);

/* Per-kernel-class timing with HIP events on the context's stream (bench.py's roofline figures).
 * Classes: 0 SpMV, 1 dots (V'w), 2 axpy (w -= Vh), 3 scale, 4 rotation, 5 reductions/decisions,
 * 6 fused axpy+dots (first projection + second-pass inner products).
 * `bytes` are ALGORITHMIC bytes accumulated per launch. */
int ks_profile_enable(ks_ctx* ctx, int on);
int ks_profile_reset(ks_ctx* ctx);
int ks_profile_get(ks_ctx* ctx, int nclass, double* ms, double* bytes, int64_t* counts);

/* Residual checks evaluated on the device: ||A*Q - Q*R||_F and ||Q'Q - I||_F for the first
 * `ncols` columns with R = H[0:ncols, 0:ncols) (test/partial_schur.jl:24-25,104-105). */
int ks_residual_norms(ks_operator* A, ks_workspace* ws, int ncols, double* resid, double* orth);
/* Arnoldi relation check ||A V_k - V_{k+1} H_k||_F and ||V'V - I||_F (test/expansion.jl:24-31). */
int ks_arnoldi_relation(ks_operator* A, ks_workspace* ws, int k, double* resid, double* orth);

/* ---- device-resident vectors ---------------------------------------------------------------
 * n_local x ncols vectors in HBM that operators are applied to and whose residuals and Gram matrices come back as a few small
 * numbers: the last two steps of the reference's recipes -- "translate back to the original problem" (Q = L^-* Y,
 * docs/src/index.md:347) and the checks A x = x lambda, A x = B x lambda, Q* A Q = R, Q* B Q = I against the ORIGINAL matrices
 * (docs/src/index.md:258, 302, 350-351) -- without a copy of the vectors to the host.  Column-major, leading dimension `ld` a
 * multiple of 64 elements, zero-filled once; every call writes rows < n_local only, so the pad rows stay zero (the stored-matrix
 * kernels may read the pad rows of their input).  1 <= ncols <= 64; single-GPU contexts only; n_local = 0 is legal and every
 * call on such vectors is a no-op.  Every call that touches device memory synchronises the context's stream before it returns. */
typedef struct ks_vectors ks_vectors;
int ks_vectors_create(ks_ctx* ctx, int64_t n_local, int ncols, int dtype, ks_vectors** out);
int ks_vectors_destroy(ks_vectors* v);
int ks_vectors_dims(const ks_vectors* v, int64_t* n_local, int* ncols, int* dtype, int64_t* ld);
/* columns j0 .. j0+ncols-1 from / to a host matrix, column-major with leading dimension ldhost >= n_local */
int ks_vectors_upload(ks_vectors* v, int j0, int ncols, const void* host, int64_t ldhost);
int ks_vectors_download(const ks_vectors* v, int j0, int ncols, void* host, int64_t ldhost);
int ks_vectors_col_ptr(ks_vectors* v, int j, void** dev_ptr);
/* ks_basis_times with the result left on the device: out[:, 0:r) = V[:, 0:c) * Y[0:c, 0:r).  `out` has n_local of the workspace,
 * at least r columns and the element type `ydtype` (a real basis times complex coefficients gives complex vectors). */
int ks_basis_times_device(ks_workspace* ws, int c, int r, const void* Y_host, int ldy, int ydtype, ks_vectors* out);
/* out[:, i] = op in[:, i] for every column, any operator kind (callbacks and products included); out != in, same shape, element
 * type and context (KS_ERR_ARGUMENT otherwise).  An error of the operator (a callback returning non-zero) comes out unchanged.
 * A Float64 operator on ComplexF64 vectors -- a real problem with complex-conjugate Ritz pairs -- is applied to the real and to the
 * imaginary part, each bit-identical to the operator applied to that part alone; a ComplexF64 operator on Float64 vectors is
 * KS_ERR_ARGUMENT. */
int ks_vectors_apply(ks_operator* op, const ks_vectors* in, ks_vectors* out);
/* resid[i] = || AX[:, i] - sum_j BX[:, j] C[j, i] ||_2 and bnorm[i] = || BX[:, i] ||_2, i < r = ncols, in ONE sweep over AX and BX
 * (r r sizeof(element) <= 48 KiB and r <= 56 / 40 columns for Float64 / ComplexF64; wider blocks sweep BX once per chunk of
 * columns).  C is r x r in the vectors' element type, host, column-major ldc: diagonal for the eigenpair check A x - lambda B x,
 * R for the Schur check A Q - B Q R.  BX may be AX's own object.  Deterministic: the same bits every time; the square roots are
 * taken on the host. */
int ks_vectors_residuals(const ks_vectors* AX, const ks_vectors* BX, const void* C_host, int ldc, double* resid, double* bnorm);
/* G = X^H Y (ncols(X) x ncols(Y), host, column-major ldg): Q* B Q - I and Q* A Q - R.  One download, one synchronisation. */
int ks_vectors_gram(const ks_vectors* X, const ks_vectors* Y, void* G_host, int ldg);

/* ---- host small dense kernels, exported for the host-logic tests (no device needed) ------ */
/* local_schurfact!(H, start, to, Q)   src/schurfact.jl:393-538; H is m x n column-major. */
int ks_host_schurfact(int dtype, void* H, int m, int n, int ldh, int start, int to, void* Q, int nq,
                      int ldq);
/* One complete restart's worth of host work on (H (maxdim+1 x maxdim), Q): Schur form of the
 * active block, Ritz values/residuals, grouping, 3-way partition, restore_arnoldi!
 * (src/run.jl:278-360).  In/out: active (0-based).  Out: k, nlock, purge, eigenvalues, residuals,
 * groups. */
int ks_host_restart_step(int dtype, void* H, int ldh, void* Q, int ldq, int maxdim, int mindim,
                         int nev, int which, double tol, int active, int* k, int* nlock, int* purge,
                         double* lams_c64, double* rs, int32_t* groups);
/* Which device layout ks_operator_csr (nghost < 0: a whole matrix on one GPU) or ks_operator_csr_dist (nghost >= 0: a row
 * block with local-extended columns, ncols = nrows_local + nghost, the first nlow ghost slots owned by lower ranks; nlow < 0:
 * neighbours not in ascending order) would give this matrix under the current KS_SPMV_* environment, planned on the host:
 * no device is touched.  `num_cu`: compute units of the device the plan is for (256 on an MI355X).  Out (each may be NULL):
 * what ks_operator_format reports, aux_bytes (index structures streamed next to the non-zeros), facts[KS_PLAN_NFACTS]
 * indexed by KS_PLAN_*, the stencil dictionary's column offsets in slot order (up to 32), the row blocks (nblk + 1 entries
 * each, at most blk_cap) and the column-block boundaries in key space (blocks + 1 entries, at most cb_cap). */
enum { KS_PLAN_PTR64 = 0, KS_PLAN_NI, KS_PLAN_NBLK, KS_PLAN_NLONG, KS_PLAN_ROW_GATHER, KS_PLAN_NSLICES, KS_PLAN_SELL_ENTRIES,
       KS_PLAN_NCOLBLOCKS, KS_PLAN_CB_RPT, KS_PLAN_CB_NI, KS_PLAN_NSTENCIL, KS_PLAN_NSTENCIL_LOCAL, KS_PLAN_STENCIL_MASK_BYTES,
       KS_PLAN_NDVI, KS_PLAN_DVI_UNROLL, KS_PLAN_NFACTS };
int ks_host_csr_plan(int64_t nrows_local, int64_t ncols, int64_t nnz, const void* ptr, const void* idx,
                     const void* val, int layout, int index_base, int index_type, int dtype, int num_cu,
                     int64_t nghost, int64_t nlow, int* plan_layout, int* ndict, double* bytes_per_nnz,
                     double* aux_bytes, int64_t* facts, int32_t* stencil_delta, int64_t* blkrow, int64_t* blkptr,
                     int64_t blk_cap, int64_t* cb_bounds, int cb_cap);
/* The halo plan ks_operator_csr_dist would upload for these arguments (the same ones, minus context, values and handle) on rank
 * `rank` with elements of `elem_size` bytes (8: Float64, 16: ComplexF64), planned on the host: no device is touched, and every
 * argument check of ks_operator_csr_dist that does not need its context fails here with the same code and message.  Out (each may
 * be NULL): facts[KS_HALO_NFACTS] indexed by KS_HALO_* -- NLOW: ghost slots owned by lower ranks (-1: a lower-ranked neighbour
 * is listed after one that is not lower); [GHOST_LO_END, GHOST_HI_BEGIN): the longest run of rows without a ghost column;
 * NSCATTER: entries that go through the pack kernel --, recv_ptr and pack_ptr (nneigh + 1 entries each), send_first (nneigh
 * entries; >= 0: the neighbour's send list is this consecutive run and goes out in place), the packed lists (NSCATTER entries, at
 * most packed_cap are written) and p2p_ghost[2] = {elements between the two ghost slots of the peer-to-peer transport, bytes of
 * the shared arena they take}; asking for p2p_ghost also applies that transport's limit of 16 neighbours. */
enum { KS_HALO_NLOW = 0, KS_HALO_GHOST_LO_END, KS_HALO_GHOST_HI_BEGIN, KS_HALO_NSCATTER, KS_HALO_NFACTS };
int ks_host_halo_plan(int64_t nrows_local, int64_t nghost, int64_t nnz, const int64_t* rowptr, const int32_t* colidx,
                      int nneigh, const int32_t* neigh, const int64_t* send_ptr, const int32_t* send_idx,
                      const int64_t* recv_cnt, int rank, int elem_size, int64_t* facts, int64_t* recv_ptr,
                      int64_t* send_first, int64_t* pack_ptr, int32_t* packed, int64_t packed_cap, int64_t* p2p_ghost);
/* The matrix that DEFINES ks_operator_grid (mul!(y, A, x), src/expansion.jl:121), as 0-based CSR with ascending columns, without
 * a device: rowptr n + 1 entries, colidx / val `cap` entries.  *nnz (may be NULL) receives the number of stored entries -- the
 * in-grid taps, n + 2 ((nx-1) ny nz + nx (ny-1) nz + nx ny (nz-1)) -- also when the call fails because cap is smaller than that
 * (KS_ERR_ARGUMENT; nothing else is written then).  Same refusals as the operator, except that no context is involved. */
int ks_host_grid_matrix(int ndim, const int64_t* dims, int dtype, const void* taps, const void* potential,
                        int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_periodic (mul!(y, A, x), src/expansion.jl:121): `periodic` and `wrap` as there,
 * every row a sub-sequence of its 13 slots, *nnz = n (1 + 2 #periodic axes) + 2 sum over the open axes a of (m_a - 1) n / m_a.  With
 * no periodic axis the arrays are those of ks_host_grid_matrix.  Same refusals as that operator, except that no context is involved. */
int ks_host_grid_matrix_periodic(int ndim, const int64_t* dims, int dtype, const void* taps, const void* potential,
                                 const int* periodic /* ndim flags, or NULL */, const void* wrap /* 2*ndim values, or NULL */,
                                 int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_star (mul!(y, A, x), src/expansion.jl:121): `radius` and the 2 ndim radius + 1
 * `taps` as there, every row a sub-sequence of its 6 radius + 1 slots, *nnz = n + sum over the axes a and d = 1...radius of
 * 2 max(m_a - d, 0) n / m_a.  With radius == 1 the arrays are those of ks_host_grid_matrix.  Same refusals as that operator, except
 * that no context is involved. */
int ks_host_grid_matrix_star(int ndim, const int64_t* dims, int radius, int dtype, const void* taps, const void* potential,
                             int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_star_periodic (mul!(y, A, x), src/expansion.jl:121): `radius`, `taps`, `periodic`
 * and the 2 ndim radius `wrap` values as there, every row in the order of (x-b), *nnz = n + sum over the axes a of
 * (periodic ? 2 radius n : sum over d = 1...radius of 2 max(m_a - d, 0) n / m_a) (also reported when cap is too small).  With no
 * periodic axis the arrays are those of ks_host_grid_matrix_star, with radius == 1 those of ks_host_grid_matrix_periodic.  Same
 * refusals as that operator, except that no context is involved. */
int ks_host_grid_matrix_star_periodic(int ndim, const int64_t* dims, int radius, int dtype, const void* taps, const void* potential,
                                      const int* periodic /* ndim flags, or NULL */, const void* wrap /* 2*ndim*radius values, or NULL */,
                                      int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_var (mul!(y, A, x), src/expansion.jl:121): `coeff` as there, the off-diagonal entries
 * fl(0.5 t_k * fl(c[r] + c[s])), every row a sub-sequence of the 7 slots, *nnz as for ks_host_grid_matrix (also reported when cap is
 * too small).  With c == 1 the arrays are those of ks_host_grid_matrix.  Same refusals as that operator, except that no context is
 * involved. */
int ks_host_grid_var_matrix(int ndim, const int64_t* dims, int dtype, const void* taps, const double* coeff, const void* potential,
                            int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_var_periodic (mul!(y, A, x), src/expansion.jl:121): `coeff`, `periodic` and `wrap` as
 * there; an interior link carries fl(0.5 t_k * fl(c[r] + c[s])), a link that crosses the boundary of a periodic axis
 * fl(0.5 wrap_k * fl(c[r] + c[s])) with s the wrap image; every row a sub-sequence of the 13 slots of (ix), *nnz as for
 * ks_host_grid_matrix_periodic (also reported when cap is too small).  With no periodic axis the arrays are those of
 * ks_host_grid_var_matrix, with c == 1 those of ks_host_grid_matrix_periodic.  Same refusals as that operator, except that no context is
 * involved. */
int ks_host_grid_var_matrix_periodic(int ndim, const int64_t* dims, int dtype, const void* taps, const double* coeff,
                                     const void* potential, const int* periodic /* ndim flags, or NULL */,
                                     const void* wrap /* 2*ndim values, or NULL */, int64_t* rowptr /* n+1 */, int32_t* colidx,
                                     void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_box (mul!(y, A, x), src/expansion.jl:121): `taps` holds 3^ndim values, every row is a
 * sub-sequence of the 27 slots (ascending columns), an entry is stored even where its tap is zero, *nnz = prod_a (3 m_a - 2) (also
 * reported when cap is too small).  In 1-D the arrays are those of ks_host_grid_matrix.  Same refusals as that operator, except that no
 * context is involved. */
int ks_host_grid_box_matrix(int ndim, const int64_t* dims, int dtype, const void* taps, const void* potential,
                            int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* ... and the matrix that DEFINES ks_operator_grid_box_periodic (mul!(y, A, x), src/expansion.jl:121): `periodic` and `links` as there,
 * every row in the order of (xii-b), *nnz = prod_a (periodic_a ? 3 m_a : 3 m_a - 2) (also reported when cap is too small).  With no
 * periodic axis the arrays are those of ks_host_grid_box_matrix, in 1-D those of ks_host_grid_matrix_periodic with
 * wrap = [links[0], links[4]].  Same refusals as that operator, except that no context is involved. */
int ks_host_grid_box_matrix_periodic(int ndim, const int64_t* dims, int dtype, const void* taps, const void* potential,
                                     const int* periodic /* ndim flags, or NULL */, const void* links /* 5^ndim values, or NULL */,
                                     int64_t* rowptr /* n+1 */, int32_t* colidx, void* val, int64_t cap, int64_t* nnz);
/* The schedule of ks_operator_chebyshev (xiii) without a device: Clenshaw's recurrence as `degree` steps
 *     out = sigma (A in - center in) - w + gamma x0.
 * With h = fl(2 / halfwidth), h1 = fl(1 / halfwidth), g = coeffs, m = degree:
 *     m = 1:   (in x0, sigma fl(g[1] h1), no w, gamma g[0], out y);
 *     step 1:  (in x0, sigma fl(g[m] h), no w, gamma g[m-1], out b_{m-1});
 *     step 2 (k = m - 2):  (in b_{m-1}, sigma h (k = 0: h1), no w, gamma fl(g[m-2] - g[m]), out b_{m-2} (k = 0: y));
 *     step s >= 3 (k = m - s):  (in b_{k+1}, sigma h (k = 0: h1), w b_{k+2}, gamma g[k], out b_k (k = 0: y)).
 * Slots: -1 = x0 as `in`, y as `out`; -2 = none; 0 ... 2 = the filter's intermediate vectors, b_k in (m - 1 - k) mod 3, so out is
 * never in, w or x0.  *temporaries = min(m - 1, 3).  Refusals as for the operator (KS_ERR_ARGUMENT). */
typedef struct ks_cheb_step {
  int32_t in, out, w, reserved;
  double sigma, gamma;
} ks_cheb_step;
int ks_host_chebyshev_plan(int degree, double center, double halfwidth, const double* coeffs /* degree + 1 */,
                           ks_cheb_step* steps /* degree */, int* temporaries);
/* The scalar step of ks_operator_cg (xiv) without a device (docs/src/index.md:234-259: the inner solver of the shift-invert recipe) --
 * the function its kernels run, compiled for the host: from rho = ||r||^2, pq = Re p^H (A - theta) p, rho_new = ||r - alpha q||^2 and
 * stop = tol^2 rho0
 *     fail   pq not finite, pq <= 0, rho / pq not finite, or rho_new not finite: alpha = beta = 0, done = 0;
 *     alpha  rho / pq;     done  rho_new <= stop (rho_new == 0 is done for every stop >= 0, without a division);
 *     beta   rho_new / rho, 0 when done.
 * Any output pointer may be NULL. */
int ks_host_cg_step(double rho, double pq, double rho_new, double stop, double* alpha, double* beta, int* done, int* fail);
/* The scalar steps of ks_operator_pcg (xvii) without a device -- the functions its kernels run, compiled for the host: from
 * tau = Re r^H M r, pq = Re p^H (A - theta) p, rho_new = ||r - alpha q||^2, stop = tol^2 rho0 and tau_new = Re r^H M r after the step
 *     fail 2  pq not finite, pq <= 0, or tau / pq not finite;   fail 4  rho_new not finite:   alpha = beta = 0, done = 0;
 *     alpha   tau / pq;     done  rho_new <= stop (rho_new == 0 is done for every stop >= 0; tau_new is then not looked at);
 *     fail 3  not done and tau_new not finite, tau_new <= 0, or tau_new / tau not finite:   beta = 0 (alpha stands);
 *     beta    tau_new / tau, 0 when done.
 * (fail 1, the right-hand side is not finite, belongs to the start of a solve.)  Any output pointer may be NULL. */
int ks_host_pcg_step(double tau, double pq, double rho_new, double stop, double tau_new, double* alpha, double* beta, int* done, int* fail);
/* The host plan of ks_operator_multigrid (xix) without a device: the dims chain validated with that operator's refusals (inv_diag may
 * be NULL, and so may any of its pointers: those entries are then not looked at), the rows of every level (nsmooth + 1), and per
 * smoothed level the restriction scale s and the smoother's coefficients a[l degree + j], b[l degree + j] of step j as (xix) defines
 * them.  Any output pointer may be NULL. */
int ks_host_multigrid_plan(int nsmooth, const int64_t* dims /* 3 (nsmooth + 1) */, const double* const* inv_diag, const double* lambda_max,
                           int degree, double ratio, double* a, double* b, double* scale, int64_t* rows);
/* The reference transfers of (xix) between two consecutive levels fine[3] and coarse[3] (checked like a link of the chain), on KS_F64
 * or KS_C64 vectors (part by part):  rc[I] = s * sum fl(b[i] - t[i])  in the order of (xix), and  x[i] = fl(x[i] + ec[I(i)]). */
int ks_host_multigrid_restrict(int dtype, const int64_t* fine, const int64_t* coarse, const void* b, const void* t, void* rc);
int ks_host_multigrid_prolong_add(int dtype, const int64_t* fine, const int64_t* coarse, const void* ec, void* x);
/* The scalar step of ks_operator_minres (xv) without a device -- the function its kernels run, compiled for the host: the new column
 * (beta, alpha, beta_new) of the Lanczos matrix through the rotations (c_prev, s_prev) and (c, s), the rotation that annihilates
 * beta_new, and the stopping test against stop = tol ||b||:
 *     eps = s_prev beta;  dbar = c_prev beta;  delta = c dbar + s alpha;  gbar = -s dbar + c alpha;
 *     gamma = hypot(gbar, beta_new), scaled by the larger of the two so that it overflows only where gamma itself does;
 *     fail  alpha, beta_new or gamma not finite, or gamma == 0: every output 0 but gamma;
 *     c' = gbar / gamma;  s' = beta_new / gamma;  phi = c' phibar;  phibar' = -s' phibar;  done  |phibar'| <= stop.
 * out = {eps, delta, gamma, c', s', phi, phibar'}.  Any output pointer may be NULL. */
int ks_host_minres_step(double alpha, double beta, double beta_new, double c, double s, double c_prev, double s_prev, double phibar,
                        double stop, double* out /* 7 */, int* done, int* fail);
/* The scalar steps of ks_operator_bicgstab (xvi) without a device -- the functions its kernels run, compiled for the host.  Every
 * scalar is a pair {re, im}; with is_complex == 0 the imaginary parts are ignored on input and 0 on output.  Only + - * /, sqrt and
 * explicit fma; a complex quotient a / b is a conj(b) / |b|^2.
 * ks_host_bicgstab_coef, one BiCG coefficient step:
 *     fail 1  rho0 zero or not finite, or beta not finite:   beta = alpha_new = 0;
 *     beta = alpha rho1 / rho0;
 *     fail 2  gamma zero or not finite, or alpha_new not finite:   alpha_new = 0 (beta stands);
 *     alpha_new = rho1 / gamma.
 * ks_host_bicgstab_mr, the Hermitian 2 x 2 minimal-residual solve [g11 g12; conj(g12) g22] g = h by Cramer's rule:
 *     det = fma(g11, g22, -|g12|^2);   fail 1  det zero or not finite, or a quotient not finite:   g = 0;
 *     g1 = (g22 h1 - g12 h2) / det;   g2 = (g11 h2 - conj(g12) h1) / det.
 * Any output pointer may be NULL. */
int ks_host_bicgstab_coef(int is_complex, const double* rho0, const double* rho1, const double* alpha, const double* gamma, double* beta,
                          double* alpha_new, int* fail);
int ks_host_bicgstab_mr(int is_complex, double g11, double g22, const double* g12, const double* h1, const double* h2, double* g1, double* g2,
                        double* det, int* fail);
/* The plan, the factors and the HOST apply of ks_operator_tridiag_solve without a device (docs/src/index.md:234-259: the
 * factorize / ldiv! pair of the shift-invert recipe): x[:, k] = (T - sigma I)^-1 b[:, k] for nrhs columns (column k at b + k ldb,
 * x + k ldx; b and x distinct), walking exactly the arrays the device kernels read, in their order.  Same refusals as the operator. */
int ks_host_tridiag_solve(int64_t n, int dtype, const void* dl, const void* d, const void* du, double sigma_re, double sigma_im,
                          int block_rows, int nrhs, const void* b, int64_t ldb, void* x, int64_t ldx, int* levels, double* max_growth,
                          double* residual);
/* ... and what ks_operator_tridiag_info would report for that input (docs/src/index.md:234-259), also without a device */
int ks_host_tridiag_info(int64_t n, int dtype, const void* dl, const void* d, const void* du, double sigma_re, double sigma_im,
                         int block_rows, int* levels, int64_t* level_rows /* cap 8 */, int64_t* shortened_blocks, double* max_growth,
                         double* residual);
/* sortschur!(H, Q, nconv, ordering)   src/run.jl:465-502 */
int ks_host_sortschur(int dtype, void* H, int m, int n, int ldh, void* Q, int nq, int ldq, int nconv,
                      int which);
/* givensAlgorithm (Julia stdlib LinearAlgebra = LAPACK dlartg/zlartg); out: c, s(re,im), r(re,im) */
int ks_host_givens(int dtype, const double* f, const double* g, double* c, double* s, double* r);

/* ---- diagnostics ---------------------------------------------------------------------------- */
/* Last words.  A measuring harness (bench.py with N > 1: a transport meets a new fabric for the first time) hands over the
 * text it wants on standard output should the process die under it -- SIGSEGV / SIGBUS / SIGABRT / SIGFPE / SIGILL (a
 * memory fault reported by the GPU runtime aborts the process) or SIGTERM (the launcher tearing the ranks down after a peer
 * died): the handler writes "\n<line>\n" to file descriptor 1 with write(2) and leaves with _exit(exit_code); nothing else
 * runs.  line == NULL uninstalls.  The text is copied.  No reference equivalent. */
int ks_last_words(const char* line, int exit_code);

#ifdef __cplusplus
}
#endif
#endif /* KSCHUR_H */
