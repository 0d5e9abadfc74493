// n x r vectors resident in HBM (ks_vectors, include/kschur.h): what the reference's recipes do AFTER the solve -- translate the
// vectors back to the original problem (Q = L^-* Y, docs/src/index.md:347) and show A x = x lambda / A x = B x lambda /
// Q* A Q = R, Q* B Q = I for the ORIGINAL matrices (docs/src/index.md:258, 302, 350-351) -- without a copy of the vectors to the host.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_backend.hpp.
//
// Storage is column-major with a leading dimension that is a multiple of 64 elements, zero-filled once; every kernel here writes
// rows < n only, so the pad rows stay zero -- the rule of ks_product.hpp's intermediates, for the same reason: the stored-matrix
// kernels may read the pad rows of their input.
#pragma once

namespace ksd {

// re[row] = x[row].x, im[row] = x[row].y  /  out[row] = (re[row], im[row]):  a ComplexF64 column seen as two Float64 columns, so
// that a Float64 operator runs on each part (rows < n only)
static __global__ void __launch_bounds__(kBlock) k_vec_split(const cd* __restrict__ x, double* __restrict__ re, double* __restrict__ im, int64_t n) {
  for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += (int64_t)gridDim.x * kBlock) {
    const cd v = x[row];
    re[row] = v.x;
    im[row] = v.y;
  }
}
static __global__ void __launch_bounds__(kBlock) k_vec_merge(const double* __restrict__ re, const double* __restrict__ im, cd* __restrict__ out, int64_t n) {
  for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += (int64_t)gridDim.x * kBlock) out[row] = cd{re[row], im[row]};
}

// Column residuals in one sweep: for the rc <= W output columns of this launch (columns boff .. boff+rc-1 of the whole block)
//   partial[i * gridDim.x + b]          = sum over the rows of workgroup b of | AX[row, i] - sum_{j < r} BX[row, j] C[j, i] |^2
//   partial[(W + i) * gridDim.x + b]    = sum over the rows of workgroup b of | BX[row, boff + i] |^2
// The shape of k_gemm_tall -- a tall-skinny product, the coefficient block in LDS -- with the store replaced by "subtract from the
// row of AX, square, accumulate".  A thread owns one 16-byte pack of rows at a time (two Float64 rows, one ComplexF64 row) and keeps
// the rc residual entries of it in registers: AX is loaded once, BX once for the products (and its rc columns of this launch once
// more, from the caches, for their norms), every coefficient read from LDS serves the whole pack, nothing n-sized is written.  The
// coefficients come NEGATED and transposed from the host, Cn[j * W + i] = -C[j, boff + i], zero for i >= rc and for the rows
// r <= j < round_up(r, 4): the unused register columns stay zero without a branch in the inner loop, and the columns of BX are
// loaded FOUR AHEAD of the products that use them (the group behind the last column loads that column again and meets zero
// coefficients): with the load next to its products the kernel waited for memory r times per pack (measured at n = 1e7, r = 20:
// 1.02 ms, 0.84 ms with the loads ahead; 3.3 ms with one row per thread and 8 columns at a time).  Packs may reach into the pad rows, which are zero in AX and BX.  The 2 rc sums of squares
// live in registers; every workgroup writes its slot (zeros where it has no rows) and k_slot_sum adds the slots in a fixed order: no
// floating-point atomics, the same bits every time.
template <class D, int W>
__global__ void __launch_bounds__(kBlock)
    k_resid_cols(const D* __restrict__ AX, int64_t lda, const D* __restrict__ BX, int64_t ldb, int64_t n, int r, int rc, int boff,
                 const D* __restrict__ Cn, double* __restrict__ partial) {
  using P = typename Pack<D>::type;
  constexpr int R = Pack<D>::R;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  D* cs = reinterpret_cast<D*>(smem_raw);
  const int r4 = (r + 3) & ~3;
  for (int i = threadIdx.x; i < r4 * W; i += kBlock) cs[i] = Cn[i];
  __syncthreads();
  double accr[W], accb[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { accr[i] = 0.0; accb[i] = 0.0; }
  const int64_t npacks = (n + R - 1) / R;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < npacks; p += (int64_t)gridDim.x * kBlock) {
    const int64_t row = p * R;
    P e[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      e[c] = zero_pack(D{});
      if (c < rc) {
        e[c] = ld_pack(AX + (int64_t)c * lda + row);
        accb[c] += nrm2_pack(ld_pack(BX + (int64_t)(boff + c) * ldb + row));
      }
    }
    P nx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) nx[u] = ld_pack(BX + (int64_t)(u < r ? u : r - 1) * ldb + row);
    for (int j0 = 0; j0 < r; j0 += 4) {
      P cur[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        cur[u] = nx[u];
        const int jn = j0 + 4 + u;
        nx[u] = ld_pack(BX + (int64_t)(jn < r ? jn : r - 1) * ldb + row);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < W; ++c) axpy_acc(e[c], cur[u], cs[(j0 + u) * W + c]);
    }
#pragma unroll
    for (int c = 0; c < W; ++c) accr[c] += nrm2_pack(e[c]);
  }
  __shared__ double red[kBlock / 64][2 * W];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const double sr = wave_sum(accr[i]), sb = wave_sum(accb[i]);
    if (lane == 0) { red[wave][i] = sr; red[wave][W + i] = sb; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * W) {
    double s = red[0][threadIdx.x];
    for (int wv = 1; wv < kBlock / 64; ++wv) s += red[wv][threadIdx.x];
    partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
  }
}

// out[c] = sum_b partial[c * nb + b], one workgroup per c, always in the same order
static __global__ void __launch_bounds__(kBlock) k_slot_sum(const double* __restrict__ partial, int nb, double* __restrict__ out) {
  __shared__ double sm[kBlock];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int b = tid; b < nb; b += kBlock) s += partial[(int64_t)blockIdx.x * nb + b];
  sm[tid] = s;
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    if (tid < w) sm[tid] += sm[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = sm[0];
}

}  // namespace ksd

struct ks_vectors {
  ks_ctx* ctx = nullptr;
  int64_t n = 0, ld = 64;
  int ncols = 0, dtype = KS_F64;
  size_t esz = 8;
  void* data = nullptr;
  // Float64 operator on ComplexF64 vectors: four real scratch columns (re / im of the input, re / im of the result), made on demand
  double* split = nullptr;
  // residuals / Gram matrices: the workgroups' slots, the reduced sums and the coefficient block, made on demand
  mutable void* red = nullptr;
  ~ks_vectors() { (void)hipFree(data); (void)hipFree(split); (void)hipFree(red); }
  void* col(int j) const { return static_cast<char*>(data) + (size_t)j * ld * esz; }
};

namespace {

constexpr int kVecMaxCols = 64;
constexpr int kResidSlot = 128;  // at most 2 * 56 sums per workgroup of k_resid_cols
constexpr int kGramBlocksPerCu = 2;

// layout of ks_vectors::red (bytes): coefficient block | slots of the workgroups | reduced sums
inline size_t vec_red_coef_bytes() { return (size_t)kVecMaxCols * kVecMaxCols * 16; }
inline size_t vec_red_slot_bytes(const ks_ctx* c) { return (size_t)c->num_cu * 4 * kResidSlot * 16; }
inline size_t vec_red_out_bytes() { return (size_t)kVecMaxCols * 64 * 16; }  // 64 Gram tiles of 64 entries (residuals need 2 x 64 doubles)
inline void vec_ensure_red(const ks_vectors* v) {
  if (v->red) return;
  const size_t bytes = vec_red_coef_bytes() + vec_red_slot_bytes(v->ctx) + vec_red_out_bytes();
  KS_HIP(hipMalloc(&v->red, bytes));
  KS_HIP(hipMemsetAsync(v->red, 0, bytes, v->ctx->stream));
}

inline int vec_stream_blocks(const ks_ctx* c, int64_t n, int per_cu) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, (int64_t)c->num_cu * per_cu));
}

inline void vec_check_pair(const char* who, const ks_vectors* a, const ks_vectors* b, bool same_cols) {
  const std::string w = who;
  KS_REQUIRE(a->ctx == b->ctx, KS_ERR_ARGUMENT, w + ": the vectors live on different contexts");
  KS_REQUIRE(a->n == b->n && (!same_cols || a->ncols == b->ncols), KS_ERR_ARGUMENT,
             w + ": shapes differ, (" + std::to_string(a->n) + ", " + std::to_string(a->ncols) + ") and (" + std::to_string(b->n) + ", " +
                 std::to_string(b->ncols) + ")");
  KS_REQUIRE(a->dtype == b->dtype, KS_ERR_ARGUMENT, w + ": the vectors do not have one element type");
}

inline ks_vectors* make_vectors(ks_ctx* ctx, int64_t n_local, int ncols, int dtype) {
  auto v = std::make_unique<ks_vectors>();
  v->ctx = ctx;
  v->n = n_local;
  v->ncols = ncols;
  v->dtype = dtype;
  v->esz = dtype == KS_F64 ? 8 : 16;
  v->ld = std::max<int64_t>(round_up(n_local, 64), 64);
  const size_t bytes = (size_t)v->ld * ncols * v->esz;
  KS_HIP(hipMalloc(&v->data, bytes));
  KS_HIP(hipMemsetAsync(v->data, 0, bytes, ctx->stream));
  KS_HIP(hipStreamSynchronize(ctx->stream));
  return v.release();
}

// out[:, i] = op in[:, i] for every column, on ctx->stream
inline void vectors_apply(ks_operator* op, const ks_vectors* in, ks_vectors* out) {
  ks_ctx* ctx = in->ctx;
  hipStream_t s = ctx->stream;
  if (in->n == 0) return;
  if (op->dtype == in->dtype) {
    for (int i = 0; i < in->ncols; ++i) {
      op->in_scale = 1.0;
      op->apply(in->col(i), out->col(i), nullptr);
    }
  } else {
    // Float64 operator, ComplexF64 vectors: the operator runs on the real and on the imaginary part, each a basis-shaped real column
    if (!out->split) {
      KS_HIP(hipMalloc(reinterpret_cast<void**>(&out->split), (size_t)4 * out->ld * 8));
      KS_HIP(hipMemsetAsync(out->split, 0, (size_t)4 * out->ld * 8, s));
    }
    double* p[4];
    for (int t = 0; t < 4; ++t) p[t] = out->split + (size_t)t * out->ld;
    const int nb = vec_stream_blocks(ctx, in->n, 8);
    for (int i = 0; i < in->ncols; ++i) {
      ksd::k_vec_split<<<nb, kBlock, 0, s>>>(static_cast<const cd*>(in->col(i)), p[0], p[1], in->n);
      KS_HIP(hipGetLastError());
      for (int t = 0; t < 2; ++t) {
        op->in_scale = 1.0;
        op->apply(p[t], p[2 + t], nullptr);
      }
      ksd::k_vec_merge<<<nb, kBlock, 0, s>>>(p[2], p[3], static_cast<cd*>(out->col(i)), in->n);
      KS_HIP(hipGetLastError());
    }
  }
}

// sums of squares of the columns of AX - BX C (r2) and of BX (b2), r values each; C host, column-major ldc
template <class T>
void vectors_residuals(const ks_vectors* AX, const ks_vectors* BX, const T* C, int ldc, double* r2, double* b2) {
  using D = typename DevT<T>::type;
  ks_ctx* ctx = AX->ctx;
  hipStream_t s = ctx->stream;
  const int r = AX->ncols;
  vec_ensure_red(AX);
  D* coef = static_cast<D*>(AX->red);
  double* slots = reinterpret_cast<double*>(static_cast<char*>(AX->red) + vec_red_coef_bytes());
  double* sums = reinterpret_cast<double*>(static_cast<char*>(AX->red) + vec_red_coef_bytes() + vec_red_slot_bytes(ctx));
  // the register columns of a launch: W <= 56 (Float64) / 40 (ComplexF64), which keeps the coefficient block of a launch
  // (round_up(r, 4) x W) below 48 KiB for every r <= 64; wider blocks are split over output-column chunks (gemm_tall_chunked's way)
  constexpr int kWMax = sizeof(D) == 8 ? 56 : 40;
  static_assert((size_t)kVecMaxCols * kWMax * sizeof(D) <= 48 * 1024, "coefficient block of a launch must fit 48 KiB of LDS");
  const int nb = ctx->num_cu * 4;
  std::vector<T> cn;
  std::vector<double> h((size_t)2 * kVecMaxCols);
  const int r4 = (r + 3) & ~3;
  for (int r0 = 0; r0 < r; r0 += kWMax) {
    const int rc = std::min(kWMax, r - r0);
    const int w = rc <= 8 ? 8 : rc <= 16 ? 16 : rc <= 20 ? 20 : rc <= 24 ? 24 : kWMax;   // (20: nev = 20, the headline)
    cn.assign((size_t)r4 * w, T(0));
    for (int j = 0; j < r; ++j)
      for (int i = 0; i < rc; ++i) cn[(size_t)j * w + i] = -C[j + (size_t)(r0 + i) * ldc];
    KS_HIP(hipMemcpyAsync(coef, cn.data(), cn.size() * sizeof(T), hipMemcpyHostToDevice, s));
    const size_t smem = (size_t)r4 * w * sizeof(D);
    const D* ax = static_cast<const D*>(AX->col(r0));
    const D* bx = static_cast<const D*>(BX->data);
    auto go = [&](auto w_tag) {
      constexpr int W = decltype(w_tag)::value;
      ksd::k_resid_cols<D, W><<<nb, kBlock, smem, s>>>(ax, AX->ld, bx, BX->ld, AX->n, r, rc, r0, coef, slots);
    };
    if (w == 8) go(std::integral_constant<int, 8>{});
    else if (w == 16) go(std::integral_constant<int, 16>{});
    else if (w == 20) go(std::integral_constant<int, 20>{});
    else if (w == 24) go(std::integral_constant<int, 24>{});
    else go(std::integral_constant<int, kWMax>{});
    KS_HIP(hipGetLastError());
    ksd::k_slot_sum<<<2 * w, kBlock, 0, s>>>(slots, nb, sums);
    KS_HIP(hipGetLastError());
    KS_HIP(hipMemcpyAsync(h.data(), sums, (size_t)2 * w * 8, hipMemcpyDeviceToHost, s));
    KS_HIP(hipStreamSynchronize(s));  // (one chunk unless r > Wmax)
    for (int i = 0; i < rc; ++i) { r2[r0 + i] = h[i]; b2[r0 + i] = h[w + i]; }
  }
}

// G = X^H Y (rx x ry, host, column-major ldg) in 8 x 8 tiles: every tile enqueued, ONE download, one synchronisation
template <class T> void vectors_gram(const ks_vectors* X, const ks_vectors* Y, T* G, int ldg) {
  using D = typename DevT<T>::type;
  ks_ctx* ctx = X->ctx;
  hipStream_t s = ctx->stream;
  vec_ensure_red(X);
  D* gp = reinterpret_cast<D*>(static_cast<char*>(X->red) + vec_red_coef_bytes());
  D* gout = reinterpret_cast<D*>(static_cast<char*>(X->red) + vec_red_coef_bytes() + vec_red_slot_bytes(ctx));
  const int gnb = vec_stream_blocks(ctx, X->n, kGramBlocksPerCu);
  const int tx = (X->ncols + 7) / 8, ty = (Y->ncols + 7) / 8;
  for (int ti = 0; ti < tx; ++ti)
    for (int tj = 0; tj < ty; ++tj) {
      const int na = std::min(8, X->ncols - 8 * ti), nbc = std::min(8, Y->ncols - 8 * tj);
      ksd::k_gram_tile<D><<<gnb, kBlock, 0, s>>>(static_cast<const D*>(X->col(8 * ti)), X->ld, na, static_cast<const D*>(Y->col(8 * tj)), Y->ld, nbc,
                                                  X->n, gp);
      ksd::k_reduce_cols<D><<<1, kBlock, 0, s>>>(gp, gnb, 64, 64, gout + (size_t)(ti * ty + tj) * 64);
    }
  KS_HIP(hipGetLastError());
  std::vector<T> tiles((size_t)tx * ty * 64);
  KS_HIP(hipMemcpyAsync(tiles.data(), gout, tiles.size() * sizeof(T), hipMemcpyDeviceToHost, s));
  KS_HIP(hipStreamSynchronize(s));
  for (int ti = 0; ti < tx; ++ti)
    for (int tj = 0; tj < ty; ++tj)
      for (int jj = 0; jj < std::min(8, Y->ncols - 8 * tj); ++jj)
        for (int ii = 0; ii < std::min(8, X->ncols - 8 * ti); ++ii)
          G[(8 * ti + ii) + (size_t)(8 * tj + jj) * ldg] = tiles[(size_t)(ti * ty + tj) * 64 + ii + 8 * jj];
}

}  // namespace
