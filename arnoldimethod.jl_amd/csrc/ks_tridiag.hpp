// Tridiagonal shift-invert operator  y = (T - sigma I)^-1 x  (ks_operator_tridiag_solve, include/kschur.h): the plan of
// ks_tridiag_plan.hpp -- partition, block factors, spikes, all made ONCE on the host -- uploaded, and the two kernels that apply it
// with every vector resident in HBM.  No vendor library, no host involvement per product.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_operators.hpp.
//
// The same operator with a second tridiagonal matrix in front of the solve,  y = T^-1 M x  (ks_operator_tridiag_pencil): level 0 of
// k_td_down forms M x while it stages its right-hand side -- three more arrays, no launch and no vector more.
//
// Per product, on ctx->stream:  one k_td_down launch per level (the direct level included: one block, one workgroup), then one
// k_td_up launch per level on the way back: 2 levels - 1 launches (5 at n = 5e5 and 7 at n = 1e7 with 64-row blocks).  Stream order
// carries every dependency: no grid-wide barrier, no atomics, and the arithmetic of an entry never depends on the launch shape, so
// products are bit-identical when repeated.
//
// k_td_down.  One lane owns one block, a workgroup of 256 threads owns kTdBlocksPerWg = 64 consecutive blocks: all four waves
// stage the slice of the right-hand side into LDS with coalesced loads (a level above 0 forms it on the fly from the g of the
// level below: two gathered values per separator), the first wave walks -- forward with the pivot flags as selects, back with the
// three bands of U -- and all four waves write g back coalesced.  The factor arrays are block-interleaved ([i * nblocks + p]), so
// the 64 lanes of the walk read 64 neighbouring entries at every step.  LDS row pitch: (block rows + 1) | 1 elements -- odd, so
// lanes striding by it fall into distinct banks for 8- and 16-byte accesses alike.  64 blocks x 65 x 16 B = 66 560 B for
// ComplexF64 (two workgroups per CU out of 160 KiB), 33 280 B for Float64 (four).
// k_td_up.  One streaming pass, one thread per slot:  x[r] = g[r] - w[r] z[left] - v[r] z[right], separators copy z; in place.
#pragma once

#include "ks_tridiag_plan.hpp"

namespace ksd {

constexpr int kTdBlocksPerWg = 64;

template <class T> struct TdLevelDev {
  int64_t n = 0;
  int cap = 0, pitch = 0;
  int nblocks = 0, nsep = 0;
  const int32_t* start = nullptr;
  const int32_t* len = nullptr;
  const T* mult = nullptr;
  const T* inv = nullptr;
  const T* u1 = nullptr;
  const T* u2 = nullptr;
  const uint8_t* flag = nullptr;
  const T* w = nullptr;
  const T* v = nullptr;
  const int32_t* sep = nullptr;
  const T* sdl = nullptr;
  const T* sdu = nullptr;
};

__device__ __forceinline__ double td_neg(double a) { return -a; }
__device__ __forceinline__ cd td_neg(cd a) { return cd{-a.x, -a.y}; }
// c - a b, in the operation order of td::nmsub
__device__ __forceinline__ double td_nmsub(double a, double b, double c) { return c - a * b; }
__device__ __forceinline__ cd td_nmsub(cd a, cd b, cd c) { return cd{(c.x + a.y * b.y) - a.x * b.x, (c.y - a.y * b.x) - a.x * b.y}; }
__device__ __forceinline__ double td_sel(bool s, double a, double b) { return s ? a : b; }
__device__ __forceinline__ cd td_sel(bool s, cd a, cd b) { return cd{s ? a.x : b.x, s ? a.y : b.y}; }

// The multiplied matrix of a pencil product  y = T^-1 M x  (ks_operator_tridiag_pencil): its three diagonals, n entries each, the
// off-diagonals padded so that row r reads entry r of all three (mdl[0] = 0, mdu[n - 1] = 0).
// UNIFORM: every diagonal is one value (the consistent mass of a uniform mesh) -- the three values travel in the kernel arguments
// and the product reads no band at all.
template <class T> struct TdPencilDev {
  const T* md = nullptr;
  const T* mdl = nullptr;
  const T* mdu = nullptr;
  int uniform = 0;
  T cd{}, cl{}, cu{};
};

// V: the level being solved; B: the level below (B.sep == nullptr at level 0: the right-hand side is src itself).
// RHS = TdPencilDev (level 0 of a pencil product): B holds the diagonals of M and the right-hand side is M src, formed row by row
// while it is staged -- the two neighbour entries lie in the lines the coalesced load of src[row] brings in, so the product costs no
// launch and no vector of its own; src and g must not overlap then (a row reads its neighbours' src).
template <class T, class RHS = TdLevelDev<T>>
__global__ __launch_bounds__(256) void k_td_down(TdLevelDev<T> V, RHS B, const T* __restrict__ src, T* __restrict__ g,
                                                 const DevState* __restrict__ st) {
  constexpr bool PENCIL = std::is_same<RHS, TdPencilDev<T>>::value;
  if (st && st->breakdown >= 0) return;
  extern __shared__ double2 td_lds_raw[];
  T* lds = reinterpret_cast<T*>(td_lds_raw);
  const int b0 = blockIdx.x * kTdBlocksPerWg;
  const int nb = min(kTdBlocksPerWg, V.nblocks - b0);
  const int slot = V.cap + 1;
  const int total = nb * slot;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / slot, i = idx - b * slot;
    const int p = b0 + b;
    const int64_t row = (int64_t)V.start[p] + i;
    if (i <= V.len[p] && row < V.n) {
      T f;
      if constexpr (PENCIL) {
        // f = md x[r] + mdl x[r - 1] + mdu x[r + 1], in this order (api.host_tridiagonal_pencil_solve forms it the same way); nothing
        // lies in front of the first or behind the last row of a basis column that this kernel may read
        const T xm = row > 0 ? src[row - 1] : zero_of(T{}), xp = row + 1 < V.n ? src[row + 1] : zero_of(T{});
        const T md = B.uniform ? B.cd : B.md[row], ml = B.uniform ? B.cl : B.mdl[row], mu = B.uniform ? B.cu : B.mdu[row];
        f = add_(add_(mul_(md, src[row]), mul_(ml, xm)), mul_(mu, xp));
      } else if (B.sep == nullptr) {
        f = src[row];
      } else {
        const int64_t s = B.sep[row];
        const T nxt = s + 1 < B.n ? src[s + 1] : zero_of(T{});
        f = td_nmsub(B.sdu[row], nxt, td_nmsub(B.sdl[row], src[s - 1], src[s]));
      }
      lds[b * V.pitch + i] = f;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    const int p = b0 + threadIdx.x;
    const int L = V.len[p];
    const int64_t stride = V.nblocks;
    T* f = lds + threadIdx.x * V.pitch;
    // The walk is one chain of dependent steps per lane, so what it costs is latency: the factor entries of the NEXT chunk of
    // steps are requested before the current chunk is walked (they depend on nothing the walk computes).
    constexpr int CF = 8, CB = 4;
    T m0[CF];
    bool s0[CF];
    auto load_fwd = [&](int c0, T (&m)[CF], bool (&sw)[CF]) {
#pragma unroll
      for (int u = 0; u < CF; ++u) {
        const int i = c0 + u;
        const bool in = i + 1 < L;
        const int64_t q = in ? i * stride + p : p;  // (out of range: entry 0 of the block, loaded and ignored)
        m[u] = V.mult[q];
        sw[u] = in && V.flag[q] != 0;
      }
    };
    load_fwd(0, m0, s0);
    T cur = f[0];
    for (int c0 = 0; c0 + 1 < L; c0 += CF) {
      T m1[CF];
      bool s1[CF];
      load_fwd(c0 + CF, m1, s1);
#pragma unroll
      for (int u = 0; u < CF; ++u) {
        const int i = c0 + u;
        if (i + 1 < L) {
          const T nxt = f[i + 1];
          const T t = td_sel(s0[u], nxt, cur), o = td_sel(s0[u], cur, nxt);
          f[i] = t;
          cur = td_nmsub(m0[u], t, o);
        }
      }
#pragma unroll
      for (int u = 0; u < CF; ++u) { m0[u] = m1[u]; s0[u] = s1[u]; }
    }
    f[L - 1] = cur;
    T ra[CB], rb[CB], rc[CB];
    auto load_back = [&](int hi, T (&a)[CB], T (&b)[CB], T (&c)[CB]) {
#pragma unroll
      for (int u = 0; u < CB; ++u) {
        const int i = hi - u;
        const int64_t q = i >= 0 ? i * stride + p : p;
        a[u] = V.inv[q];
        b[u] = V.u1[q];
        c[u] = V.u2[q];
      }
    };
    load_back(L - 1, ra, rb, rc);
    T xp1 = zero_of(T{}), xp2 = zero_of(T{});
    for (int hi = L - 1; hi >= 0; hi -= CB) {
      T a1[CB], b1[CB], c1[CB];
      load_back(hi - CB, a1, b1, c1);
#pragma unroll
      for (int u = 0; u < CB; ++u) {
        const int i = hi - u;
        if (i >= 0) {
          const T xi = mul_(td_nmsub(rc[u], xp2, td_nmsub(rb[u], xp1, f[i])), ra[u]);
          f[i] = xi;
          xp2 = xp1;
          xp1 = xi;
        }
      }
#pragma unroll
      for (int u = 0; u < CB; ++u) { ra[u] = a1[u]; rb[u] = b1[u]; rc[u] = c1[u]; }
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int b = idx / slot, i = idx - b * slot;
    const int p = b0 + b;
    const int64_t row = (int64_t)V.start[p] + i;
    if (i <= V.len[p] && row < V.n) g[row] = lds[b * V.pitch + i];
  }
}

// g: this level's g, overwritten by its solution; z: the solution of the level above (one entry per separator)
template <class T>
__global__ __launch_bounds__(256) void k_td_up(TdLevelDev<T> V, T* __restrict__ g, const T* __restrict__ z, const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  const int slot = V.cap + 1;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)V.nblocks * slot) return;
  const int p = (int)(idx / slot), i = (int)(idx - (int64_t)p * slot);
  const int L = V.len[p];
  const int64_t row = (int64_t)V.start[p] + i;
  if (i > L || row >= V.n) return;
  if (i == L) { g[row] = z[p]; return; }
  const T zl = p > 0 ? z[p - 1] : zero_of(T{}), zr = p < V.nsep ? z[p] : zero_of(T{});
  g[row] = td_nmsub(V.v[idx], zr, td_nmsub(V.w[idx], zl, g[row]));
}

}  // namespace ksd

namespace {

template <class D> struct TridiagSolveOp : ks_operator {
  using H = typename HostT<D>::type;
  std::vector<ksd::TdLevelDev<D>> lv;
  std::vector<D*> scratch;        // scratch[l]: right-hand side, then solution, of level l >= 1 (allocated at upload)
  std::vector<void*> owned;
  std::vector<int64_t> level_rows;
  int64_t shortened = 0;
  double max_growth = 0.0, residual = 0.0;
  double bytes = 0.0;             // algorithmic bytes of one product (DESIGN: tridiagonal solve)
  ksd::TdPencilDev<D> pencil{};   // ks_operator_tridiag_pencil: the diagonals of M (null: the plain solve)
  ~TridiagSolveOp() override {
    for (void* p : owned) (void)hipFree(p);
  }
  template <class X> const X* up(const std::vector<X>& h) {
    void* d = nullptr;
    KS_HIP(hipMalloc(&d, std::max<size_t>(h.size() * sizeof(X), 16)));
    owned.push_back(d);
    if (!h.empty()) KS_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(X), hipMemcpyHostToDevice));
    return static_cast<const X*>(d);
  }
  template <class X> const D* upv(const std::vector<X>& h) {  // (std::complex<double> and cd share their layout)
    static_assert(sizeof(X) == sizeof(D), "element layout");
    return reinterpret_cast<const D*>(up(h));
  }
  static size_t lds_bytes(const ksd::TdLevelDev<D>& V) { return (size_t)std::min(ksd::kTdBlocksPerWg, V.nblocks) * V.pitch * sizeof(D); }
  void upload(const td::Plan<H>& P) {
    size_t lds_max = 0;
    for (size_t l = 0; l < P.levels.size(); ++l) {
      const td::Level<H>& V = P.levels[l];
      KS_REQUIRE(V.nblocks < (int64_t)2147483647 / (V.cap + 1), KS_ERR_ARGUMENT, "tridiagonal solve: too many blocks");
      ksd::TdLevelDev<D> d;
      d.n = V.n; d.cap = V.cap; d.pitch = V.pitch(); d.nblocks = (int)V.nblocks; d.nsep = (int)V.nsep;
      d.start = up(V.start); d.len = up(V.len);
      d.mult = upv(V.mult); d.inv = upv(V.inv); d.u1 = upv(V.u1); d.u2 = upv(V.u2); d.flag = up(V.flag);
      if (!V.direct) { d.w = upv(V.w); d.v = upv(V.v); d.sep = up(V.sep); d.sdl = upv(V.sdl); d.sdu = upv(V.sdu); }
      lv.push_back(d);
      level_rows.push_back(V.n);
      D* s = nullptr;
      if (l > 0) {
        KS_HIP(hipMalloc(&s, std::max<size_t>((size_t)V.n * sizeof(D), 16)));
        owned.push_back(s);
        KS_HIP(hipMemset(s, 0, std::max<size_t>((size_t)V.n * sizeof(D), 16)));
      }
      scratch.push_back(s);
      lds_max = std::max(lds_max, lds_bytes(d));
      // per row of a level: 4 factor values and the flag, f read, g written and read back; below the direct level 2 spike values
      bytes += (double)V.n * (7.0 * sizeof(D) + 1.0 + (V.direct ? 0.0 : 2.0 * sizeof(D)));
    }
    KS_REQUIRE(lds_max <= (size_t)160 * 1024, KS_ERR_INTERNAL, "tridiagonal solve: a workgroup's slice exceeds the LDS");
    KS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ksd::k_td_down<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(lds_max, 64 * 1024)));
    shortened = P.shortened; max_growth = P.max_growth; residual = P.residual;
  }
  // y = T^-1 M x: the diagonals of M next to the plan of T (off-diagonals padded to n entries, see TdPencilDev)
  void upload_pencil(int64_t n, const H* mdl, const H* md, const H* mdu) {
    std::vector<H> lo((size_t)n, H(0)), di(md, md + n), up_((size_t)n, H(0));
    for (int64_t i = 0; i + 1 < n; ++i) { lo[i + 1] = mdl[i]; up_[i] = mdu[i]; }
    for (int64_t i = 0; i < n; ++i)
      KS_REQUIRE(td::is_finite(lo[i]) && td::is_finite(di[i]) && td::is_finite(up_[i]), KS_ERR_ARGUMENT,
                 "tridiagonal pencil: non-finite entry of M in row " + std::to_string(i));
    // a uniform M (same bits in every entry of a diagonal; the pads at lo[0] and up_[n - 1] are covered by the kernel's guards)
    // is passed by value: no arrays, no band bytes
    bool uni = true;
    for (int64_t i = 1; i < n && uni; ++i)
      uni = std::memcmp(&di[i], &di[0], sizeof(H)) == 0 && (i < 2 || std::memcmp(&lo[i], &lo[1], sizeof(H)) == 0) &&
            (i + 1 >= n || std::memcmp(&up_[i], &up_[0], sizeof(H)) == 0);
    if (uni) {
      pencil.uniform = 1;
      pencil.md = upv(std::vector<H>(1, di[0]));   // (non-null: marks the pencil path)
      std::memcpy(&pencil.cd, &di[0], sizeof(H));
      if (n > 1) { std::memcpy(&pencil.cl, &lo[1], sizeof(H)); std::memcpy(&pencil.cu, &up_[0], sizeof(H)); }
    } else {
      pencil.md = upv(di); pencil.mdl = upv(lo); pencil.mdu = upv(up_);
      bytes += 3.0 * (double)n * sizeof(D);
    }
    KS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ksd::k_td_down<D, ksd::TdPencilDev<D>>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(lds_bytes(lv[0]), 64 * 1024)));
  }
  void apply(const void* xv, void* yv, const DevState* st) override {
    ProfScope ps(ctx, KSP_SPMV, bytes);
    const D* x = static_cast<const D*>(xv);
    D* y = static_cast<D*>(yv);
    hipStream_t s = ctx->stream;
    const int nl = (int)lv.size();
    KS_REQUIRE(!pencil.md || x != y, KS_ERR_ARGUMENT, "tridiagonal pencil: the product needs distinct x and y");
    auto gof = [&](int l) { return l == 0 ? y : scratch[l]; };
    for (int l = 0; l < nl; ++l) {
      const ksd::TdLevelDev<D>& V = lv[l];
      const int grid = (V.nblocks + ksd::kTdBlocksPerWg - 1) / ksd::kTdBlocksPerWg;
      if (l == 0 && pencil.md) ksd::k_td_down<D, ksd::TdPencilDev<D>><<<grid, kBlock, lds_bytes(V), s>>>(V, pencil, x, y, st);
      else ksd::k_td_down<D><<<grid, kBlock, lds_bytes(V), s>>>(V, l > 0 ? lv[l - 1] : ksd::TdLevelDev<D>{}, l > 0 ? gof(l - 1) : x, gof(l), st);
      KS_HIP(hipGetLastError());
    }
    for (int l = nl - 2; l >= 0; --l) {
      const ksd::TdLevelDev<D>& V = lv[l];
      const int64_t slots = (int64_t)V.nblocks * (V.cap + 1);
      ksd::k_td_up<D><<<(int)((slots + kBlock - 1) / kBlock), kBlock, 0, s>>>(V, gof(l), scratch[l + 1], st);
      KS_HIP(hipGetLastError());
    }
  }
};

template <class D>
ks_operator* make_tridiag(ks_ctx* ctx, int64_t n, const void* dl, const void* d, const void* du, double sre, double sim, int block_rows) {
  using H = typename HostT<D>::type;
  H sigma;
  if constexpr (std::is_same<D, double>::value) sigma = sre;
  else sigma = H(sre, sim);
  const td::Plan<H> P = td::build_plan<H>(n, static_cast<const H*>(dl), static_cast<const H*>(d), static_cast<const H*>(du), sigma, block_rows);
  auto op = std::make_unique<TridiagSolveOp<D>>();
  op->ctx = ctx;
  op->n_local = n;
  op->nnz = 3 * n - 2;
  op->dtype = sizeof(D) == 8 ? KS_F64 : KS_C64;
  op->upload(P);
  return op.release();
}

// y = T^-1 M x: the operator of make_tridiag on T (shift 0: the caller formed T = K - sigma M) with M's diagonals next to it
template <class D>
ks_operator* make_tridiag_pencil(ks_ctx* ctx, int64_t n, const void* dl, const void* d, const void* du, const void* mdl, const void* md,
                                 const void* mdu, int block_rows) {
  using H = typename HostT<D>::type;
  std::unique_ptr<TridiagSolveOp<D>> op(static_cast<TridiagSolveOp<D>*>(make_tridiag<D>(ctx, n, dl, d, du, 0.0, 0.0, block_rows)));
  KS_REQUIRE(md && (n == 1 || (mdl && mdu)), KS_ERR_ARGUMENT, "tridiagonal pencil: null diagonal of M");
  op->upload_pencil(n, static_cast<const H*>(mdl), static_cast<const H*>(md), static_cast<const H*>(mdu));
  op->nnz = 2 * (3 * n - 2);
  return op.release();
}

}  // namespace
