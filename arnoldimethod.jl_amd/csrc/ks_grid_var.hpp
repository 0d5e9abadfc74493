// Matrix-free VARIABLE-COEFFICIENT grid operator  y = A x  for A = -div(c(x) grad) + V(x) and its kin on an nx x ny x nz grid
// (ks_operator_grid_var, include/kschur.h (xi)): mul!(y, A, x), src/expansion.jl:121, for the 3-, 5- or 7-point stencil whose
// off-diagonal entries vary from link to link -- heterogeneous diffusion, a position-dependent effective mass, div (1 / eps) grad --
// still with NOTHING stored per non-zero.  The coefficient lives on the grid points (cell-centred, one Float64 per point, real also
// for ComplexF64 operators); the entry of the link from row r to its neighbour s in direction k is
//     A[r, s] = fl(h_k * fl(c[r] + c[s])),   h_k = 0.5 * tap_k   (ComplexF64: the two real products h_k.re * m, h_k.im * m)
// formed in registers; the six half taps travel in the kernel arguments (halved once on the host at upload).  The diagonal entry is
// centre + potential[r] as in ks_grid.hpp.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip right after ks_grid.hpp, whose launch constants,
// checks and host loops it shares.
//
// The operator IS the matrix ks_host_grid_var_matrix returns: the kernel forms every entry by exactly these two roundings, rounds
// every product on its own and adds the products of a row to +0.0 in ascending column order (-z, -y, -x, centre, +x, +y, +z; a link
// whose neighbour lies outside the grid is skipped), so y carries the bits every stored layout of that matrix gives.
//
// k_grid_var.  The scheme of k_grid (ks_grid.hpp), with c travelling exactly like x: a workgroup of 256 threads owns an in-plane
// tile and walks up a range of z-planes; per plane every thread keeps its own points of x AND of c of the planes z - 1, z, z + 1 in
// registers (the +-z links need c of the planes z +- 1) and the planes z + 2 in flight; the points of plane z of both go into LDS
// tiles together with the tile's halo (one cell per thread, loaded two planes ahead), from which the +-x and +-y links read the
// neighbour's x and the neighbour's c.  Two pairs of LDS tiles alternate: one barrier per plane.  The z-loop is unrolled by four
// so that the register sets rotate by name.  Compulsory traffic: x, c and the diagonal read once, y written once -- 32 bytes per row
// in Float64 (24 without a potential), 56 / 40 in ComplexF64 (c stays 8 bytes); the halo and plane re-reads are those of k_grid, of
// x and of c alike.
// Tiles (VarTile; the resource report behind the choice is in DESIGN.md): Float64 32 x 32 and 1024 x 1 (ny == 1), four points
// per thread; ComplexF64 32 x 16 and 512 x 1, two points per thread -- with four points the ComplexF64 kernel takes 223 registers
// and 55 KB of LDS, two waves per SIMD either way, with two points 128 registers and 29 KB, four waves (as StarTile for R >= 3).
#pragma once

namespace ksd {

template <class T> struct GridVarDev {
  int nx = 1, ny = 1, nz = 1;
  int ntx = 1, nty = 1;   // tiles along x and y
  int zc = 1;             // planes per z-range
  T tap[7] = {};          // -z, -y, -x, centre, +x, +y, +z: the six off-diagonal slots hold the HALF taps h_k, slot 3 the centre
};
// the in-plane tile of k_grid_var: four points per thread in Float64, two in ComplexF64
template <class T> struct VarTile {
  static constexpr bool kHalf = sizeof(T) == 16;
  static constexpr int TX = 32, TY = kHalf ? 16 : 32;   // ny > 1
  static constexpr int WX = kHalf ? 512 : 1024;         // ny == 1: WX x 1
};

// the entry of a link: h * m with m = fl(c[r] + c[s]) already rounded; ComplexF64: two real products, each rounded on its own
__device__ __forceinline__ double var_entry(double h, double m) {
  double e = h * m;
  keep(e);
  return e;
}
__device__ __forceinline__ cd var_entry(cd h, double m) {
  double er = h.x * m, ei = h.y * m;
  keep(er); keep(ei);
  return cd{er, ei};
}

// shifted, diag, st: as k_grid.  c: the n coefficients.
template <class T, int TX, int TY>
__global__ void __launch_bounds__(kBlock)
    k_grid_var(const GridVarDev<T> g, const T* __restrict__ x, const double* __restrict__ c, const T* __restrict__ diag,
               T* __restrict__ y, const DevState* __restrict__ st, int shifted, T theta, double sigma) {
  if (st && st->breakdown >= 0) return;
  constexpr int PPT = TX * TY / kBlock;          // points per thread
  constexpr int HY = TY > 1 ? 1 : 0;             // halo rows in y (a one-row tile belongs to a grid with ny == 1: no y neighbours)
  constexpr int LW = TX + 2, LH = TY + 2 * HY;   // LDS tile with its halo
  constexpr int NHALO = 2 * TY + 2 * HY * TX;    // halo cells (corners are never read)
  static_assert(TX * TY % kBlock == 0 && NHALO <= kBlock, "whole points and at most one halo cell per thread");
  __shared__ T tile[2][LH * LW];
  __shared__ double ctile[2][LH * LW];
  const int ntiles = g.ntx * g.nty;
  const int item = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int zr = item / ntiles, t2 = item - zr * ntiles;
  const int tyi = t2 / g.ntx, txi = t2 - tyi * g.ntx;
  const int x0 = txi * TX, y0 = tyi * TY;
  const int za = zr * g.zc, zb = min(g.nz, za + g.zc);
  const int64_t P = (int64_t)g.nx * g.ny;
  const int tid = (int)threadIdx.x;

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tiles
  bool in[PPT], hxm[PPT], hxp[PPT], hym[PPT], hyp[PPT];   // inside the grid; has a -x / +x / -y / +y neighbour
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = tid + k * kBlock;
    const int lx = p % TX, ly = p / TX;
    const int gx = x0 + lx, gy = y0 + ly;
    in[k] = gx < g.nx && gy < g.ny;
    off[k] = (int64_t)gy * g.nx + gx;
    li[k] = (ly + HY) * LW + lx + 1;
    hxm[k] = in[k] && gx > 0;
    hxp[k] = in[k] && gx + 1 < g.nx;
    hym[k] = in[k] && gy > 0;
    hyp[k] = in[k] && gy + 1 < g.ny;
  }
  // this thread's halo cell: left column, right column, row below, row above
  bool hin = false;
  int64_t hoff = 0;
  int hli = 0;
  if (tid < NHALO) {
    int hx, hy;
    if (tid < TY) { hx = -1; hy = tid; }
    else if (tid < 2 * TY) { hx = TX; hy = tid - TY; }
    else if (tid < 2 * TY + TX) { hx = tid - 2 * TY; hy = -1; }
    else { hx = tid - 2 * TY - TX; hy = TY; }
    const int gx = x0 + hx, gy = y0 + hy;
    hin = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
    hoff = (int64_t)gy * g.nx + gx;
    hli = (hy + HY) * LW + hx + 1;
  }
  // (a point outside the grid or the planes is never loaded: zero stands in -- for x and for c -- and is never part of a stored row)
  auto ldx = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };
  auto ldc = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? c[(int64_t)z * P + o] : 0.0; };
  auto ldd = [&](int z, int64_t o, bool ok) { return ok && z < g.nz ? ld_val(diag + ((int64_t)z * P + o), true) : zero_of(T{}); };

  // Register sets, as in k_grid: xr[0..3] / cr[0..3] hold the owned points of four consecutive planes and rotate by NAME (the
  // z-loop is unrolled by four); hr / hc [0..1]: this thread's halo cell of the planes of even / odd steps, dr[0..1]: the diagonal.
  T xr[4][PPT], dr[2][PPT], hr[2];
  double cr[4][PPT], hc[2];
  hr[0] = ldx(za, hoff, hin);
  hc[0] = ldc(za, hoff, hin);
  hr[1] = ldx(za + 1, hoff, hin && za + 1 < zb);
  hc[1] = ldc(za + 1, hoff, hin && za + 1 < zb);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    xr[0][k] = ldx(za - 1, off[k], in[k]);
    xr[1][k] = ldx(za, off[k], in[k]);
    xr[2][k] = ldx(za + 1, off[k], in[k]);
    cr[0][k] = ldc(za - 1, off[k], in[k]);
    cr[1][k] = ldc(za, off[k], in[k]);
    cr[2][k] = ldc(za + 1, off[k], in[k]);
    dr[0][k] = diag ? ldd(za, off[k], in[k]) : g.tap[3];
    dr[1][k] = dr[0][k];
  }
  const bool plain_st = (shifted & 2) != 0;
  // one plane: xm / xc / xp = planes z - 1 / z / z + 1 of x, xn receives plane z + 2 (cm / cc / cp / cn: of c); hw / hcw = the halo
  // cell of plane z, then of z + 2
  auto step = [&](int z, const T (&xm)[PPT], const T (&xc)[PPT], const T (&xp)[PPT], T (&xn)[PPT], const double (&cm)[PPT],
                  const double (&cc)[PPT], const double (&cp)[PPT], double (&cn)[PPT], T& hw, double& hcw, const T (&dc)[PPT],
                  T (&dn)[PPT], T* __restrict__ tl, double* __restrict__ cl) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      tl[li[k]] = xc[k];
      cl[li[k]] = cc[k];
    }
    if (tid < NHALO) {
      tl[hli] = hw;
      cl[hli] = hcw;
    }
    hw = ldx(z + 2, hoff, hin && z + 2 < zb);
    hcw = ldc(z + 2, hoff, hin && z + 2 < zb);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(z + 2, off[k], in[k] && z + 2 <= zb);   // (plane zb is the +z link of the range's last plane)
      cn[k] = ldc(z + 2, off[k], in[k] && z + 2 <= zb);
      if (diag) dn[k] = ldd(z + 1, off[k], in[k] && z + 1 < zb);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T s = zero_of(T{});
      const double cr_ = cc[k];
      // a link: entry = h (c_r + c_s), the sum rounded, then the product(s); then the entry times x_s, rounded on its own
      auto link = [&](const T& h, double cs, const T& xs) { return add_(s, mul_nc(var_entry(h, cr_ + cs), xs)); };
      if (z > 0) s = link(g.tap[0], cm[k], xm[k]);
      if constexpr (HY) {
        if (hym[k]) s = link(g.tap[1], cl[li[k] - LW], tl[li[k] - LW]);
      }
      if (hxm[k]) s = link(g.tap[2], cl[li[k] - 1], tl[li[k] - 1]);
      s = add_(s, mul_nc(dc[k], xc[k]));
      if (hxp[k]) s = link(g.tap[4], cl[li[k] + 1], tl[li[k] + 1]);
      if constexpr (HY) {
        if (hyp[k]) s = link(g.tap[5], cl[li[k] + LW], tl[li[k] + LW]);
      }
      if (z + 1 < g.nz) s = link(g.tap[6], cp[k], xp[k]);
      if (shifted & 1) s = scl(sub_s(s, mul_(theta, xc[k])), sigma);
      if (in[k]) {
        T* dst = y + ((int64_t)z * P + off[k]);
        if (plain_st) *dst = s;
        else st_elem_nt(dst, s);
      }
    }
  };
  // (the exits are uniform over the workgroup: the barriers match)
  for (int z = za; z < zb; z += 4) {
    step(z, xr[0], xr[1], xr[2], xr[3], cr[0], cr[1], cr[2], cr[3], hr[0], hc[0], dr[0], dr[1], tile[0], ctile[0]);
    if (z + 1 >= zb) break;
    step(z + 1, xr[1], xr[2], xr[3], xr[0], cr[1], cr[2], cr[3], cr[0], hr[1], hc[1], dr[1], dr[0], tile[1], ctile[1]);
    if (z + 2 >= zb) break;
    step(z + 2, xr[2], xr[3], xr[0], xr[1], cr[2], cr[3], cr[0], cr[1], hr[0], hc[0], dr[0], dr[1], tile[0], ctile[0]);
    if (z + 3 >= zb) break;
    step(z + 3, xr[3], xr[0], xr[1], xr[2], cr[3], cr[0], cr[1], cr[2], hr[1], hc[1], dr[1], dr[0], tile[1], ctile[1]);
  }
}

}  // namespace ksd

namespace {
namespace grid {

// h_k = 0.5 t_k (exact but for underflow; componentwise for ComplexF64), and the entry fl(h_k * m) of a link with m = fl(c[r] + c[s]):
// in ComplexF64 two real multiplications, written out so that no compiler option can contract them with anything
inline double half_tap(double t) { return 0.5 * t; }
inline cplx half_tap(cplx t) { return cplx(0.5 * t.real(), 0.5 * t.imag()); }
inline double var_entry(double h, double m) { return h * m; }
inline cplx var_entry(cplx h, double m) {
  const double re = h.real() * m, im = h.imag() * m;
  return cplx(re, im);
}

// the checks both entry points of the variable-coefficient operator make: those of grid::check, then the coefficient
template <class H>
Shape check_var(const std::string& who, int ndim, const int64_t* dims, const void* taps_v, const double* coeff, const void* pot_v) {
  const Shape s = check<H>(who, ndim, dims, taps_v, pot_v);
  KS_REQUIRE(coeff, KS_ERR_ARGUMENT, who + ": null coeff");
  for (int64_t r = 0; r < s.n; ++r)
    KS_REQUIRE(std::isfinite(coeff[r]), KS_ERR_ARGUMENT, who + ": coefficient entry " + std::to_string(r) + " is not finite");
  return s;
}

// The matrix that defines the variable-coefficient operator (ks_host_grid_var_matrix, include/kschur.h (xi)): the loops and the
// `put` order of host_matrix, open boundaries, the off-diagonal entries formed from the coefficient.
template <class H>
void host_var_matrix(const std::string& who, const Shape& s, int ndim, const H* taps, const double* coeff, const H* pot, int64_t* rowptr,
                     int32_t* colidx, H* val, int64_t cap, int64_t* nnz) {
  if (nnz) *nnz = s.nnz;
  KS_REQUIRE(cap >= s.nnz, KS_ERR_ARGUMENT,
             who + ": cap = " + std::to_string(cap) + " is too small, the matrix has " + std::to_string(s.nnz) + " entries");
  KS_REQUIRE(rowptr && (s.nnz == 0 || (colidx && val)), KS_ERR_ARGUMENT, who + ": null output array");
  H t[7], h[7];
  seven_taps(ndim, taps, t);
  for (int k = 0; k < 7; ++k) h[k] = half_tap(t[k]);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        auto put = [&](int64_t c, const H& v) { colidx[q] = (int32_t)c; val[q] = v; ++q; };
        auto link = [&](int k, int64_t c) {
          const double m = coeff[r] + coeff[c];
          put(c, var_entry(h[k], m));
        };
        if (iz > 0) link(0, r - P);
        if (iy > 0) link(1, r - s.nx);
        if (ix > 0) link(2, r - 1);
        put(r, pot ? diag_add(t[3], pot[r]) : t[3]);
        if (ix + 1 < s.nx) link(4, r + 1);
        if (iy + 1 < s.ny) link(5, r + s.nx);
        if (iz + 1 < s.nz) link(6, r + P);
      }
  rowptr[s.n] = q;
}

// the host entry point: the checks, then the matrix
template <class H>
void host_var_matrix_entry(const std::string& who, int ndim, const int64_t* dims, const void* taps, const double* coeff, const void* pot,
                           int64_t* rowptr, int32_t* colidx, void* val, int64_t cap, int64_t* nnz) {
  const Shape s = check_var<H>(who, ndim, dims, taps, coeff, pot);
  host_var_matrix<H>(who, s, ndim, static_cast<const H*>(taps), coeff, static_cast<const H*>(pot), rowptr, colidx, static_cast<H*>(val), cap, nnz);
}

}  // namespace grid

template <class D> struct VarGridOp : ks_operator {
  ksd::GridVarDev<D> g{};
  double* coeff = nullptr;   // c[r], always Float64
  D* diag = nullptr;         // centre + potential[r] (null: no potential)
  int nitems = 0;            // workgroups of a launch
  bool wide = false;         // the one-row tile (ny == 1)
  double bytes = 0.0;        // algorithmic bytes of one product
  ~VarGridOp() override {
    (void)hipFree(coeff);
    (void)hipFree(diag);
  }
  void launch(const void* xv, void* yv, const DevState* st, int shifted, D theta, double sigma) {
    KS_REQUIRE(xv != yv, KS_ERR_ARGUMENT, "grid operator: the product needs distinct x and y");
    ProfScope ps(ctx, KSP_SPMV, bytes);
    using TL = ksd::VarTile<D>;
    const D* x = static_cast<const D*>(xv);
    D* y = static_cast<D*>(yv);
    if (wide) ksd::k_grid_var<D, TL::WX, 1><<<nitems, kBlock, 0, ctx->stream>>>(g, x, coeff, diag, y, st, shifted, theta, sigma);
    else ksd::k_grid_var<D, TL::TX, TL::TY><<<nitems, kBlock, 0, ctx->stream>>>(g, x, coeff, diag, y, st, shifted, theta, sigma);
    KS_HIP(hipGetLastError());
  }
  void apply(const void* x, void* y, const DevState* st) override { launch(x, y, st, 0, D{}, 1.0); }
  // the Newton step in the same launch (KS_SHIFT_FUSED=0: the product and a streaming pass, like the stored layouts)
  void apply_shifted(const void* x, void* y, double tre, double tim, double sigma, int64_t ld, const DevState* st) override {
    if (!env_int("KS_SHIFT_FUSED", 1)) { ks_operator::apply_shifted(x, y, tre, tim, sigma, ld, st); return; }
    static const int env = env_int("KS_SHIFT_PLAIN", -1);
    const bool plain = env >= 0 ? env != 0 : shift_store_cacheable;
    D theta;
    if constexpr (sizeof(D) == 8) theta = tre; else theta = D{tre, tim};
    launch(x, y, st, 1 | (plain ? 2 : 0), theta, sigma);
  }
};

template <class D>
ks_operator* make_grid_var(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps, const double* coeff,
                           const void* potential) {
  using H = typename HostT<D>::type;
  using TL = ksd::VarTile<D>;
  const grid::Shape s = grid::check_var<H>(who, ndim, dims, taps, coeff, potential);
  auto op = std::make_unique<VarGridOp<D>>();
  op->ctx = ctx;
  op->n_local = s.n;
  op->nnz = s.nnz;
  op->dtype = sizeof(D) == 8 ? KS_F64 : KS_C64;
  static_assert(sizeof(H) == sizeof(D), "element layout");
  H t[7], h[7];
  grid::seven_taps(ndim, static_cast<const H*>(taps), t);
  for (int k = 0; k < 7; ++k) h[k] = k == 3 ? t[3] : grid::half_tap(t[k]);
  std::memcpy(op->g.tap, h, sizeof(h));
  op->g.nx = (int)s.nx; op->g.ny = (int)s.ny; op->g.nz = (int)s.nz;
  op->wide = s.ny == 1;
  const int64_t tx = op->wide ? TL::WX : TL::TX, ty = op->wide ? 1 : TL::TY;
  op->g.ntx = (int)((s.nx + tx - 1) / tx);
  op->g.nty = (int)((s.ny + ty - 1) / ty);
  const int64_t tiles = (int64_t)op->g.ntx * op->g.nty;
  const int64_t ranges = std::max<int64_t>(1, ksd::kGridWant / tiles);
  op->g.zc = (int)std::max<int64_t>(ksd::kGridMinZ, (s.nz + ranges - 1) / ranges);
  const int64_t items = tiles * ((s.nz + op->g.zc - 1) / op->g.zc);
  KS_REQUIRE(items < (int64_t)2147483647, KS_ERR_ARGUMENT, who + ": too many tiles for one launch");
  op->nitems = (int)items;
  KS_HIP(hipMalloc(&op->coeff, (size_t)s.n * sizeof(double)));
  KS_HIP(hipMemcpy(op->coeff, coeff, (size_t)s.n * sizeof(double), hipMemcpyHostToDevice));
  if (potential) {
    const H* v = static_cast<const H*>(potential);
    std::vector<H> d((size_t)s.n);
    for (int64_t r = 0; r < s.n; ++r) d[r] = grid::diag_add(t[3], v[r]);
    KS_HIP(hipMalloc(&op->diag, (size_t)s.n * sizeof(D)));
    KS_HIP(hipMemcpy(op->diag, d.data(), (size_t)s.n * sizeof(D), hipMemcpyHostToDevice));
  }
  op->bytes = (double)s.n * (sizeof(D) * (potential ? 3.0 : 2.0) + 8.0);
  return op.release();
}

}  // namespace
