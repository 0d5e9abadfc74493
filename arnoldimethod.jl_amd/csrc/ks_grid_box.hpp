// Matrix-free BOX-STENCIL grid operator  y = A x  on an nx x ny x nz grid (ks_operator_grid_box, include/kschur.h (xii)): mul!(y, A, x),
// src/expansion.jl:121, for the 3-, 9- or 27-point stencil that links a point to ALL its neighbours at distance one, the diagonal
// ones included -- the mixed derivatives of -div(D grad) + V with a full constant tensor D, compact (Mehrstellen) Laplacians, the
// stiffness and mass matrices of multilinear (Q1) finite elements on a uniform grid -- still with NOTHING stored per non-zero: the
// 3^ndim taps travel in the kernel arguments, the only per-row datum is the diagonal entry centre + potential[r].
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip right after ks_grid_var.hpp; ks_grid.hpp describes
// the scheme and holds everything this operator shares with the star operators.
//
// The operator IS the matrix ks_host_grid_box_matrix returns: open boundaries, the 27 slots k = 9 (dz + 1) + 3 (dy + 1) + (dx + 1)
// in ascending column order, every product rounded on its own and added to +0.0 in slot order, an absent slot not multiplied.
//
// k_grid_box: ONE LDS PASS PER PLANE, THREE ACCUMULATORS.  The 18 out-of-plane neighbours of a point are in-plane neighbours within
// the planes z - 1 and z + 1; instead of reading three LDS planes per output the kernel puts every plane p into an LDS tile once,
// with a halo one cell deep that includes the four corners (2 TX + 2 TY + 4 cells, at most one per thread), and while the plane is
// there every owned point reads its eight in-plane neighbours once (the ninth value is its own register) and feeds three rows:
//   row p + 1  starts at +0.0 with its nine dz = -1 terms,
//   row p      continues with its nine dz = 0 terms (the centre: the diagonal register),
//   row p - 1  finishes with its nine dz = +1 terms and is stored through GridStore with the x of plane p - 1, kept in registers.
// Every row so receives its 27 terms strictly in slot order.  Two accumulators per point live across steps (the started and the
// continued row); a z-range [za, zb) runs the steps p = za - 1 ... zb, of which the first only starts and the last only finishes;
// steps outside [0, nz) contribute nothing.  The plane p + 1, its diagonal and the halo cell of plane p + 2 are in flight during
// the arithmetic of step p and move into place after it; two LDS tiles alternate, one barrier per plane, as in k_grid.
// An in-plane neighbour exists where the (up to two) grid_neighbours flags of its direction hold; a wave all of whose points have
// all eight -- every wave but those at an edge of the grid -- adds the nine terms in straight-line code (as k_grid_star's grp).
// Tiles: 32 x 32, and 1024 x 1 for ny == 1, four points per thread, in both element types (the resource report behind the
// ComplexF64 choice is in DESIGN.md).  z-ranges: grid::plan with radius 1, at least 8 planes (the two extra steps: 25 %).
#pragma once

namespace ksd {

template <class T> struct GridBoxDev : GridGeom {
  T tap[27] = {};         // slot 9 (dz + 1) + 3 (dy + 1) + (dx + 1) (slots of a missing dimension: zero, never used)
};
static_assert(sizeof(GridBoxDev<double>) == 24 + 27 * 8 && sizeof(GridBoxDev<cd>) == 24 + 27 * 16,
              "kernel arguments: six ints, then the taps with nothing between");

// The nine terms of one dz added to s in slot order: tp = the nine taps, v = the nine values of the plane (v[4]: the point's own).
// MID: the centre term is the diagonal entry dc.  HY == 0 (a one-row tile: ny == 1): the three terms of dy = 0 alone.  full: every
// lane of the wave has all its in-plane neighbours; elsewhere an absent neighbour is not multiplied.
template <bool MID, int HY, class T>
__device__ __forceinline__ T grid_box_nine(T s, const T* __restrict__ tp, const T (&v)[9], const T& dc, bool full, bool hxm, bool hxp,
                                           bool hym, bool hyp) {
  if (full) {
#pragma unroll
    for (int j = HY ? 0 : 3; j < (HY ? 9 : 6); ++j) s = add_(s, mul_nc(MID && j == 4 ? dc : tp[j], v[j]));
  } else {
    if constexpr (HY > 0) {
      if (hym && hxm) s = add_(s, mul_nc(tp[0], v[0]));
      if (hym) s = add_(s, mul_nc(tp[1], v[1]));
      if (hym && hxp) s = add_(s, mul_nc(tp[2], v[2]));
    }
    if (hxm) s = add_(s, mul_nc(tp[3], v[3]));
    s = add_(s, mul_nc(MID ? dc : tp[4], v[4]));
    if (hxp) s = add_(s, mul_nc(tp[5], v[5]));
    if constexpr (HY > 0) {
      if (hyp && hxm) s = add_(s, mul_nc(tp[6], v[6]));
      if (hyp) s = add_(s, mul_nc(tp[7], v[7]));
      if (hyp && hxp) s = add_(s, mul_nc(tp[8], v[8]));
    }
  }
  return s;
}

template <class T, int TX, int TY>
__global__ void __launch_bounds__(kBlock)
    k_grid_box(const GridBoxDev<T> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
               const DevState* __restrict__ st, int shifted, T theta, double sigma) {
  if (st && st->breakdown >= 0) return;
  using L = GridLds<TX, TY, 1>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW;
  constexpr int NHALO = L::NHALO + (HY ? 4 : 0);   // ... with the four corners
  static_assert(NHALO <= kBlock, "at most one halo cell per thread");
  __shared__ T tile[2][L::LH * LW];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T> store{y, P, shifted, theta, sigma};

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT], hxm[PPT], hxp[PPT], hym[PPT], hyp[PPT];   // inside the grid; has a -x / +x / -y / +y neighbour
  bool full[PPT];     // every point k of this wave has its eight in-plane neighbours (uniform)
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, 1>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
    grid_neighbours(g, gx, gy, in[k], hxm[k], hxp[k], hym[k], hyp[k]);
    // (a point outside the grid has no row: nothing of it is stored, its neighbours in the tile are zeros or points of the grid,
    // and it does not keep the waves of a partial tile from the straight-line sums)
    full[k] = __all(!in[k] || (hxm[k] && hxp[k] && (HY == 0 || (hym[k] && hyp[k])))) != 0;
  }
  // this thread's halo cell: left column, right column, row below, row above, then the four corners
  bool hin = false;
  int64_t hoff = 0;
  int hli = 0;
  if (tid < NHALO) {
    int hx, hy;
    if (tid < TY) { hx = -1; hy = tid; }
    else if (tid < 2 * TY) { hx = TX; hy = tid - TY; }
    else if (tid < 2 * TY + HY * TX) { hx = tid - 2 * TY; hy = -1; }
    else if (tid < L::NHALO) { hx = tid - 2 * TY - TX; hy = TY; }
    else { hx = (tid - L::NHALO) & 1 ? TX : -1; hy = (tid - L::NHALO) & 2 ? TY : -1; }
    const int gx = it.x0 + hx, gy = it.y0 + hy;
    hin = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
    hoff = (int64_t)gy * g.nx + gx;
    hli = (hy + HY) * LW + hx + 1;
  }
  auto ldx = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };

  // Registers: xm / xc = the owned points of the planes p - 1 / p, xn receives plane p + 1; dc / dn = the diagonal of the planes
  // p / p + 1; h0 / h1 = this thread's halo cell of the planes p / p + 1, hn receives that of p + 2; a1 = the rows of plane p with
  // their dz = -1 terms, a2 = the rows of plane p - 1 with their dz = -1 and dz = 0 terms.
  T xm[PPT], xc[PPT], xn[PPT], dc[PPT], dn[PPT], a1[PPT], a2[PPT];
  T h0 = ldx(za - 1, hoff, hin), h1 = ldx(za, hoff, hin), hn = zero_of(T{});
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    xm[k] = zero_of(T{});
    xc[k] = ldx(za - 1, off[k], in[k]);
    xn[k] = zero_of(T{});
    dc[k] = diag ? zero_of(T{}) : g.tap[13];   // (the first step continues no row: the diagonal of plane za arrives with it)
    dn[k] = dc[k];
    a1[k] = zero_of(T{});
    a2[k] = zero_of(T{});
  }
  // (the trip count is uniform over the workgroup: the barriers match)
  for (int p = za - 1; p <= zb; ++p) {
    T* __restrict__ tl = tile[(p - za + 1) & 1];
#pragma unroll
    for (int k = 0; k < PPT; ++k) tl[li[k]] = xc[k];
    if (tid < NHALO) tl[hli] = h0;
    hn = ldx(p + 2, hoff, hin && p + 2 <= zb);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(p + 1, off[k], in[k] && p + 1 <= zb);   // (plane zb feeds the dz = +1 terms of the range's last plane)
      if (diag) dn[k] = grid_ldd(diag, g, P, p + 1, off[k], in[k] && p + 1 < zb);
    }
    __syncthreads();
    // uniform: plane p lies in the grid; row p - 1 / p / p + 1 belongs to this range
    const bool here = p >= 0 && p < g.nz, fin = p - 1 >= za, cont = p >= za && p < zb, start = p + 1 < zb;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      // the nine values of plane p around the point, read whether or not the neighbour exists (every place lies inside the tile
      // with its halo): the reads of a point are in flight together, what is conditional below is arithmetic on registers alone
      T v[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) v[j] = zero_of(T{});
      if constexpr (HY > 0) {
        v[0] = tl[li[k] - LW - 1]; v[1] = tl[li[k] - LW]; v[2] = tl[li[k] - LW + 1];
        v[6] = tl[li[k] + LW - 1]; v[7] = tl[li[k] + LW]; v[8] = tl[li[k] + LW + 1];
      }
      v[3] = tl[li[k] - 1];
      v[4] = xc[k];
      v[5] = tl[li[k] + 1];
      if (fin) {
        T s = a2[k];
        if (here) s = grid_box_nine<false, HY>(s, g.tap + 18, v, dc[k], full[k], hxm[k], hxp[k], hym[k], hyp[k]);
        store(p - 1, off[k], in[k], s, xm[k]);
      }
      if (cont) a2[k] = grid_box_nine<true, HY>(a1[k], g.tap + 9, v, dc[k], full[k], hxm[k], hxp[k], hym[k], hyp[k]);
      T s = zero_of(T{});
      if (start && here) s = grid_box_nine<false, HY>(s, g.tap, v, dc[k], full[k], hxm[k], hxp[k], hym[k], hyp[k]);
      a1[k] = s;
    }
    // what was in flight moves into place
    h0 = h1;
    h1 = hn;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xm[k] = xc[k];
      xc[k] = xn[k];
      dc[k] = dn[k];
    }
  }
}

}  // namespace ksd

namespace {
namespace grid {

// the 3^ndim taps in the 27 slots (slots of a missing dimension: zero, never used)
template <class H> void box_taps(int ndim, const H* t, H (&out)[27]) {
  for (H& o : out) o = H(0);
  const int cnt = ndim == 1 ? 3 : ndim == 2 ? 9 : 27;
  for (int k = 0; k < cnt; ++k) out[(27 - cnt) / 2 + k] = t[k];
}

// the checks both entry points of the box operator make: those of grid::check (which reads the first 2 ndim + 1 taps), then the
// other taps; nnz = prod_a (3 m_a - 2)
template <class H> Shape check_box(const std::string& who, int ndim, const int64_t* dims, const void* taps_v, const void* pot_v) {
  Shape s = check<H>(who, ndim, dims, taps_v, pot_v);
  const H* t = static_cast<const H*>(taps_v);
  const int cnt = ndim == 1 ? 3 : ndim == 2 ? 9 : 27;
  for (int k = 2 * ndim + 1; k < cnt; ++k)
    KS_REQUIRE(finite_(t[k]), KS_ERR_ARGUMENT, who + ": tap " + std::to_string(k) + " is not finite");
  s.nnz = (3 * s.nx - 2) * (3 * s.ny - 2) * (3 * s.nz - 2);
  return s;
}

// the host entry point (ks_host_grid_box_matrix, include/kschur.h (xii)): the checks, then every row as a sub-sequence of the 27
// slots -- ascending columns, because the columns are lexicographic in (jz, jy, jx)
template <class H>
void host_box_matrix_entry(const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* pot_v, int64_t* rowptr,
                           int32_t* colidx, void* val_v, int64_t cap, int64_t* nnz) {
  const Shape s = check_box<H>(who, ndim, dims, taps, pot_v);
  H* val = static_cast<H*>(val_v);
  const H* pot = static_cast<const H*>(pot_v);
  csr_begin(who, s, rowptr, colidx, val, cap, nnz);
  H t[27];
  box_taps(ndim, static_cast<const H*>(taps), t);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int64_t jx = ix + dx, jy = iy + dy, jz = iz + dz;
              if (jx < 0 || jx >= s.nx || jy < 0 || jy >= s.ny || jz < 0 || jz >= s.nz) continue;
              const int k = 9 * (dz + 1) + 3 * (dy + 1) + (dx + 1);
              colidx[q] = (int32_t)(r + dx + s.nx * dy + P * dz);
              val[q] = k != 13 ? t[k] : pot ? diag_add(t[13], pot[r]) : t[13];
              ++q;
            }
      }
  rowptr[s.n] = q;
}

}  // namespace grid

template <class D> struct BoxGridOp : GridOpBase<D> {
  using GridOpBase<D>::ctx; using GridOpBase<D>::diag; using GridOpBase<D>::nitems; using GridOpBase<D>::wide;
  ksd::GridBoxDev<D> g{};
  void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma) override {
    using TL = ksd::GridTile<false>;
    if (wide) ksd::k_grid_box<D, TL::WX, 1><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma);
    else ksd::k_grid_box<D, TL::TX, TL::TY><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma);
  }
};

template <class D>
ks_operator* make_grid_box(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* potential) {
  using H = typename HostT<D>::type;
  const grid::Shape s = grid::check_box<H>(who, ndim, dims, taps, potential);
  auto op = std::make_unique<BoxGridOp<D>>();
  H t[27];
  grid::box_taps(ndim, static_cast<const H*>(taps), t);
  std::memcpy(op->g.tap, t, sizeof(t));
  op->init(ctx, who, s, 1, false, op->g);   // (radius 1 without a coefficient: full tiles in both element types, 8-plane z-ranges)
  op->upload_diag(t[13], potential);
  return op.release();
}

}  // namespace
