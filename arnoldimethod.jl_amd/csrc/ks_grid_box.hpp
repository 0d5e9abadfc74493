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
// With periodic axes (ks_operator_grid_box_periodic, (xii-b)): the sibling kernel k_grid_box_per, further down; k_grid_box is untouched.
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

template <class T, int TX, int TY, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid_box(const GridBoxDev<T> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
               const DevState* __restrict__ st, int shifted, T theta, double sigma, const GridTail<T> tail) {
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
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};

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

// ------------------------------------------------------------------------------------------------------------- periodic axes
// ks_operator_grid_box_periodic, include/kschur.h (xii-b).  A link has a CLASS per axis -- 0: -1 across the boundary, 1: -1, 2: 0,
// 3: +1, 4: +1 across -- and its entry is link[25 e_z + 5 e_y + e_x], a table of 125 values in HBM that the host fills from the taps
// (every class 1 ... 3) and the caller's links (the classes that cross periodic axes alone; the others zero, never read).  A row is
// summed over the positions j = 0, 1, 2 of z, inside y, inside x; along an axis the offsets / classes at the positions are
//   interior, and the edges of an open axis (whose missing neighbour is absent)   (-1, 0, +1) / (1, 2, 3)
//   i = 0 of a periodic axis                                                       (0, +1, -1) / (2, 3, 0)   rotated left
//   i = m - 1 of a periodic axis                                                   (+1, -1, 0) / (4, 1, 2)   rotated right
// k_grid_box_per is k_grid_box with three additions.
// x and y: a cell one step outside the grid -- a halo cell, or beyond a partial last tile the LDS slot of an OWNED point with
//   gx == nx, gy == ny or both -- loads the wrap image from the other end of its line (both: point (0, 0)); such an owned slot is
//   never stored (off[] is the LOAD offset; stores and the diagonal are guarded by in[]).  The nine values of a point are read at
//   their places as before, so position j of an edge point is a rotation of the three values per axis: selects, no indexed registers.
// Waves with an edge point take the entries from the table, copied into LDS at the start, at 25 e_z + 5 e_y + e_x with the classes and
//   the present positions of the point packed into one register (pk); every other wave runs the straight-line sums of k_grid_box on
//   the 27 taps in the kernel arguments.
// z: the march hands plane p to the rows p + 1, p, p - 1 as dz = -1, 0, +1 (classes 1, 2, 3).  Row nz - 1 BEGINS with its links to
//   plane 0 (class 4) and row 0 ENDS with those to plane nz - 1 (class 0): the work item with row nz - 1 runs a pass over plane 0
//   BEFORE its march and leaves the nine terms in y, where the step that starts the row finds them instead of +0.0; the work item
//   with row 0 leaves that row in y without its Newton step and runs a pass over plane nz - 1 AFTER its march, which adds the nine
//   terms and finishes the row (the passes are described where they stand).  Outside the march the passes hold none of its
//   registers; inside it (the form tried first: DESIGN.md) they cost 40 VGPRs.  Two plane reads of x and one write and read of y
//   per tile column.
template <class T> struct GridBoxPerDev : GridBoxDev<T> {
  int px = 0, py = 0, pz = 0;   // the axis wraps
  const T* link = nullptr;      // the 125 entries
};

// the three values of one axis at the positions 0, 1, 2: c = 0 as they lie, 1 rotated left, 2 rotated right
// (selects on doubles: a select between cd structs goes through an indexed array in scratch memory)
__device__ __forceinline__ void grid_box_rot(unsigned c, double& a, double& b, double& d) {
  const double p = a, q = b, r = d;
  a = c == 1u ? q : c == 2u ? r : p;
  b = c == 1u ? r : c == 2u ? p : q;
  d = c == 1u ? p : c == 2u ? q : r;
}
__device__ __forceinline__ void grid_box_rot(unsigned c, cd& a, cd& b, cd& d) {
  grid_box_rot(c, a.x, b.x, d.x);
  grid_box_rot(c, a.y, b.y, d.y);
}

__device__ __forceinline__ double grid_box_sel(bool c, double a, double b) { return c ? a : b; }
__device__ __forceinline__ cd grid_box_sel(bool c, cd a, cd b) { return cd{c ? a.x : b.x, c ? a.y : b.y}; }

// pk of a point, per axis: bits 0-8 the classes at the positions 0, 1, 2; bits 9-11 the position is present; bits 12-13 the rotation
__device__ __forceinline__ unsigned grid_box_axis(bool in, bool per, int i, int m) {
  const bool lo = in && per && i == 0, hi = in && per && i + 1 == m;
  if (lo) return (2u | 3u << 3 | 0u << 6) | 7u << 9 | 1u << 12;
  if (hi) return (4u | 1u << 3 | 2u << 6) | 7u << 9 | 2u << 12;
  return (1u | 2u << 3 | 3u << 6) | ((in && i > 0 ? 1u : 0u) | 2u | (in && i + 1 < m ? 4u : 0u)) << 9;
}

// The nine terms of one z class added to s in position order: le = the 25 entries of that class, w = the nine values of the plane
// at their POSITIONS (rotated), pkx / pky = the classes and present positions of the point along x and y.  MID: the centre term is the diagonal entry dc.
template <bool MID, int HY, class T>
__device__ __forceinline__ T grid_box_nine_per(T s, const T* le, const T (&w)[9], const T& dc, unsigned pkx, unsigned pky) {
#pragma unroll
  for (int jy = HY ? 0 : 1; jy < (HY ? 3 : 2); ++jy) {
    const unsigned ey = pky >> (3 * jy) & 7u;
#pragma unroll
    for (int jx = 0; jx < 3; ++jx) {
      const unsigned ex = pkx >> (3 * jx) & 7u;
      T e = le[5u * ey + ex];
      if constexpr (MID) e = grid_box_sel(ex == 2u && ey == 2u, dc, e);
      if ((pkx >> (9 + jx) & 1u) && (pky >> (9 + jy) & 1u)) s = add_(s, mul_nc(e, w[3 * jy + jx]));
    }
  }
  return s;
}

template <class T, int TX, int TY, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid_box_per(const GridBoxPerDev<T> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
                   const DevState* __restrict__ st, int shifted, T theta, double sigma, const GridTail<T> tail) {
  if (st && st->breakdown >= 0) return;
  using L = GridLds<TX, TY, 1>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW;
  constexpr int NHALO = L::NHALO + (HY ? 4 : 0);   // ... with the four corners
  static_assert(NHALO <= kBlock, "at most one halo cell per thread");
  __shared__ T tile[2][L::LH * LW];
  __shared__ T lt[125];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};
  if (tid < 125) lt[tid] = g.link[tid];   // (first read after the first barrier of the z-loop)

  // a coordinate as it is LOADED: inside the grid itself, one step outside a periodic axis the other end, else -1
  auto img = [](int c, int m, int per) { return c >= 0 && c < m ? c : !per ? -1 : c == -1 ? m - 1 : c == m ? 0 : -1; };

  int64_t off[PPT];   // in-plane offset the owned point is loaded from (inside the grid: its own)
  int li[PPT];        // ... and its place in the LDS tile
  bool in[PPT];       // inside the grid
  bool ldk[PPT];      // loaded: inside the grid, or the wrap image one step beyond it
  unsigned pk[PPT];   // grid_box_axis along x (bits 0-13) and along y (bits 14-27)
  bool full[PPT];     // every point k of this wave has its eight in-plane neighbours at their interior positions (uniform)
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, 1>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
    const unsigned pkx = grid_box_axis(in[k], g.px != 0, gx, g.nx), pky = grid_box_axis(in[k], g.py != 0, gy, g.ny);
    pk[k] = pkx | pky << 14;
    const int mx = img(gx, g.nx, g.px), my = img(gy, g.ny, g.py);
    ldk[k] = mx >= 0 && my >= 0;
    if (ldk[k]) off[k] = (int64_t)my * g.nx + mx;
    constexpr unsigned kInterior = (1u | 2u << 3 | 3u << 6) | 7u << 9;
    full[k] = __all(!in[k] || (pkx == kInterior && (HY == 0 || pky == kInterior))) != 0;
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
    const int gx = img(it.x0 + hx, g.nx, g.px), gy = img(it.y0 + hy, g.ny, g.py);
    hin = gx >= 0 && gy >= 0;
    hoff = hin ? (int64_t)gy * g.nx + gx : 0;
    hli = (hy + HY) * LW + hx + 1;
  }
  auto ldx = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };
  // the nine values of tile t around point k (own: its own), at their places; then, in a wave with an edge point, at their positions
  auto rd = [&](const T* __restrict__ t, int k, const T& own, T(&w)[9], bool rot) {
#pragma unroll
    for (int j = 0; j < 9; ++j) w[j] = zero_of(T{});
    if constexpr (HY > 0) {
      w[0] = t[li[k] - LW - 1]; w[1] = t[li[k] - LW]; w[2] = t[li[k] - LW + 1];
      w[6] = t[li[k] + LW - 1]; w[7] = t[li[k] + LW]; w[8] = t[li[k] + LW + 1];
    }
    w[3] = t[li[k] - 1];
    w[4] = own;
    w[5] = t[li[k] + 1];
    if (rot) {
      unsigned q = pk[k];
      asm volatile("" : "+v"(q));
      const unsigned qx = q & 0x3fffu, qy = q >> 14;   // (see nine)
      const unsigned cx = qx >> 12, cy = qy >> 12;
#pragma unroll
      for (int r = HY ? 0 : 1; r < (HY ? 3 : 2); ++r) grid_box_rot(cx, w[3 * r], w[3 * r + 1], w[3 * r + 2]);
      if constexpr (HY > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) grid_box_rot(cy, w[c], w[3 + c], w[6 + c]);
      }
    }
  };
  // The links that cross z.  The range with row nz - 1 (wlast) runs a pass over plane 0 BEFORE its march and leaves the nine class-4
  // terms of that row in y, from where the step that starts the row takes them instead of +0.0; the range with row 0 (wfirst)
  // leaves that row in y without its Newton step and runs a pass over plane nz - 1 AFTER its march, which adds the nine class-0
  // terms and finishes the row.  Either way the row receives its terms in its order, and the passes hold none of the march's
  // registers.  A pass loads its plane straight into the LDS tile tb, which nobody reads at that time: tile[1] before the march
  // (the first step writes tile[0], and its barrier lies between these reads and the second step's writes), after it the tile of
  // the last step but one (every thread is past the last step's barrier).  Uniform over the workgroup: the barriers match.
  const bool wlast = g.pz && zb == g.nz, wfirst = g.pz && za == 0;
  auto pass = [&](T* __restrict__ tb, int zp, bool last) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) tb[li[k]] = ldx(zp, off[k], ldk[k]);
    if (tid < NHALO) tb[hli] = ldx(zp, hoff, hin);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T w[9];
      rd(tb, k, tb[li[k]], w, true);
      unsigned q = pk[k];
      asm volatile("" : "+v"(q));
      const unsigned qx = q & 0x3fffu, qy = q >> 14;   // (see nine)
      if (last) {   // row nz - 1 begins
        const T s = grid_box_nine_per<false, HY>(zero_of(T{}), lt + 100, w, w[4], qx, qy);
        if (in[k]) y[(int64_t)(g.nz - 1) * P + off[k]] = s;
      } else {      // row 0 ends
        T s = in[k] ? y[off[k]] : zero_of(T{});
        s = grid_box_nine_per<false, HY>(s, lt, w, w[4], qx, qy);
        store(0, off[k], in[k], s, ldx(0, off[k], in[k]));
      }
    }
  };
  if (wlast) pass(tile[1], 0, true);

  // Registers: as in k_grid_box.
  T xm[PPT], xc[PPT], xn[PPT], dc[PPT], dn[PPT], a1[PPT], a2[PPT];
  T h0 = ldx(za - 1, hoff, hin), h1 = ldx(za, hoff, hin), hn = zero_of(T{});
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    xm[k] = zero_of(T{});
    xc[k] = ldx(za - 1, off[k], ldk[k]);
    xn[k] = zero_of(T{});
    dc[k] = diag ? zero_of(T{}) : g.tap[13];
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
      xn[k] = ldx(p + 1, off[k], ldk[k] && p + 1 <= zb);
      if (diag) dn[k] = grid_ldd(diag, g, P, p + 1, off[k], in[k] && p + 1 < zb);
    }
    __syncthreads();
    const bool here = p >= 0 && p < g.nz, fin = p - 1 >= za, cont = p >= za && p < zb, start = p + 1 < zb;
    // row p - 1 = 0 waits in y for the pass over plane nz - 1; row p + 1 = nz - 1 begins with what the pass over plane 0 left in y
    const bool post = wfirst && p == 1, pre = wlast && p + 2 == g.nz;
    // the nine terms of the z class EZ = 1, 2, 3 (the taps 9 (EZ - 1) ...) of plane p
    auto nine = [&](auto ezc, int k, T s, const T(&w)[9]) {
      constexpr int EZ = decltype(ezc)::value;
      // (keeps the tests on classes and positions on these two registers: hoisted out of the z-loop every one of them would take
      // a scalar register pair, spilled to vector lanes and read back per use -- as in k_grid_star)
      unsigned q = pk[k];
      asm volatile("" : "+v"(q));
      const unsigned qx = q & 0x3fffu, qy = q >> 14;
      if (full[k]) return grid_box_nine<EZ == 2, HY>(s, g.tap + 9 * (EZ - 1), w, dc[k], true, true, true, true, true);
      return grid_box_nine_per<EZ == 2, HY>(s, lt + 25 * EZ, w, dc[k], qx, qy);
    };
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T w[9];
      rd(tl, k, xc[k], w, !full[k]);
      if (fin) {
        T s = a2[k];
        if (here) s = nine(std::integral_constant<int, 3>{}, k, s, w);
        if (!post) store(p - 1, off[k], in[k], s, xm[k]);
        else if (in[k]) y[off[k]] = s;
      }
      if (cont) a2[k] = nine(std::integral_constant<int, 2>{}, k, a1[k], w);
      T s = pre && in[k] ? y[(int64_t)(g.nz - 1) * P + off[k]] : zero_of(T{});
      if (start && here) s = nine(std::integral_constant<int, 1>{}, k, s, w);
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
  if (wfirst) pass(tile[(zb - za) & 1], g.nz - 1, false);
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

// The periodic axes of a box operator and its 125 entries by class (ks_host_grid_box_matrix_periodic, include/kschur.h (xii-b)):
// lk[25 e_z + 5 e_y + e_x], the class of a missing dimension being 2.  Every class 1 ... 3: the tap of the slot.  Some class 0 or 4,
// all of them on periodic axes: the caller's links[5^ndim flat index] (null: the tap of the slot), checked for finiteness.  Every
// other entry: zero, never used.  nnz = prod_a (periodic_a ? 3 m_a : 3 m_a - 2).
template <class H> struct BoxLinks {
  bool per[3] = {false, false, false};   // x, y, z
  H lk[125] = {};
  bool any() const { return per[0] || per[1] || per[2]; }
};
template <class H>
BoxLinks<H> check_box_links(const std::string& who, Shape& s, int ndim, const void* taps_v, const int* periodic, const void* links_v) {
  BoxLinks<H> B;
  if (!periodic) return B;
  {   // the flags and the extents: the refusal of every periodic grid operator (of the taps it reads the first 2 ndim + 1, finite)
    Shape tmp = s;
    const Wrap<H> W = check_wrap<H>(who, tmp, ndim, taps_v, periodic, nullptr);
    for (int a = 0; a < 3; ++a) B.per[a] = W.per[a];
  }
  H t[27];
  box_taps(ndim, static_cast<const H*>(taps_v), t);
  const H* links = static_cast<const H*>(links_v);
  for (int ez = 0; ez < 5; ++ez)
    for (int ey = 0; ey < 5; ++ey)
      for (int ex = 0; ex < 5; ++ex) {
        const int e[3] = {ex, ey, ez};
        bool cross = false, ok = true;
        int slot = 13, flat = 0, stride = 1;
        const int w3[3] = {1, 3, 9};
        for (int a = 0; a < 3; ++a) {
          if (a >= ndim && e[a] != 2) ok = false;
          if (e[a] == 0 || e[a] == 4) {
            cross = true;
            if (!B.per[a]) ok = false;
          }
          slot += w3[a] * (e[a] < 2 ? -1 : e[a] > 2 ? 1 : 0);
          if (a < ndim) { flat += stride * e[a]; stride *= 5; }
        }
        if (!ok) continue;
        H& out = B.lk[25 * ez + 5 * ey + ex];
        if (!cross) out = t[slot];
        else {
          out = links ? links[flat] : t[slot];
          KS_REQUIRE(finite_(out), KS_ERR_ARGUMENT, who + ": link value " + std::to_string(flat) + " is not finite");
        }
      }
  const int64_t ext[3] = {s.nx, s.ny, s.nz};
  s.nnz = 1;
  for (int a = 0; a < 3; ++a) s.nnz *= B.per[a] ? 3 * ext[a] : 3 * ext[a] - 2;
  return B;
}

// the offsets and classes of the links of point i along an axis of extent m, in row order; returns their number
inline int box_axis_links(int64_t i, int64_t m, bool per, int (&d)[3], int (&e)[3]) {
  int n = 0;
  auto put = [&](int dd, int ee) { d[n] = dd; e[n] = ee; ++n; };
  if (per && i == 0) { put(0, 2); put(1, 3); put(-1, 0); }
  else if (per && i + 1 == m) { put(1, 4); put(-1, 1); put(0, 2); }
  else {
    if (i > 0) put(-1, 1);
    put(0, 2);
    if (i + 1 < m) put(1, 3);
  }
  return n;
}

// the host entry point (ks_host_grid_box_matrix_periodic): the checks, then every row over the links of z, inside those of y,
// inside those of x -- ascending columns, because the columns are lexicographic in (jz, jy, jx)
template <class H>
void host_box_matrix_periodic_entry(const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* pot_v,
                                    const int* periodic, const void* links, int64_t* rowptr, int32_t* colidx, void* val_v, int64_t cap,
                                    int64_t* nnz) {
  Shape s = check_box<H>(who, ndim, dims, taps, pot_v);
  const BoxLinks<H> B = check_box_links<H>(who, s, ndim, taps, periodic, links);
  if (!B.any()) { host_box_matrix_entry<H>(who, ndim, dims, taps, pot_v, rowptr, colidx, val_v, cap, nnz); return; }
  H* val = static_cast<H*>(val_v);
  const H* pot = static_cast<const H*>(pot_v);
  csr_begin(who, s, rowptr, colidx, val, cap, nnz);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        int dx[3], ex[3], dy[3], ey[3], dz[3], ez[3];
        const int cx = box_axis_links(ix, s.nx, B.per[0], dx, ex), cy = box_axis_links(iy, s.ny, B.per[1], dy, ey),
                  cz = box_axis_links(iz, s.nz, B.per[2], dz, ez);
        for (int a = 0; a < cz; ++a)
          for (int b = 0; b < cy; ++b)
            for (int c = 0; c < cx; ++c) {
              const int64_t jx = (ix + dx[c] + s.nx) % s.nx, jy = (iy + dy[b] + s.ny) % s.ny, jz = (iz + dz[a] + s.nz) % s.nz;
              const int k = 25 * ez[a] + 5 * ey[b] + ex[c];
              colidx[q] = (int32_t)(jx + s.nx * jy + P * jz);
              val[q] = k != 62 ? B.lk[k] : pot ? diag_add(B.lk[62], pot[r]) : B.lk[62];
              ++q;
            }
      }
  rowptr[s.n] = q;
}

}  // namespace grid

template <class D> struct BoxGridOp : GridOpBase<D> {
  BoxGridOp() { this->cheb_fused_default = true; }   // (measured: GridOpBase)
  using GridOpBase<D>::ctx; using GridOpBase<D>::diag; using GridOpBase<D>::nitems; using GridOpBase<D>::wide;
  ksd::GridBoxDev<D> g{};
  // (bit 4 of `shifted`: the kernel instantiation with the tail of a Clenshaw step)
  void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) override {
    if (shifted & 16) launch_t<true>(x, y, st, shifted, theta, sigma, tail);
    else launch_t<false>(x, y, st, shifted, theta, sigma, tail);
  }
  template <bool TAIL> void launch_t(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) {
    using TL = ksd::GridTile<false>;
    if (wide) ksd::k_grid_box<D, TL::WX, 1, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
    else ksd::k_grid_box<D, TL::TX, TL::TY, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
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

// ... with periodic axes (ks_operator_grid_box_periodic): k_grid_box_per with the 125 entries by class in HBM
template <class D> struct BoxGridPerOp : GridOpBase<D> {
  using GridOpBase<D>::ctx; using GridOpBase<D>::diag; using GridOpBase<D>::nitems; using GridOpBase<D>::wide;
  ksd::GridBoxPerDev<D> g{};
  D* link = nullptr;
  ~BoxGridPerOp() override { (void)hipFree(link); }
  // (bit 4 of `shifted`: the kernel instantiation with the tail of a Clenshaw step)
  void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) override {
    if (shifted & 16) launch_t<true>(x, y, st, shifted, theta, sigma, tail);
    else launch_t<false>(x, y, st, shifted, theta, sigma, tail);
  }
  template <bool TAIL> void launch_t(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) {
    using TL = ksd::GridTile<false>;
    if (wide) ksd::k_grid_box_per<D, TL::WX, 1, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
    else ksd::k_grid_box_per<D, TL::TX, TL::TY, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
  }
};

template <class D>
ks_operator* make_grid_box_periodic(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps,
                                    const void* potential, const int* periodic, const void* links) {
  using H = typename HostT<D>::type;
  grid::Shape s = grid::check_box<H>(who, ndim, dims, taps, potential);
  const grid::BoxLinks<H> B = grid::check_box_links<H>(who, s, ndim, taps, periodic, links);
  if (!B.any()) return make_grid_box<D>(ctx, who, ndim, dims, taps, potential);   // the open operator: same matrix, same kernel
  auto op = std::make_unique<BoxGridPerOp<D>>();
  H t[27];
  grid::box_taps(ndim, static_cast<const H*>(taps), t);
  std::memcpy(op->g.tap, t, sizeof(t));
  op->g.px = B.per[0]; op->g.py = B.per[1]; op->g.pz = B.per[2];
  KS_HIP(hipMalloc(&op->link, sizeof(B.lk)));
  KS_HIP(hipMemcpy(op->link, B.lk, sizeof(B.lk), hipMemcpyHostToDevice));
  op->g.link = op->link;
  op->init(ctx, who, s, 1, false, op->g);
  op->upload_diag(t[13], potential);
  return op.release();
}

}  // namespace
