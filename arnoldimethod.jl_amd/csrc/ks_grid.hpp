// Matrix-free grid operator  y = A x  for a constant-coefficient 3-, 5- or 7-point stencil plus a per-point diagonal term on an
// nx x ny x nz grid (ks_operator_grid, include/kschur.h): mul!(y, A, x), src/expansion.jl:121, for A = -Laplacian + V(x) and its
// kin, with NOTHING stored per non-zero.  The grid shape gives the boundary rows by index arithmetic, the seven taps travel in the
// kernel arguments, the only per-row datum is the diagonal entry centre + potential[r] (formed once on the host at upload, by the
// code that ks_host_grid_matrix runs).
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_tridiag.hpp.
//
// The operator IS the matrix ks_host_grid_matrix returns: the kernel rounds every product on its own and adds the products of a row
// to +0.0 in ascending column order (-z, -y, -x, centre, +x, +y, +z; a tap whose neighbour lies outside the grid is skipped), so y
// carries the bits every stored layout of that matrix gives.
//
// k_grid.  A workgroup of 256 threads owns an in-plane tile of TX x TY points (four points per thread) and walks up a range of
// z-planes.  Per plane every thread keeps its own points of the planes z - 1, z, z + 1 in registers (the +-z taps never touch
// memory a second time) and the planes z + 2 in flight; the points of plane z go into an LDS tile together with the tile's halo
// (one cell per thread, loaded two planes ahead), from which the +-x and +-y taps are read.  Two LDS tiles alternate: one barrier
// per plane.  The z-loop is unrolled by four so that the four register sets rotate by name: nothing waits for a load before the
// step that uses it.  Compulsory traffic: x read once, the diagonal read once, y written once -- 24 bytes per row in Float64 (16 without
// a potential), twice that in ComplexF64; on top of it the halo of a tile (2 (TX + TY) / (TX TY) of x: 12.5 % for 32 x 32) and
// the two planes a z-range reads beyond its own, which neighbouring workgroups of the same XCD bring into its L2.
// Every access is one element wide (8 bytes in Float64): a row starts at r = nx (...), for odd nx not 16-byte aligned, and nothing
// here depends on it.
// Tiles: 32 x 32 for grids with ny > 1, 1024 x 1 for ny == 1 (1-D grids, and nx x 1 x nz).  Work items are (z-range, tile), z-range
// major, dealt to the XCDs in contiguous runs (xcd_remap) so that neighbouring tiles meet in one L2.
//
// k_grid_star.  The star stencil of radius R = 2, 3, 4 (ks_operator_grid_star: central differences of order 4, 6, 8), open
// boundaries, a kernel of its own so that k_grid is what it was.  Same scheme, R deep: every thread keeps its own points of the
// 2 R + 1 planes z - R ... z + R in registers and plane z + R + 1 in flight, the LDS tile has a halo R cells deep on each side
// (2 R (TX + TY) cells: up to two per thread), and the existence of the +-x / +-y taps of every distance d is one bit per tap in
// one register per point, computed once per thread.  A row is summed in the 6 R + 1 slots -R z ... -1 z, -R y ... -1 y,
// -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z; an absent tap is not multiplied.
// The 2 R + 2 register sets rotate by MOVES at the end of a plane, not by name: unrolled by 2 R + 2 the z-loop of R = 4 is 180 KB
// of code and ran at 264 us per product on 216^3 against 111 us in this form (profiles/grid_operator.txt); the plane in flight
// lands in a set of its own and is waited for after the plane's arithmetic.  The z-loop is unrolled by two (the LDS tiles, the
// halo and the diagonal registers alternate).  The 4 R in-plane neighbours of a point are read from the tile before any of them
// is used, and a wave all of whose lanes have the R taps of a direction -- every wave but those at an edge of the grid -- adds
// them in straight-line code; only the other waves test tap by tap.
// Traffic: the same 24 / 16 bytes per row; the halo re-read is R 2 (TX + TY) / (TX TY) of x (R x 12.5 % for 32 x 32) and a z-range
// reads R planes beyond each end, 2 R / zc of x.  RULE for the z-ranges: at least kGridMinZ * R = 8 R planes each, so that the
// plane re-read stays at most 25 % as at radius 1 (and the 2 R + 1 planes of the prologue are at most a quarter of the loads).
// Tiles: Float64 32 x 32 and 1024 x 1 at every radius; ComplexF64 32 x 32 and 1024 x 1 at R = 2, 32 x 16 and 512 x 1 (two points
// per thread) at R = 3 and 4, where four points of ten planes would take the kernel to one wave per SIMD (StarTile, DESIGN).
#pragma once

namespace ksd {

constexpr int kGridMinZ = 8;       // planes per z-range, at least: a range reads two planes beyond its own (radius R: 8 R, 2 R beyond)
constexpr int kGridWant = 1024;    // work items per launch, at most, while z can be split: what an MI355X holds at once (4 per CU)

template <class T> struct GridDev {
  int nx = 1, ny = 1, nz = 1;
  int ntx = 1, nty = 1;   // tiles along x and y
  int zc = 1;             // planes per z-range
  T tap[7] = {};          // -z, -y, -x, centre, +x, +y, +z
};
// ... with periodic axes (ks_operator_grid_periodic): the entries of the links that cross the cell boundary and the axes that wrap.
// A type of its own, so that the open operator's kernel and its arguments are what they were.
template <class T> struct GridPerDev : GridDev<T> {
  T wrap[6] = {};         // -z, -y, -x, +x, +y, +z
  int px = 0, py = 0, pz = 0;
};

// shifted: bit 0 -- y = sigma (A x - theta x), the Newton step of the s-step expansion (as k_spmv_stencil2 stores it), bit 1 --
// cacheable instead of streaming stores.  diag == nullptr: no potential, the diagonal entry is tap[3].
//
// G = GridPerDev<T>: periodic axes.  A row is summed in the 13-slot order of include/kschur.h (ix), a wrap link at ANOTHER place than
// the interior link of its direction: the column of a +wrap link lies below every other column of its axis, that of a -wrap link
// above.  x and y: a halo cell one step outside the grid loads from the other end of its line.  When the last tile is partial the
// +x neighbour of gx = nx - 1 is no halo cell but the LDS slot of the OWNED point gx = nx, which then holds x[0] of the line
// (ldk, loff; likewise gy = ny); such a point is still never stored, and no row without that neighbour reads it.  z: plane -1 is
// plane nz - 1, plane nz is plane 0 (only the first and the last z-range meet them).
template <class T, int TX, int TY, class G>
__global__ void __launch_bounds__(kBlock)
    k_grid(const G g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y, const DevState* __restrict__ st,
           int shifted, T theta, double sigma) {
  if (st && st->breakdown >= 0) return;
  constexpr bool PER = !std::is_same<G, GridDev<T>>::value;
  constexpr int PPT = TX * TY / kBlock;          // points per thread
  constexpr int HY = TY > 1 ? 1 : 0;             // halo rows in y (a one-row tile belongs to a grid with ny == 1: no y neighbours)
  constexpr int LW = TX + 2, LH = TY + 2 * HY;   // LDS tile with its halo
  constexpr int NHALO = 2 * TY + 2 * HY * TX;    // halo cells (corners are never read)
  static_assert(TX * TY % kBlock == 0 && NHALO <= kBlock, "four points and at most one halo cell per thread");
  __shared__ T tile[2][LH * LW];
  const int ntiles = g.ntx * g.nty;
  const int item = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int zr = item / ntiles, t2 = item - zr * ntiles;
  const int tyi = t2 / g.ntx, txi = t2 - tyi * g.ntx;
  const int x0 = txi * TX, y0 = tyi * TY;
  const int za = zr * g.zc, zb = min(g.nz, za + g.zc);
  const int64_t P = (int64_t)g.nx * g.ny;
  const int tid = (int)threadIdx.x;

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT], hxm[PPT], hxp[PPT], hym[PPT], hyp[PPT];   // inside the grid; has a -x / +x / -y / +y neighbour
  // periodic: the point is loaded (in the grid, or the wrap image one step beyond it) from loff; its -x / +x / -y / +y link wraps
  bool ldk[PPT], wxm[PPT], wxp[PPT], wym[PPT], wyp[PPT];
  int64_t loff[PPT];
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
    if constexpr (PER) {
      wxm[k] = in[k] && g.px && gx == 0;
      wxp[k] = in[k] && g.px && gx + 1 == g.nx;
      wym[k] = in[k] && g.py && gy == 0;
      wyp[k] = in[k] && g.py && gy + 1 == g.ny;
      const bool ix = g.px && gx == g.nx && gy < g.ny, iy = g.py && gy == g.ny && gx < g.nx;   // the image of x[0, gy] / of x[gx, 0]
      ldk[k] = in[k] || ix || iy;
      loff[k] = ix ? (int64_t)gy * g.nx : iy ? (int64_t)gx : off[k];
    }
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
    int gx = x0 + hx, gy = y0 + hy;
    if constexpr (PER) {
      if (g.px) gx = gx == -1 ? g.nx - 1 : gx == g.nx ? 0 : gx;
      if (g.py) gy = gy == -1 ? g.ny - 1 : gy == g.ny ? 0 : gy;
    }
    hin = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
    hoff = (int64_t)gy * g.nx + gx;
    hli = (hy + HY) * LW + hx + 1;
  }
  // (a point outside the grid or the planes is never loaded: zero stands in and is never multiplied into a stored row)
  auto ldx = [&](int z, int64_t o, bool ok) {
    if constexpr (PER) {
      if (g.pz) z = z < 0 ? g.nz - 1 : z >= g.nz ? 0 : z;   // (z is never further out than one plane)
    }
    return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{});
  };
  // the owned points as they are LOADED: with periodic axes also the wrap images beyond a partial last tile
  auto ldo = [&](int z, int k, bool ok) {
    if constexpr (PER) return ldx(z, loff[k], ldk[k] && ok);
    else return ldx(z, off[k], in[k] && ok);
  };
  auto ldd = [&](int z, int64_t o, bool ok) { return ok && z < g.nz ? ld_val(diag + ((int64_t)z * P + o), true) : zero_of(T{}); };

  // Register sets: xr[0..3] hold the owned points of four consecutive planes and rotate by NAME, not by moves (the z-loop is
  // unrolled by four): a load issued in one step lands in the set that step no longer needs and is first read one barrier and
  // one step later.  hr[0..1]: this thread's halo cell of the planes of even / odd steps, dr[0..1]: the diagonal likewise.
  T xr[4][PPT], dr[2][PPT], hr[2];
  hr[0] = ldx(za, hoff, hin);
  hr[1] = ldx(za + 1, hoff, hin && za + 1 < zb);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    xr[0][k] = ldo(za - 1, k, true);
    xr[1][k] = ldo(za, k, true);
    xr[2][k] = ldo(za + 1, k, true);
    dr[0][k] = diag ? ldd(za, off[k], in[k]) : g.tap[3];
    dr[1][k] = dr[0][k];
  }
  const bool plain_st = (shifted & 2) != 0;
  // one plane: xm / xc / xp = planes z - 1 / z / z + 1, xn receives plane z + 2; hw = the halo cell of plane z, then of z + 2
  auto step = [&](int z, const T (&xm)[PPT], const T (&xc)[PPT], const T (&xp)[PPT], T (&xn)[PPT], T& hw, const T (&dc)[PPT], T (&dn)[PPT],
                  T* __restrict__ tl) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) tl[li[k]] = xc[k];
    if (tid < NHALO) tl[hli] = hw;
    hw = ldx(z + 2, hoff, hin && z + 2 < zb);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldo(z + 2, k, z + 2 <= zb);   // (plane zb is the +z tap of the range's last plane)
      if (diag) dn[k] = ldd(z + 1, off[k], in[k] && z + 1 < zb);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T s = zero_of(T{});
      if constexpr (PER) {
        if (g.pz && z + 1 == g.nz) s = add_(s, mul_nc(g.wrap[5], xp[k]));
      }
      if (z > 0) s = add_(s, mul_nc(g.tap[0], xm[k]));
      if constexpr (HY) {
        if constexpr (PER) {
          if (wyp[k]) s = add_(s, mul_nc(g.wrap[4], tl[li[k] + LW]));
        }
        if (hym[k]) s = add_(s, mul_nc(g.tap[1], tl[li[k] - LW]));
      }
      if constexpr (PER) {
        if (wxp[k]) s = add_(s, mul_nc(g.wrap[3], tl[li[k] + 1]));
      }
      if (hxm[k]) s = add_(s, mul_nc(g.tap[2], tl[li[k] - 1]));
      s = add_(s, mul_nc(dc[k], xc[k]));
      if (hxp[k]) s = add_(s, mul_nc(g.tap[4], tl[li[k] + 1]));
      if constexpr (PER) {
        if (wxm[k]) s = add_(s, mul_nc(g.wrap[2], tl[li[k] - 1]));
      }
      if constexpr (HY) {
        if (hyp[k]) s = add_(s, mul_nc(g.tap[5], tl[li[k] + LW]));
        if constexpr (PER) {
          if (wym[k]) s = add_(s, mul_nc(g.wrap[1], tl[li[k] - LW]));
        }
      }
      if (z + 1 < g.nz) s = add_(s, mul_nc(g.tap[6], xp[k]));
      if constexpr (PER) {
        if (g.pz && z == 0) s = add_(s, mul_nc(g.wrap[0], xm[k]));
      }
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
    step(z, xr[0], xr[1], xr[2], xr[3], hr[0], dr[0], dr[1], tile[0]);
    if (z + 1 >= zb) break;
    step(z + 1, xr[1], xr[2], xr[3], xr[0], hr[1], dr[1], dr[0], tile[1]);
    if (z + 2 >= zb) break;
    step(z + 2, xr[2], xr[3], xr[0], xr[1], hr[0], dr[0], dr[1], tile[0]);
    if (z + 3 >= zb) break;
    step(z + 3, xr[3], xr[0], xr[1], xr[2], hr[1], dr[1], dr[0], tile[1]);
  }
}

// ---------------------------------------------------------------------------------------------- radius 2, 3, 4 (open boundaries)
template <class T, int R> struct GridStarDev {
  int nx = 1, ny = 1, nz = 1;
  int ntx = 1, nty = 1;   // tiles along x and y
  int zc = 1;             // planes per z-range
  T tap[6 * R + 1] = {};  // -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z
};
// the in-plane tile of k_grid_star: four points per thread, two where four would cost the second wave per SIMD (ComplexF64, R >= 3)
template <class T, int R> struct StarTile {
  static constexpr bool kHalf = sizeof(T) == 16 && R >= 3;
  static constexpr int TX = 32, TY = kHalf ? 16 : 32;   // ny > 1
  static constexpr int WX = kHalf ? 512 : 1024;         // ny == 1: WX x 1
};

// steps J, J + 1, ..., N - 1 of one turn of the unrolled z-loop, each with its number as a compile-time constant (its parity
// picks the LDS tile and the halo and diagonal registers); stops after the range's last plane (uniform over the workgroup: the
// barriers match)
template <int J, int N, class F> __device__ __forceinline__ void grid_star_steps(int z, int zb, F& f) {
  f(z + J, std::integral_constant<int, J>{});
  if constexpr (J + 1 < N) {
    if (z + J + 1 < zb) grid_star_steps<J + 1, N>(z, zb, f);
  }
}

// shifted, diag: as k_grid.
template <class T, int TX, int TY, int R>
__global__ void __launch_bounds__(kBlock)
    k_grid_star(const GridStarDev<T, R> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
                const DevState* __restrict__ st, int shifted, T theta, double sigma) {
  if (st && st->breakdown >= 0) return;
  constexpr int PPT = TX * TY / kBlock;                  // points per thread
  constexpr int HY = TY > 1 ? R : 0;                     // halo rows in y on each side (a one-row tile: ny == 1, no y neighbours)
  constexpr int LW = TX + 2 * R, LH = TY + 2 * HY;       // LDS tile with its halo
  constexpr int NHALO = 2 * R * TY + 2 * HY * TX;        // halo cells (corners are never read)
  constexpr int NH = (NHALO + kBlock - 1) / kBlock;      // ... per thread, at most
  constexpr int N = 2 * R + 2;                           // register sets: planes z - R ... z + R and the one in flight
  static_assert(TX * TY % kBlock == 0 && R >= 2 && R <= 4 && NH <= 2, "whole points per thread, at most two halo cells");
  __shared__ T tile[2][LH * LW];
  const int ntiles = g.ntx * g.nty;
  const int item = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int zr = item / ntiles, t2 = item - zr * ntiles;
  const int tyi = t2 / g.ntx, txi = t2 - tyi * g.ntx;
  const int x0 = txi * TX, y0 = tyi * TY;
  const int za = zr * g.zc, zb = min(g.nz, za + g.zc);
  const int64_t P = (int64_t)g.nx * g.ny;
  const int tid = (int)threadIdx.x;

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT];       // inside the grid
  unsigned msk[PPT];  // bit d - 1 / 4 + d - 1 / 8 + d - 1 / 12 + d - 1: has a neighbour at -d x / +d x / -d y / +d y
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = tid + k * kBlock;
    const int lx = p % TX, ly = p / TX;
    const int gx = x0 + lx, gy = y0 + ly;
    in[k] = gx < g.nx && gy < g.ny;
    off[k] = (int64_t)gy * g.nx + gx;
    li[k] = (ly + HY) * LW + lx + R;
    msk[k] = 0u;
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      if (in[k] && gx >= d) msk[k] |= 1u << (d - 1);
      if (in[k] && gx + d < g.nx) msk[k] |= 1u << (4 + d - 1);
      if (in[k] && gy >= d) msk[k] |= 1u << (8 + d - 1);
      if (in[k] && gy + d < g.ny) msk[k] |= 1u << (12 + d - 1);
    }
    // (a point outside the grid has no row: nothing of it is stored, its neighbours in the tile are zeros or points of the
    // grid, and with every bit set it does not keep the waves of a partial tile from the straight-line sums)
    if (!in[k]) msk[k] = 0xffffu;
  }
  // this thread's halo cells: the R columns to the left, the R to the right, the R rows below, the R above
  bool hin[NH];
  int64_t hoff[NH];
  int hli[NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) {
    const int c = tid + j * kBlock;
    hin[j] = false;
    hoff[j] = 0;
    hli[j] = 0;
    if (c < NHALO) {
      int hx, hy;
      if (c < R * TY) { hx = -1 - c / TY; hy = c % TY; }
      else if (c < 2 * R * TY) { hx = TX + (c - R * TY) / TY; hy = (c - R * TY) % TY; }
      else if (c < 2 * R * TY + R * TX) { hx = (c - 2 * R * TY) % TX; hy = -1 - (c - 2 * R * TY) / TX; }
      else { hx = (c - 2 * R * TY - R * TX) % TX; hy = TY + (c - 2 * R * TY - R * TX) / TX; }
      const int gx = x0 + hx, gy = y0 + hy;
      hin[j] = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
      hoff[j] = (int64_t)gy * g.nx + gx;
      hli[j] = (hy + HY) * LW + hx + R;
    }
  }
  // (a point outside the grid or the planes is never loaded: zero stands in and is never multiplied into a stored row)
  auto ldx = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };
  auto ldd = [&](int z, int64_t o, bool ok) { return ok && z < g.nz ? ld_val(diag + ((int64_t)z * P + o), true) : zero_of(T{}); };

  // Register sets: at plane z set R + d holds the owned points of plane z + d, d = -R ... R, and set N - 1 receives plane
  // z + R + 1; after the plane's arithmetic every set moves down by one.  hr[0..1]: the halo cells of the planes of even / odd
  // steps (loaded two planes ahead), dr[0..1]: the diagonal likewise (one plane ahead).
  T xr[N][PPT], dr[2][PPT], hr[2][NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) {
    hr[0][j] = ldx(za, hoff[j], hin[j]);
    hr[1][j] = ldx(za + 1, hoff[j], hin[j] && za + 1 < zb);
  }
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
#pragma unroll
    for (int s = 0; s <= 2 * R; ++s) xr[s][k] = ldx(za - R + s, off[k], in[k]);
    xr[N - 1][k] = zero_of(T{});
    dr[0][k] = diag ? ldd(za, off[k], in[k]) : g.tap[3 * R];
    dr[1][k] = dr[0][k];
  }
  const bool plain_st = (shifted & 2) != 0;
  // The R taps of one direction, added to s in slot order: the tap of distance d is g.tap[BASE + SGN d], its neighbour v[d - 1],
  // and it exists where bit d - 1 of gm is set; SGN = -1: d = R ... 1, SGN = +1: d = 1 ... R.  Where every lane of the wave has
  // all R taps -- every wave but those at an edge of the grid -- the sum is straight-line code; elsewhere each tap is
  // conditional.  Either way an absent tap is not multiplied.
  auto grp = [&](T s, unsigned gm, auto basec, auto sgnc, const T(&v)[R]) {
    constexpr int BASE = decltype(basec)::value, SGN = decltype(sgnc)::value;
    constexpr unsigned FULL = (1u << R) - 1u;
    if (__all((gm & FULL) == FULL)) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int d = SGN < 0 ? R - i : i + 1;
        s = add_(s, mul_nc(g.tap[BASE + SGN * d], v[d - 1]));
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int d = SGN < 0 ? R - i : i + 1;
        if (gm >> (d - 1) & 1u) s = add_(s, mul_nc(g.tap[BASE + SGN * d], v[d - 1]));
      }
    }
    return s;
  };
  auto step = [&](int z, auto jc) {
    constexpr int B = decltype(jc)::value & 1;
    T* __restrict__ tl = tile[B];
    const T(&xc)[PPT] = xr[R];
    T(&xn)[PPT] = xr[N - 1];
#pragma unroll
    for (int k = 0; k < PPT; ++k) tl[li[k]] = xc[k];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      if (tid + j * kBlock < NHALO) tl[hli[j]] = hr[B][j];
      hr[B][j] = ldx(z + 2, hoff[j], hin[j] && z + 2 < zb);
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(z + R + 1, off[k], in[k] && z + 1 < zb);   // (the +R z tap of the next plane; beyond zb for the range's last R)
      if (diag) dr[1 - B][k] = ldd(z + 1, off[k], in[k] && z + 1 < zb);
    }
    __syncthreads();
    // the z taps as masks of the same kind (uniform): -d z exists for d <= z, +d z for d <= nz - 1 - z
    const unsigned zmm = (1u << min(R, z)) - 1u, zmp = (1u << min(R, g.nz - 1 - z)) - 1u;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T s = zero_of(T{});
      unsigned m = msk[k];
      asm volatile("" : "+v"(m));   // (keeps the 4 R tests per point on this one register: hoisted out of the z-loop they
                                    // would take a scalar register pair each, spilled to vector lanes and read back per use)
      // the 4 R in-plane neighbours, read whether or not the tap exists (every place lies inside the tile with its halo): the
      // reads of a point are in flight together, and what is conditional below is arithmetic on registers alone
      T vxm[R], vxp[R], vym[R], vyp[R];
#pragma unroll
      for (int d = 1; d <= R; ++d) {
        vxm[d - 1] = tl[li[k] - d];
        vxp[d - 1] = tl[li[k] + d];
        if constexpr (HY > 0) {
          vym[d - 1] = tl[li[k] - d * LW];
          vyp[d - 1] = tl[li[k] + d * LW];
        }
      }
      T vzm[R], vzp[R];
#pragma unroll
      for (int d = 1; d <= R; ++d) {
        vzm[d - 1] = xr[R - d][k];
        vzp[d - 1] = xr[R + d][k];
      }
      using M = std::integral_constant<int, -1>;
      using Q = std::integral_constant<int, 1>;
      s = grp(s, zmm, std::integral_constant<int, R>{}, M{}, vzm);
      if constexpr (HY > 0) s = grp(s, m >> 8, std::integral_constant<int, 2 * R>{}, M{}, vym);
      s = grp(s, m, std::integral_constant<int, 3 * R>{}, M{}, vxm);
      s = add_(s, mul_nc(dr[B][k], xc[k]));
      s = grp(s, m >> 4, std::integral_constant<int, 3 * R>{}, Q{}, vxp);
      if constexpr (HY > 0) s = grp(s, m >> 12, std::integral_constant<int, 4 * R>{}, Q{}, vyp);
      s = grp(s, zmp, std::integral_constant<int, 5 * R>{}, Q{}, vzp);
      if (shifted & 1) s = scl(sub_s(s, mul_(theta, xc[k])), sigma);
      if (in[k]) {
        T* dst = y + ((int64_t)z * P + off[k]);
        if (plain_st) *dst = s;
        else st_elem_nt(dst, s);
      }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
#pragma unroll
      for (int q = 0; q + 1 < N; ++q) xr[q][k] = xr[q + 1][k];
    }
  };
  for (int z = za; z < zb; z += 2) grid_star_steps<0, 2>(z, zb, step);
}

}  // namespace ksd

namespace {
namespace grid {

template <class H> inline bool finite_(const H& v) {
  if constexpr (std::is_same<H, double>::value) return std::isfinite(v);
  else return std::isfinite(v.real()) && std::isfinite(v.imag());
}
// centre + potential[r]: one addition, rounded once (componentwise for ComplexF64)
inline double diag_add(double c, double v) { return c + v; }
inline cplx diag_add(cplx c, cplx v) { return cplx(c.real() + v.real(), c.imag() + v.imag()); }

struct Shape {
  int64_t nx = 1, ny = 1, nz = 1, n = 0, nnz = 0;
};

// the checks both entry points make (include/kschur.h); `who` starts the message
// radius: 2 ndim radius + 1 taps, the star stencil of ks_operator_grid_star
template <class H>
Shape check(const std::string& who, int ndim, const int64_t* dims, const void* taps_v, const void* pot_v, int radius = 1) {
  KS_REQUIRE(radius >= 1 && radius <= 4, KS_ERR_ARGUMENT, who + ": radius = " + std::to_string(radius) + " (1, 2, 3 or 4 are supported)");
  KS_REQUIRE(ndim >= 1 && ndim <= 3, KS_ERR_ARGUMENT, who + ": ndim = " + std::to_string(ndim) + " (1, 2 or 3 are supported)");
  KS_REQUIRE(dims && taps_v, KS_ERR_ARGUMENT, who + ": null dims or taps");
  Shape s;
  int64_t* ext[3] = {&s.nx, &s.ny, &s.nz};
  constexpr int64_t kMax = 2147483646;   // rows and columns are 32-bit, like those of every stored matrix
  int64_t n = 1;
  for (int a = 0; a < ndim; ++a) {
    KS_REQUIRE(dims[a] >= 1, KS_ERR_ARGUMENT, who + ": extent " + std::to_string(a) + " is " + std::to_string(dims[a]) + " (must be at least 1)");
    KS_REQUIRE(dims[a] <= kMax / n, KS_ERR_ARGUMENT,
               who + ": the grid has more than " + std::to_string(kMax) + " points: n and the plane stride must fit the 32-bit row index");
    *ext[a] = dims[a];
    n *= dims[a];
  }
  s.n = n;
  s.nnz = n + 2 * ((s.nx - 1) * s.ny * s.nz + s.nx * (s.ny - 1) * s.nz + s.nx * s.ny * (s.nz - 1));
  for (int d = 2; d <= radius; ++d)   // the links of distance d: 2 max(m - d, 0) per line of m points
    s.nnz += 2 * (std::max<int64_t>(s.nx - d, 0) * s.ny * s.nz + s.nx * std::max<int64_t>(s.ny - d, 0) * s.nz +
                  s.nx * s.ny * std::max<int64_t>(s.nz - d, 0));
  const H* t = static_cast<const H*>(taps_v);
  for (int k = 0; k < 2 * ndim * radius + 1; ++k)
    KS_REQUIRE(finite_(t[k]), KS_ERR_ARGUMENT, who + ": tap " + std::to_string(k) + " is not finite");
  if (pot_v) {
    const H* v = static_cast<const H*>(pot_v);
    for (int64_t r = 0; r < n; ++r)
      KS_REQUIRE(finite_(v[r]), KS_ERR_ARGUMENT, who + ": potential entry " + std::to_string(r) + " is not finite");
  }
  return s;
}

// The periodic axes and the entries of their boundary-crossing links (ks_host_grid_matrix_periodic, include/kschur.h): flags in the
// order of dims, wrap = 2 ndim values in the order of the taps without the centre, null = the taps themselves.
template <class H> struct Wrap {
  bool per[3] = {false, false, false};   // x, y, z
  H w[6] = {};                           // -z, -y, -x, +x, +y, +z (an axis that does not wrap: zero, never used)
  bool any() const { return per[0] || per[1] || per[2]; }
};
template <class H>
Wrap<H> check_wrap(const std::string& who, Shape& s, int ndim, const void* taps_v, const int* periodic, const void* wrap_v) {
  Wrap<H> W;
  if (!periodic) return W;
  static const char* const axis[3] = {"x", "y", "z"};
  const int64_t ext[3] = {s.nx, s.ny, s.nz};
  const H* t = static_cast<const H*>(taps_v);
  const H* w = static_cast<const H*>(wrap_v);
  for (int a = 0; a < ndim; ++a) {
    if (!periodic[a]) continue;
    KS_REQUIRE(ext[a] >= 3, KS_ERR_ARGUMENT,
               who + ": periodic axis " + std::to_string(a) + " (" + axis[a] + ") has extent " + std::to_string(ext[a]) +
                   " (a periodic axis needs at least 3 points: at 2 the two neighbours coincide, at 1 the link is a self-link)");
    W.per[a] = true;
    // axis a: its - link is entry ndim - 1 - a of wrap (entry ndim - 1 - a of the taps), its + link entry ndim + a (tap ndim + 1 + a)
    const int km = ndim - 1 - a, kp = ndim + a;
    const H vm = w ? w[km] : t[km], vp = w ? w[kp] : t[kp + 1];
    KS_REQUIRE(finite_(vm), KS_ERR_ARGUMENT, who + ": wrap value " + std::to_string(km) + " (-" + axis[a] + ") is not finite");
    KS_REQUIRE(finite_(vp), KS_ERR_ARGUMENT, who + ": wrap value " + std::to_string(kp) + " (+" + axis[a] + ") is not finite");
    W.w[2 - a] = vm;
    W.w[3 + a] = vp;
    s.nnz += 2 * (s.n / ext[a]);   // the two links per line that truncation leaves out
  }
  return W;
}

// the 2 ndim + 1 taps in the seven slots -z, -y, -x, centre, +x, +y, +z (slots of a missing dimension: zero, never used)
template <class H> void seven_taps(int ndim, const H* t, H (&out)[7]) {
  for (H& o : out) o = H(0);
  for (int k = 0; k < 2 * ndim + 1; ++k) out[3 - ndim + k] = t[k];
}

// The matrix the operator is defined by, as 0-based CSR with ascending columns.  rowptr is always filled; colidx / val only when
// cap >= nnz.  With periodic axes a row is a sub-sequence of the 13 slots of include/kschur.h (ix): the link of the last point of a
// line to the first has the lowest column of its axis, that of the first to the last the highest.
template <class H>
void host_matrix(const std::string& who, const Shape& s, int ndim, const H* taps, const H* pot, const Wrap<H>& W, int64_t* rowptr,
                 int32_t* colidx, H* val, int64_t cap, int64_t* nnz) {
  if (nnz) *nnz = s.nnz;
  KS_REQUIRE(cap >= s.nnz, KS_ERR_ARGUMENT,
             who + ": cap = " + std::to_string(cap) + " is too small, the matrix has " + std::to_string(s.nnz) + " entries");
  KS_REQUIRE(rowptr && (s.nnz == 0 || (colidx && val)), KS_ERR_ARGUMENT, who + ": null output array");
  H t[7];
  seven_taps(ndim, taps, t);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        auto put = [&](int64_t c, const H& v) { colidx[q] = (int32_t)c; val[q] = v; ++q; };
        if (W.per[2] && iz + 1 == s.nz) put(r - (s.nz - 1) * P, W.w[5]);
        if (iz > 0) put(r - P, t[0]);
        if (W.per[1] && iy + 1 == s.ny) put(r - (s.ny - 1) * s.nx, W.w[4]);
        if (iy > 0) put(r - s.nx, t[1]);
        if (W.per[0] && ix + 1 == s.nx) put(r - (s.nx - 1), W.w[3]);
        if (ix > 0) put(r - 1, t[2]);
        put(r, pot ? diag_add(t[3], pot[r]) : t[3]);
        if (ix + 1 < s.nx) put(r + 1, t[4]);
        if (W.per[0] && ix == 0) put(r + (s.nx - 1), W.w[2]);
        if (iy + 1 < s.ny) put(r + s.nx, t[5]);
        if (W.per[1] && iy == 0) put(r + (s.ny - 1) * s.nx, W.w[1]);
        if (iz + 1 < s.nz) put(r + P, t[6]);
        if (W.per[2] && iz == 0) put(r + (s.nz - 1) * P, W.w[0]);
      }
  rowptr[s.n] = q;
}

// the 2 ndim R + 1 taps of a star stencil in the 6 R + 1 slots -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x,
// +1 y ... +R y, +1 z ... +R z (slots of a missing dimension: zero, never used)
template <class H> void star_taps(int ndim, int R, const H* t, H (&out)[25]) {
  for (H& o : out) o = H(0);
  for (int k = 0; k < 2 * ndim * R + 1; ++k) out[(3 - ndim) * R + k] = t[k];
}

// The matrix that defines the star operator of radius R (ks_host_grid_matrix_star, include/kschur.h (x)): open boundaries, a row is
// a sub-sequence of the 6 R + 1 slots.
template <class H>
void host_matrix_star(const std::string& who, const Shape& s, int ndim, int R, const H* taps, const H* pot, int64_t* rowptr,
                      int32_t* colidx, H* val, int64_t cap, int64_t* nnz) {
  if (nnz) *nnz = s.nnz;
  KS_REQUIRE(cap >= s.nnz, KS_ERR_ARGUMENT,
             who + ": cap = " + std::to_string(cap) + " is too small, the matrix has " + std::to_string(s.nnz) + " entries");
  KS_REQUIRE(rowptr && (s.nnz == 0 || (colidx && val)), KS_ERR_ARGUMENT, who + ": null output array");
  H t[25];
  star_taps(ndim, R, taps, t);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        auto put = [&](int64_t c, const H& v) { colidx[q] = (int32_t)c; val[q] = v; ++q; };
        for (int d = R; d >= 1; --d) if (iz >= d) put(r - d * P, t[R - d]);
        for (int d = R; d >= 1; --d) if (iy >= d) put(r - d * s.nx, t[2 * R - d]);
        for (int d = R; d >= 1; --d) if (ix >= d) put(r - d, t[3 * R - d]);
        put(r, pot ? diag_add(t[3 * R], pot[r]) : t[3 * R]);
        for (int d = 1; d <= R; ++d) if (ix + d < s.nx) put(r + d, t[3 * R + d]);
        for (int d = 1; d <= R; ++d) if (iy + d < s.ny) put(r + d * s.nx, t[4 * R + d]);
        for (int d = 1; d <= R; ++d) if (iz + d < s.nz) put(r + d * P, t[5 * R + d]);
      }
  rowptr[s.n] = q;
}

// both host entry points: the checks, then the matrix
template <class H>
void host_matrix_entry(const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* pot, const int* periodic,
                       const void* wrap, int64_t* rowptr, int32_t* colidx, void* val, int64_t cap, int64_t* nnz) {
  Shape s = check<H>(who, ndim, dims, taps, pot);
  const Wrap<H> W = check_wrap<H>(who, s, ndim, taps, periodic, wrap);
  host_matrix<H>(who, s, ndim, static_cast<const H*>(taps), static_cast<const H*>(pot), W, rowptr, colidx, static_cast<H*>(val), cap, nnz);
}

// ... and the star entry point (radius 1: the arrays of ks_host_grid_matrix, by its code)
template <class H>
void host_matrix_star_entry(const std::string& who, int ndim, const int64_t* dims, int radius, const void* taps, const void* pot,
                            int64_t* rowptr, int32_t* colidx, void* val, int64_t cap, int64_t* nnz) {
  const Shape s = check<H>(who, ndim, dims, taps, pot, radius);
  if (radius == 1)
    host_matrix<H>(who, s, ndim, static_cast<const H*>(taps), static_cast<const H*>(pot), Wrap<H>{}, rowptr, colidx, static_cast<H*>(val), cap, nnz);
  else
    host_matrix_star<H>(who, s, ndim, radius, static_cast<const H*>(taps), static_cast<const H*>(pot), rowptr, colidx, static_cast<H*>(val), cap, nnz);
}

}  // namespace grid

template <class D> struct GridOp : ks_operator {
  ksd::GridPerDev<D> g{};   // (the open operator's kernel takes its GridDev part)
  bool periodic = false;  // some axis wraps: the kernel's periodic instantiation
  D* diag = nullptr;   // centre + potential[r] (null: no potential)
  int nitems = 0;      // workgroups of a launch
  bool wide = false;   // the 1024 x 1 tile (ny == 1)
  int radius = 1;      // > 1: the star stencil, k_grid_star with the taps of `star`
  D star[25] = {};     // its 6 radius + 1 slots
  double bytes = 0.0;  // algorithmic bytes of one product
  ~GridOp() override { (void)hipFree(diag); }
  void launch(const void* xv, void* yv, const DevState* st, int shifted, D theta, double sigma) {
    KS_REQUIRE(xv != yv, KS_ERR_ARGUMENT, "grid operator: the product needs distinct x and y");
    ProfScope ps(ctx, KSP_SPMV, bytes);
    const D* x = static_cast<const D*>(xv);
    D* y = static_cast<D*>(yv);
    const ksd::GridDev<D>& go = g;
    if (radius == 2) launch_star<2>(x, y, st, shifted, theta, sigma);
    else if (radius == 3) launch_star<3>(x, y, st, shifted, theta, sigma);
    else if (radius == 4) launch_star<4>(x, y, st, shifted, theta, sigma);
    else if (periodic) {
      if (wide) ksd::k_grid<D, 1024, 1, ksd::GridPerDev<D>><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma);
      else ksd::k_grid<D, 32, 32, ksd::GridPerDev<D>><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma);
    } else if (wide) ksd::k_grid<D, 1024, 1, ksd::GridDev<D>><<<nitems, kBlock, 0, ctx->stream>>>(go, x, diag, y, st, shifted, theta, sigma);
    else ksd::k_grid<D, 32, 32, ksd::GridDev<D>><<<nitems, kBlock, 0, ctx->stream>>>(go, x, diag, y, st, shifted, theta, sigma);
    KS_HIP(hipGetLastError());
  }
  template <int R> void launch_star(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma) {
    using TL = ksd::StarTile<D, R>;
    ksd::GridStarDev<D, R> gs;
    gs.nx = g.nx; gs.ny = g.ny; gs.nz = g.nz; gs.ntx = g.ntx; gs.nty = g.nty; gs.zc = g.zc;
    for (int k = 0; k < 6 * R + 1; ++k) gs.tap[k] = star[k];
    if (wide) ksd::k_grid_star<D, TL::WX, 1, R><<<nitems, kBlock, 0, ctx->stream>>>(gs, x, diag, y, st, shifted, theta, sigma);
    else ksd::k_grid_star<D, TL::TX, TL::TY, R><<<nitems, kBlock, 0, ctx->stream>>>(gs, x, diag, y, st, shifted, theta, sigma);
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
ks_operator* make_grid(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* potential,
                       const int* periodic, const void* wrap, int radius = 1) {
  using H = typename HostT<D>::type;
  grid::Shape s = grid::check<H>(who, ndim, dims, taps, potential, radius);
  KS_REQUIRE(radius == 1 || !periodic, KS_ERR_ARGUMENT, who + ": periodic axes take radius 1");
  const grid::Wrap<H> W = grid::check_wrap<H>(who, s, ndim, taps, periodic, wrap);
  auto op = std::make_unique<GridOp<D>>();
  op->ctx = ctx;
  op->n_local = s.n;
  op->nnz = s.nnz;
  op->dtype = sizeof(D) == 8 ? KS_F64 : KS_C64;
  static_assert(sizeof(H) == sizeof(D), "element layout");
  H t[7], centre;
  if (radius == 1) {
    grid::seven_taps(ndim, static_cast<const H*>(taps), t);
    std::memcpy(op->g.tap, t, sizeof(t));
    centre = t[3];
  } else {
    H ts[25];
    grid::star_taps(ndim, radius, static_cast<const H*>(taps), ts);
    std::memcpy(op->star, ts, sizeof(ts));
    centre = ts[3 * radius];
  }
  op->radius = radius;
  std::memcpy(op->g.wrap, W.w, sizeof(W.w));
  op->g.px = W.per[0]; op->g.py = W.per[1]; op->g.pz = W.per[2];
  op->periodic = W.any();
  op->g.nx = (int)s.nx; op->g.ny = (int)s.ny; op->g.nz = (int)s.nz;
  op->wide = s.ny == 1;
  const bool half = radius > 1 && (radius == 2 ? ksd::StarTile<D, 2>::kHalf : radius == 3 ? ksd::StarTile<D, 3>::kHalf : ksd::StarTile<D, 4>::kHalf);
  const int64_t tx = op->wide ? (half ? 512 : 1024) : 32, ty = op->wide ? 1 : half ? 16 : 32;
  op->g.ntx = (int)((s.nx + tx - 1) / tx);
  op->g.nty = (int)((s.ny + ty - 1) / ty);
  const int64_t tiles = (int64_t)op->g.ntx * op->g.nty;
  const int64_t ranges = std::max<int64_t>(1, ksd::kGridWant / tiles);
  op->g.zc = (int)std::max<int64_t>(ksd::kGridMinZ * radius, (s.nz + ranges - 1) / ranges);
  const int64_t items = tiles * ((s.nz + op->g.zc - 1) / op->g.zc);
  KS_REQUIRE(items < (int64_t)2147483647, KS_ERR_ARGUMENT, who + ": too many tiles for one launch");
  op->nitems = (int)items;
  if (potential) {
    const H* v = static_cast<const H*>(potential);
    std::vector<H> d((size_t)s.n);
    for (int64_t r = 0; r < s.n; ++r) d[r] = grid::diag_add(centre, v[r]);
    KS_HIP(hipMalloc(&op->diag, (size_t)s.n * sizeof(D)));
    KS_HIP(hipMemcpy(op->diag, d.data(), (size_t)s.n * sizeof(D), hipMemcpyHostToDevice));
  }
  op->bytes = (double)s.n * sizeof(D) * (potential ? 3.0 : 2.0);
  return op.release();
}

}  // namespace
