// Matrix-free grid operators  y = A x  on an nx x ny x nz grid: mul!(y, A, x), src/expansion.jl:121, for A = -Laplacian + V(x) and
// its kin, with NOTHING stored per non-zero.  The grid shape gives the boundary rows by index arithmetic, the taps travel in the
// kernel arguments, the only per-row datum is the diagonal entry centre + potential[r] (formed once on the host at upload, by the
// code that the host matrix runs).  This file: what every grid kernel shares, then the constant-coefficient operators (k_grid: 3-, 5-
// or 7-point stencil with open or periodic boundaries, ks_operator_grid / ks_operator_grid_periodic; k_grid_star: star stencils of
// radius 2, 3, 4, ks_operator_grid_star; k_grid_star_per: the same with periodic axes, ks_operator_grid_star_periodic).  ks_grid_var.hpp: the variable-coefficient operator (k_grid_var; open or periodic boundaries).
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_tridiag.hpp.
//
// An operator IS the matrix its ks_host_grid_* entry returns: the kernel rounds every product on its own and adds the products of a
// row to +0.0 in ascending column order (a tap whose neighbour lies outside the grid is skipped), so y carries the bits every stored
// layout of that matrix gives.
//
// The scheme, for halo depth R (the stencil's radius).  A workgroup of 256 threads owns an in-plane tile of TX x TY points
// (GridTile: four points per thread, or two) and walks up a range of z-planes.  Per plane every thread keeps its own points of the
// planes z - R ... z + R in registers (the +-z taps never touch memory a second time) and a further plane in flight; the points of
// plane z go into an LDS tile together with the tile's halo, R cells deep on each side (2 R (TX + TY) cells, dealt to the threads
// and loaded two planes ahead; corners are never read), from which the +-x and +-y taps are read.  Two LDS tiles alternate: one
// barrier per plane.  Work items are (z-range, tile), z-range major, dealt to the XCDs in contiguous runs (xcd_remap) so that
// neighbouring tiles meet in one L2.  Every access is one element wide (8 bytes in Float64): a row starts at r = nx (...), for odd
// nx not 16-byte aligned, and nothing here depends on it.
// Compulsory traffic: x read once, the diagonal read once, y written once -- 24 bytes per row in Float64 (16 without a potential),
// twice that in ComplexF64; on top of it the halo of a tile (R 2 (TX + TY) / (TX TY) of x: R x 12.5 % for 32 x 32) and the R planes
// a z-range reads beyond each end, 2 R / zc of x, which neighbouring workgroups of the same XCD bring into its L2.  RULE for the
// z-ranges (grid::plan): at least kGridMinZ * R = 8 R planes each, so that the plane re-read stays at most 25 %.
// Every kernel argument `shifted`: bit 0 -- y = sigma (A x - theta x), the Newton step of the s-step expansion (as k_spmv_stencil2
// stores it), bit 1 -- cacheable instead of streaming stores, bit 4 -- the tail of a Clenshaw step (GridTail; the launches pick the
// kernel's TAIL instantiation by it).  diag == nullptr: no potential, the diagonal entry is the centre tap.
// st: a breakdown of the batch ends the kernel at once.
// Shared by the three kernels, below: the geometry at the head of the arguments (GridGeom), the tiles (GridTile, GridLds), the
// work-item decode (grid_item), the owned points and their neighbour flags (grid_owned, grid_neighbours), the diagonal load
// (grid_ldd) and the end of a row (GridStore).  Written out in each kernel: the guarded plane load `ldx` and the assignment of halo
// cells to threads -- as a function either one changes the order of the Float64 kernels' instructions (DESIGN).
//
// k_grid (R = 1).  Rows are summed in the slots -z, -y, -x, centre, +x, +y, +z.  Planes z - 1, z, z + 1 in registers and z + 2 in
// flight; one halo cell per thread.  The z-loop is unrolled by four so that the four register sets rotate by name: nothing waits
// for a load before the step that uses it.  Tiles: 32 x 32, and 1024 x 1 for ny == 1 (1-D grids, and nx x 1 x nz).
//
// k_grid_star (R = 2, 3, 4: central differences of order 4, 6, 8; open boundaries).  Up to two halo cells per thread, and the
// existence of the +-x / +-y taps of every distance d is one bit per tap in one register per point, computed once per thread.  A
// row is summed in the 6 R + 1 slots -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y,
// +1 z ... +R z; an absent tap is not multiplied.  The 2 R + 2 register sets rotate by MOVES at the end of a plane, not by name:
// unrolled by 2 R + 2 the z-loop of R = 4 is 180 KB of code and ran at 264 us per product on 216^3 against 111 us in this form
// (profiles/grid_operator.txt); the plane in flight lands in a set of its own and is waited for after the plane's arithmetic.  The
// z-loop is unrolled by two (the LDS tiles, the halo and the diagonal registers alternate).  The 4 R in-plane neighbours of a point
// are read from the tile before any of them is used, and a wave all of whose lanes have the R taps of a direction -- every wave
// but those at an edge of the grid -- adds them in straight-line code; only the other waves test tap by tap.
// Tiles: Float64 32 x 32 and 1024 x 1 at every radius; ComplexF64 the same at R = 2, 32 x 16 and 512 x 1 (two points per thread)
// at R = 3 and 4, where four points of ten planes would take the kernel to one wave per SIMD (DESIGN).
//
// k_grid_star_per (R = 2, 3, 4 with periodic axes): a sibling of k_grid_star with the same march and the same tiles; its additions
// are described at the kernel.
#pragma once

namespace ksd {

constexpr int kGridMinZ = 8;       // planes per z-range, at least, per unit of radius
constexpr int kGridWant = 1024;    // work items per launch, at most, while z can be split: what an MI355X holds at once (4 per CU)

// what every grid kernel's argument struct starts with
struct GridGeom {
  int nx = 1, ny = 1, nz = 1;
  int ntx = 1, nty = 1;   // tiles along x and y
  int zc = 1;             // planes per z-range
};
// k_grid, k_grid_var (whose six off-diagonal slots hold the HALF taps)
template <class T> struct GridDev : GridGeom {
  T tap[7] = {};          // -z, -y, -x, centre, +x, +y, +z
};
// ... with periodic axes: the entries of the links that cross the cell boundary and the axes that wrap
template <class T> struct GridPerDev : GridDev<T> {
  T wrap[6] = {};         // -z, -y, -x, +x, +y, +z (k_grid_var: the HALF wrap values)
  int px = 0, py = 0, pz = 0;
};
template <class T, int R> struct GridStarDev : GridGeom {
  T tap[6 * R + 1] = {};  // -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z
};
// ... with periodic axes: the entries of the links of every distance where they cross the cell boundary, in the slots of the taps
// with the centre left out (grid_wslot), and the axes that wrap
template <class T, int R> struct GridStarPerDev : GridStarDev<T, R> {
  T wrap[6 * R] = {};     // -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, +1 x ... +R x, +1 y ... +R y, +1 z ... +R z
  int px = 0, py = 0, pz = 0;
};
// the place in `wrap` of the link whose tap stands in slot k of the 6 R + 1
template <int R> constexpr int grid_wslot(int k) { return k < 3 * R ? k : k - 1; }
static_assert(sizeof(GridDev<double>) == 24 + 7 * 8 && sizeof(GridDev<cd>) == 24 + 7 * 16 && sizeof(GridStarDev<cd, 2>) == 24 + 13 * 16,
              "kernel arguments: six ints, then the taps with nothing between");
static_assert(sizeof(GridStarPerDev<cd, 4>) <= 24 + 25 * 16 + 24 * 16 + 16, "kernel arguments of the periodic star kernel: below 1 KB");
// The wrap values of the kernel's FIRST argument g (a GridStarPerDev<T, R>) as ONE 8-byte word per lane of every wave -- 6 R words
// in Float64, 12 R in ComplexF64, lane j holds word j -- read back by lane number (grid_wrap_at, a compile-time lane) where a link
// wraps.  Named as g.wrap[k] the compiler loads all 6 R values ahead of the z-loop, next to the taps they do not fit the scalar
// registers, and every wave -- also those that never wrap -- pays for moving them to vector lanes and back; loaded from the argument
// segment inside the branches of the waves at a periodic edge, each group waits for scalar memory once per point and plane
// (DESIGN).  This costs two vector registers and two v_readlane per use.  The word is loaded through the argument segment's
// address: g.wrap[lane] would make the compiler copy the struct to scratch.
using GridArgWord = const double __attribute__((address_space(4)));
template <class T, int R> __device__ __forceinline__ double grid_wrap_lane(int lane) {
  static_assert(sizeof(GridStarPerDev<T, R>) == sizeof(GridStarDev<T, R>) + 6 * R * sizeof(T) + 16 && sizeof(GridStarDev<T, R>) % 8 == 0,
                "wrap follows the taps with nothing between");
  constexpr int NW = 6 * R * (int)(sizeof(T) / 8);
  static_assert(NW <= 64, "one word per lane");
#if defined(__HIP_DEVICE_COMPILE__)
  using Byte = const char __attribute__((address_space(4)));
  GridArgWord* w = (GridArgWord*)((Byte*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(GridStarDev<T, R>));
  return lane < NW ? w[lane] : 0.0;
#else
  return 0.0;
#endif
}
__device__ __forceinline__ double grid_lane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// s plus the product c v of a link that exists or not (k).  Float64: the product where the link exists, else -0.0, is added --
// s + (-0.0) has the bits of s for every s (+-0, NaN and Inf included), so this IS skipping an absent link, in straight-line code
// where the sums of a thread's points overlap (the product of an absent link is formed and dropped: it never reaches s).
// ComplexF64: a branch -- the straight-line form takes k_grid_star_per<ComplexF64, 32, 16, 4> to 255 + 6 registers and one wave per
// SIMD (DESIGN).
__device__ __forceinline__ double grid_add_if(double s, bool k, double c, double v) {
  const double p = mul_nc(c, v);   // (formed ahead of the choice: inside it the compiler branches)
  return add_(s, k ? p : -0.0);
}
__device__ __forceinline__ cd grid_add_if(cd s, bool k, cd c, cd v) { return k ? add_(s, mul_nc(c, v)) : s; }
// wrap value k of the words in wl
template <class T> __device__ __forceinline__ T grid_wrap_at(double wl, int k) {
  if constexpr (sizeof(T) == 8) return grid_lane_f64(wl, k);
  else return T{grid_lane_f64(wl, 2 * k), grid_lane_f64(wl, 2 * k + 1)};
}

// The in-plane tiles: TX x TY for ny > 1, WX x 1 for ny == 1.  Four points per thread; two (HALF) where four would cost the second
// wave per SIMD: ComplexF64 with the planes of R >= 3 or with a coefficient beside x in registers and LDS (DESIGN).
template <bool HALF> struct GridTile {
  static constexpr int TX = 32, TY = HALF ? 16 : 32;
  static constexpr int WX = HALF ? 512 : 1024;
};
constexpr bool grid_half(size_t elem, int R, bool var) { return elem == 16 && (R >= 3 || var); }
template <class T, int R = 1, bool VAR = false> using GridTileOf = GridTile<grid_half(sizeof(T), R, VAR)>;
// k_grid_star_per has a tile choice of its own (its registers are not those of k_grid_star)
constexpr bool grid_star_per_half(size_t elem, int R) { return grid_half(elem, R, false); }

// the LDS tile of a TX x TY tile with its halo of depth R
template <int TX, int TY, int R> struct GridLds {
  static constexpr int PPT = TX * TY / kBlock;             // points per thread
  static constexpr int HY = TY > 1 ? R : 0;                // halo rows in y on each side (a one-row tile: ny == 1, no y neighbours)
  static constexpr int LW = TX + 2 * R, LH = TY + 2 * HY;  // extents
  static constexpr int NHALO = 2 * R * TY + 2 * HY * TX;   // halo cells (corners are never read)
  static constexpr int NH = (NHALO + kBlock - 1) / kBlock; // ... per thread, at most
  static_assert(TX * TY % kBlock == 0 && R >= 1 && R <= 4 && NH <= 2, "whole points per thread, at most two halo cells");
};

// the work item of this workgroup: its tile's first point, its planes [za, zb), and the plane stride
struct GridItem {
  int x0, y0, za, zb;
  int64_t P;
};
template <int TX, int TY> __device__ __forceinline__ GridItem grid_item(const GridGeom& g) {
  const int ntiles = g.ntx * g.nty;
  const int item = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int zr = item / ntiles, t2 = item - zr * ntiles;
  const int tyi = t2 / g.ntx, txi = t2 - tyi * g.ntx;
  const int za = zr * g.zc;
  return {txi * TX, tyi * TY, za, min(g.nz, za + g.zc), (int64_t)g.nx * g.ny};
}

// owned point p of the tile (this thread's k-th: p = tid + k kBlock): grid coordinates, inside the grid, in-plane offset, place in
// the LDS tile
template <int TX, int TY, int R>
__device__ __forceinline__ void grid_owned(const GridGeom& g, const GridItem& it, int p, int& gx, int& gy, bool& in, int64_t& off, int& li) {
  using L = GridLds<TX, TY, R>;
  const int lx = p % TX, ly = p / TX;
  gx = it.x0 + lx;
  gy = it.y0 + ly;
  in = gx < g.nx && gy < g.ny;
  off = (int64_t)gy * g.nx + gx;
  li = (ly + L::HY) * L::LW + lx + R;
}
// ... has a -x / +x / -y / +y neighbour (R = 1)
__device__ __forceinline__ void grid_neighbours(const GridGeom& g, const int& gx, const int& gy, const bool& in, bool& hxm, bool& hxp, bool& hym,
                                                bool& hyp) {
  hxm = in && gx > 0;
  hxp = in && gx + 1 < g.nx;
  hym = in && gy > 0;
  hyp = in && gy + 1 < g.ny;
}

// Element o of plane z of the diagonal.  Like every load of these kernels: a point outside the grid or the planes is never loaded,
// zero stands in and is never multiplied into a stored row.
template <class T> __device__ __forceinline__ T grid_ldd(const T* diag, const GridGeom& g, int64_t P, int z, int64_t o, bool ok) {
  return ok && z < g.nz ? ld_val(diag + ((int64_t)z * P + o), true) : zero_of(T{});
}

// the tail of a Clenshaw step (ks_operator::apply_clenshaw), the last argument of every grid kernel; read only by the
// instantiations with TAIL, which the launches pick where bit 4 of `shifted` is set
template <class T> struct GridTail {
  const T* w = nullptr;    // null: no such term
  const T* x0 = nullptr;   // null: no such term
  double gamma = 0.0;
};
// the end of a row: the fused Newton step, then -- TAIL -- the tail of a Clenshaw step, y = (t - w) + gamma x0 with w and x0 read
// at the row's own position, then the store (cacheable or streaming); tail and store if the point lies inside the grid.
// TAIL is a template parameter of every kernel: as a runtime branch the two loads per point cost the plain product 12 to 28
// vector registers and 19 of the 48 instantiations an occupancy step (DESIGN); without TAIL the kernels are the ones they were.
template <class T, bool TAIL = false> struct GridStore {
  T* const y;
  const int64_t P;
  const int shifted;
  const T theta;
  const double sigma;
  const GridTail<T> tail;
  const bool plain = (shifted & 2) != 0;
  // s: the row's sum, xc: its own point, at offset o of plane z
  __device__ __forceinline__ void operator()(int z, int64_t o, bool in, T s, const T& xc) const {
    if (shifted & 1) s = scl(sub_s(s, mul_(theta, xc)), sigma);
    if (in) {
      if constexpr (TAIL) s = clenshaw_tail(s, tail.w, tail.x0, tail.gamma, (int64_t)z * P + o);
      T* dst = y + ((int64_t)z * P + o);
      if (plain) *dst = s;
      else st_elem_nt(dst, s);
    }
  }
};

// G = GridPerDev<T>: periodic axes.  A row is summed in the 13-slot order of include/kschur.h (ix), a wrap link at ANOTHER place than
// the interior link of its direction: the column of a +wrap link lies below every other column of its axis, that of a -wrap link
// above.  x and y: a halo cell one step outside the grid loads from the other end of its line.  When the last tile is partial the
// +x neighbour of gx = nx - 1 is no halo cell but the LDS slot of the OWNED point gx = nx, which then holds x[0] of the line
// (ldk, loff; likewise gy = ny); such a point is still never stored, and no row without that neighbour reads it.  z: plane -1 is
// plane nz - 1, plane nz is plane 0 (only the first and the last z-range meet them).
template <class T, int TX, int TY, class G, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid(const G g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y, const DevState* __restrict__ st,
           int shifted, T theta, double sigma, const GridTail<T> tail) {
  if (st && st->breakdown >= 0) return;
  constexpr bool PER = !std::is_same<G, GridDev<T>>::value;
  using L = GridLds<TX, TY, 1>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW;
  static_assert(L::NH == 1, "at most one halo cell per thread");
  __shared__ T tile[2][L::LH * LW];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT], hxm[PPT], hxp[PPT], hym[PPT], hyp[PPT];   // inside the grid; has a -x / +x / -y / +y neighbour
  // periodic: the point is loaded (in the grid, or the wrap image one step beyond it) from loff; its -x / +x / -y / +y link wraps
  bool ldk[PPT], wxm[PPT], wxp[PPT], wym[PPT], wyp[PPT];
  int64_t loff[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, 1>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
    grid_neighbours(g, gx, gy, in[k], hxm[k], hxp[k], hym[k], hyp[k]);
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
  if (tid < L::NHALO) {
    int hx, hy;
    if (tid < TY) { hx = -1; hy = tid; }
    else if (tid < 2 * TY) { hx = TX; hy = tid - TY; }
    else if (tid < 2 * TY + TX) { hx = tid - 2 * TY; hy = -1; }
    else { hx = tid - 2 * TY - TX; hy = TY; }
    int gx = it.x0 + hx, gy = it.y0 + hy;
    if constexpr (PER) {
      if (g.px) gx = gx == -1 ? g.nx - 1 : gx == g.nx ? 0 : gx;
      if (g.py) gy = gy == -1 ? g.ny - 1 : gy == g.ny ? 0 : gy;
    }
    hin = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
    hoff = (int64_t)gy * g.nx + gx;
    hli = (hy + HY) * LW + hx + 1;
  }
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
    dr[0][k] = diag ? grid_ldd(diag, g, P, za, off[k], in[k]) : g.tap[3];
    dr[1][k] = dr[0][k];
  }
  // one plane: xm / xc / xp = planes z - 1 / z / z + 1, xn receives plane z + 2; hw = the halo cell of plane z, then of z + 2
  auto step = [&](int z, const T (&xm)[PPT], const T (&xc)[PPT], const T (&xp)[PPT], T (&xn)[PPT], T& hw, const T (&dc)[PPT], T (&dn)[PPT],
                  T* __restrict__ tl) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) tl[li[k]] = xc[k];
    if (tid < L::NHALO) tl[hli] = hw;
    hw = ldx(z + 2, hoff, hin && z + 2 < zb);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldo(z + 2, k, z + 2 <= zb);   // (plane zb is the +z tap of the range's last plane)
      if (diag) dn[k] = grid_ldd(diag, g, P, z + 1, off[k], in[k] && z + 1 < zb);
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
      store(z, off[k], in[k], s, xc[k]);
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
// steps J, J + 1, ..., N - 1 of one turn of the unrolled z-loop, each with its number as a compile-time constant (its parity
// picks the LDS tile and the halo and diagonal registers); stops after the range's last plane (uniform over the workgroup: the
// barriers match)
template <int J, int N, class F> __device__ __forceinline__ void grid_star_steps(int z, int zb, F& f) {
  f(z + J, std::integral_constant<int, J>{});
  if constexpr (J + 1 < N) {
    if (z + J + 1 < zb) grid_star_steps<J + 1, N>(z, zb, f);
  }
}

template <class T, int TX, int TY, int R, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid_star(const GridStarDev<T, R> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
                const DevState* __restrict__ st, int shifted, T theta, double sigma, const GridTail<T> tail) {
  if (st && st->breakdown >= 0) return;
  using L = GridLds<TX, TY, R>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW, NH = L::NH;
  constexpr int N = 2 * R + 2;                           // register sets: planes z - R ... z + R and the one in flight
  static_assert(R >= 2, "radius 1 is k_grid");
  __shared__ T tile[2][L::LH * LW];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT];       // inside the grid
  unsigned msk[PPT];  // bit d - 1 / 4 + d - 1 / 8 + d - 1 / 12 + d - 1: has a neighbour at -d x / +d x / -d y / +d y
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, R>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
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
    if (c < L::NHALO) {
      int hx, hy;
      if (c < R * TY) { hx = -1 - c / TY; hy = c % TY; }
      else if (c < 2 * R * TY) { hx = TX + (c - R * TY) / TY; hy = (c - R * TY) % TY; }
      else if (c < 2 * R * TY + R * TX) { hx = (c - 2 * R * TY) % TX; hy = -1 - (c - 2 * R * TY) / TX; }
      else { hx = (c - 2 * R * TY - R * TX) % TX; hy = TY + (c - 2 * R * TY - R * TX) / TX; }
      const int gx = it.x0 + hx, gy = it.y0 + hy;
      hin[j] = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
      hoff[j] = (int64_t)gy * g.nx + gx;
      hli[j] = (hy + HY) * LW + hx + R;
    }
  }
  auto ldx = [&](int z, int64_t o, bool ok) { return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };

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
    dr[0][k] = diag ? grid_ldd(diag, g, P, za, off[k], in[k]) : g.tap[3 * R];
    dr[1][k] = dr[0][k];
  }
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
      if (tid + j * kBlock < L::NHALO) tl[hli[j]] = hr[B][j];
      hr[B][j] = ldx(z + 2, hoff[j], hin[j] && z + 2 < zb);
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(z + R + 1, off[k], in[k] && z + 1 < zb);   // (the +R z tap of the next plane; beyond zb for the range's last R)
      if (diag) dr[1 - B][k] = grid_ldd(diag, g, P, z + 1, off[k], in[k] && z + 1 < zb);
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
      store(z, off[k], in[k], s, xc[k]);
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
#pragma unroll
      for (int q = 0; q + 1 < N; ++q) xr[q][k] = xr[q + 1][k];
    }
  };
  for (int z = za; z < zb; z += 2) grid_star_steps<0, 2>(z, zb, step);
}

// ------------------------------------------------------------------------------------- radius 2, 3, 4 with periodic axes
// k_grid_star_per: the march of k_grid_star (2 R + 2 register sets rotated by moves, two LDS tiles, one barrier per plane) on a
// grid some of whose axes wrap (g.px, g.py, g.pz; extent >= 2 R + 1 each, so one wrap suffices everywhere).  A row is summed in
// the order of include/kschur.h (x-b): per axis the +d links that wrap stand BEFORE the interior -d links, the -d links that wrap
// AFTER the interior +d links, each with the wrap value of its direction and distance.
// x and y: every LDS cell, owned or halo, whose coordinate c lies in [m, m + R) on a periodic axis is loaded from c - m, one in
// [-R, 0) from c + m (the periodic k_grid's ldk / loff, R deep).  Beyond a partial last tile up to R slots of OWNED points hold
// such images: they are loaded, written to the tile and never stored (`off` is the offset they LOAD from; it is the point's own
// wherever in[] holds, and only there it serves the diagonal and the store).  A cell beyond the grid on both axes is read by no row.
// Masks: bits 0 ... 15 as in k_grid_star (the interior tap exists), bits 16 ... 31 in the same layout: the tap wraps -- at R = 4
// one full register per point.  A wave all of whose lanes have the R interior taps of a direction has no lane that wraps in it:
// it skips the wrapped group with one uniform test and adds the interior group in straight-line code; only the other waves take
// every slot link by link (grid_add_if).  The wrap values travel in the kernel arguments and stand in the lanes of one vector
// register pair, read by compile-time lane number (grid_wrap_lane).
// z: the plane index wraps in the plane load (uniform); the planes within R of either end of a periodic z add the wrapped z groups,
// under a uniform test, from the register sets that hold those planes already.
template <class T, int TX, int TY, int R, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid_star_per(const GridStarPerDev<T, R> g, const T* __restrict__ x, const T* __restrict__ diag, T* __restrict__ y,
                    const DevState* __restrict__ st, int shifted, T theta, double sigma, const GridTail<T> tail) {
  if (st && st->breakdown >= 0) return;
  using L = GridLds<TX, TY, R>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW, NH = L::NH;
  constexpr int N = 2 * R + 2;                           // register sets: planes z - R ... z + R and the one in flight
  constexpr unsigned FULL = (1u << R) - 1u;
  static_assert(R >= 2, "radius 1 is k_grid");
  __shared__ T tile[2][L::LH * LW];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};
  const double wl = grid_wrap_lane<T, R>(tid & 63);   // the wrap values, a word per lane
  // coordinate c of an LDS cell along an axis of extent m: where it is loaded from (outside [0, m): not at all)
  auto img = [](int c, int m, int per) { return !per ? c : c < 0 ? c + m : c >= m && c < m + R ? c - m : c; };

  int64_t off[PPT];   // in-plane offset the owned points are loaded from: their own, or that of the point they are the image of
  int li[PPT];        // ... and their place in the LDS tile
  bool in[PPT];       // inside the grid (a row of its own: diagonal, store)
  bool ldk[PPT];      // loaded: inside the grid, or an image
  unsigned msk[PPT];  // bit d - 1 / 4 + d - 1 / 8 + d - 1 / 12 + d - 1: has an interior neighbour at -d x / +d x / -d y / +d y;
                      // 16 more: that link wraps
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, R>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
    msk[k] = 0u;
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      if (in[k] && gx >= d) msk[k] |= 1u << (d - 1);
      else if (in[k] && g.px) msk[k] |= 1u << (16 + d - 1);
      if (in[k] && gx + d < g.nx) msk[k] |= 1u << (4 + d - 1);
      else if (in[k] && g.px) msk[k] |= 1u << (20 + d - 1);
      if (in[k] && gy >= d) msk[k] |= 1u << (8 + d - 1);
      else if (in[k] && g.py) msk[k] |= 1u << (24 + d - 1);
      if (in[k] && gy + d < g.ny) msk[k] |= 1u << (12 + d - 1);
      else if (in[k] && g.py) msk[k] |= 1u << (28 + d - 1);
    }
    // (a point outside the grid has no row: with every interior bit set and no wrap bit it keeps no wave from the straight-line sums)
    if (!in[k]) msk[k] = 0xffffu;
    const int sx = img(gx, g.nx, g.px), sy = img(gy, g.ny, g.py);
    ldk[k] = sx < g.nx && sy < g.ny;
    off[k] = (int64_t)sy * g.nx + sx;
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
    if (c < L::NHALO) {
      int hx, hy;
      if (c < R * TY) { hx = -1 - c / TY; hy = c % TY; }
      else if (c < 2 * R * TY) { hx = TX + (c - R * TY) / TY; hy = (c - R * TY) % TY; }
      else if (c < 2 * R * TY + R * TX) { hx = (c - 2 * R * TY) % TX; hy = -1 - (c - 2 * R * TY) / TX; }
      else { hx = (c - 2 * R * TY - R * TX) % TX; hy = TY + (c - 2 * R * TY - R * TX) / TX; }
      const int gx = img(it.x0 + hx, g.nx, g.px), gy = img(it.y0 + hy, g.ny, g.py);
      hin[j] = gx >= 0 && gx < g.nx && gy >= 0 && gy < g.ny;
      hoff[j] = (int64_t)gy * g.nx + gx;
      hli[j] = (hy + HY) * LW + hx + R;
    }
  }
  // plane z of a periodic z: planes -R ... -1 are the last R, planes nz ... nz + R - 1 the first (no load reaches further)
  auto ldx = [&](int z, int64_t o, bool ok) {
    if (g.pz) z = z < 0 ? z + g.nz : z >= g.nz ? z - g.nz : z;
    return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{});
  };

  // Register sets, halo and diagonal registers: as in k_grid_star (with a periodic z set R + d holds plane z + d modulo nz).
  T xr[N][PPT], dr[2][PPT], hr[2][NH];
#pragma unroll
  for (int j = 0; j < NH; ++j) {
    hr[0][j] = ldx(za, hoff[j], hin[j]);
    hr[1][j] = ldx(za + 1, hoff[j], hin[j] && za + 1 < zb);
  }
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
#pragma unroll
    for (int s = 0; s <= 2 * R; ++s) xr[s][k] = ldx(za - R + s, off[k], ldk[k]);
    xr[N - 1][k] = zero_of(T{});
    dr[0][k] = diag ? grid_ldd(diag, g, P, za, off[k], in[k]) : g.tap[3 * R];
    dr[1][k] = dr[0][k];
  }
  // the R interior taps of one direction, as in k_grid_star
  auto grp = [&](T s, unsigned gm, auto basec, auto sgnc, const T(&v)[R]) {
    constexpr int BASE = decltype(basec)::value, SGN = decltype(sgnc)::value;
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
        s = grid_add_if(s, gm >> (d - 1) & 1u, g.tap[BASE + SGN * d], v[d - 1]);
      }
    }
    return s;
  };
  // ... and its links that wrap (bit d - 1 of wm), in the same order of d, with the wrap values: tap by tap
  auto grw = [&](T s, unsigned wm, auto basec, auto sgnc, const T(&v)[R]) {
    constexpr int BASE = decltype(basec)::value, SGN = decltype(sgnc)::value;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int d = SGN < 0 ? R - i : i + 1;
      s = grid_add_if(s, wm >> (d - 1) & 1u, grid_wrap_at<T>(wl, grid_wslot<R>(BASE + SGN * d)), v[d - 1]);
    }
    return s;
  };
  // true in the waves that may hold a lane whose links of this direction wrap: those without all R interior taps, on a periodic axis
  auto edge = [&](int per, unsigned gm) { return per && !__all((gm & FULL) == FULL); };
  auto step = [&](int z, auto jc) {
    constexpr int B = decltype(jc)::value & 1;
    T* __restrict__ tl = tile[B];
    const T(&xc)[PPT] = xr[R];
    T(&xn)[PPT] = xr[N - 1];
#pragma unroll
    for (int k = 0; k < PPT; ++k) tl[li[k]] = xc[k];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      if (tid + j * kBlock < L::NHALO) tl[hli[j]] = hr[B][j];
      hr[B][j] = ldx(z + 2, hoff[j], hin[j] && z + 2 < zb);
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(z + R + 1, off[k], ldk[k] && z + 1 < zb);   // (the +R z tap of the next plane; beyond zb for the range's last R)
      if (diag) dr[1 - B][k] = grid_ldd(diag, g, P, z + 1, off[k], in[k] && z + 1 < zb);
    }
    __syncthreads();
    // the z taps as masks of the same kind (uniform): -d z is interior for d <= z, +d z for d <= nz - 1 - z; the others wrap
    const unsigned zmm = (1u << min(R, z)) - 1u, zmp = (1u << min(R, g.nz - 1 - z)) - 1u;
    const unsigned wzm = g.pz ? FULL & ~zmm : 0u, wzp = g.pz ? FULL & ~zmp : 0u;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      T s = zero_of(T{});
      unsigned m = msk[k];
      asm volatile("" : "+v"(m));   // (as in k_grid_star: the 8 R tests per point stay on this one register)
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
      using BZ = std::integral_constant<int, R>;
      using BY = std::integral_constant<int, 2 * R>;
      using BX = std::integral_constant<int, 3 * R>;
      using CY = std::integral_constant<int, 4 * R>;
      using CZ = std::integral_constant<int, 5 * R>;
      if (wzp) s = grw(s, wzp, CZ{}, Q{}, vzp);
      s = grp(s, zmm, BZ{}, M{}, vzm);
      if constexpr (HY > 0) {
        if (edge(g.py, m >> 12)) s = grw(s, m >> 28, CY{}, Q{}, vyp);
        s = grp(s, m >> 8, BY{}, M{}, vym);
      }
      if (edge(g.px, m >> 4)) s = grw(s, m >> 20, BX{}, Q{}, vxp);
      s = grp(s, m, BX{}, M{}, vxm);
      s = add_(s, mul_nc(dr[B][k], xc[k]));
      s = grp(s, m >> 4, BX{}, Q{}, vxp);
      if (edge(g.px, m)) s = grw(s, m >> 16, BX{}, M{}, vxm);
      if constexpr (HY > 0) {
        s = grp(s, m >> 12, CY{}, Q{}, vyp);
        if (edge(g.py, m >> 8)) s = grw(s, m >> 24, BY{}, M{}, vym);
      }
      s = grp(s, zmp, CZ{}, Q{}, vzp);
      if (wzm) s = grw(s, wzm, BZ{}, M{}, vzm);
      store(z, off[k], in[k], s, xc[k]);
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

// ... of a star stencil of radius R (ks_host_grid_matrix_star_periodic, include/kschur.h (x-b)): wrap = 2 ndim R values in the order of
// the taps without the centre, null = the taps themselves; a periodic axis needs 2 R + 1 points.  s.nnz: the 2 d links of distance d
// per line that truncation leaves out are added.
template <class H> struct WrapStar {
  bool per[3] = {false, false, false};   // x, y, z
  H w[24] = {};                          // the 6 R slots -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, +1 x ... +R x, +1 y ..., +1 z ...
                                         // (an axis that does not wrap, a missing dimension: zero, never used)
  bool any() const { return per[0] || per[1] || per[2]; }
};
template <class H>
WrapStar<H> check_wrap_star(const std::string& who, Shape& s, int ndim, int R, const void* taps_v, const int* periodic, const void* wrap_v) {
  WrapStar<H> W;
  if (!periodic) return W;
  static const char* const axis[3] = {"x", "y", "z"};
  const int64_t ext[3] = {s.nx, s.ny, s.nz};
  const H* t = static_cast<const H*>(taps_v);
  const H* w = static_cast<const H*>(wrap_v);
  const int c = ndim * R;   // the centre among the taps; wrap has it left out
  for (int a = 0; a < ndim; ++a) {
    if (!periodic[a]) continue;
    KS_REQUIRE(ext[a] >= 2 * R + 1, KS_ERR_ARGUMENT,
               who + ": periodic axis " + std::to_string(a) + " (" + axis[a] + ") has extent " + std::to_string(ext[a]) + " at radius " +
                   std::to_string(R) + " (a periodic axis needs at least 2 radius + 1 = " + std::to_string(2 * R + 1) +
                   " points: below that two links of a row coincide or a link is a self-link)");
    W.per[a] = true;
    for (int d = 1; d <= R; ++d) {
      // axis a, distance d: its - link is entry c - a R - d of wrap (and of the taps), its + link entry c + a R + d - 1 (tap c + a R + d)
      const int km = c - a * R - d, kp = c + a * R + d - 1;
      const H vm = w ? w[km] : t[km], vp = w ? w[kp] : t[kp + 1];
      KS_REQUIRE(finite_(vm), KS_ERR_ARGUMENT,
                 who + ": wrap value " + std::to_string(km) + " (-" + std::to_string(d) + " " + axis[a] + ") is not finite");
      KS_REQUIRE(finite_(vp), KS_ERR_ARGUMENT,
                 who + ": wrap value " + std::to_string(kp) + " (+" + std::to_string(d) + " " + axis[a] + ") is not finite");
      W.w[(3 - a) * R - d] = vm;
      W.w[(3 + a) * R + d - 1] = vp;
      s.nnz += 2 * d * (s.n / ext[a]);
    }
  }
  return W;
}

// the 2 ndim + 1 taps in the seven slots -z, -y, -x, centre, +x, +y, +z (slots of a missing dimension: zero, never used)
template <class H> void seven_taps(int ndim, const H* t, H (&out)[7]) {
  for (H& o : out) o = H(0);
  for (int k = 0; k < 2 * ndim + 1; ++k) out[3 - ndim + k] = t[k];
}
// the 2 ndim R + 1 taps of a star stencil in the 6 R + 1 slots -R z ... -1 z, -R y ... -1 y, -R x ... -1 x, centre, +1 x ... +R x,
// +1 y ... +R y, +1 z ... +R z (slots of a missing dimension: zero, never used)
template <class H> void star_taps(int ndim, int R, const H* t, H (&out)[25]) {
  for (H& o : out) o = H(0);
  for (int k = 0; k < 2 * ndim * R + 1; ++k) out[(3 - ndim) * R + k] = t[k];
}

// Every host matrix: 0-based CSR with ascending columns, the diagonal entry centre + potential[r] stored even where it is zero.
// nnz is always reported; the arrays are filled only when cap >= nnz.
template <class H>
void csr_begin(const std::string& who, const Shape& s, const int64_t* rowptr, const int32_t* colidx, const H* val, int64_t cap, int64_t* nnz) {
  if (nnz) *nnz = s.nnz;
  KS_REQUIRE(cap >= s.nnz, KS_ERR_ARGUMENT,
             who + ": cap = " + std::to_string(cap) + " is too small, the matrix has " + std::to_string(s.nnz) + " entries");
  KS_REQUIRE(rowptr && (s.nnz == 0 || (colidx && val)), KS_ERR_ARGUMENT, who + ": null output array");
}

// The rows of a radius-1 matrix.  link(k, r, c, wrapped) is the entry of the link from row r to column c in tap slot k; on a
// periodic axis (per: x, y, z) a row is a sub-sequence of the 13 slots of include/kschur.h (ix): the link of the last point of a
// line to the first (wrapped) has the lowest column of its axis, that of the first to the last the highest.
template <class H, class F>
void seven_slot_rows(const Shape& s, const bool (&per)[3], const H& centre, const H* pot, int64_t* rowptr, int32_t* colidx, H* val, F link) {
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        auto put = [&](int64_t c, const H& v) { colidx[q] = (int32_t)c; val[q] = v; ++q; };
        auto to = [&](int k, int64_t c, bool wrapped) { put(c, link(k, r, c, wrapped)); };
        if (per[2] && iz + 1 == s.nz) to(6, r - (s.nz - 1) * P, true);
        if (iz > 0) to(0, r - P, false);
        if (per[1] && iy + 1 == s.ny) to(5, r - (s.ny - 1) * s.nx, true);
        if (iy > 0) to(1, r - s.nx, false);
        if (per[0] && ix + 1 == s.nx) to(4, r - (s.nx - 1), true);
        if (ix > 0) to(2, r - 1, false);
        put(r, pot ? diag_add(centre, pot[r]) : centre);
        if (ix + 1 < s.nx) to(4, r + 1, false);
        if (per[0] && ix == 0) to(2, r + (s.nx - 1), true);
        if (iy + 1 < s.ny) to(5, r + s.nx, false);
        if (per[1] && iy == 0) to(1, r + (s.ny - 1) * s.nx, true);
        if (iz + 1 < s.nz) to(6, r + P, false);
        if (per[2] && iz == 0) to(0, r + (s.nz - 1) * P, true);
      }
  rowptr[s.n] = q;
}

// the matrix of ks_host_grid_matrix and ks_host_grid_matrix_periodic: the taps, and the wrap values for the links that cross
template <class H>
void host_matrix(const std::string& who, const Shape& s, int ndim, const H* taps, const H* pot, const Wrap<H>& W, int64_t* rowptr,
                 int32_t* colidx, H* val, int64_t cap, int64_t* nnz) {
  csr_begin(who, s, rowptr, colidx, val, cap, nnz);
  H t[7];
  seven_taps(ndim, taps, t);
  seven_slot_rows(s, W.per, t[3], pot, rowptr, colidx, val,
                  [&](int k, int64_t, int64_t, bool wrapped) { return wrapped ? W.w[k - (k > 3)] : t[k]; });
}

// The matrix that defines the star operator of radius R (ks_host_grid_matrix_star, ks_host_grid_matrix_star_periodic,
// include/kschur.h (x), (x-b)): a row is a sub-sequence of the 6 R + 1 slots and, on a periodic axis (W.per), of the wrapped links
// around them -- before the centre the +d links of an axis that wrap (the lowest columns of the axis) precede its -d links, after
// it the -d links that wrap (the highest) follow its +d links.
template <class H>
void host_matrix_star(const std::string& who, const Shape& s, int ndim, int R, const H* taps, const H* pot, const WrapStar<H>& W,
                      int64_t* rowptr, int32_t* colidx, H* val, int64_t cap, int64_t* nnz) {
  csr_begin(who, s, rowptr, colidx, val, cap, nnz);
  H t[25];
  star_taps(ndim, R, taps, t);
  const int64_t P = s.nx * s.ny;
  int64_t q = 0, r = 0;
  for (int64_t iz = 0; iz < s.nz; ++iz)
    for (int64_t iy = 0; iy < s.ny; ++iy)
      for (int64_t ix = 0; ix < s.nx; ++ix, ++r) {
        rowptr[r] = q;
        auto put = [&](int64_t c, const H& v) { colidx[q] = (int32_t)c; val[q] = v; ++q; };
        if (W.per[2]) for (int d = 1; d <= R; ++d) if (iz + d >= s.nz) put(r + (d - s.nz) * P, W.w[5 * R + d - 1]);
        for (int d = R; d >= 1; --d) if (iz >= d) put(r - d * P, t[R - d]);
        if (W.per[1]) for (int d = 1; d <= R; ++d) if (iy + d >= s.ny) put(r + (d - s.ny) * s.nx, W.w[4 * R + d - 1]);
        for (int d = R; d >= 1; --d) if (iy >= d) put(r - d * s.nx, t[2 * R - d]);
        if (W.per[0]) for (int d = 1; d <= R; ++d) if (ix + d >= s.nx) put(r + (d - s.nx), W.w[3 * R + d - 1]);
        for (int d = R; d >= 1; --d) if (ix >= d) put(r - d, t[3 * R - d]);
        put(r, pot ? diag_add(t[3 * R], pot[r]) : t[3 * R]);
        for (int d = 1; d <= R; ++d) if (ix + d < s.nx) put(r + d, t[3 * R + d]);
        if (W.per[0]) for (int d = R; d >= 1; --d) if (ix < d) put(r + (s.nx - d), W.w[3 * R - d]);
        for (int d = 1; d <= R; ++d) if (iy + d < s.ny) put(r + d * s.nx, t[4 * R + d]);
        if (W.per[1]) for (int d = R; d >= 1; --d) if (iy < d) put(r + (s.ny - d) * s.nx, W.w[2 * R - d]);
        for (int d = 1; d <= R; ++d) if (iz + d < s.nz) put(r + d * P, t[5 * R + d]);
        if (W.per[2]) for (int d = R; d >= 1; --d) if (iz < d) put(r + (s.nz - d) * P, W.w[R - d]);
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
    host_matrix_star<H>(who, s, ndim, radius, static_cast<const H*>(taps), static_cast<const H*>(pot), WrapStar<H>{}, rowptr, colidx,
                        static_cast<H*>(val), cap, nnz);
}

// ... and the periodic star entry point (radius 1: the arrays of ks_host_grid_matrix_periodic, no periodic axis: those of
// ks_host_grid_matrix_star, either by its code)
template <class H>
void host_matrix_star_periodic_entry(const std::string& who, int ndim, const int64_t* dims, int radius, const void* taps, const void* pot,
                                     const int* periodic, const void* wrap, int64_t* rowptr, int32_t* colidx, void* val, int64_t cap,
                                     int64_t* nnz) {
  Shape s = check<H>(who, ndim, dims, taps, pot, radius);
  if (radius == 1) {
    const Wrap<H> W = check_wrap<H>(who, s, ndim, taps, periodic, wrap);
    host_matrix<H>(who, s, ndim, static_cast<const H*>(taps), static_cast<const H*>(pot), W, rowptr, colidx, static_cast<H*>(val), cap, nnz);
  } else {
    const WrapStar<H> W = check_wrap_star<H>(who, s, ndim, radius, taps, periodic, wrap);
    host_matrix_star<H>(who, s, ndim, radius, static_cast<const H*>(taps), static_cast<const H*>(pot), W, rowptr, colidx,
                        static_cast<H*>(val), cap, nnz);
  }
}

// the tile the kernels of an operator are launched with (ksd::GridTile; var: with a coefficient)
struct Tile {
  int64_t tx, ty;
};
inline Tile tile_of(const Shape& s, bool half) {
  auto of = [&](auto tl) { return s.ny == 1 ? Tile{decltype(tl)::WX, 1} : Tile{decltype(tl)::TX, decltype(tl)::TY}; };
  return half ? of(ksd::GridTile<true>{}) : of(ksd::GridTile<false>{});
}
template <class D> Tile tile(const Shape& s, int radius, bool var) { return tile_of(s, ksd::grid_half(sizeof(D), radius, var)); }
// The launch shape: the tiles along x and y, and the z-ranges -- as many as fill kGridWant work items, of at least
// kGridMinZ * radius planes each.
struct Plan {
  ksd::GridGeom g;
  int nitems = 0;   // workgroups of a launch
};
inline Plan plan(const std::string& who, const Shape& s, Tile tile, int radius) {
  Plan p;
  p.g.nx = (int)s.nx; p.g.ny = (int)s.ny; p.g.nz = (int)s.nz;
  p.g.ntx = (int)((s.nx + tile.tx - 1) / tile.tx);
  p.g.nty = (int)((s.ny + tile.ty - 1) / tile.ty);
  const int64_t tiles = (int64_t)p.g.ntx * p.g.nty;
  const int64_t ranges = std::max<int64_t>(1, ksd::kGridWant / tiles);
  p.g.zc = (int)std::max<int64_t>(ksd::kGridMinZ * radius, (s.nz + ranges - 1) / ranges);
  const int64_t items = tiles * ((s.nz + p.g.zc - 1) / p.g.zc);
  KS_REQUIRE(items < (int64_t)2147483647, KS_ERR_ARGUMENT, who + ": too many tiles for one launch");
  p.nitems = (int)items;
  return p;
}

}  // namespace grid

// What the grid operators share: the diagonal, the launch shape, and the two products around the kernel launch of the subclass.
template <class D> struct GridOpBase : ks_operator {
  using H = typename HostT<D>::type;
  static_assert(sizeof(H) == sizeof(D), "element layout");
  D* diag = nullptr;   // centre + potential[r] (null: no potential)
  int nitems = 0;      // workgroups of a launch
  bool wide = false;   // the one-row tile (ny == 1)
  double bytes = 0.0;  // algorithmic bytes of one product
  // The Clenshaw step runs in the product's launch by default.  Only where that MEASURED faster than the product and a streaming
  // pass (216^3, Float64, profiles/grid_operator.txt): the 7-point operator, open and periodic, and the radius-2 star and the box
  // operator with open boundaries.  The kernels run near half the HBM rate and take the two tail streams at that rate, the streaming
  // pass takes its five at three quarters of it: with the long rows of radius 3 and 4, a coefficient stream, or the wrapped links of
  // a periodic star or box edge the fused step is the slower one.  KS_CHEB_FUSED=1 / 0 forces either path for every grid operator.
  bool cheb_fused_default = false;
  ~GridOpBase() override { (void)hipFree(diag); }
  virtual void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) = 0;

  // ctx, sizes, element type and the launch shape (geometry into g)
  void init(ks_ctx* c, const std::string& who, const grid::Shape& s, int radius, bool var, ksd::GridGeom& g) {
    init(c, who, s, radius, grid::tile<D>(s, radius, var), g);
  }
  void init(ks_ctx* c, const std::string& who, const grid::Shape& s, int radius, grid::Tile tile, ksd::GridGeom& g) {
    ctx = c;
    n_local = s.n;
    nnz = s.nnz;
    dtype = sizeof(D) == 8 ? KS_F64 : KS_C64;
    const grid::Plan p = grid::plan(who, s, tile, radius);
    g = p.g;
    nitems = p.nitems;
    wide = s.ny == 1;
  }
  // the diagonal centre + potential[r] (none without a potential), and the bytes of a product: x, y and the diagonal
  void upload_diag(const H& centre, const void* potential) {
    if (potential) {
      const H* v = static_cast<const H*>(potential);
      std::vector<H> d((size_t)n_local);
      for (int64_t r = 0; r < n_local; ++r) d[r] = grid::diag_add(centre, v[r]);
      KS_HIP(hipMalloc(&diag, (size_t)n_local * sizeof(D)));
      KS_HIP(hipMemcpy(diag, d.data(), (size_t)n_local * sizeof(D), hipMemcpyHostToDevice));
    }
    bytes = (double)n_local * sizeof(D) * (potential ? 3.0 : 2.0);
  }
  void product(const void* x, void* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail = ksd::GridTail<D>{}) {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "grid operator: the product needs distinct x and y");
    ProfScope ps(ctx, KSP_SPMV, bytes + (double)n_local * sizeof(D) * ((tail.w ? 1.0 : 0.0) + (tail.x0 ? 1.0 : 0.0)));
    launch(static_cast<const D*>(x), static_cast<D*>(y), st, shifted, theta, sigma, tail);
    KS_HIP(hipGetLastError());
  }
  void apply(const void* x, void* y, const DevState* st) override { product(x, y, st, 0, D{}, 1.0); }
  // the Clenshaw step in the same launch: the Newton step and the two-vector tail in the kernels' shared epilogue (GridStore), 40
  // instead of 64 bytes per row in Float64 with a potential (KS_CHEB_FUSED, read per call: 0 the product and a streaming pass, 1
  // this launch, unset cheb_fused_default)
  void apply_clenshaw(const void* x, void* y, double tre, double tim, double sigma, const void* w, double gamma, const void* x0, int64_t ld,
                      const DevState* st) override {
    const int env = env_int("KS_CHEB_FUSED", -1);
    if (!(env >= 0 ? env != 0 : cheb_fused_default)) { ks_operator::apply_clenshaw(x, y, tre, tim, sigma, w, gamma, x0, ld, st); return; }
    KS_REQUIRE(y != x && y != w && y != x0, KS_ERR_ARGUMENT, "Clenshaw step: y must be distinct from x, w and x0");
    D theta;
    if constexpr (sizeof(D) == 8) theta = tre; else theta = D{tre, tim};
    product(x, y, st, 1 | (shift_store_cacheable ? 2 : 0) | 16, theta, sigma, ksd::GridTail<D>{static_cast<const D*>(w), static_cast<const D*>(x0), gamma});
    ++this->clenshaw_fused;
  }
  // the Newton step in the same launch (KS_SHIFT_FUSED=0: the product and a streaming pass, like the stored layouts)
  void apply_shifted(const void* x, void* y, double tre, double tim, double sigma, int64_t ld, const DevState* st) override {
    if (!env_int("KS_SHIFT_FUSED", 1)) { ks_operator::apply_shifted(x, y, tre, tim, sigma, ld, st); return; }
    static const int env = env_int("KS_SHIFT_PLAIN", -1);
    const bool plain = env >= 0 ? env != 0 : shift_store_cacheable;
    D theta;
    if constexpr (sizeof(D) == 8) theta = tre; else theta = D{tre, tim};
    product(x, y, st, 1 | (plain ? 2 : 0), theta, sigma);
  }
};

template <class D> struct GridOp : GridOpBase<D> {
  using GridOpBase<D>::ctx; using GridOpBase<D>::diag; using GridOpBase<D>::nitems; using GridOpBase<D>::wide;
  ksd::GridPerDev<D> g{};   // (the open operator's kernel takes its GridDev part)
  bool periodic = false;  // some axis wraps: the kernel's periodic instantiation
  int radius = 1;      // > 1: the star stencil, k_grid_star with the taps of `star` (k_grid_star_per where some axis wraps)
  D star[25] = {};     // its 6 radius + 1 slots
  D starw[24] = {};    // ... and the wrap values of its 6 radius links
  // (bit 4 of `shifted`: the kernel instantiation with the tail of a Clenshaw step)
  void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) override {
    if (shifted & 16) launch_t<true>(x, y, st, shifted, theta, sigma, tail);
    else launch_t<false>(x, y, st, shifted, theta, sigma, tail);
  }
  template <bool TAIL> void launch_t(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) {
    using TL = ksd::GridTileOf<D>;
    const ksd::GridDev<D>& go = g;
    if (radius == 2) launch_star<2, TAIL>(x, y, st, shifted, theta, sigma, tail);
    else if (radius == 3) launch_star<3, TAIL>(x, y, st, shifted, theta, sigma, tail);
    else if (radius == 4) launch_star<4, TAIL>(x, y, st, shifted, theta, sigma, tail);
    else if (periodic) {
      if (wide) ksd::k_grid<D, TL::WX, 1, ksd::GridPerDev<D>, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
      else ksd::k_grid<D, TL::TX, TL::TY, ksd::GridPerDev<D>, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, diag, y, st, shifted, theta, sigma, tail);
    } else if (wide) ksd::k_grid<D, TL::WX, 1, ksd::GridDev<D>, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(go, x, diag, y, st, shifted, theta, sigma, tail);
    else ksd::k_grid<D, TL::TX, TL::TY, ksd::GridDev<D>, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(go, x, diag, y, st, shifted, theta, sigma, tail);
  }
  template <int R, bool TAIL> void launch_star(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) {
    if (periodic) {
      using TP = ksd::GridTile<ksd::grid_star_per_half(sizeof(D), R)>;
      ksd::GridStarPerDev<D, R> gp;
      static_cast<ksd::GridGeom&>(gp) = g;
      for (int k = 0; k < 6 * R + 1; ++k) gp.tap[k] = star[k];
      for (int k = 0; k < 6 * R; ++k) gp.wrap[k] = starw[k];
      gp.px = g.px; gp.py = g.py; gp.pz = g.pz;
      if (wide) ksd::k_grid_star_per<D, TP::WX, 1, R, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(gp, x, diag, y, st, shifted, theta, sigma, tail);
      else ksd::k_grid_star_per<D, TP::TX, TP::TY, R, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(gp, x, diag, y, st, shifted, theta, sigma, tail);
      return;
    }
    using TL = ksd::GridTileOf<D, R>;
    ksd::GridStarDev<D, R> gs;
    static_cast<ksd::GridGeom&>(gs) = g;
    for (int k = 0; k < 6 * R + 1; ++k) gs.tap[k] = star[k];
    if (wide) ksd::k_grid_star<D, TL::WX, 1, R, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(gs, x, diag, y, st, shifted, theta, sigma, tail);
    else ksd::k_grid_star<D, TL::TX, TL::TY, R, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(gs, x, diag, y, st, shifted, theta, sigma, tail);
  }
};

template <class D>
ks_operator* make_grid(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps, const void* potential,
                       const int* periodic, const void* wrap, int radius = 1) {
  using H = typename HostT<D>::type;
  grid::Shape s = grid::check<H>(who, ndim, dims, taps, potential, radius);
  auto op = std::make_unique<GridOp<D>>();
  H t[7], centre;
  bool half = ksd::grid_half(sizeof(D), radius, false);
  if (radius == 1) {
    const grid::Wrap<H> W = grid::check_wrap<H>(who, s, ndim, taps, periodic, wrap);
    grid::seven_taps(ndim, static_cast<const H*>(taps), t);
    std::memcpy(op->g.tap, t, sizeof(t));
    centre = t[3];
    std::memcpy(op->g.wrap, W.w, sizeof(W.w));
    op->g.px = W.per[0]; op->g.py = W.per[1]; op->g.pz = W.per[2];
    op->periodic = W.any();
  } else {
    const grid::WrapStar<H> W = grid::check_wrap_star<H>(who, s, ndim, radius, taps, periodic, wrap);
    H ts[25];
    grid::star_taps(ndim, radius, static_cast<const H*>(taps), ts);
    std::memcpy(op->star, ts, sizeof(ts));
    centre = ts[3 * radius];
    std::memcpy(op->starw, W.w, sizeof(W.w));
    op->g.px = W.per[0]; op->g.py = W.per[1]; op->g.pz = W.per[2];
    op->periodic = W.any();
    if (op->periodic) half = ksd::grid_star_per_half(sizeof(D), radius);
  }
  op->radius = radius;
  op->cheb_fused_default = radius == 1 || (radius == 2 && !op->periodic);
  op->init(ctx, who, s, radius, grid::tile_of(s, half), op->g);
  op->upload_diag(centre, potential);
  return op.release();
}

}  // namespace
