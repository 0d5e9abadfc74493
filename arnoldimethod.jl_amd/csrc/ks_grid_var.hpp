// Matrix-free VARIABLE-COEFFICIENT grid operator  y = A x  for A = -div(c(x) grad) + V(x) and its kin on an nx x ny x nz grid
// (ks_operator_grid_var, include/kschur.h (xi)): mul!(y, A, x), src/expansion.jl:121, for the 3-, 5- or 7-point stencil whose
// off-diagonal entries vary from link to link -- heterogeneous diffusion, a position-dependent effective mass, div (1 / eps) grad --
// still with NOTHING stored per non-zero.  The coefficient lives on the grid points (cell-centred, one Float64 per point, real also
// for ComplexF64 operators); the entry of the link from row r to its neighbour s in direction k is
//     A[r, s] = fl(h_k * fl(c[r] + c[s])),   h_k = 0.5 * tap_k   (ComplexF64: the two real products h_k.re * m, h_k.im * m)
// formed in registers; the six half taps travel in the kernel arguments (halved once on the host at upload).  The diagonal entry is
// centre + potential[r].
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip right after ks_grid.hpp, which describes the scheme
// and holds everything this operator shares with the constant-coefficient ones.
//
// The operator IS the matrix ks_host_grid_var_matrix returns: the kernel forms every entry by exactly these two roundings (open
// boundaries, slots -z, -y, -x, centre, +x, +y, +z).
// With periodic axes (ks_operator_grid_var_periodic, (xi-b): photonic crystals, a superlattice with a position-dependent mass, diffusion
// on a torus) it is the matrix of ks_host_grid_var_matrix_periodic: a link that crosses the boundary of a periodic axis carries
// fl(hw_k * fl(c[r] + c[s])), hw_k = 0.5 * wrap_k, s the wrap image at the other end of the line, and a row is summed in the 13-slot
// order of (ix).  Periodicity is a compile-time variant of the one kernel, as for k_grid; the open instantiation is the kernel as it was.
//
// k_grid_var (R = 1).  c travels exactly like x: registers for the planes z - 1, z, z + 1 (the +-z links need c of the planes
// z +- 1) and z + 2 in flight, an LDS tile of its own beside that of x, the halo cell of both, from which the +-x and +-y links
// read the neighbour's x and the neighbour's c.  The z-loop is unrolled by four, the register sets rotate by name.  Compulsory
// traffic: x, c and the diagonal read once, y written once -- 32 bytes per row in Float64 (24 without a potential), 56 / 40 in
// ComplexF64 (c stays 8 bytes); the halo and plane re-reads are of x and of c alike.
// Tiles (the resource report behind the choice is in DESIGN.md): Float64 32 x 32 and 1024 x 1 (ny == 1), four points per thread;
// ComplexF64 32 x 16 and 512 x 1, two points per thread -- with four points the ComplexF64 kernel takes 223 registers and 55 KB of
// LDS, two waves per SIMD either way, with two points 128 registers and 29 KB, four waves.
#pragma once

namespace ksd {

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

// g.tap: the six off-diagonal slots hold the HALF taps h_k, slot 3 the centre.  c: the n coefficients.
// G = GridPerDev<T>: periodic axes (ks_operator_grid_var_periodic, include/kschur.h (xi-b)), the variant k_grid has: g.wrap holds the
// HALF wrap values hw_k, a row is summed in the 13-slot order of (ix), and c wraps wherever x wraps -- the halo cell one step
// outside the grid, the owned point gx = nx / gy = ny of a partial last tile (never stored, its diagonal never loaded), plane -1 and
// plane nz.  No per-point state is added to the open form's: a link of a point in the grid wraps exactly where the interior link of
// its direction is absent (in && !hxm: gx == 0, ...), and off[] is the offset the point is LOADED from, negative for a point that is
// not loaded -- stores and diagonal loads use it only under in[], where it is the point's own offset.  The row of a point is
// instantiated twice in the periodic form, with and without the two z-wrap links, and a uniform branch per plane picks one: only
// plane 0 and plane nz - 1 have them, and with them in the one row every plane would keep x and c of plane z - 1 to the end of its
// rows (DESIGN.md has the register counts of each form).
template <class T, int TX, int TY, class G, bool TAIL = false>
__global__ void __launch_bounds__(kBlock)
    k_grid_var(const G g, const T* __restrict__ x, const double* __restrict__ c, const T* __restrict__ diag,
               T* __restrict__ y, const DevState* __restrict__ st, int shifted, T theta, double sigma, const GridTail<T> tail) {
  if (st && st->breakdown >= 0) return;
  constexpr bool PER = !std::is_same<G, GridDev<T>>::value;
  using L = GridLds<TX, TY, 1>;
  constexpr int PPT = L::PPT, HY = L::HY, LW = L::LW;
  static_assert(L::NH == 1, "at most one halo cell per thread");
  __shared__ T tile[2][L::LH * LW];
  __shared__ double ctile[2][L::LH * LW];
  const GridItem it = grid_item<TX, TY>(g);
  const int za = it.za, zb = it.zb;
  const int64_t P = it.P;
  const int tid = (int)threadIdx.x;
  const GridStore<T, TAIL> store{y, P, shifted, theta, sigma, tail};

  int64_t off[PPT];   // in-plane offset of the owned points
  int li[PPT];        // ... and their place in the LDS tiles
  bool in[PPT], hxm[PPT], hxp[PPT], hym[PPT], hyp[PPT];   // inside the grid; has a -x / +x / -y / +y neighbour
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    int gx, gy;
    grid_owned<TX, TY, 1>(g, it, tid + k * kBlock, gx, gy, in[k], off[k], li[k]);
    grid_neighbours(g, gx, gy, in[k], hxm[k], hxp[k], hym[k], hyp[k]);
    if constexpr (PER) {
      const bool ix = g.px && gx == g.nx && gy < g.ny, iy = g.py && gy == g.ny && gx < g.nx;   // the image of [0, gy] / of [gx, 0]
      off[k] = in[k] ? off[k] : ix ? (int64_t)gy * g.nx : iy ? (int64_t)gx : (int64_t)-1;
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
  // periodic in z: plane -1 is plane nz - 1, plane nz is plane 0 (z is never further out than one plane)
  auto pl = [&](int z) {
    if constexpr (PER) {
      if (g.pz) z = z < 0 ? g.nz - 1 : z >= g.nz ? 0 : z;
    }
    return z;
  };
  auto ldx = [&](int z, int64_t o, bool ok) { z = pl(z); return ok && z >= 0 && z < g.nz ? x[(int64_t)z * P + o] : zero_of(T{}); };
  auto ldc = [&](int z, int64_t o, bool ok) { z = pl(z); return ok && z >= 0 && z < g.nz ? c[(int64_t)z * P + o] : 0.0; };
  // the owned point k is LOADED: with periodic axes also the wrap images beyond a partial last tile
  auto lk = [&](int k) {
    if constexpr (PER) return off[k] >= 0;
    else return in[k];
  };

  // Register sets: xr[0..3] / cr[0..3] hold the owned points of four consecutive planes and rotate by NAME (the z-loop is
  // unrolled by four); hr / hc [0..1]: this thread's halo cell of the planes of even / odd steps, dr[0..1]: the diagonal.
  T xr[4][PPT], dr[2][PPT], hr[2];
  double cr[4][PPT], hc[2];
  hr[0] = ldx(za, hoff, hin);
  hc[0] = ldc(za, hoff, hin);
  hr[1] = ldx(za + 1, hoff, hin && za + 1 < zb);
  hc[1] = ldc(za + 1, hoff, hin && za + 1 < zb);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    xr[0][k] = ldx(za - 1, off[k], lk(k));
    xr[1][k] = ldx(za, off[k], lk(k));
    xr[2][k] = ldx(za + 1, off[k], lk(k));
    cr[0][k] = ldc(za - 1, off[k], lk(k));
    cr[1][k] = ldc(za, off[k], lk(k));
    cr[2][k] = ldc(za + 1, off[k], lk(k));
    dr[0][k] = diag ? grid_ldd(diag, g, P, za, off[k], in[k]) : g.tap[3];
    dr[1][k] = dr[0][k];
  }
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
    if (tid < L::NHALO) {
      tl[hli] = hw;
      cl[hli] = hcw;
    }
    hw = ldx(z + 2, hoff, hin && z + 2 < zb);
    hcw = ldc(z + 2, hoff, hin && z + 2 < zb);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      xn[k] = ldx(z + 2, off[k], lk(k) && z + 2 <= zb);   // (plane zb is the +z link of the range's last plane)
      cn[k] = ldc(z + 2, off[k], lk(k) && z + 2 <= zb);
      if (diag) dn[k] = grid_ldd(diag, g, P, z + 1, off[k], in[k] && z + 1 < zb);
    }
    __syncthreads();
    // the row of point k; ZW: this plane has a z-wrap link (periodic form, plane 0 or nz - 1)
    auto row = [&](int k, auto zwc) {
      [[maybe_unused]] constexpr bool ZW = decltype(zwc)::value;
      T s = zero_of(T{});
      const double cr_ = cc[k];
      // a link: entry = h (c_r + c_s), the sum rounded, then the product(s); then the entry times x_s, rounded on its own
      auto link = [&](const T& h, double cs, const T& xs) { return add_(s, mul_nc(var_entry(h, cr_ + cs), xs)); };
      if constexpr (PER) {
        if (ZW && z + 1 == g.nz) s = link(g.wrap[5], cp[k], xp[k]);
      }
      if (z > 0) s = link(g.tap[0], cm[k], xm[k]);
      if constexpr (HY) {
        if constexpr (PER) {
          if (g.py && in[k] && !hyp[k]) s = link(g.wrap[4], cl[li[k] + LW], tl[li[k] + LW]);
        }
        if (hym[k]) s = link(g.tap[1], cl[li[k] - LW], tl[li[k] - LW]);
      }
      if constexpr (PER) {
        if (g.px && in[k] && !hxp[k]) s = link(g.wrap[3], cl[li[k] + 1], tl[li[k] + 1]);
      }
      if (hxm[k]) s = link(g.tap[2], cl[li[k] - 1], tl[li[k] - 1]);
      s = add_(s, mul_nc(dc[k], xc[k]));
      if (hxp[k]) s = link(g.tap[4], cl[li[k] + 1], tl[li[k] + 1]);
      if constexpr (PER) {
        if (g.px && in[k] && !hxm[k]) s = link(g.wrap[2], cl[li[k] - 1], tl[li[k] - 1]);
      }
      if constexpr (HY) {
        if (hyp[k]) s = link(g.tap[5], cl[li[k] + LW], tl[li[k] + LW]);
        if constexpr (PER) {
          if (g.py && in[k] && !hym[k]) s = link(g.wrap[1], cl[li[k] - LW], tl[li[k] - LW]);
        }
      }
      if (z + 1 < g.nz) s = link(g.tap[6], cp[k], xp[k]);
      if constexpr (PER) {
        if (ZW && z == 0) s = link(g.wrap[0], cm[k], xm[k]);
      }
      store(z, off[k], in[k], s, xc[k]);
    };
    if constexpr (PER) {
      if (g.pz && (z == 0 || z + 1 == g.nz)) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) row(k, std::true_type{});
      } else {
#pragma unroll
        for (int k = 0; k < PPT; ++k) row(k, std::false_type{});
      }
    } else {
#pragma unroll
      for (int k = 0; k < PPT; ++k) row(k, std::false_type{});
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
// the seven slots of grid::seven_taps with the six off-diagonal taps halved (slot 3: the centre as it is)
template <class H> void half_taps(int ndim, const H* t, H (&out)[7]) {
  seven_taps(ndim, t, out);
  for (int k = 0; k < 7; ++k)
    if (k != 3) out[k] = half_tap(out[k]);
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

// the six wrap values halved like the taps: hw_k = 0.5 wrap_k (-z, -y, -x, +x, +y, +z; an axis that does not wrap: zero, never used)
template <class H> void half_wrap(const Wrap<H>& W, H (&out)[6]) {
  for (int k = 0; k < 6; ++k) out[k] = half_tap(W.w[k]);
}

// both host entry points (ks_host_grid_var_matrix, ks_host_grid_var_matrix_periodic, include/kschur.h (xi), (xi-b)): the checks, then
// the radius-1 rows with the entry of every link formed from the coefficient -- a link that crosses the boundary of a periodic axis
// from the half wrap value of its direction and the coefficient of the wrap image
template <class H>
void host_var_matrix_entry(const std::string& who, int ndim, const int64_t* dims, const void* taps, const double* coeff, const void* pot,
                           const int* periodic, const void* wrap, int64_t* rowptr, int32_t* colidx, void* val, int64_t cap, int64_t* nnz) {
  Shape s = check_var<H>(who, ndim, dims, taps, coeff, pot);
  const Wrap<H> W = check_wrap<H>(who, s, ndim, taps, periodic, wrap);
  csr_begin(who, s, rowptr, colidx, static_cast<H*>(val), cap, nnz);
  H h[7], hw[6];
  half_taps(ndim, static_cast<const H*>(taps), h);
  half_wrap(W, hw);
  seven_slot_rows(s, W.per, h[3], static_cast<const H*>(pot), rowptr, colidx, static_cast<H*>(val), [&](int k, int64_t r, int64_t c, bool wrapped) {
    const double m = coeff[r] + coeff[c];
    return var_entry(wrapped ? hw[k - (k > 3)] : h[k], m);
  });
}

}  // namespace grid

template <class D> struct VarGridOp : GridOpBase<D> {
  using GridOpBase<D>::ctx; using GridOpBase<D>::diag; using GridOpBase<D>::nitems; using GridOpBase<D>::wide;
  ksd::GridPerDev<D> g{};    // (tap: the half taps, wrap: the half wrap values; the open operator's kernel takes its GridDev part)
  bool periodic = false;     // some axis wraps: the kernel's periodic instantiation
  double* coeff = nullptr;   // c[r], always Float64
  ~VarGridOp() override { (void)hipFree(coeff); }
  // (bit 4 of `shifted`: the kernel instantiation with the tail of a Clenshaw step)
  void launch(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) override {
    if (shifted & 16) launch_t<true>(x, y, st, shifted, theta, sigma, tail);
    else launch_t<false>(x, y, st, shifted, theta, sigma, tail);
  }
  template <bool TAIL> void launch_t(const D* x, D* y, const DevState* st, int shifted, D theta, double sigma, const ksd::GridTail<D>& tail) {
    using TL = ksd::GridTileOf<D, 1, true>;
    using GP = ksd::GridPerDev<D>;
    using GO = ksd::GridDev<D>;
    const GO& go = g;
    if (periodic) {
      if (wide) ksd::k_grid_var<D, TL::WX, 1, GP, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, coeff, diag, y, st, shifted, theta, sigma, tail);
      else ksd::k_grid_var<D, TL::TX, TL::TY, GP, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(g, x, coeff, diag, y, st, shifted, theta, sigma, tail);
    } else if (wide) ksd::k_grid_var<D, TL::WX, 1, GO, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(go, x, coeff, diag, y, st, shifted, theta, sigma, tail);
    else ksd::k_grid_var<D, TL::TX, TL::TY, GO, TAIL><<<nitems, kBlock, 0, ctx->stream>>>(go, x, coeff, diag, y, st, shifted, theta, sigma, tail);
  }
};

template <class D>
ks_operator* make_grid_var(ks_ctx* ctx, const std::string& who, int ndim, const int64_t* dims, const void* taps, const double* coeff,
                           const void* potential, const int* periodic, const void* wrap) {
  using H = typename HostT<D>::type;
  grid::Shape s = grid::check_var<H>(who, ndim, dims, taps, coeff, potential);
  const grid::Wrap<H> W = grid::check_wrap<H>(who, s, ndim, taps, periodic, wrap);
  auto op = std::make_unique<VarGridOp<D>>();
  H h[7], hw[6];
  grid::half_taps(ndim, static_cast<const H*>(taps), h);
  grid::half_wrap(W, hw);
  std::memcpy(op->g.tap, h, sizeof(h));
  std::memcpy(op->g.wrap, hw, sizeof(hw));
  op->g.px = W.per[0]; op->g.py = W.per[1]; op->g.pz = W.per[2];
  op->periodic = W.any();
  op->init(ctx, who, s, 1, true, op->g);
  KS_HIP(hipMalloc(&op->coeff, (size_t)s.n * sizeof(double)));
  KS_HIP(hipMemcpy(op->coeff, coeff, (size_t)s.n * sizeof(double), hipMemcpyHostToDevice));
  op->upload_diag(h[3], potential);
  op->bytes += (double)s.n * 8.0;   // ... and c
  return op.release();
}

}  // namespace
