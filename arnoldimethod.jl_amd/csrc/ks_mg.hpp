// Geometric multigrid V-cycle  y = M x,  M ~ (A - theta I)^-1  (ks_operator_multigrid, include/kschur.h (xix)): ONE symmetric V-cycle
// over a chain of grids as a fixed linear map -- Hermitian positive definite by construction, so ks_operator_pcg takes it as its
// preconditioner on the generic path.  The host plan (ks_mg_plan.hpp) holds the chain, the smoother's coefficients and the
// definition; this file runs it.  Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_pcg.hpp.
//
//   down, l = 0 ... L-1:   x_l = S(b_l) from x = 0          k_mg_cheb_first<PRE>, then k - 1 times { t = (A_l - theta) x;  k_mg_cheb_step }
//                          t = (A_l - theta) x_l;  b_{l+1} = s P^T (b_l - t)                                  k_mg_restrict
//   level L:               x_L = coarse b_L
//   up, l = L-1 ... 0:     x_l += P x_{l+1}                                                                   k_mg_prolong_add
//                          x_l = S(b_l, x_l)                k times { t = (A_l - theta) x;  k_mg_cheb_first<POST> / k_mg_cheb_step }
//
// 2 k products per smoothed level and application.  The level operators and `coarse` are BORROWED; t comes from their apply_shifted
// (theta == 0: apply), so a grid operator forms A x - theta x in its own store.  b_0 is the caller's x, x_0 the caller's y; every other
// vector is a temporary of the operator, allocated like ChebOp's (a multiple of 64 elements, zero-filled once; every kernel writes
// rows < n only).  Nothing is decided on the device and the host reads nothing: the cycle is enqueued ahead like a stored matrix.
//
// The smoother kernels run on the real view like the CG kernels (block_range over 16-byte packs, the odd tail is cg_owns_tail's); in
// ComplexF64 a pack is one element and takes one dinv[i].  The transfers take one thread per coarse x-cell of a line: 16-byte paired
// accesses of the two fine x-cells where the pair is 16-byte aligned (Float64: an even fine row; ComplexF64: always one pack per
// cell), two 8-byte ones where a line starts at an odd element (nx odd).
#pragma once

namespace ksd {

struct MgGeom {
  int nxf, nyf, nzf, nxc, nyc, nzc;
  int hx, hy, hz;   // 1: the axis is halved
};

// first smoother step:  d = b_0 dinv o res,  res = rhs (PRE: from x = 0, x = d) or rhs - t (x += d)
template <bool PRE, bool C>
__global__ void __launch_bounds__(kBlock)
    k_mg_cheb_first(const double* __restrict__ rhs, const double* __restrict__ t, const double* __restrict__ dinv, double* __restrict__ d,
                    double* __restrict__ x, double b0, int64_t nd, const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 r = ld_pack(rhs + 2 * i);
    if constexpr (!PRE) {
      const double2 tv = ld_pack_nt(t + 2 * i);
      r.x -= tv.x;
      r.y -= tv.y;
    }
    const double2 w = pcg_dmul(pcg_ld_d<C>(dinv, i), r);
    const double2 dv = make_double2(mul_nc(b0, w.x), mul_nc(b0, w.y));
    st_pack(d + 2 * i, dv);
    if constexpr (PRE) {
      st_pack(x + 2 * i, dv);
    } else {
      double2 xv = ld_pack(x + 2 * i);
      xv.x += dv.x;
      xv.y += dv.y;
      st_pack(x + 2 * i, xv);
    }
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    double r = rhs[i];
    if constexpr (!PRE) r -= t[i];
    const double dv = mul_nc(b0, mul_nc(dinv[i], r));
    d[i] = dv;
    x[i] = PRE ? dv : x[i] + dv;
  }
}

// smoother step j >= 1:  d = fma(a, d, b (dinv o (rhs - t))),  x += d     reads rhs, t, dinv, d, x, writes d, x: 56 B/row in Float64
template <bool C>
__global__ void __launch_bounds__(kBlock)
    k_mg_cheb_step(const double* __restrict__ rhs, const double* __restrict__ t, const double* __restrict__ dinv, double* __restrict__ d,
                   double* __restrict__ x, double a, double b, int64_t nd, const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 r = ld_pack(rhs + 2 * i);
    const double2 tv = ld_pack_nt(t + 2 * i);
    double2 dv = ld_pack(d + 2 * i);
    double2 xv = ld_pack(x + 2 * i);
    r.x -= tv.x;
    r.y -= tv.y;
    const double2 w = pcg_dmul(pcg_ld_d<C>(dinv, i), r);
    dv.x = fma(a, dv.x, mul_nc(b, w.x));
    dv.y = fma(a, dv.y, mul_nc(b, w.y));
    xv.x += dv.x;
    xv.y += dv.y;
    st_pack(d + 2 * i, dv);
    st_pack(x + 2 * i, xv);   // (cacheable: the next product gathers exactly this vector)
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    const double dv = fma(a, d[i], mul_nc(b, mul_nc(dinv[i], rhs[i] - t[i])));
    d[i] = dv;
    x[i] = x[i] + dv;
  }
}

// rc[I] = s * sum over the aggregate of (b - t), the terms added to +0.0 in ascending fine row order.  One thread per coarse cell,
// 64 consecutive coarse x-cells per wave: 128 contiguous fine values of each of the up to four fine lines.  The loads of a cell that
// lies outside the grid (odd extents) are clamped onto the cell next to it and their term replaced by +0.0, which changes no bit of a
// sum that started at +0.0; so every load is issued before the first add.
template <bool C>
__global__ void __launch_bounds__(kBlock)
    k_mg_restrict(const double* __restrict__ b, const double* __restrict__ t, double* __restrict__ rc, MgGeom g, double scale,
                  const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  const uint32_t ncoarse = (uint32_t)g.nxc * (uint32_t)g.nyc * (uint32_t)g.nzc;
  const uint32_t ic = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (ic >= ncoarse) return;
  const uint32_t I = ic % (uint32_t)g.nxc, jk = ic / (uint32_t)g.nxc, J = jk % (uint32_t)g.nyc, K = jk / (uint32_t)g.nyc;
  const int i0 = (int)(I << g.hx), j0 = (int)(J << g.hy), k0 = (int)(K << g.hz);
  const bool two = g.hx && i0 + 1 < g.nxf;
  double vx[2][2][2], vy[2][2][2];   // [dz][dy][dx]: b - t (ComplexF64: the real and the imaginary parts)
#pragma unroll
  for (int dz = 0; dz < 2; ++dz) {
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const bool in = (dz == 0 || (g.hz && k0 + 1 < g.nzf)) && (dy == 0 || (g.hy && j0 + 1 < g.nyf));
      const int j = j0 + (in ? dy : 0), k = k0 + (in ? dz : 0);
      const int64_t row = i0 + (int64_t)g.nxf * (j + (int64_t)g.nyf * k);
      if constexpr (C) {
        const int64_t row1 = row + (two ? 1 : 0);
        const double2 b0 = ld_pack(b + 2 * row), t0 = ld_pack_nt(t + 2 * row);
        const double2 b1 = ld_pack(b + 2 * row1), t1 = ld_pack_nt(t + 2 * row1);
        vx[dz][dy][0] = in ? b0.x - t0.x : 0.0;
        vy[dz][dy][0] = in ? b0.y - t0.y : 0.0;
        vx[dz][dy][1] = in && two ? b1.x - t1.x : 0.0;
        vy[dz][dy][1] = in && two ? b1.y - t1.y : 0.0;
      } else {
        double2 p, q;   // the two x-cells of b and of t
        if (two && (row & 1) == 0) {
          p = ld_pack(b + row);
          q = ld_pack_nt(t + row);
        } else {   // a line that starts at an odd element, the single cell of an odd tail, or an axis that is not halved
          const int64_t row1 = row + (two ? 1 : 0);
          p = make_double2(b[row], b[row1]);
          q = make_double2(t[row], t[row1]);
        }
        vx[dz][dy][0] = in ? p.x - q.x : 0.0;
        vx[dz][dy][1] = in && two ? p.y - q.y : 0.0;
      }
    }
  }
  double ax = 0.0, ay = 0.0;
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        ax += vx[dz][dy][dx];
        if constexpr (C) ay += vy[dz][dy][dx];
      }
  if constexpr (C) st_pack(rc + 2 * (int64_t)ic, make_double2(scale * ax, scale * ay));
  else rc[ic] = scale * ax;
}

// x[i] += ec[aggregate of i]: one thread per coarse x-cell of a FINE line, its coarse value loaded once for the two fine x-cells
template <bool C>
__global__ void __launch_bounds__(kBlock)
    k_mg_prolong_add(const double* __restrict__ ec, double* __restrict__ x, MgGeom g, const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  const uint32_t total = (uint32_t)g.nxc * (uint32_t)g.nyf * (uint32_t)g.nzf;
  const uint32_t id = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (id >= total) return;
  const uint32_t I = id % (uint32_t)g.nxc, jk = id / (uint32_t)g.nxc, j = jk % (uint32_t)g.nyf, k = jk / (uint32_t)g.nyf;
  const int i0 = (int)(I << g.hx);
  const bool two = g.hx && i0 + 1 < g.nxf;
  const int64_t rowc = I + (int64_t)g.nxc * ((j >> g.hy) + (int64_t)g.nyc * (k >> g.hz));
  const int64_t row = i0 + (int64_t)g.nxf * (j + (int64_t)g.nyf * k);
  if constexpr (C) {
    const double2 e = ld_pack(ec + 2 * rowc);
    double2 v = ld_pack(x + 2 * row);
    v.x += e.x;
    v.y += e.y;
    st_pack(x + 2 * row, v);
    if (two) {
      double2 w = ld_pack(x + 2 * row + 2);
      w.x += e.x;
      w.y += e.y;
      st_pack(x + 2 * row + 2, w);
    }
  } else {
    const double e = ec[rowc];
    if (two && (row & 1) == 0) {
      double2 v = ld_pack(x + row);
      v.x += e;
      v.y += e;
      st_pack(x + row, v);
    } else {
      x[row] = x[row] + e;
      if (two) x[row + 1] = x[row + 1] + e;
    }
  }
}

}  // namespace ksd

namespace {

struct MgOp : ks_operator {
  MgPlan plan;
  std::vector<ks_operator*> A;          // nsmooth level operators (borrowed)
  ks_operator* coarse = nullptr;        // (borrowed)
  double theta = 0.0;
  std::vector<double*> dinv;            // per smoothed level: rows(l) values, allocated like a basis column
  std::vector<void*> rhs, sol, dir, tt; // per level: b_l and x_l (l >= 1), d_l and t_l (l < L)
  int64_t applications = 0;
  std::vector<int64_t> products;        // per level: products with A_l (level L: applications of `coarse`) since creation
  ~MgOp() override {
    for (double* p : dinv) (void)hipFree(p);
    for (auto* v : {&rhs, &sol, &dir, &tt})
      for (void* p : *v) (void)hipFree(p);
  }
  static ksd::MgGeom geom(const MgLevel& f, const MgLevel& c) {
    return ksd::MgGeom{(int)f.dims[0], (int)f.dims[1], (int)f.dims[2], (int)c.dims[0], (int)c.dims[1], (int)c.dims[2],
                       f.halved[0], f.halved[1], f.halved[2]};
  }
  // t = (A_l - theta) x
  void residual_product(int l, const void* xv, void* tv, const DevState* st) {
    A[l]->in_scale = in_scale;
    if (theta == 0.0) A[l]->apply(xv, tv, st);
    else A[l]->apply_shifted(xv, tv, theta, 0.0, 1.0, round_up(A[l]->n_local, 64), st);
    ++products[l];
  }
  // (no ProfScope around the cycle: the level operators book their own time; of the cycle's own kernels the smoother steps are booked
  // as `fused` -- two updates in one pass --, the prolongation as `axpy` and the restriction as `scale`)
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "multigrid cycle: the product needs distinct x and y");
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "multigrid cycle: a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    hipStream_t s = ctx->stream;
    const int L = (int)A.size(), k = plan.degree;
    const bool cx = dtype != KS_F64;
    const double W = cx ? 16.0 : 8.0;
    ++applications;
    if (L == 0) {
      coarse->in_scale = in_scale;
      coarse->apply(x, y, st);
      ++products[0];
      return;
    }
    auto B = [&](int l) { return l == 0 ? static_cast<const double*>(x) : static_cast<const double*>(rhs[l]); };
    auto X = [&](int l) { return l == 0 ? static_cast<double*>(y) : static_cast<double*>(sol[l]); };
    auto D = [&](int l) { return static_cast<double*>(dir[l]); };
    auto T = [&](int l) { return static_cast<double*>(tt[l]); };
    auto nd_of = [&](int l) { return plan.levels[l].rows * (cx ? 2 : 1); };
    auto step = [&](int l, int j) {   // smoother step j >= 1 behind t = (A_l - theta) x
      const int64_t nd = nd_of(l);
      residual_product(l, X(l), T(l), st);
      ProfScope ps(ctx, KSP_FUSED, 6.0 * 8.0 * (double)nd + 8.0 * (double)plan.levels[l].rows);
      const int nb = CgOp::cg_blocks(ctx, nd);
      if (cx) ksd::k_mg_cheb_step<true><<<nb, kBlock, 0, s>>>(B(l), T(l), dinv[l], D(l), X(l), plan.levels[l].a[j], plan.levels[l].b[j], nd, st);
      else ksd::k_mg_cheb_step<false><<<nb, kBlock, 0, s>>>(B(l), T(l), dinv[l], D(l), X(l), plan.levels[l].a[j], plan.levels[l].b[j], nd, st);
    };
    for (int l = 0; l < L; ++l) {
      const MgLevel& lv = plan.levels[l];
      const int64_t nd = nd_of(l);
      const int nb = CgOp::cg_blocks(ctx, nd);
      {
        ProfScope ps(ctx, KSP_FUSED, 3.0 * 8.0 * (double)nd + 8.0 * (double)lv.rows);
        if (cx) ksd::k_mg_cheb_first<true, true><<<nb, kBlock, 0, s>>>(B(l), nullptr, dinv[l], D(l), X(l), lv.b[0], nd, st);
        else ksd::k_mg_cheb_first<true, false><<<nb, kBlock, 0, s>>>(B(l), nullptr, dinv[l], D(l), X(l), lv.b[0], nd, st);
      }
      for (int j = 1; j < k; ++j) step(l, j);
      residual_product(l, X(l), T(l), st);
      const MgLevel& nx = plan.levels[l + 1];
      const ksd::MgGeom g = geom(lv, nx);
      double* rc = static_cast<double*>(rhs[l + 1]);
      const int nbr = (int)((nx.rows + kBlock - 1) / kBlock);
      ProfScope ps(ctx, KSP_SCALE, W * (2.0 * (double)lv.rows + (double)nx.rows));
      if (cx) ksd::k_mg_restrict<true><<<nbr, kBlock, 0, s>>>(B(l), T(l), rc, g, lv.scale, st);
      else ksd::k_mg_restrict<false><<<nbr, kBlock, 0, s>>>(B(l), T(l), rc, g, lv.scale, st);
      KS_HIP(hipGetLastError());
    }
    coarse->in_scale = in_scale;
    coarse->apply(rhs[L], sol[L], st);
    ++products[L];
    for (int l = L - 1; l >= 0; --l) {
      const MgLevel& lv = plan.levels[l];
      const MgLevel& nx = plan.levels[l + 1];
      const ksd::MgGeom g = geom(lv, nx);
      const int64_t nd = nd_of(l);
      {
        const int64_t threads = nx.dims[0] * lv.dims[1] * lv.dims[2];
        const int nbp = (int)((threads + kBlock - 1) / kBlock);
        ProfScope ps(ctx, KSP_AXPY, W * (2.0 * (double)lv.rows + (double)nx.rows));
        if (cx) ksd::k_mg_prolong_add<true><<<nbp, kBlock, 0, s>>>(static_cast<const double*>(sol[l + 1]), X(l), g, st);
        else ksd::k_mg_prolong_add<false><<<nbp, kBlock, 0, s>>>(static_cast<const double*>(sol[l + 1]), X(l), g, st);
      }
      residual_product(l, X(l), T(l), st);
      {
        const int nb = CgOp::cg_blocks(ctx, nd);
        ProfScope ps(ctx, KSP_FUSED, 5.0 * 8.0 * (double)nd + 8.0 * (double)lv.rows);
        if (cx) ksd::k_mg_cheb_first<false, true><<<nb, kBlock, 0, s>>>(B(l), T(l), dinv[l], D(l), X(l), lv.b[0], nd, st);
        else ksd::k_mg_cheb_first<false, false><<<nb, kBlock, 0, s>>>(B(l), T(l), dinv[l], D(l), X(l), lv.b[0], nd, st);
      }
      for (int j = 1; j < k; ++j) step(l, j);
      KS_HIP(hipGetLastError());
    }
  }
};

inline ks_operator* make_multigrid(ks_ctx* ctx, int nsmooth, ks_operator* const* A, const int64_t* dims, const double* const* inv_diag,
                                   const double* lambda_max, ks_operator* coarse, double shift, int degree, double ratio) {
  const std::string who = "ks_operator_multigrid";
  KS_REQUIRE(nsmooth >= 0 && nsmooth + 1 <= kMgMaxLevels, KS_ERR_ARGUMENT,
             who + ": " + std::to_string((int64_t)nsmooth + 1) + " levels (1 to " + std::to_string(kMgMaxLevels) + " are supported)");
  KS_REQUIRE(coarse, KS_ERR_ARGUMENT, who + ": the coarse operator is null");
  KS_REQUIRE(nsmooth == 0 || (A && inv_diag && lambda_max), KS_ERR_ARGUMENT, who + ": null argument");
  KS_REQUIRE(std::isfinite(shift), KS_ERR_ARGUMENT, who + ": shift is not finite");
  auto check_op = [&](const ks_operator* f, const std::string& name, int dtype) {
    KS_REQUIRE(f, KS_ERR_ARGUMENT, who + ": " + name + " is null");
    KS_REQUIRE(f->ctx == ctx, KS_ERR_ARGUMENT, who + ": " + name + " lives on another context");
    KS_REQUIRE(f->dtype == KS_F64 || f->dtype == KS_C64, KS_ERR_ARGUMENT, who + ": " + name + " is neither Float64 nor ComplexF64");
    KS_REQUIRE(f->dtype == dtype, KS_ERR_ARGUMENT, who + ": " + name + " does not have the element type of the coarse operator");
    KS_REQUIRE(f->async_capable, KS_ERR_ARGUMENT,
               who + ": " + name + " cannot be enqueued ahead (a host callback, an iterative solve, or a product or filter of one)");
  };
  check_op(coarse, "the coarse operator", coarse->dtype);
  for (int l = 0; l < nsmooth; ++l) {
    check_op(A[l], "the operator of level " + std::to_string(l), coarse->dtype);
    KS_REQUIRE(inv_diag[l], KS_ERR_ARGUMENT, who + ": inv_diag of level " + std::to_string(l) + " is null");
  }
  auto op = std::make_unique<MgOp>();
  op->ctx = ctx;
  op->plan = mg_plan(nsmooth, dims, lambda_max, degree, ratio, nullptr, who);
  for (int l = 0; l <= nsmooth; ++l) {
    const ks_operator* f = l < nsmooth ? A[l] : coarse;
    const MgLevel& lv = op->plan.levels[l];
    KS_REQUIRE(f->n_local == lv.rows, KS_ERR_ARGUMENT,
               who + ": " + (l < nsmooth ? "the operator of level " + std::to_string(l) : std::string("the coarse operator")) + " has " +
                   std::to_string(f->n_local) + " rows, the extents " + mg_dims_text(lv.dims) + " of level " + std::to_string(l) + " give " +
                   std::to_string(lv.rows));
  }
  op->plan = mg_plan(nsmooth, dims, lambda_max, degree, ratio, inv_diag, who);   // ... and the entries of inv_diag, now that the sizes are known
  op->coarse = coarse;
  op->theta = shift;
  op->dtype = coarse->dtype;
  op->n_local = op->plan.levels[0].rows;
  op->async_capable = true;
  op->products.assign((size_t)nsmooth + 1, 0);
  const size_t esz = op->dtype == KS_F64 ? 8 : 16;
  auto vec = [&](int64_t rows) {
    void* p = nullptr;
    const size_t bytes = (size_t)std::max<int64_t>(round_up(rows, 64), 64) * esz;
    KS_HIP(hipMalloc(&p, bytes));
    KS_HIP(hipMemset(p, 0, bytes));
    return p;
  };
  op->rhs.assign((size_t)nsmooth + 1, nullptr);
  op->sol.assign((size_t)nsmooth + 1, nullptr);
  op->dir.assign((size_t)nsmooth + 1, nullptr);
  op->tt.assign((size_t)nsmooth + 1, nullptr);
  op->dinv.assign((size_t)nsmooth, nullptr);
  for (int l = 0; l <= nsmooth; ++l) {
    const int64_t rows = op->plan.levels[l].rows;
    if (l >= 1) {
      op->rhs[l] = vec(rows);
      op->sol[l] = vec(rows);
    }
    if (l < nsmooth) {
      op->A.push_back(A[l]);
      op->nnz += 2 * (int64_t)degree * A[l]->nnz;
      op->dir[l] = vec(rows);
      op->tt[l] = vec(rows);
      const size_t bytes = (size_t)round_up(rows, 64) * sizeof(double);
      KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->dinv[l]), bytes));
      KS_HIP(hipMemset(op->dinv[l], 0, bytes));
      KS_HIP(hipMemcpy(op->dinv[l], inv_diag[l], (size_t)rows * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  op->nnz += coarse->nnz;
  return op.release();
}

}  // namespace
