// Preconditioned conjugate-gradient solve  y ~ (A - theta I)^-1 x  for a Hermitian positive definite A - theta I and a Hermitian
// positive definite device operator M ~ (A - theta I)^-1  (ks_operator_pcg, include/kschur.h), and the cheapest such M, the diagonal
// operator  y = d o x  (ks_operator_diagonal).  A sibling of ks_operator_cg (ks_cg.hpp) at every layer: the same products, launch
// shape, partial sums (cg_sum / cg_put), two-slot record protocol and chunked host loop; ks_cg.hpp itself is untouched.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_cg.hpp.
//
//   init:  y = 0, r = b, rho0 = ||b||^2;  z = M r;  tau = Re r^H z;  p = z
//   k = 1, 2, ...
//     A:   q = (A - theta) p                                           A->apply_shifted (theta == 0: A->apply)
//     B:   pq = Re p^H q                                               k_pcg_pq     reads p, q                  16 B/row
//     C:   alpha = tau / pq;  r -= alpha q;  rho' = ||r||^2             k_pcg_resid  reads r, q, writes r        24 B/row
//     M:   z = M r                                                     M->apply
//     D:   tau' = Re r^H z                                             k_pcg_rz     reads r, z                  16 B/row
//     E:   y += alpha p;  done if rho' <= tol^2 rho0;                  k_pcg_dir    reads y, p, z, writes y, p  40 B/row
//          else beta = tau' / tau;  p = z + beta p;  tau = tau'
//
// TWO PATHS, chosen at construction.  GENERIC: M is any operator that can be enqueued ahead; the solver owns r, p, q and z.  FUSED
// JACOBI: M is a diagonal operator (KS_PCG_FUSED=0 forces the generic path): z = d o r is never stored -- k_pcg_resid<true> also reads
// d and sums d r^2 next to r^2 (32 B/row), k_pcg_dir<true> reads r and d instead of z (48 B/row): three launches per iteration like
// ks_operator_cg, 96 B/row against its 80.  The two paths give the SAME BITS: the same grid and block_range partition, z = d r formed
// as one rounded product (mul_nc: the device compiler contracts a plain product into the sum that follows it), and that value fed to
// the very fma chains the generic kernels run on the stored z.
//
// ComplexF64 runs on the real view of 2 n doubles like the CG kernels; one 16-byte pack is then ONE complex element and takes one
// d[i], in Float64 a pack takes d[2 i], d[2 i + 1] (template parameter C).  The odd last element of a Float64 vector is cg_owns_tail's.
//
// SCALARS, RECORD, HOST LOOP: as in ks_cg.hpp with the steps of ks_pcg_plan.hpp.  Every workgroup derives alpha, beta and `done` from
// read-only partial sums; only workgroup 0 of k_pcg_dir (iteration 0: k_pcg_start) writes the record, into slot k & 1.  After done the
// remaining products and M applications of a chunk still run, into q and z only.
#pragma once

namespace ksd {

template <bool C> __device__ __forceinline__ double2 pcg_ld_d(const double* __restrict__ d, int64_t i) {
  if constexpr (C) {
    const double v = d[i];
    return make_double2(v, v);
  } else {
    return ld_pack(d + 2 * i);
  }
}

// z = d o r, each product rounded on its own
__device__ __forceinline__ double2 pcg_dmul(double2 d, double2 r) { return make_double2(mul_nc(d.x, r.x), mul_nc(d.y, r.y)); }

// acc + Re r^H z over one pack: the ONE chain both paths run
__device__ __forceinline__ double pcg_rz_acc(double2 r, double2 z, double acc) { return fma(r.x, z.x, fma(r.y, z.y, acc)); }

// y = d o x: the diagonal operator (24 B/row in Float64).  x and y may be the same vector (every element is read before it is
// written, by the one thread that owns it), so neither is declared __restrict__.
template <bool C>
__global__ void __launch_bounds__(kBlock)
    k_diag_apply(const double* __restrict__ d, const double* x, double* y, int64_t nd, const DevState* __restrict__ st) {
  if (st && st->breakdown >= 0) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) st_pack_nt(y + 2 * i, pcg_dmul(pcg_ld_d<C>(d, i), ld_pack(x + 2 * i)));
  if (cg_owns_tail(nd)) y[nd - 1] = mul_nc(d[nd - 1], x[nd - 1]);
}

// y = 0, r = b, part_rr[workgroup] = sum b^2;  J: p = d o b, part_rz[workgroup] = sum b (d b)
template <bool J, bool C>
__global__ void __launch_bounds__(kBlock)
    k_pcg_init(const double* __restrict__ b, double* __restrict__ y, double* __restrict__ r, double* __restrict__ p,
               const double* __restrict__ d, int64_t nd, double* __restrict__ part_rr, double* __restrict__ part_rz) {
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0, acz = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 v = ld_pack(b + 2 * i);
    st_pack_nt(y + 2 * i, make_double2(0.0, 0.0));
    st_pack(r + 2 * i, v);
    acc += nrm2_pack(v);
    if constexpr (J) {
      const double2 z = pcg_dmul(pcg_ld_d<C>(d, i), v);
      st_pack(p + 2 * i, z);
      acz = pcg_rz_acc(v, z, acz);
    }
  }
  if (cg_owns_tail(nd)) {
    const double v = b[nd - 1];
    y[nd - 1] = 0.0;
    r[nd - 1] = v;
    acc = fma(v, v, acc);
    if constexpr (J) {
      const double z = mul_nc(d[nd - 1], v);
      p[nd - 1] = z;
      acz = fma(v, z, acz);
    }
  }
  cg_put(acc, part_rr, red);
  if constexpr (J) cg_put(acz, part_rz, red);
}

// D: part_rz[workgroup] = sum r z  (k == 0: the start, no record yet)
__global__ void __launch_bounds__(kBlock)
    k_pcg_rz(const double* __restrict__ r, const double* __restrict__ z, int64_t nd, double* __restrict__ part_rz,
             const PcgRecord* __restrict__ rec, int k) {
  if (k > 0) {
    const PcgRecord* in = rec + ((k - 1) & 1);
    if (in->done || in->fail) return;
  }
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) acc = pcg_rz_acc(ld_pack(r + 2 * i), ld_pack(z + 2 * i), acc);
  if (cg_owns_tail(nd)) acc = fma(r[nd - 1], z[nd - 1], acc);
  cg_put(acc, part_rz, red);
}

// rho0 and tau0 from the partial sums of the start, the record of iteration 0 into slot 0 (pcg_start: b not finite and a
// preconditioner that is not positive definite fail, rho0 == 0 is done and y = 0 stands);  z given (the generic path, launched on the
// grid of the other kernels): p = z.  The fused path made p in k_pcg_init and runs ONE workgroup with z == nullptr.
__global__ void __launch_bounds__(kBlock)
    k_pcg_start(const double* __restrict__ z, double* __restrict__ p, int64_t nd, const double* __restrict__ part_rr,
                const double* __restrict__ part_rz, int nb, PcgRecord* __restrict__ rec) {
  __shared__ double red[kBlock / 64];
  const double rho0 = cg_sum(part_rr, nb, red);
  const double tau0 = cg_sum(part_rz, nb, red);
  const PcgStep s = pcg_start(rho0, tau0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    PcgRecord R{};
    R.iteration = 0;
    R.done = s.done;
    R.fail = s.fail;
    R.rho = rho0;
    R.rho0 = rho0;
    R.pq = 0.0;
    R.rho_prev = rho0;
    R.tau = tau0;
    R.tau_prev = tau0;
    rec[0] = R;
  }
  if (!z || s.done || s.fail) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) st_pack(p + 2 * i, ld_pack_nt(z + 2 * i));
  if (cg_owns_tail(nd)) p[nd - 1] = z[nd - 1];
}

// B: part_pq[workgroup] = sum p q
__global__ void __launch_bounds__(kBlock)
    k_pcg_pq(const double* __restrict__ p, const double* __restrict__ q, int64_t nd, double* __restrict__ part_pq,
             const PcgRecord* __restrict__ rec, int k) {
  const PcgRecord* in = rec + ((k - 1) & 1);
  if (in->done || in->fail) return;
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 pv = ld_pack(p + 2 * i), qv = ld_pack(q + 2 * i);
    acc = fma(pv.x, qv.x, fma(pv.y, qv.y, acc));
  }
  if (cg_owns_tail(nd)) acc = fma(p[nd - 1], q[nd - 1], acc);
  cg_put(acc, part_pq, red);
}

// C: alpha = tau / pq;  r -= alpha q;  part_rr[workgroup] = sum r^2;  J: part_rz[workgroup] = sum r (d r).  A step that failed on pq
// (pcg_step) touches nothing: k_pcg_dir reports it.
template <bool J, bool C>
__global__ void __launch_bounds__(kBlock)
    k_pcg_resid(double* __restrict__ r, const double* __restrict__ q, const double* __restrict__ d, int64_t nd,
                const double* __restrict__ part_pq, double* __restrict__ part_rr, double* __restrict__ part_rz, int nb,
                const PcgRecord* __restrict__ rec, int k) {
  const PcgRecord* in = rec + ((k - 1) & 1);
  if (in->done || in->fail) return;
  __shared__ double red[kBlock / 64];
  const double pq = cg_sum(part_pq, nb, red);
  const PcgStep s = pcg_step(in->tau, pq, 0.0, 0.0);
  if (s.fail) return;
  const double alpha = s.alpha;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0, acz = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 rv = ld_pack(r + 2 * i);
    const double2 qv = ld_pack_nt(q + 2 * i);
    rv.x = fma(-alpha, qv.x, rv.x);
    rv.y = fma(-alpha, qv.y, rv.y);
    st_pack(r + 2 * i, rv);
    acc += nrm2_pack(rv);
    if constexpr (J) acz = pcg_rz_acc(rv, pcg_dmul(pcg_ld_d<C>(d, i), rv), acz);
  }
  if (cg_owns_tail(nd)) {
    const double v = fma(-alpha, q[nd - 1], r[nd - 1]);
    r[nd - 1] = v;
    acc = fma(v, v, acc);
    if constexpr (J) acz = fma(v, mul_nc(d[nd - 1], v), acz);
  }
  cg_put(acc, part_rr, red);
  if constexpr (J) cg_put(acz, part_rz, red);
}

// E: y += alpha p;  done: nothing else;  else p = z + beta p with z = zr (generic, its last use) or d o zr (J: zr is r).  Every
// workgroup derives the step from the partial sums; workgroup 0 writes the record of iteration k into slot k & 1 (a finished or
// failed solve: the record it found, carried forward).
template <bool J, bool C>
__global__ void __launch_bounds__(kBlock)
    k_pcg_dir(double* __restrict__ y, double* __restrict__ p, const double* __restrict__ zr, const double* __restrict__ d, int64_t nd,
              const double* __restrict__ part_pq, const double* __restrict__ part_rr, const double* __restrict__ part_rz, int nb,
              double tol2, PcgRecord* __restrict__ rec, int k) {
  const PcgRecord* in = rec + ((k - 1) & 1);
  PcgRecord* out = rec + (k & 1);
  const PcgRecord was = *in;
  if (was.done || was.fail) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = was;
    return;
  }
  __shared__ double red[kBlock / 64];
  const double pq = cg_sum(part_pq, nb, red);
  const double rho_new = cg_sum(part_rr, nb, red);   // (of a step that failed on pq: stale sums, which the steps do not look at)
  const double tau_new = cg_sum(part_rz, nb, red);
  const PcgStep s = pcg_step(was.tau, pq, rho_new, tol2 * was.rho0);
  PcgBeta bt{0.0, 0};
  if (!s.fail && !s.done) bt = pcg_beta(was.tau, tau_new);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    PcgRecord R = was;
    R.iteration = k;
    R.done = s.done;
    R.fail = s.fail ? s.fail : bt.fail;
    R.pq = pq;
    R.rho_prev = was.rho;
    R.rho = s.fail == KS_PCG_FAIL_CURVATURE ? was.rho : rho_new;   // (a step that failed on pq left r alone)
    R.tau_prev = was.tau;
    R.tau = s.fail ? was.tau : tau_new;
    *out = R;
  }
  if (s.fail) return;
  const double alpha = s.alpha, beta = bt.beta;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  if (s.done || bt.fail) {   // (a preconditioner that failed now: y still takes the step r has taken)
    for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
      double2 yv = ld_pack(y + 2 * i);
      const double2 pv = ld_pack(p + 2 * i);
      yv.x = fma(alpha, pv.x, yv.x);
      yv.y = fma(alpha, pv.y, yv.y);
      st_pack_nt(y + 2 * i, yv);
    }
    if (cg_owns_tail(nd)) y[nd - 1] = fma(alpha, p[nd - 1], y[nd - 1]);
    return;
  }
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 yv = ld_pack(y + 2 * i);
    double2 pv = ld_pack(p + 2 * i);
    double2 zv;
    if constexpr (J) zv = pcg_dmul(pcg_ld_d<C>(d, i), ld_pack(zr + 2 * i));
    else zv = ld_pack_nt(zr + 2 * i);
    yv.x = fma(alpha, pv.x, yv.x);
    yv.y = fma(alpha, pv.y, yv.y);
    pv.x = fma(beta, pv.x, zv.x);
    pv.y = fma(beta, pv.y, zv.y);
    st_pack_nt(y + 2 * i, yv);
    st_pack(p + 2 * i, pv);   // (cacheable: the next product gathers exactly this vector)
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    const double pv = p[i];
    double zv = zr[i];
    if constexpr (J) zv = mul_nc(d[i], zv);
    y[i] = fma(alpha, pv, y[i]);
    p[i] = fma(beta, pv, zv);
  }
}

}  // namespace ksd

namespace {

// y = d o x with a real d (Float64 or ComplexF64 vectors): one streaming kernel, enqueued ahead like a stored matrix
struct DiagOp : ks_operator {
  double* d = nullptr;   // n_local values, allocated like a basis column (a multiple of 64, the pad zero)
  ~DiagOp() override { (void)hipFree(d); }
  void apply(const void* x, void* y, const DevState* st) override {
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "diagonal operator: a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    const int64_t nd = n_local * (dtype == KS_F64 ? 1 : 2);
    const int nb = CgOp::cg_blocks(ctx, nd);
    ProfScope ps(ctx, KSP_SPMV, 8.0 * (double)(nd + nd + n_local));
    if (dtype == KS_F64) ksd::k_diag_apply<false><<<nb, kBlock, 0, ctx->stream>>>(d, static_cast<const double*>(x), static_cast<double*>(y), nd, st);
    else ksd::k_diag_apply<true><<<nb, kBlock, 0, ctx->stream>>>(d, static_cast<const double*>(x), static_cast<double*>(y), nd, st);
    KS_HIP(hipGetLastError());
  }
};

inline ks_operator* make_diagonal(ks_ctx* ctx, int64_t n, int dtype, const double* d) {
  KS_REQUIRE(n >= 1 && n < (int64_t)2147483647, KS_ERR_ARGUMENT, "ks_operator_diagonal: n must be in [1, 2^31)");
  for (int64_t i = 0; i < n; ++i)
    KS_REQUIRE(std::isfinite(d[i]), KS_ERR_ARGUMENT, "ks_operator_diagonal: entry " + std::to_string(i) + " is not finite");
  auto op = std::make_unique<DiagOp>();
  op->ctx = ctx;
  op->n_local = n;
  op->nnz = n;
  op->dtype = dtype;
  const size_t bytes = (size_t)round_up(n, 64) * sizeof(double);
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->d), bytes));
  KS_HIP(hipMemset(op->d, 0, bytes));
  KS_HIP(hipMemcpy(op->d, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
  return op.release();
}

struct PcgOp : ks_operator {
  ks_operator* A = nullptr;
  ks_operator* M = nullptr;
  const double* jacobi = nullptr;   // the fused path: M's diagonal (borrowed with M)
  double theta = 0.0, tol = 0.0;
  int maxit = 0, check_every = kCgDefaultCheckEvery;
  void* vec[4] = {nullptr, nullptr, nullptr, nullptr};   // r, p, q and, on the generic path, z
  double* part = nullptr;                                // [3][nb]: partial sums of p q, of r^2 and of r z
  PcgRecord* rec = nullptr;                              // device, two slots
  PcgRecord* rec_h = nullptr;                            // pinned copy of both
  hipEvent_t ev = nullptr;
  int nb = 1;
  int64_t applications = 0, iterations = 0, precond_applications = 0;
  int last_iterations = 0;
  double last_relres = 0.0, worst_relres = 0.0;
  ~PcgOp() override {
    for (void* v : vec) (void)hipFree(v);
    (void)hipFree(part); (void)hipFree(rec);
    (void)hipHostFree(rec_h);
    if (ev) (void)hipEventDestroy(ev);
  }
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "preconditioned conjugate gradients: the solve needs distinct x and y");
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "preconditioned conjugate gradients: a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    hipStream_t s = ctx->stream;
    const bool cx = dtype != KS_F64;
    const int64_t nd = n_local * (cx ? 2 : 1), ld = round_up(n_local, 64);
    const double B = 8.0 * (double)nd, D = 8.0 * (double)n_local;
    double* r = static_cast<double*>(vec[0]);
    double* p = static_cast<double*>(vec[1]);
    double* q = static_cast<double*>(vec[2]);
    double* z = static_cast<double*>(vec[3]);
    double* yd = static_cast<double*>(y);
    const double* b = static_cast<const double*>(x);
    double *part_pq = part, *part_rr = part + nb, *part_rz = part + 2 * nb;
    auto precondition = [&](int k) {   // the generic path: z = M r, part_rz = sum r z
      M->in_scale = 1.0;
      M->apply(r, z, st);
      ++precond_applications;
      ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
      ksd::k_pcg_rz<<<nb, kBlock, 0, s>>>(r, z, nd, part_rz, rec, k);
    };
    if (jacobi) {
      ProfScope ps(ctx, KSP_SCALE, 4.0 * B + D);
      if (cx) ksd::k_pcg_init<true, true><<<nb, kBlock, 0, s>>>(b, yd, r, p, jacobi, nd, part_rr, part_rz);
      else ksd::k_pcg_init<true, false><<<nb, kBlock, 0, s>>>(b, yd, r, p, jacobi, nd, part_rr, part_rz);
      ksd::k_pcg_start<<<1, kBlock, 0, s>>>(nullptr, p, nd, part_rr, part_rz, nb, rec);
      ++precond_applications;
    } else {
      {
        ProfScope ps(ctx, KSP_SCALE, 3.0 * B);
        ksd::k_pcg_init<false, false><<<nb, kBlock, 0, s>>>(b, yd, r, p, nullptr, nd, part_rr, part_rz);
      }
      precondition(0);
      ProfScope ps(ctx, KSP_SCALE, 2.0 * B);
      ksd::k_pcg_start<<<nb, kBlock, 0, s>>>(z, p, nd, part_rr, part_rz, nb, rec);
    }
    KS_HIP(hipGetLastError());
    ++applications;
    const int every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
    const double tol2 = tol * tol;
    int k = 0;
    PcgRecord R{};
    for (;;) {
      const int upto = std::min(maxit, k + every);
      while (k < upto) {
        ++k;
        A->in_scale = 1.0;
        if (theta == 0.0) A->apply(p, q, st);
        else A->apply_shifted(p, q, theta, 0.0, 1.0, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_pcg_pq<<<nb, kBlock, 0, s>>>(p, q, nd, part_pq, rec, k);
        }
        if (jacobi) {
          {
            ProfScope ps(ctx, KSP_AXPY, 3.0 * B + D);
            if (cx) ksd::k_pcg_resid<true, true><<<nb, kBlock, 0, s>>>(r, q, jacobi, nd, part_pq, part_rr, part_rz, nb, rec, k);
            else ksd::k_pcg_resid<true, false><<<nb, kBlock, 0, s>>>(r, q, jacobi, nd, part_pq, part_rr, part_rz, nb, rec, k);
          }
          ProfScope ps(ctx, KSP_FUSED, 5.0 * B + D);
          if (cx) ksd::k_pcg_dir<true, true><<<nb, kBlock, 0, s>>>(yd, p, r, jacobi, nd, part_pq, part_rr, part_rz, nb, tol2, rec, k);
          else ksd::k_pcg_dir<true, false><<<nb, kBlock, 0, s>>>(yd, p, r, jacobi, nd, part_pq, part_rr, part_rz, nb, tol2, rec, k);
        } else {
          {
            ProfScope ps(ctx, KSP_AXPY, 3.0 * B);
            ksd::k_pcg_resid<false, false><<<nb, kBlock, 0, s>>>(r, q, nullptr, nd, part_pq, part_rr, part_rz, nb, rec, k);
          }
          precondition(k);
          ProfScope ps(ctx, KSP_FUSED, 5.0 * B);
          ksd::k_pcg_dir<false, false><<<nb, kBlock, 0, s>>>(yd, p, z, nullptr, nd, part_pq, part_rr, part_rz, nb, tol2, rec, k);
        }
        KS_HIP(hipGetLastError());
      }
      KS_HIP(hipMemcpyAsync(rec_h, rec, 2 * sizeof(PcgRecord), hipMemcpyDeviceToHost, s));
      KS_HIP(hipEventRecord(ev, s));
      KS_HIP(hipEventSynchronize(ev));
      R = rec_h[k & 1];
      if (R.done || R.fail || k >= maxit) break;
    }
    if (jacobi) precond_applications += R.iteration;   // (d o r is formed once per iteration that ran, inside k_pcg_resid)
    last_iterations = R.iteration;
    iterations += R.iteration;
    last_relres = R.rho0 > 0.0 ? std::sqrt(R.rho / R.rho0) : 0.0;
    if (!(last_relres <= worst_relres)) worst_relres = last_relres;   // (a NaN sticks)
    auto sci = [](double v) { char buf[40]; std::snprintf(buf, sizeof buf, "%.6g", v); return std::string(buf); };
    const std::string at = " at iteration " + std::to_string(R.iteration);
    switch (R.fail) {
      case 0: break;
      case KS_PCG_FAIL_RHS: throw KsError{KS_ERR_OPERATOR, "ks_operator_pcg: the right-hand side is not finite"};
      case KS_PCG_FAIL_CURVATURE: throw KsError{KS_ERR_OPERATOR, "ks_operator_pcg: not positive definite: p^H (A - theta) p = " + sci(R.pq) + at};
      case KS_PCG_FAIL_PRECONDITIONER:
        throw KsError{KS_ERR_OPERATOR, "ks_operator_pcg: the preconditioner is not positive definite: r^H M r = " + sci(R.tau) + at};
      default: throw KsError{KS_ERR_OPERATOR, "ks_operator_pcg: the residual is not finite" + at};
    }
    if (!R.done)
      throw KsError{KS_ERR_OPERATOR, "ks_operator_pcg: did not converge: relative residual " + sci(last_relres) + " after " + std::to_string(maxit) + " iterations"};
  }
};

inline ks_operator* make_pcg(ks_ctx* ctx, ks_operator* A, ks_operator* M, double shift, double tol, int maxit, int check_every) {
  auto op = std::make_unique<PcgOp>();
  op->ctx = ctx;
  KS_REQUIRE(A->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_pcg: the operator lives on another context");
  KS_REQUIRE(A->dtype == KS_F64 || A->dtype == KS_C64, KS_ERR_ARGUMENT, "ks_operator_pcg: the operator is neither Float64 nor ComplexF64");
  KS_REQUIRE(A->async_capable, KS_ERR_ARGUMENT,
             "ks_operator_pcg: the operator cannot be enqueued ahead (a host callback, an iterative solve, or a product or filter of one)");
  KS_REQUIRE(M->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_pcg: the preconditioner lives on another context");
  KS_REQUIRE(M->dtype == A->dtype, KS_ERR_ARGUMENT, "ks_operator_pcg: the preconditioner does not have the element type of the operator");
  KS_REQUIRE(M->n_local == A->n_local, KS_ERR_ARGUMENT,
             "ks_operator_pcg: the preconditioner has " + std::to_string(M->n_local) + " rows, the operator has " + std::to_string(A->n_local));
  KS_REQUIRE(M->async_capable, KS_ERR_ARGUMENT,
             "ks_operator_pcg: the preconditioner cannot be enqueued ahead (a host callback, an iterative solve, or a product or filter of "
             "one: a solve as preconditioner varies from step to step and needs flexible conjugate gradients)");
  KS_REQUIRE(std::isfinite(tol) && tol > 0.0 && tol < 1.0, KS_ERR_ARGUMENT, "ks_operator_pcg: tol = " + std::to_string(tol) + " (must lie in (0, 1))");
  KS_REQUIRE(maxit >= 1, KS_ERR_ARGUMENT, "ks_operator_pcg: maxit = " + std::to_string(maxit) + " (must be at least 1)");
  KS_REQUIRE(check_every >= 0, KS_ERR_ARGUMENT, "ks_operator_pcg: check_every = " + std::to_string(check_every) + " (must not be negative; 0: the library default)");
  KS_REQUIRE(std::isfinite(shift), KS_ERR_ARGUMENT, "ks_operator_pcg: shift is not finite");
  op->A = A;
  op->M = M;
  if (const DiagOp* dg = dynamic_cast<const DiagOp*>(M); dg && env_int("KS_PCG_FUSED", 1) != 0) op->jacobi = dg->d;
  op->theta = shift;
  op->tol = tol;
  op->maxit = maxit;
  op->check_every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
  op->n_local = A->n_local;
  op->dtype = A->dtype;
  op->async_capable = false;   // the host reads the record between chunks: one step per batch, like a host callback
  op->nnz = A->nnz;
  const int64_t nd = op->n_local * (op->dtype == KS_F64 ? 1 : 2);
  op->nb = CgOp::cg_blocks(ctx, nd);
  const size_t bytes = (size_t)std::max<int64_t>(round_up(op->n_local, 64), 64) * (op->dtype == KS_F64 ? 8 : 16);
  for (int t = 0; t < (op->jacobi ? 3 : 4); ++t) {
    KS_HIP(hipMalloc(&op->vec[t], bytes));
    KS_HIP(hipMemset(op->vec[t], 0, bytes));
  }
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->part), (size_t)3 * op->nb * sizeof(double)));
  KS_HIP(hipMemset(op->part, 0, (size_t)3 * op->nb * sizeof(double)));
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->rec), 2 * sizeof(PcgRecord)));
  KS_HIP(hipMemset(op->rec, 0, 2 * sizeof(PcgRecord)));
  KS_HIP(hipHostMalloc(reinterpret_cast<void**>(&op->rec_h), 2 * sizeof(PcgRecord)));
  KS_HIP(hipEventCreateWithFlags(&op->ev, hipEventDisableTiming));
  return op.release();
}

}  // namespace
