// Conjugate-gradient solve  y ~ (A - theta I)^-1 x  for a Hermitian positive definite A - theta I  (ks_operator_cg, include/kschur.h):
// the inner iterative solver of the reference's "LinearMap around a solve" (docs/src/index.md:234-259, 273-287) for operators that
// have nothing to factor -- M^-1 K of matrix-free finite elements, (A - sigma)^-1 with sigma below the spectrum.
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_cheb.hpp.
//
// A is BORROWED like a product's factors.  The solver owns r, p and q, allocated like ProductOp's temporaries (a multiple of 64
// elements, zero-filled once: stored-matrix kernels may read the pad rows of p; every kernel writes rows < n_local only).
//
//   init:  y = 0, r = p = b, rho = rho0 = ||b||^2                       k_cg_init (32 B/row) + k_cg_start (one workgroup)
//   k = 1, 2, ...
//     A:   q = (A - theta) p                                           A->apply_shifted (theta == 0: A->apply)
//     B:   pq = Re p^H q                                               k_cg_pq      reads p, q                  16 B/row
//     C:   alpha = rho / pq;  r -= alpha q;  rho' = ||r||^2             k_cg_resid   reads r, q, writes r        24 B/row
//     D:   y += alpha p;  done if rho' <= tol^2 rho0;                  k_cg_dir     reads y, p, r, writes y, p  40 B/row
//          else beta = rho' / rho;  p = r + beta p;  rho = rho'
//
// ONE set of kernels: ComplexF64 runs them on the real view of 2 n doubles (Re p^H q is the real dot product of the two views, alpha
// and beta are real).  Launch shape of k_dots / k_axpy: 256 threads, a contiguous range of 16-byte packs per workgroup, the odd last
// element of a Float64 vector alone in straight-line code; the grid is a fixed function of n and the device (cg_blocks).
//
// SCALARS.  Per-workgroup partial sums go to a [workgroup] array; every consumer workgroup adds them in one fixed order (cg_sum) and
// runs the scalar step (cg_step, ks_cg_plan.hpp) itself: identical inputs, identical code, identical alpha, beta and `done` in every
// workgroup and in every run.  Only workgroup 0 of k_cg_dir writes state, the record of ks_cg_plan.hpp, into slot k & 1; the kernels
// of iteration k read slot (k - 1) & 1 at entry and return when it says done or fail (k_cg_dir then carries the record forward into
// its slot).  No kernel acts on a word that a sibling workgroup of the same launch may be writing.
//
// THE HOST enqueues check_every iterations, copies both slots into pinned memory and waits for an event behind that copy; it goes on
// until done, fail or maxit.  After done the remaining products of a chunk still run into q, nothing else is touched: y and the
// iteration count do not depend on check_every.
#pragma once

namespace ksd {

// sum of part[0 .. nb) in a fixed order, the same value in every thread of every workgroup that asks (all 256 threads call it)
__device__ __forceinline__ double cg_sum(const double* __restrict__ part, int nb, double* red) {
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += kBlock) s += part[b];
  s = wave_sum(s);
  __syncthreads();   // (red may still be read from an earlier sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// this workgroup's sum -> part[blockIdx.x]
__device__ __forceinline__ void cg_put(double acc, double* __restrict__ part, double* red) {
  const double s = wave_sum(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the odd last element of the real view (Float64, odd n) belongs to thread 0 of the last workgroup
__device__ __forceinline__ bool cg_owns_tail(int64_t nd) { return (nd & 1) && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0; }

// y = 0, r = p = b, part_rr[workgroup] = sum b^2
__global__ void __launch_bounds__(kBlock)
    k_cg_init(const double* __restrict__ b, double* __restrict__ y, double* __restrict__ r, double* __restrict__ p, int64_t nd,
              double* __restrict__ part_rr) {
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 v = ld_pack(b + 2 * i);
    st_pack_nt(y + 2 * i, make_double2(0.0, 0.0));
    st_pack(r + 2 * i, v);
    st_pack(p + 2 * i, v);
    acc += nrm2_pack(v);
  }
  if (cg_owns_tail(nd)) {
    const double v = b[nd - 1];
    y[nd - 1] = 0.0;
    r[nd - 1] = v;
    p[nd - 1] = v;
    acc = fma(v, v, acc);
  }
  cg_put(acc, part_rr, red);
}

// ONE workgroup: rho0 from the partial sums of k_cg_init, the record of iteration 0 into slot 0.  rho0 == 0: done, y = 0 stands;
// rho0 not finite: fail.
__global__ void __launch_bounds__(kBlock) k_cg_start(const double* __restrict__ part_rr, int nb, CgRecord* __restrict__ rec) {
  __shared__ double red[kBlock / 64];
  const double rho0 = cg_sum(part_rr, nb, red);
  if (threadIdx.x == 0) {
    CgRecord R{};
    R.iteration = 0;
    R.done = rho0 == 0.0 ? 1 : 0;
    R.fail = cg_finite(rho0) ? 0 : 1;
    R.rho = rho0;
    R.rho0 = rho0;
    R.pq = 0.0;
    R.rho_prev = rho0;
    rec[0] = R;
  }
}

// B: part_pq[workgroup] = sum p q
__global__ void __launch_bounds__(kBlock)
    k_cg_pq(const double* __restrict__ p, const double* __restrict__ q, int64_t nd, double* __restrict__ part_pq,
            const CgRecord* __restrict__ rec, int k) {
  const CgRecord* in = rec + ((k - 1) & 1);
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

// C: alpha = rho / pq;  r -= alpha q;  part_rr[workgroup] = sum r^2.  A failed step (cg_step) touches nothing: k_cg_dir reports it.
__global__ void __launch_bounds__(kBlock)
    k_cg_resid(double* __restrict__ r, const double* __restrict__ q, int64_t nd, const double* __restrict__ part_pq,
               double* __restrict__ part_rr, int nb, const CgRecord* __restrict__ rec, int k) {
  const CgRecord* in = rec + ((k - 1) & 1);
  if (in->done || in->fail) return;
  __shared__ double red[kBlock / 64];
  const double pq = cg_sum(part_pq, nb, red);
  const CgStep s = cg_step(in->rho, pq, 0.0, 0.0);
  if (s.fail) return;
  const double alpha = s.alpha;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 rv = ld_pack(r + 2 * i);
    const double2 qv = ld_pack_nt(q + 2 * i);
    rv.x = fma(-alpha, qv.x, rv.x);
    rv.y = fma(-alpha, qv.y, rv.y);
    st_pack(r + 2 * i, rv);
    acc += nrm2_pack(rv);
  }
  if (cg_owns_tail(nd)) {
    const double v = fma(-alpha, q[nd - 1], r[nd - 1]);
    r[nd - 1] = v;
    acc = fma(v, v, acc);
  }
  cg_put(acc, part_rr, red);
}

// D: y += alpha p;  done: nothing else;  else p = r + beta p.  Every workgroup derives the step from the partial sums; workgroup 0
// writes the record of iteration k into slot k & 1 (a finished or failed solve: the record it found, carried forward).
__global__ void __launch_bounds__(kBlock)
    k_cg_dir(double* __restrict__ y, double* __restrict__ p, const double* __restrict__ r, int64_t nd,
             const double* __restrict__ part_pq, const double* __restrict__ part_rr, int nb, double tol2, CgRecord* __restrict__ rec, int k) {
  const CgRecord* in = rec + ((k - 1) & 1);
  CgRecord* out = rec + (k & 1);
  const CgRecord was = *in;
  if (was.done || was.fail) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = was;
    return;
  }
  __shared__ double red[kBlock / 64];
  const double pq = cg_sum(part_pq, nb, red);
  const double rho_new = cg_sum(part_rr, nb, red);   // (of a step that failed on pq: a stale sum, which cg_step does not look at)
  const CgStep s = cg_step(was.rho, pq, rho_new, tol2 * was.rho0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    CgRecord R = was;
    R.iteration = k;
    R.done = s.done;
    R.fail = s.fail;
    R.pq = pq;
    R.rho_prev = was.rho;
    R.rho = (s.fail && cg_step(was.rho, pq, 0.0, 0.0).fail) ? was.rho : rho_new;   // (a step that failed on pq left r alone)
    *out = R;
  }
  if (s.fail) return;
  const double alpha = s.alpha, beta = s.beta;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  if (s.done) {
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
    const double2 rv = ld_pack(r + 2 * i);
    yv.x = fma(alpha, pv.x, yv.x);
    yv.y = fma(alpha, pv.y, yv.y);
    pv.x = fma(beta, pv.x, rv.x);
    pv.y = fma(beta, pv.y, rv.y);
    st_pack_nt(y + 2 * i, yv);
    st_pack(p + 2 * i, pv);   // (cacheable: the next product gathers exactly this vector)
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    const double pv = p[i];
    y[i] = fma(alpha, pv, y[i]);
    p[i] = fma(beta, pv, r[i]);
  }
}

}  // namespace ksd

namespace {

struct CgOp : ks_operator {
  ks_operator* A = nullptr;
  double theta = 0.0, tol = 0.0;
  int maxit = 0, check_every = kCgDefaultCheckEvery;
  void* vec[3] = {nullptr, nullptr, nullptr};   // r, p, q
  double* part = nullptr;                       // [2][nb]: partial sums of p q and of r^2
  CgRecord* rec = nullptr;                      // device, two slots
  CgRecord* rec_h = nullptr;                    // pinned copy of both
  hipEvent_t ev = nullptr;
  int nb = 1;
  int64_t applications = 0, iterations = 0;
  int last_iterations = 0;
  double last_relres = 0.0, worst_relres = 0.0;
  ~CgOp() override {
    (void)hipFree(vec[0]); (void)hipFree(vec[1]); (void)hipFree(vec[2]); (void)hipFree(part); (void)hipFree(rec);
    (void)hipHostFree(rec_h);
    if (ev) (void)hipEventDestroy(ev);
  }
  // workgroups of every CG kernel: a fixed function of the number of 16-byte packs and the device (two packs per lane at least)
  static int cg_blocks(const ks_ctx* ctx, int64_t nd) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->num_cu * 4, (nd / 2 + 2 * kBlock - 1) / (2 * kBlock)));
  }
  // (the profile classes name the shape of the work: inner products / update and norm / two updates in one pass)
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "conjugate gradients: the solve needs distinct x and y");
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "conjugate gradients: a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    hipStream_t s = ctx->stream;
    const int64_t nd = n_local * (dtype == KS_F64 ? 1 : 2), ld = round_up(n_local, 64);
    const double B = 8.0 * (double)nd;
    double* r = static_cast<double*>(vec[0]);
    double* p = static_cast<double*>(vec[1]);
    double* q = static_cast<double*>(vec[2]);
    double* yd = static_cast<double*>(y);
    double *part_pq = part, *part_rr = part + nb;
    {
      ProfScope ps(ctx, KSP_SCALE, 4.0 * B);
      ksd::k_cg_init<<<nb, kBlock, 0, s>>>(static_cast<const double*>(x), yd, r, p, nd, part_rr);
      ksd::k_cg_start<<<1, kBlock, 0, s>>>(part_rr, nb, rec);
      KS_HIP(hipGetLastError());
    }
    ++applications;
    const int every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
    int k = 0;
    CgRecord R{};
    for (;;) {
      const int upto = std::min(maxit, k + every);
      while (k < upto) {
        ++k;
        A->in_scale = 1.0;
        if (theta == 0.0) A->apply(p, q, st);
        else A->apply_shifted(p, q, theta, 0.0, 1.0, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_cg_pq<<<nb, kBlock, 0, s>>>(p, q, nd, part_pq, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_AXPY, 3.0 * B);
          ksd::k_cg_resid<<<nb, kBlock, 0, s>>>(r, q, nd, part_pq, part_rr, nb, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_FUSED, 5.0 * B);
          ksd::k_cg_dir<<<nb, kBlock, 0, s>>>(yd, p, r, nd, part_pq, part_rr, nb, tol * tol, rec, k);
        }
        KS_HIP(hipGetLastError());
      }
      KS_HIP(hipMemcpyAsync(rec_h, rec, 2 * sizeof(CgRecord), hipMemcpyDeviceToHost, s));
      KS_HIP(hipEventRecord(ev, s));
      KS_HIP(hipEventSynchronize(ev));
      R = rec_h[k & 1];
      if (R.done || R.fail || k >= maxit) break;
    }
    last_iterations = R.iteration;
    iterations += R.iteration;
    last_relres = R.rho0 > 0.0 ? std::sqrt(R.rho / R.rho0) : 0.0;
    if (!(last_relres <= worst_relres)) worst_relres = last_relres;   // (a NaN sticks)
    auto sci = [](double v) { char buf[40]; std::snprintf(buf, sizeof buf, "%.6g", v); return std::string(buf); };
    if (R.fail) {
      if (R.iteration == 0) throw KsError{KS_ERR_OPERATOR, "ks_operator_cg: the right-hand side is not finite"};
      if (!cg_finite(R.pq) || !(R.pq > 0.0) || cg_finite(R.rho))
        throw KsError{KS_ERR_OPERATOR, "ks_operator_cg: not positive definite: p^H (A - theta) p = " + sci(R.pq) + " at iteration " + std::to_string(R.iteration)};
      throw KsError{KS_ERR_OPERATOR, "ks_operator_cg: the residual is not finite at iteration " + std::to_string(R.iteration)};
    }
    if (!R.done)
      throw KsError{KS_ERR_OPERATOR, "ks_operator_cg: did not converge: relative residual " + sci(last_relres) + " after " + std::to_string(maxit) + " iterations"};
  }
};

inline ks_operator* make_cg(ks_ctx* ctx, ks_operator* A, double shift, double tol, int maxit, int check_every) {
  auto op = std::make_unique<CgOp>();
  op->ctx = ctx;
  KS_REQUIRE(A->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_cg: the operator lives on another context");
  KS_REQUIRE(A->dtype == KS_F64 || A->dtype == KS_C64, KS_ERR_ARGUMENT, "ks_operator_cg: the operator is neither Float64 nor ComplexF64");
  KS_REQUIRE(A->async_capable, KS_ERR_ARGUMENT,
             "ks_operator_cg: the operator cannot be enqueued ahead (a host callback, another conjugate-gradient solve, or a product or filter of one)");
  KS_REQUIRE(std::isfinite(tol) && tol > 0.0 && tol < 1.0, KS_ERR_ARGUMENT, "ks_operator_cg: tol = " + std::to_string(tol) + " (must lie in (0, 1))");
  KS_REQUIRE(maxit >= 1, KS_ERR_ARGUMENT, "ks_operator_cg: maxit = " + std::to_string(maxit) + " (must be at least 1)");
  KS_REQUIRE(check_every >= 0, KS_ERR_ARGUMENT, "ks_operator_cg: check_every = " + std::to_string(check_every) + " (must not be negative; 0: the library default)");
  KS_REQUIRE(std::isfinite(shift), KS_ERR_ARGUMENT, "ks_operator_cg: shift is not finite");
  op->A = A;
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
  for (int t = 0; t < 3; ++t) {
    KS_HIP(hipMalloc(&op->vec[t], bytes));
    KS_HIP(hipMemset(op->vec[t], 0, bytes));
  }
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->part), (size_t)2 * op->nb * sizeof(double)));
  KS_HIP(hipMemset(op->part, 0, (size_t)2 * op->nb * sizeof(double)));
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->rec), 2 * sizeof(CgRecord)));
  KS_HIP(hipMemset(op->rec, 0, 2 * sizeof(CgRecord)));
  KS_HIP(hipHostMalloc(reinterpret_cast<void**>(&op->rec_h), 2 * sizeof(CgRecord)));
  KS_HIP(hipEventCreateWithFlags(&op->ev, hipEventDisableTiming));
  return op.release();
}

}  // namespace
