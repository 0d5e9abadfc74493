// MINRES solve  y ~ (A - theta I)^-1 x  for a Hermitian A and ANY real theta that is not an eigenvalue (ks_operator_minres,
// include/kschur.h): shift-invert inside the spectrum of an operator that has nothing to factor -- the inner iterative solver of the
// reference's "LinearMap around a solve" (docs/src/index.md:234-259) where ks_operator_cg (ks_cg.hpp) stops at its first negative
// curvature.  Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_cg.hpp, whose record protocol,
// partial sums (cg_sum / cg_put), launch shape and host loop it shares.
//
// A is BORROWED like a product's factors.  The solver owns five vectors, allocated like CgOp's (a multiple of 64 elements,
// zero-filled once; every kernel writes rows < n_local only): the Lanczos vectors v and v_ (two buffers that swap roles every
// iteration), q (the product, then r in place) and the directions w_ and w__ (two buffers that swap roles: the new w is written over
// w__, which nothing reads again).
//
//   init:  y = 0, beta1 = ||b||, v = b / beta1, (c, s) = (c_, s_) = (1, 0), beta = 0, phibar = beta1
//                                                            k_mr_init (16 B/row) + k_mr_start (16 B/row)
//   k = 1, 2, ...
//     A:   q = (A - theta) v                                                      A->apply_shifted (theta == 0: A->apply)
//     B:   alpha = Re v^H q                                  k_mr_alpha  reads v, q                                   16 B/row
//     C:   r = q - beta v_ - alpha v (over q);  beta' = ||r||  k_mr_resid  reads q, v_, v, writes r                     32 B/row
//     D:   the step (mr_step, ks_minres_plan.hpp);  w = (v - eps w__ - delta w_) / gamma;  y += phi w;
//          done if |phibar'| <= tol beta1, else v+ = r / beta' over v_, w over w__
//                                                            k_mr_step   reads v, w__, w_, y, r, writes w, y, v+      64 B/row
//                                                                        (a finishing step: reads v, w__, w_, y, writes y: 40 B/row)
//
// The first iteration reads neither v_ nor a direction, the second no w__: their coefficients are exactly zero there (beta = 0,
// delta = eps = 0 under the identity rotations), and the buffers may hold what a failed solve left behind.  k is a kernel argument,
// so the choice is uniform over the launch.
//
// ONE set of kernels: ComplexF64 runs them on the real view of 2 n doubles (alpha, beta and every rotation are real).  Scalars,
// record and host loop: as in ks_cg.hpp -- every workgroup derives the step from the per-workgroup partial sums added in one fixed
// order, only workgroup 0 of k_mr_step writes the record of iteration k, into slot k & 1; the kernels of iteration k read slot
// (k - 1) & 1 at entry and return when it says done or fail.
//
// THE HOST enqueues check_every iterations, copies both slots into pinned memory and waits for an event behind that copy; it goes on
// until done, fail or maxit.  After done the remaining PRODUCTS of a chunk still run in full, into q; only the k_mr_* kernels return
// at entry.  Nothing but q is touched, so y and the iteration count do not depend on check_every.
#pragma once

namespace ksd {

// y = 0, part_bb[workgroup] = sum b^2
__global__ void __launch_bounds__(kBlock)
    k_mr_init(const double* __restrict__ b, double* __restrict__ y, int64_t nd, double* __restrict__ part_bb) {
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 v = ld_pack(b + 2 * i);
    st_pack_nt(y + 2 * i, make_double2(0.0, 0.0));
    acc += nrm2_pack(v);
  }
  if (cg_owns_tail(nd)) {
    const double v = b[nd - 1];
    y[nd - 1] = 0.0;
    acc = fma(v, v, acc);
  }
  cg_put(acc, part_bb, red);
}

// beta1 = ||b|| from the partial sums of k_mr_init (every workgroup, one fixed order), v = b / beta1; workgroup 0 writes the record of
// iteration 0 into slot 0.  beta1 == 0: done, y = 0 stands; beta1 not finite: fail; v is left alone in both.
__global__ void __launch_bounds__(kBlock)
    k_mr_start(const double* __restrict__ b, double* __restrict__ v, int64_t nd, const double* __restrict__ part_bb, int nb,
               MrRecord* __restrict__ rec) {
  __shared__ double red[kBlock / 64];
  const double bb = cg_sum(part_bb, nb, red);
  const double beta1 = sqrt(bb);
  const bool fail = !cg_finite(bb), done = bb == 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    MrRecord R{};
    R.iteration = 0;
    R.done = done ? 1 : 0;
    R.fail = fail ? 1 : 0;
    R.beta1 = beta1;
    R.beta = 0.0;
    R.c = 1.0; R.s = 0.0;
    R.c_prev = 1.0; R.s_prev = 0.0;
    R.phibar = beta1;
    R.alpha = 0.0; R.gamma = 0.0;
    rec[0] = R;
  }
  if (fail || done) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 bv = ld_pack(b + 2 * i);
    st_pack(v + 2 * i, make_double2(bv.x / beta1, bv.y / beta1));   // (cacheable: the first product gathers exactly this vector)
  }
  if (cg_owns_tail(nd)) v[nd - 1] = b[nd - 1] / beta1;
}

// B: part_a[workgroup] = sum v q
__global__ void __launch_bounds__(kBlock)
    k_mr_alpha(const double* __restrict__ v, const double* __restrict__ q, int64_t nd, double* __restrict__ part_a,
               const MrRecord* __restrict__ rec, int k) {
  const MrRecord* in = rec + ((k - 1) & 1);
  if (in->done || in->fail) return;
  __shared__ double red[kBlock / 64];
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 vv = ld_pack(v + 2 * i), qv = ld_pack(q + 2 * i);
    acc = fma(vv.x, qv.x, fma(vv.y, qv.y, acc));
  }
  if (cg_owns_tail(nd)) acc = fma(v[nd - 1], q[nd - 1], acc);
  cg_put(acc, part_a, red);
}

// C: r = q - beta v_ - alpha v, in place over q;  part_r[workgroup] = sum r^2.  k == 1: beta is 0 and v_ is not read.  An alpha that is
// not finite goes into r and from there into beta': k_mr_step reports it.
__global__ void __launch_bounds__(kBlock)
    k_mr_resid(double* __restrict__ q, const double* __restrict__ vm, const double* __restrict__ v, int64_t nd,
               const double* __restrict__ part_a, double* __restrict__ part_r, int nb, const MrRecord* __restrict__ rec, int k) {
  const MrRecord* in = rec + ((k - 1) & 1);
  if (in->done || in->fail) return;
  __shared__ double red[kBlock / 64];
  const double alpha = cg_sum(part_a, nb, red);
  const double beta = in->beta;
  const bool first = k == 1;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 rv = ld_pack(q + 2 * i);
    const double2 vv = ld_pack(v + 2 * i);
    if (!first) {
      const double2 mv = ld_pack_nt(vm + 2 * i);   // (its last use as v_: k_mr_step writes v+ over it)
      rv.x = fma(-beta, mv.x, rv.x);
      rv.y = fma(-beta, mv.y, rv.y);
    }
    rv.x = fma(-alpha, vv.x, rv.x);
    rv.y = fma(-alpha, vv.y, rv.y);
    st_pack(q + 2 * i, rv);
    acc += nrm2_pack(rv);
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    double r = q[i];
    if (!first) r = fma(-beta, vm[i], r);
    r = fma(-alpha, v[i], r);
    q[i] = r;
    acc = fma(r, r, acc);
  }
  cg_put(acc, part_r, red);
}

// D: the step; w = (v - eps w__ - delta w_) / gamma, y += phi w; not done: w over w__, v+ = r / beta' over v_.  Every workgroup derives
// the step from the partial sums; workgroup 0 writes the record of iteration k into slot k & 1 (a finished or failed solve: the record
// it found, carried forward).  A failed step touches no vector.  wmm is read and written at the same index by the same thread; vm is
// written only (k_mr_resid was its last reader).
__global__ void __launch_bounds__(kBlock)
    k_mr_step(double* __restrict__ y, const double* __restrict__ v, double* __restrict__ vm, const double* __restrict__ r,
              double* __restrict__ wmm, const double* __restrict__ wm, int64_t nd, const double* __restrict__ part_a,
              const double* __restrict__ part_r, int nb, double tol, MrRecord* __restrict__ rec, int k) {
  const MrRecord* in = rec + ((k - 1) & 1);
  MrRecord* out = rec + (k & 1);
  const MrRecord was = *in;
  if (was.done || was.fail) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = was;
    return;
  }
  __shared__ double red[kBlock / 64];
  const double alpha = cg_sum(part_a, nb, red);
  const double rr = cg_sum(part_r, nb, red);
  const double beta_new = sqrt(rr);
  const MrStep s = mr_step(alpha, was.beta, beta_new, was.c, was.s, was.c_prev, was.s_prev, was.phibar, tol * was.beta1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    MrRecord R = was;
    R.iteration = k;
    R.done = s.done;
    R.fail = s.fail;
    R.alpha = alpha;
    R.gamma = s.gamma;
    if (!s.fail) {
      R.beta = beta_new;
      R.c_prev = was.c; R.s_prev = was.s;
      R.c = s.c; R.s = s.s;
      R.phibar = s.phibar;
    }
    *out = R;
  }
  if (s.fail) return;
  const double eps = s.eps, delta = s.delta, gamma = s.gamma, phi = s.phi;
  const bool use_wm = k >= 2, use_wmm = k >= 3;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 w = ld_pack(v + 2 * i);
    if (use_wmm) {
      const double2 t = ld_pack(wmm + 2 * i);
      w.x = fma(-eps, t.x, w.x);
      w.y = fma(-eps, t.y, w.y);
    }
    if (use_wm) {
      const double2 t = ld_pack(wm + 2 * i);
      w.x = fma(-delta, t.x, w.x);
      w.y = fma(-delta, t.y, w.y);
    }
    w.x = w.x / gamma;
    w.y = w.y / gamma;
    double2 yv = ld_pack(y + 2 * i);
    yv.x = fma(phi, w.x, yv.x);
    yv.y = fma(phi, w.y, yv.y);
    st_pack_nt(y + 2 * i, yv);
    if (!s.done) {
      const double2 rv = ld_pack_nt(r + 2 * i);   // (its last use: the next product overwrites it)
      st_pack(wmm + 2 * i, w);
      st_pack(vm + 2 * i, make_double2(rv.x / beta_new, rv.y / beta_new));   // (cacheable: the next product gathers exactly this vector)
    }
  }
  if (cg_owns_tail(nd)) {
    const int64_t i = nd - 1;
    double w = v[i];
    if (use_wmm) w = fma(-eps, wmm[i], w);
    if (use_wm) w = fma(-delta, wm[i], w);
    w = w / gamma;
    y[i] = fma(phi, w, y[i]);
    if (!s.done) {
      wmm[i] = w;
      vm[i] = r[i] / beta_new;
    }
  }
}

}  // namespace ksd

namespace {

struct MinresOp : ks_operator {
  ks_operator* A = nullptr;
  double theta = 0.0, tol = 0.0;
  int maxit = 0, check_every = kCgDefaultCheckEvery;
  void* vec[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // v (two roles), q, w (two roles)
  double* part = nullptr;                                         // [2][nb]: partial sums of v q and of r^2 (k_mr_init: of b^2)
  MrRecord* rec = nullptr;                                        // device, two slots
  MrRecord* rec_h = nullptr;                                      // pinned copy of both
  hipEvent_t ev = nullptr;
  int nb = 1;
  int64_t applications = 0, iterations = 0;
  int last_iterations = 0;
  double last_relres = 0.0, worst_relres = 0.0;
  ~MinresOp() override {
    for (void* p : vec) (void)hipFree(p);
    (void)hipFree(part); (void)hipFree(rec);
    (void)hipHostFree(rec_h);
    if (ev) (void)hipEventDestroy(ev);
  }
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "MINRES: the solve needs distinct x and y");
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "MINRES: a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    hipStream_t s = ctx->stream;
    const int64_t nd = n_local * (dtype == KS_F64 ? 1 : 2), ld = round_up(n_local, 64);
    const double B = 8.0 * (double)nd;
    double* vv[2] = {static_cast<double*>(vec[0]), static_cast<double*>(vec[1])};
    double* q = static_cast<double*>(vec[2]);
    double* ww[2] = {static_cast<double*>(vec[3]), static_cast<double*>(vec[4])};
    const double* xd = static_cast<const double*>(x);
    double* yd = static_cast<double*>(y);
    double *part_a = part, *part_r = part + nb;
    {
      ProfScope ps(ctx, KSP_SCALE, 4.0 * B);
      ksd::k_mr_init<<<nb, kBlock, 0, s>>>(xd, yd, nd, part_r);
      ksd::k_mr_start<<<nb, kBlock, 0, s>>>(xd, vv[0], nd, part_r, nb, rec);
      KS_HIP(hipGetLastError());
    }
    ++applications;
    const int every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
    int k = 0;
    MrRecord R{};
    for (;;) {
      const int upto = std::min(maxit, k + every);
      while (k < upto) {
        ++k;
        // roles of iteration k: v = vv[(k - 1) & 1], v_ (then v+) the other; w_ = ww[k & 1], w__ (then w) = ww[(k - 1) & 1]
        double *v = vv[(k - 1) & 1], *vm = vv[k & 1], *wm = ww[k & 1], *wmm = ww[(k - 1) & 1];
        A->in_scale = 1.0;
        if (theta == 0.0) A->apply(v, q, st);
        else A->apply_shifted(v, q, theta, 0.0, 1.0, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_mr_alpha<<<nb, kBlock, 0, s>>>(v, q, nd, part_a, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_AXPY, 4.0 * B);
          ksd::k_mr_resid<<<nb, kBlock, 0, s>>>(q, vm, v, nd, part_a, part_r, nb, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_FUSED, 8.0 * B);
          ksd::k_mr_step<<<nb, kBlock, 0, s>>>(yd, v, vm, q, wmm, wm, nd, part_a, part_r, nb, tol, rec, k);
        }
        KS_HIP(hipGetLastError());
      }
      KS_HIP(hipMemcpyAsync(rec_h, rec, 2 * sizeof(MrRecord), hipMemcpyDeviceToHost, s));
      KS_HIP(hipEventRecord(ev, s));
      KS_HIP(hipEventSynchronize(ev));
      R = rec_h[k & 1];
      if (R.done || R.fail || k >= maxit) break;
    }
    last_iterations = R.iteration;
    iterations += R.iteration;
    last_relres = R.beta1 > 0.0 ? std::fabs(R.phibar) / R.beta1 : 0.0;
    if (!(last_relres <= worst_relres)) worst_relres = last_relres;   // (a NaN sticks)
    auto sci = [](double v) { char buf[40]; std::snprintf(buf, sizeof buf, "%.6g", v); return std::string(buf); };
    if (R.fail) {
      if (R.iteration == 0) throw KsError{KS_ERR_OPERATOR, "ks_operator_minres: the right-hand side is not finite"};
      throw KsError{KS_ERR_OPERATOR, "ks_operator_minres: singular: gamma = " + sci(R.gamma) + " at iteration " + std::to_string(R.iteration) +
                                         " (the shift is an eigenvalue, or the operator returned values that are not finite)"};
    }
    if (!R.done)
      throw KsError{KS_ERR_OPERATOR, "ks_operator_minres: did not converge: relative residual " + sci(last_relres) + " after " + std::to_string(maxit) + " iterations"};
  }
};

inline ks_operator* make_minres(ks_ctx* ctx, ks_operator* A, double shift, double tol, int maxit, int check_every) {
  auto op = std::make_unique<MinresOp>();
  op->ctx = ctx;
  KS_REQUIRE(A->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_minres: the operator lives on another context");
  KS_REQUIRE(A->dtype == KS_F64 || A->dtype == KS_C64, KS_ERR_ARGUMENT, "ks_operator_minres: the operator is neither Float64 nor ComplexF64");
  KS_REQUIRE(A->async_capable, KS_ERR_ARGUMENT,
             "ks_operator_minres: the operator cannot be enqueued ahead (a host callback, a conjugate-gradient or MINRES solve, or a product or filter of one)");
  KS_REQUIRE(std::isfinite(tol) && tol > 0.0 && tol < 1.0, KS_ERR_ARGUMENT, "ks_operator_minres: tol = " + std::to_string(tol) + " (must lie in (0, 1))");
  KS_REQUIRE(maxit >= 1, KS_ERR_ARGUMENT, "ks_operator_minres: maxit = " + std::to_string(maxit) + " (must be at least 1)");
  KS_REQUIRE(check_every >= 0, KS_ERR_ARGUMENT, "ks_operator_minres: check_every = " + std::to_string(check_every) + " (must not be negative; 0: the library default)");
  KS_REQUIRE(std::isfinite(shift), KS_ERR_ARGUMENT, "ks_operator_minres: shift is not finite");
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
  for (int t = 0; t < 5; ++t) {
    KS_HIP(hipMalloc(&op->vec[t], bytes));
    KS_HIP(hipMemset(op->vec[t], 0, bytes));
  }
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->part), (size_t)2 * op->nb * sizeof(double)));
  KS_HIP(hipMemset(op->part, 0, (size_t)2 * op->nb * sizeof(double)));
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->rec), 2 * sizeof(MrRecord)));
  KS_HIP(hipMemset(op->rec, 0, 2 * sizeof(MrRecord)));
  KS_HIP(hipHostMalloc(reinterpret_cast<void**>(&op->rec_h), 2 * sizeof(MrRecord)));
  KS_HIP(hipEventCreateWithFlags(&op->ev, hipEventDisableTiming));
  return op.release();
}

}  // namespace
