// Chebyshev polynomial filter  y = p(A) x,  p(A) = sum_{k=0..m} gamma_k T_k((A - c) / e)  (ks_operator_chebyshev, include/kschur.h):
// the spectral transformation for operators that cannot be factored -- the eigensolver runs on p(A), whose largest eigenvalues are
// the ones the coefficients select (an interior window, a clustered low end; extras.chebyshev_window / chebyshev_damping).
// Part of the ONE translation unit of libkschur_hip.so: included by ks_hip.hip after ks_product.hpp.
//
// apply() runs the host plan (ks_cheb_plan.hpp): m Clenshaw steps through A->apply_clenshaw, m products and no other pass over the
// vectors where A fuses the step into its product (the grid operators), m products and m streaming passes elsewhere.  A is
// BORROWED like a product's factors.  The b's rotate through at most three temporaries the filter owns, allocated like ProductOp's
// (a multiple of 64 elements, zero-filled once: stored-matrix kernels may read pad rows of their input; every step writes rows
// < n_local only).  Every intermediate step stores cacheably -- the next step's product gathers exactly that vector -- and the
// last one streams (KS_CHEB_PLAIN=0: every step streams; read per product).
#pragma once

namespace {

struct ChebOp : ks_operator {
  ks_operator* A = nullptr;
  ChebPlan plan;
  double center = 0.0;
  void* tmp[3] = {nullptr, nullptr, nullptr};
  ~ChebOp() override { (void)hipFree(tmp[0]); (void)hipFree(tmp[1]); (void)hipFree(tmp[2]); }
  // (no ProfScope: A books its own time and bytes)
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "Chebyshev filter: the product needs distinct x and y");
    const bool saved = A->shift_store_cacheable;
    const int64_t f0 = A->clenshaw_fused, g0 = A->clenshaw_generic;
    auto count = [&] {
      clenshaw_fused += A->clenshaw_fused - f0;
      clenshaw_generic += A->clenshaw_generic - g0;
      A->shift_store_cacheable = saved;
    };
    A->in_scale = in_scale;  // (as in ProductOp: a host-callback A scales its input and unscales its result, the product does not depend on it)
    try {
      const size_t ns = plan.steps.size();
      for (size_t i = 0; i < ns; ++i) {
        const ChebStep& s = plan.steps[i];
        const void* in = s.in == kChebSlotVec ? x : tmp[s.in];
        void* out = s.out == kChebSlotVec ? y : tmp[s.out];
        const void* w = s.w == kChebSlotNone ? nullptr : tmp[s.w];
        A->shift_store_cacheable = i + 1 < ns && env_int("KS_CHEB_PLAIN", 1) != 0;
        A->apply_clenshaw(in, out, center, 0.0, s.sigma, w, s.gamma, x, round_up(n_local, 64), st);
      }
    } catch (...) {
      count();
      throw;
    }
    count();
  }
};

inline ks_operator* make_chebyshev(ks_ctx* ctx, ks_operator* A, int degree, double center, double halfwidth, const double* coeffs) {
  auto op = std::make_unique<ChebOp>();
  op->ctx = ctx;
  KS_REQUIRE(A->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_chebyshev: the operator lives on another context");
  KS_REQUIRE(A->dtype == KS_F64 || A->dtype == KS_C64, KS_ERR_ARGUMENT, "ks_operator_chebyshev: the operator is neither Float64 nor ComplexF64");
  op->plan = chebyshev_plan(degree, center, halfwidth, coeffs);
  op->A = A;
  op->center = center;
  op->n_local = A->n_local;
  op->dtype = A->dtype;
  op->async_capable = A->async_capable;
  op->nnz = A->nnz * degree;
  const size_t bytes = (size_t)std::max<int64_t>(round_up(op->n_local, 64), 64) * (op->dtype == KS_F64 ? 8 : 16);
  for (int t = 0; t < op->plan.temporaries; ++t) {
    KS_HIP(hipMalloc(&op->tmp[t], bytes));
    KS_HIP(hipMemset(op->tmp[t], 0, bytes));
  }
  return op.release();
}

}  // namespace
