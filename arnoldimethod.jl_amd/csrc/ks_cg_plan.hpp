// CONJUGATE GRADIENTS, the scalar step: what one iteration of ks_operator_cg (ks_cg.hpp) decides from its three reductions, and the
// device record the kernels hand from launch to launch.  A host-and-device function in a host-only header (no HIP header: a plain
// host compiler builds it; under hipcc the same text is compiled for the device, so the kernels and the host model cannot drift
// apart).  Exported without a device as ks_host_cg_step (include/kschur.h) and held to hand-computed values by
// tests/test_cg_model_cpu.py.
//
//   rho      ||r||^2 before the step          (> 0 inside the iteration: rho0 == 0 and rho' == 0 both end it)
//   pq       Re p^H (A - theta) p             the curvature: positive and finite for a Hermitian positive definite operator
//   rho_new  ||r - alpha q||^2                what k_cg_resid measured with alpha = rho / pq
//   stop     tol^2 rho0
//
//   fail   pq is not finite, pq <= 0, alpha = rho / pq is not finite, or rho_new is not finite  ->  alpha = beta = 0, not done
//   alpha  rho / pq
//   done   rho_new <= stop                    (rho_new == 0 is done for every stop >= 0: no division by it or of it)
//   beta   rho_new / rho, 0 when done
//
// k_cg_resid needs alpha before rho_new exists: it calls the step with rho_new = 0, stop = 0 and reads alpha and fail only -- the
// tests of pq come first, so its `fail` is the part of the decision that does not depend on rho_new.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KS_CG_HD __host__ __device__
#else
#define KS_CG_HD
#endif

constexpr int kCgDefaultCheckEvery = 8;   // iterations enqueued between two reads of the record (ks_operator_cg: check_every = 0)

struct CgStep {
  double alpha, beta;
  int done, fail;
};

// (x - x is 0 for every finite x and NaN for inf and NaN: no <cmath> overload set to resolve on the device)
KS_CG_HD inline bool cg_finite(double x) { return x - x == 0.0; }

KS_CG_HD inline CgStep cg_step(double rho, double pq, double rho_new, double stop) {
  CgStep s{0.0, 0.0, 0, 0};
  if (!cg_finite(pq) || !(pq > 0.0)) { s.fail = 1; return s; }
  const double alpha = rho / pq;
  if (!cg_finite(alpha) || !cg_finite(rho_new)) { s.fail = 1; return s; }
  s.alpha = alpha;
  if (rho_new <= stop) { s.done = 1; return s; }
  s.beta = rho_new / rho;
  return s;
}

// What workgroup 0 of k_cg_dir leaves for the kernels of LATER launches and for the host.  Two of them, used in turn: iteration k
// reads slot (k - 1) & 1 and writes slot k & 1, so no workgroup ever reads a slot that a sibling of its own launch may be writing.
struct CgRecord {
  int32_t iteration;   // the iteration that wrote this state (0: the start); stays at the last one once done or fail is set
  int32_t done, fail, reserved;
  double rho;          // ||r||^2 now (after `iteration` iterations)
  double rho0;         // ||b||^2
  double pq;           // Re p^H (A - theta) p of that iteration
  double rho_prev;     // ||r||^2 before it
};
static_assert(sizeof(CgRecord) == 48, "CgRecord is copied to the host as plain bytes");
