// PRECONDITIONED CONJUGATE GRADIENTS, the scalar steps: what one iteration of ks_operator_pcg (ks_pcg.hpp) decides from its four
// reductions, and the device record the kernels hand from launch to launch.  Host-and-device functions in a host-only header, like
// ks_cg_plan.hpp (whose KS_CG_HD and cg_finite they use).  Exported without a device as ks_host_pcg_step (include/kschur.h) and held
// to hand-computed values by tests/test_pcg_model_cpu.py.
//
//   tau      Re r^H M r before the step        (> 0 for a Hermitian positive definite preconditioner M and r != 0)
//   pq       Re p^H (A - theta) p              the curvature: positive and finite for a Hermitian positive definite operator
//   rho_new  ||r - alpha q||^2                 what k_pcg_resid measured with alpha = tau / pq
//   stop     tol^2 rho0                        the stopping test of ks_operator_cg: the 2-norm of the recurrence's residual
//   tau_new  Re r^H M r after the step
//
// pcg_step (tau, pq, rho_new, stop):
//   fail   KS_PCG_FAIL_CURVATURE  pq is not finite, pq <= 0, or alpha = tau / pq is not finite
//          KS_PCG_FAIL_RESIDUAL   rho_new is not finite                                          ->  alpha = 0, not done
//   alpha  tau / pq
//   done   rho_new <= stop                     (rho_new == 0 is done for every stop >= 0: tau_new, then 0 too, is never looked at)
// pcg_beta (tau, tau_new), of a step that neither failed nor ended the solve:
//   fail   KS_PCG_FAIL_PRECONDITIONER  tau_new is not finite, tau_new <= 0, or beta = tau_new / tau is not finite  ->  beta = 0
//   beta   tau_new / tau
// pcg_start (rho0, tau0), iteration 0:  KS_PCG_FAIL_RHS when rho0 is not finite;  done when rho0 == 0 (y = 0 stands);  otherwise
//   KS_PCG_FAIL_PRECONDITIONER when tau0 is not finite or <= 0.
//
// k_pcg_resid needs alpha before rho_new exists: it calls pcg_step with rho_new = 0, stop = 0 and reads alpha and fail only -- the
// tests of pq come first, so that `fail` is the part of the decision that does not depend on rho_new.
#pragma once

#include "ks_cg_plan.hpp"

constexpr int KS_PCG_FAIL_RHS = 1;              // b is not finite
constexpr int KS_PCG_FAIL_CURVATURE = 2;        // p^H (A - theta) p is not positive and finite
constexpr int KS_PCG_FAIL_PRECONDITIONER = 3;   // r^H M r is not positive and finite
constexpr int KS_PCG_FAIL_RESIDUAL = 4;         // ||r||^2 is not finite

struct PcgStep {
  double alpha;
  int done, fail;
};

struct PcgBeta {
  double beta;
  int fail;
};

KS_CG_HD inline PcgStep pcg_step(double tau, double pq, double rho_new, double stop) {
  PcgStep s{0.0, 0, 0};
  if (!cg_finite(pq) || !(pq > 0.0)) { s.fail = KS_PCG_FAIL_CURVATURE; return s; }
  const double alpha = tau / pq;
  if (!cg_finite(alpha)) { s.fail = KS_PCG_FAIL_CURVATURE; return s; }
  if (!cg_finite(rho_new)) { s.fail = KS_PCG_FAIL_RESIDUAL; return s; }
  s.alpha = alpha;
  s.done = rho_new <= stop ? 1 : 0;
  return s;
}

KS_CG_HD inline PcgBeta pcg_beta(double tau, double tau_new) {
  PcgBeta b{0.0, 0};
  if (!cg_finite(tau_new) || !(tau_new > 0.0)) { b.fail = KS_PCG_FAIL_PRECONDITIONER; return b; }
  const double beta = tau_new / tau;
  if (!cg_finite(beta)) { b.fail = KS_PCG_FAIL_PRECONDITIONER; return b; }
  b.beta = beta;
  return b;
}

KS_CG_HD inline PcgStep pcg_start(double rho0, double tau0) {
  PcgStep s{0.0, 0, 0};
  if (!cg_finite(rho0)) { s.fail = KS_PCG_FAIL_RHS; return s; }
  if (rho0 == 0.0) { s.done = 1; return s; }
  if (!cg_finite(tau0) || !(tau0 > 0.0)) s.fail = KS_PCG_FAIL_PRECONDITIONER;
  return s;
}

// What workgroup 0 of k_pcg_dir (iteration 0: k_pcg_start) leaves for the kernels of LATER launches and for the host.  Two of them,
// used in turn like CgRecord: iteration k reads slot (k - 1) & 1 and writes slot k & 1.
struct PcgRecord {
  int32_t iteration;   // the iteration that wrote this state (0: the start); stays at the last one once done or fail is set
  int32_t done, fail, reserved;   // fail: 0, or the KS_PCG_FAIL_* reason
  double rho;          // ||r||^2 now (after `iteration` iterations)
  double rho0;         // ||b||^2
  double pq;           // Re p^H (A - theta) p of that iteration
  double rho_prev;     // ||r||^2 before it
  double tau;          // Re r^H M r now (a step that failed on it: the offending value)
  double tau_prev;     // ... before that iteration
};
static_assert(sizeof(PcgRecord) == 64, "PcgRecord is copied to the host as plain bytes");
