// MINRES, the scalar step: what one iteration of ks_operator_minres (ks_minres.hpp) decides from its two reductions -- the new
// column of the Lanczos tridiagonal matrix pushed through the two previous plane rotations, the rotation that annihilates its
// subdiagonal entry, and the stopping test -- and the device record the kernels hand from launch to launch.  A host-and-device
// function in a host-only header like ks_cg_plan.hpp (a plain host compiler builds it; under hipcc the same text is compiled for
// the device).  Exported without a device as ks_host_minres_step (include/kschur.h) and held to hand-computed values by
// tests/test_minres_model_cpu.py.  Only + - * /, sqrt and explicit fma: nothing a compiler may contract differently on the two sides.
//
//   alpha     Re v^H (A - theta) v            the diagonal entry of the Lanczos matrix
//   beta      ||r|| of the previous iteration  its entry above the diagonal (0 in the first iteration)
//   beta_new  ||r|| of this iteration          the entry below the diagonal
//   c, s      the previous rotation, c_prev, s_prev the one before it  ((1, 0) before there is one)
//   phibar    the residual norm of the recurrence before the step (signed), stop = tol ||b||
//
//   eps    = s_prev beta                             the entry two above the diagonal of R
//   dbar   = c_prev beta
//   delta  = c dbar + s alpha                        the entry one above
//   gbar   = -s dbar + c alpha
//   gamma  = hypot(gbar, beta_new)                   the diagonal entry; formed as m sqrt((gbar/m)^2 + (beta_new/m)^2) with
//                                                    m = max(|gbar|, beta_new): no overflow where gamma itself is representable
//   fail   alpha, beta_new or gamma not finite, or gamma == 0 ("singular")  ->  every other output 0 except gamma
//   c_new  = gbar / gamma;  s_new = beta_new / gamma
//   phi    = c_new phibar;  phibar_new = -s_new phibar
//   done   |phibar_new| <= stop                      (beta_new == 0 gives s_new = 0 and phibar_new = 0: done for every stop >= 0)
#pragma once

#include <cmath>
#include <cstdint>

#include "ks_cg_plan.hpp"   // cg_finite, KS_CG_HD, kCgDefaultCheckEvery

struct MrStep {
  double eps, delta, gamma, c, s, phi, phibar;
  int done, fail;
};

KS_CG_HD inline double mr_abs(double x) { return x < 0.0 ? -x : x; }

KS_CG_HD inline MrStep mr_step(double alpha, double beta, double beta_new, double c, double s, double c_prev, double s_prev, double phibar,
                               double stop) {
  MrStep r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
  const double eps = s_prev * beta;
  const double dbar = c_prev * beta;
  const double delta = std::fma(c, dbar, s * alpha);
  const double gbar = std::fma(c, alpha, -(s * dbar));
  if (!cg_finite(alpha) || !cg_finite(beta_new) || !cg_finite(gbar)) {
    r.gamma = (alpha - alpha) + (beta_new - beta_new) + (gbar - gbar);   // NaN: what the failure reports
    r.fail = 1;
    return r;
  }
  const double ag = mr_abs(gbar);
  const double m = ag > beta_new ? ag : beta_new;
  double gamma = 0.0;
  if (m > 0.0) {
    const double a = gbar / m, b = beta_new / m;
    gamma = m * std::sqrt(std::fma(a, a, b * b));
  }
  if (!cg_finite(gamma) || gamma == 0.0) {
    r.gamma = gamma;
    r.fail = 1;
    return r;
  }
  r.eps = eps;
  r.delta = delta;
  r.gamma = gamma;
  r.c = gbar / gamma;
  r.s = beta_new / gamma;
  r.phi = r.c * phibar;
  r.phibar = -(r.s * phibar);
  r.done = mr_abs(r.phibar) <= stop ? 1 : 0;
  return r;
}

// What workgroup 0 of k_mr_step leaves for the kernels of LATER launches and for the host.  Two of them, used in turn as CgRecord's:
// iteration k reads slot (k - 1) & 1 and writes slot k & 1.
struct MrRecord {
  int32_t iteration;   // the iteration that wrote this state (0: the start); stays at the last one once done or fail is set
  int32_t done, fail, reserved;
  double beta1;        // ||b||
  double beta;         // ||r|| of that iteration: the next one's beta
  double c, s;         // its rotation
  double c_prev, s_prev;   // the rotation before it
  double phibar;       // the recurrence's residual norm after it (signed)
  double alpha, gamma; // of that iteration (what a failure reports)
};
static_assert(sizeof(MrRecord) == 88, "MrRecord is copied to the host as plain bytes");
