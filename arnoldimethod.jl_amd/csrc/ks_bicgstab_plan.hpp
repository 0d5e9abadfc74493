// BiCGStab(2), the scalar steps: what one iteration of ks_operator_bicgstab (ks_bicgstab.hpp) decides from its reductions -- the two
// BiCG coefficient steps, the Hermitian 2 x 2 minimal-residual solve, the three stopping tests -- and the device record the kernels
// hand from iteration to iteration.  Host-and-device functions in a host-only header like ks_cg_plan.hpp and ks_minres_plan.hpp (a
// plain host compiler builds it; under hipcc the same text is compiled for the device).  Exported without a device as
// ks_host_bicgstab_coef and ks_host_bicgstab_mr (include/kschur.h) and held to hand-computed values by
// tests/test_bicgstab_model_cpu.py.  Only + - * /, sqrt and explicit fma, for real scalars (double) and complex ones (BsZ): nothing a
// compiler may contract differently on the two sides.
//
//   bs_coef(rho0, rho1, alpha, gamma)       beta = alpha rho1 / rho0;  alpha' = rho1 / gamma
//       fail 1   rho0 zero or not finite, or beta not finite   ->  beta = alpha' = 0
//       fail 2   gamma zero or not finite, or alpha' not finite ->  alpha' = 0 (beta stands)
//     beta is needed one product before gamma exists: the kernels call it with gamma = 1 and read beta, then with rho0 = 1,
//     alpha = 0 and read alpha' -- each call's `fail` is the part of the decision that its real arguments make.
//   bs_mr(g11, g22, g12, h1, h2)            [g11 g12; conj(g12) g22] g = h by Cramer's rule;  det = fma(g11, g22, -|g12|^2)
//       fail     det zero or not finite, or a quotient not finite  ->  g = 0
//   bs_iter<S, LEVEL>(record, tol, sums)    the chain of one iteration up to LEVEL, from the record of the previous iteration and
//                                            the sums this one has produced so far (BsRows): which stage ended it, or which step broke
//
// Complex quotients a / b are formed as a conj(b) / |b|^2 with |b|^2 by fma; a |b|^2 that is zero or overflows counts as a divisor
// that is zero or not finite (|b| outside 1e-154 ... 1e154: far outside what an inner product of a converging solve takes).
#pragma once

#include <cmath>
#include <cstdint>

#include "ks_cg_plan.hpp"   // cg_finite, KS_CG_HD, kCgDefaultCheckEvery

struct BsZ {
  double re, im;
};

KS_CG_HD inline bool bs_finite(double x) { return cg_finite(x); }
KS_CG_HD inline bool bs_finite(BsZ x) { return cg_finite(x.re) && cg_finite(x.im); }
KS_CG_HD inline bool bs_zero(double x) { return x == 0.0; }
KS_CG_HD inline bool bs_zero(BsZ x) { return x.re == 0.0 && x.im == 0.0; }
KS_CG_HD inline double bs_neg(double x) { return -x; }
KS_CG_HD inline BsZ bs_neg(BsZ x) { return BsZ{-x.re, -x.im}; }
KS_CG_HD inline double bs_conj(double x) { return x; }
KS_CG_HD inline BsZ bs_conj(BsZ x) { return BsZ{x.re, -x.im}; }
// (the real product as an explicit fma: a plain a * b may be contracted into a neighbour -- cg_finite(x) is x - x == 0, and with
// x = -(omega rho0) a device compiler fuses that into fma(omega, rho0, -x), the rounding error of the product, which is not 0)
KS_CG_HD inline double bs_mul(double a, double b) { return std::fma(a, b, 0.0); }
KS_CG_HD inline BsZ bs_mul(BsZ a, BsZ b) { return BsZ{std::fma(a.re, b.re, -(a.im * b.im)), std::fma(a.re, b.im, a.im * b.re)}; }
KS_CG_HD inline double bs_abs2(double x) { return std::fma(x, x, 0.0); }
KS_CG_HD inline double bs_abs2(BsZ x) { return std::fma(x.re, x.re, x.im * x.im); }
// a / b; a divisor whose |b|^2 is zero or not finite gives NaN, which every caller tests for
KS_CG_HD inline double bs_div(double a, double b) { return a / b; }
KS_CG_HD inline BsZ bs_div(BsZ a, BsZ b) {
  const double d = bs_abs2(b);
  const BsZ n = bs_mul(a, bs_conj(b));
  if (d == 0.0 || !cg_finite(d)) return BsZ{(d - d) / (d - d), 0.0};   // (0 / 0: NaN)
  return BsZ{n.re / d, n.im / d};
}
// s x - t for a real s (a diagonal entry of G)
KS_CG_HD inline double bs_rsub(double s, double x, double t) { return std::fma(s, x, -t); }
KS_CG_HD inline BsZ bs_rsub(double s, BsZ x, BsZ t) { return BsZ{std::fma(s, x.re, -t.re), std::fma(s, x.im, -t.im)}; }
KS_CG_HD inline double bs_rdiv(double x, double d) { return x / d; }
KS_CG_HD inline BsZ bs_rdiv(BsZ x, double d) { return BsZ{x.re / d, x.im / d}; }
template <class S> KS_CG_HD inline S bs_real(double x);
template <> KS_CG_HD inline double bs_real<double>(double x) { return x; }
template <> KS_CG_HD inline BsZ bs_real<BsZ>(double x) { return BsZ{x, 0.0}; }
// a scalar in two doubles (the record, the exported functions, a row pair of partial sums): the second one is ignored for double
KS_CG_HD inline void bs_store(double* p, double x) { p[0] = x; p[1] = 0.0; }
KS_CG_HD inline void bs_store(double* p, BsZ x) { p[0] = x.re; p[1] = x.im; }
template <class S> KS_CG_HD inline S bs_load(const double* p);
template <> KS_CG_HD inline double bs_load<double>(const double* p) { return p[0]; }
template <> KS_CG_HD inline BsZ bs_load<BsZ>(const double* p) { return BsZ{p[0], p[1]}; }

template <class S>
struct BsCoef {
  S beta, alpha;
  int fail;
};

template <class S>
KS_CG_HD inline BsCoef<S> bs_coef(S rho0, S rho1, S alpha, S gamma) {
  BsCoef<S> c{bs_real<S>(0.0), bs_real<S>(0.0), 0};
  if (bs_zero(rho0) || !bs_finite(rho0)) { c.fail = 1; return c; }
  const S beta = bs_div(bs_mul(alpha, rho1), rho0);
  if (!bs_finite(beta)) { c.fail = 1; return c; }
  c.beta = beta;
  if (bs_zero(gamma) || !bs_finite(gamma)) { c.fail = 2; return c; }
  const S a = bs_div(rho1, gamma);
  if (!bs_finite(a)) { c.fail = 2; return c; }
  c.alpha = a;
  return c;
}

template <class S>
struct BsMr {
  S g1, g2;
  double det;
  int fail;
};

template <class S>
KS_CG_HD inline BsMr<S> bs_mr(double g11, double g22, S g12, S h1, S h2) {
  BsMr<S> m{bs_real<S>(0.0), bs_real<S>(0.0), 0.0, 0};
  m.det = std::fma(g11, g22, -bs_abs2(g12));
  if (m.det == 0.0 || !cg_finite(m.det)) { m.fail = 1; return m; }
  const S g1 = bs_rdiv(bs_rsub(g22, h1, bs_mul(g12, h2)), m.det);
  const S g2 = bs_rdiv(bs_rsub(g11, h2, bs_mul(bs_conj(g12), h1)), m.det);
  if (!bs_finite(g1) || !bs_finite(g2)) { m.fail = 1; return m; }
  m.g1 = g1;
  m.g2 = g2;
  return m;
}

// What the closing launch of iteration k leaves for the kernels of LATER iterations and for the host.  Two of them, used in turn as
// CgRecord's: iteration k reads slot (k - 1) & 1 and writes slot k & 1.  Scalars are pairs (re, im); im is 0 for Float64.
struct BsRecord {
  int32_t iteration;   // the iteration that wrote this state (0: the start); stays at the last one once done or fail is set
  int32_t done;
  int32_t fail;        // 0, or the step that broke: 1 rho (step 1), 2 gamma (step 1), 3 rho (step 2), 4 gamma (step 2), 5 det G, 6 b not finite
  int32_t stage;       // the stage (1, 2, 3) at which `iteration` ended: where the test passed, or 3 for an iteration run in full
  double beta1;        // ||b||
  double rr;           // ||r0||^2 of the recurrence after that stage
  double rho0[2], alpha[2], omega[2];   // the BiCG scalars after it
  double rho1[2];      // <rt, r0> after it: the next iteration's rho1
  double bad[2];       // what a breakdown reports: the rho0, gamma or det that was zero or not finite
};
static_assert(sizeof(BsRecord) == 112, "BsRecord is copied to the host as plain bytes");

// Rows of the partial-sum array part[row][workgroup], in the order the iteration produces them, so that what a kernel needs is a
// prefix.  A complex inner product takes two rows.
template <class S>
struct BsRows {
  static constexpr int W = (int)(sizeof(S) / sizeof(double));
  static constexpr int G1 = 0;            // <rt, u1>
  static constexpr int N1 = W;            // ||r0||^2 after step 1
  static constexpr int R2 = W + 1;        // <rt, r1>
  static constexpr int G2 = 2 * W + 1;    // <rt, u2>
  static constexpr int N2 = 3 * W + 1;    // ||r0||^2 after step 2
  static constexpr int M11 = 3 * W + 2;   // <r1, r1>
  static constexpr int M22 = 3 * W + 3;   // <r2, r2>
  static constexpr int M12 = 3 * W + 4;   // <r1, r2>
  static constexpr int H1 = 4 * W + 4;    // <r1, r0>
  static constexpr int H2 = 5 * W + 4;    // <r2, r0>
  static constexpr int RHO = 6 * W + 4;   // <rt, r0> after the MR step
  static constexpr int NN = 7 * W + 4;    // ||r0||^2 after the MR step
  static constexpr int COUNT = 7 * W + 5;
  // rows [0, upto(LEVEL)) are what bs_iter<S, LEVEL> reads
  static constexpr int upto(int level) {
    return level <= 0 ? 0 : level == 1 ? N1 : level == 2 ? R2 : level == 3 ? G2 : level == 4 ? N2 : level == 5 ? M11 : level == 6 ? RHO : COUNT;
  }
};
constexpr int kBsMaxRows = 19;

// One iteration's scalars as far as LEVEL:
//   0  beta of step 1                      (the record alone)
//   1  + alpha of step 1                   (G1)
//   2  + the stage 1 test                  (N1)
//   3  + beta of step 2                    (R2)
//   4  + alpha of step 2                   (G2)
//   5  + the stage 2 test                  (N2)
//   6  + g1, g2 of the MR step             (M11 ... H2)
//   7  + rho1 and the stage 3 test         (RHO, NN)
// `ended` != 0 or `fail` != 0: the chain stopped there and nothing behind it is set.  The tests come in the order of the recurrence,
// so a breakdown behind a passed test does not exist.
template <class S>
struct BsIter {
  S beta_1, alpha_1, beta_2, alpha_2, g1, g2;
  S rho0, alpha, omega, rho1;   // the BiCG scalars where the chain stopped
  S bad;
  double rr;
  int ended, fail;
};

template <class S, int LEVEL>
KS_CG_HD inline BsIter<S> bs_iter(const BsRecord& was, double tol, const double* sums) {
  using R = BsRows<S>;
  const S zero = bs_real<S>(0.0), one = bs_real<S>(1.0);
  BsIter<S> it{zero, zero, zero, zero, zero, zero, zero, zero, zero, zero, zero, 0.0, 0, 0};
  const double stop = tol * was.beta1;
  it.omega = bs_load<S>(was.omega);
  it.alpha = bs_load<S>(was.alpha);
  it.rho1 = bs_load<S>(was.rho1);
  it.rho0 = bs_neg(bs_mul(it.omega, bs_load<S>(was.rho0)));
  it.rr = was.rr;
  // BiCG step 1
  BsCoef<S> c = bs_coef(it.rho0, it.rho1, it.alpha, one);
  if (c.fail) { it.fail = 1; it.bad = it.rho0; return it; }
  it.beta_1 = c.beta;
  it.rho0 = it.rho1;
  if constexpr (LEVEL >= 1) {
    const S gamma = bs_load<S>(sums + R::G1);
    c = bs_coef(one, it.rho0, zero, gamma);
    if (c.fail) { it.fail = 2; it.bad = gamma; return it; }
    it.alpha_1 = it.alpha = c.alpha;
  }
  if constexpr (LEVEL >= 2) {
    it.rr = sums[R::N1];
    if (std::sqrt(it.rr) <= stop) { it.ended = 1; return it; }
  }
  // BiCG step 2
  if constexpr (LEVEL >= 3) {
    it.rho1 = bs_load<S>(sums + R::R2);
    c = bs_coef(it.rho0, it.rho1, it.alpha, one);
    if (c.fail) { it.fail = 3; it.bad = it.rho0; return it; }
    it.beta_2 = c.beta;
    it.rho0 = it.rho1;
  }
  if constexpr (LEVEL >= 4) {
    const S gamma = bs_load<S>(sums + R::G2);
    c = bs_coef(one, it.rho0, zero, gamma);
    if (c.fail) { it.fail = 4; it.bad = gamma; return it; }
    it.alpha_2 = it.alpha = c.alpha;
  }
  if constexpr (LEVEL >= 5) {
    it.rr = sums[R::N2];
    if (std::sqrt(it.rr) <= stop) { it.ended = 2; return it; }
  }
  // the minimal-residual step
  if constexpr (LEVEL >= 6) {
    const BsMr<S> m = bs_mr(sums[R::M11], sums[R::M22], bs_load<S>(sums + R::M12), bs_load<S>(sums + R::H1), bs_load<S>(sums + R::H2));
    if (m.fail) { it.fail = 5; it.bad = bs_real<S>(m.det); return it; }
    it.g1 = m.g1;
    it.g2 = it.omega = m.g2;
  }
  if constexpr (LEVEL >= 7) {
    it.rho1 = bs_load<S>(sums + R::RHO);
    it.rr = sums[R::NN];
    if (std::sqrt(it.rr) <= stop) it.ended = 3;
  }
  return it;
}
