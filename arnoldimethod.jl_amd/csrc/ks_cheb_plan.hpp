// CHEBYSHEV FILTER, the schedule: Clenshaw's recurrence for  y = sum_{k=0..m} gamma_k T_k(Ahat) x,  Ahat = (A - c) / e,  as m
// operator steps of the form  out = sigma (A in - c in) - w + gamma x0  (ks_operator::apply_clenshaw) and nothing else -- no
// scaling pass, no copy.  Host only, no HIP: exported as ks_host_chebyshev_plan (include/kschur.h) and held to literal tables and to
// exact rational arithmetic by tests/test_chebyshev_cpu.py.
//
// Clenshaw: b_{m+1} = b_{m+2} = 0,  b_k = gamma_k x + 2 Ahat b_{k+1} - b_{k+2}  (k = m ... 1),  y = gamma_0 x + Ahat b_1 - b_2.
// b_m = gamma_m x is never formed: its factor goes into the scale of the first step.  With h = fl(2 / e), h1 = fl(1 / e):
//
//   step            in        sigma               w         gamma                     out
//   m = 1 only      x0        fl(gamma_1 h1)      -         gamma_0                   y
//   1 (m >= 2)      x0        fl(gamma_m h)       -         gamma_{m-1}               b_{m-1}
//   2 (k = m - 2)   b_{m-1}   h (k = 0: h1)       -         fl(gamma_{m-2} - gamma_m) b_{m-2} (k = 0: y)
//   s >= 3 (k=m-s)  b_{k+1}   h (k = 0: h1)       b_{k+2}   gamma_k                   b_k (k = 0: y)
//
// theta = c in every step.  b_k lives in temporary (m - 1 - k) mod 3, so a step's output is never its input, its w or x0; a filter
// of degree m needs min(m - 1, 3) temporaries.  Slots: -1 = x0 as `in` / y as `out`, -2 = none, 0 ... 2 = temporaries.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ks_host_defs.hpp"

constexpr int kChebMaxDegree = 256;
constexpr int kChebSlotVec = -1;    // x0 (in) / y (out)
constexpr int kChebSlotNone = -2;

struct ChebStep {
  int32_t in, out, w;
  double sigma, gamma;
};

struct ChebPlan {
  std::vector<ChebStep> steps;   // `degree` of them
  int temporaries = 0;
};

inline ChebPlan chebyshev_plan(int degree, double center, double halfwidth, const double* coeffs) {
  const std::string who = "ks_host_chebyshev_plan";
  KS_REQUIRE(degree >= 1 && degree <= kChebMaxDegree, KS_ERR_ARGUMENT,
             who + ": degree = " + std::to_string(degree) + " (1 to " + std::to_string(kChebMaxDegree) + " are supported)");
  KS_REQUIRE(std::isfinite(halfwidth) && halfwidth > 0.0, KS_ERR_ARGUMENT, who + ": halfwidth = " + std::to_string(halfwidth) + " (must be positive and finite)");
  KS_REQUIRE(std::isfinite(center), KS_ERR_ARGUMENT, who + ": center is not finite");
  KS_REQUIRE(coeffs, KS_ERR_ARGUMENT, who + ": null coeffs");
  for (int k = 0; k <= degree; ++k)
    KS_REQUIRE(std::isfinite(coeffs[k]), KS_ERR_ARGUMENT, who + ": coefficient " + std::to_string(k) + " is not finite");
  const int m = degree;
  const double h = 2.0 / halfwidth, h1 = 1.0 / halfwidth;
  auto slot = [&](int k) { return k == 0 ? kChebSlotVec : (m - 1 - k) % 3; };   // where b_k (k = 0: y) is written
  ChebPlan P;
  P.temporaries = std::min(m - 1, 3);
  P.steps.reserve(m);
  if (m == 1) {
    P.steps.push_back({kChebSlotVec, kChebSlotVec, kChebSlotNone, coeffs[1] * h1, coeffs[0]});
    return P;
  }
  P.steps.push_back({kChebSlotVec, slot(m - 1), kChebSlotNone, coeffs[m] * h, coeffs[m - 1]});
  for (int k = m - 2; k >= 0; --k) {
    const bool second = k == m - 2;
    P.steps.push_back({slot(k + 1), slot(k), second ? kChebSlotNone : slot(k + 2), k == 0 ? h1 : h, second ? coeffs[k] - coeffs[m] : coeffs[k]});
  }
  return P;
}
