// GEOMETRIC MULTIGRID V-CYCLE, the host plan: the chain of grids, the Chebyshev smoother's coefficients, the restriction scale and the
// reference transfers of ks_operator_multigrid (include/kschur.h (xix) holds the definition; ks_mg.hpp runs it on the device).  Host
// only, no HIP: exported as ks_host_multigrid_plan / _restrict / _prolong_add and held to closed forms, to a numpy loop written from
// the definition and to every refusal by tests/test_mg_model_cpu.py.
//
// LEVELS  l = 0 ... L, dims[l] = (nx, ny, nz), unused axes 1.  Per axis dims[l+1][a] is dims[l][a] (kept) or ceil(dims[l][a] / 2)
// (halved; an extent of 1 counts as kept), at least one axis halved per level.  Coarse cell I holds the fine cells 2 I and 2 I + 1
// along a halved axis, the last one of an odd extent a single cell.
//
// SMOOTHER of level l < L: k = degree steps of the Chebyshev iteration for B = D^-1 (A_l - theta) on [lambda / ratio, lambda]:
//     lo = fl(lambda / ratio);  thc = fl(fl(lambda + lo) / 2);  del = fl(fl(lambda - lo) / 2);  sig = fl(thc / del);  rho_0 = fl(1 / sig)
//     a_0 = 0,  b_0 = fl(1 / thc);     rho_j = fl(1 / fl(fl(2 sig) - rho_{j-1})),  a_j = fl(rho_j rho_{j-1}),  b_j = fl(fl(2 rho_j) / del)
// and step j is  d = a_j d + b_j dinv o (rhs - t),  x += d  with t = (A_l - theta) x  (j = 0 from x = 0: d = b_0 dinv o rhs, x = d).
// In exact arithmetic rho_j = T_j(sig) / T_{j+1}(sig).
//
// TRANSFERS: P copies the coarse value to its aggregate; R = s P^T with s = 2^-(halved axes) (exact), the terms of an aggregate added
// to +0.0 in ascending fine row order (x fastest, then y, then z).  ComplexF64 runs both on the real view, part by part (`ncomp` 2).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ks_host_defs.hpp"

constexpr int kMgMaxLevels = 16;

struct MgLevel {
  int64_t dims[3] = {1, 1, 1};
  int64_t rows = 1;
  int halved[3] = {0, 0, 0};   // towards the next level (all 0 on the coarsest)
  double scale = 1.0;          // s of the restriction towards the next level
  std::vector<double> a, b;    // `degree` smoother coefficients each (empty on the coarsest level)
};

struct MgPlan {
  std::vector<MgLevel> levels;   // nsmooth + 1
  int degree = 0;
  double ratio = 0.0;
};

inline std::string mg_dims_text(const int64_t* d) {
  return std::to_string(d[0]) + " x " + std::to_string(d[1]) + " x " + std::to_string(d[2]);
}

// `inv_diag`: null, or nsmooth pointers (a null one is not looked at) to rows(l) entries each
inline MgPlan mg_plan(int nsmooth, const int64_t* dims, const double* lambda_max, int degree, double ratio, const double* const* inv_diag,
                      const std::string& who) {
  KS_REQUIRE(nsmooth >= 0, KS_ERR_ARGUMENT, who + ": nsmooth = " + std::to_string(nsmooth) + " (must not be negative)");
  KS_REQUIRE(nsmooth + 1 <= kMgMaxLevels, KS_ERR_ARGUMENT,
             who + ": " + std::to_string(nsmooth + 1) + " levels (at most " + std::to_string(kMgMaxLevels) + " are supported)");
  KS_REQUIRE(dims, KS_ERR_ARGUMENT, who + ": null dims");
  KS_REQUIRE(nsmooth == 0 || lambda_max, KS_ERR_ARGUMENT, who + ": null lambda_max");
  KS_REQUIRE(degree >= 1, KS_ERR_ARGUMENT, who + ": degree = " + std::to_string(degree) + " (must be at least 1)");
  KS_REQUIRE(std::isfinite(ratio) && ratio > 1.0, KS_ERR_ARGUMENT, who + ": ratio = " + std::to_string(ratio) + " (must be finite and above 1)");
  MgPlan P;
  P.degree = degree;
  P.ratio = ratio;
  P.levels.resize((size_t)nsmooth + 1);
  for (int l = 0; l <= nsmooth; ++l) {
    MgLevel& L = P.levels[l];
    const std::string lv = who + ": level " + std::to_string(l);
    L.rows = 1;
    for (int a = 0; a < 3; ++a) {
      L.dims[a] = dims[3 * l + a];
      KS_REQUIRE(L.dims[a] >= 1, KS_ERR_ARGUMENT, lv + " has the extents " + mg_dims_text(dims + 3 * l) + " (every extent must be at least 1)");
      KS_REQUIRE(L.dims[a] < (int64_t)2147483647 && L.rows * L.dims[a] < (int64_t)2147483647, KS_ERR_ARGUMENT,
                 lv + " has the extents " + mg_dims_text(dims + 3 * l) + " (a level must have fewer than 2^31 rows)");
      L.rows *= L.dims[a];
    }
  }
  for (int l = 0; l < nsmooth; ++l) {
    MgLevel& L = P.levels[l];
    const MgLevel& N = P.levels[l + 1];
    const std::string lv = who + ": level " + std::to_string(l);
    int nh = 0;
    for (int a = 0; a < 3; ++a) {
      const int64_t half = (L.dims[a] + 1) / 2;
      KS_REQUIRE(N.dims[a] == L.dims[a] || N.dims[a] == half, KS_ERR_ARGUMENT,
                 lv + " has the extents " + mg_dims_text(L.dims) + ", level " + std::to_string(l + 1) + " the extents " + mg_dims_text(N.dims) +
                     ": axis " + std::to_string(a) + " must keep its extent " + std::to_string(L.dims[a]) + " or halve it to " + std::to_string(half));
      L.halved[a] = N.dims[a] != L.dims[a] ? 1 : 0;
      nh += L.halved[a];
    }
    KS_REQUIRE(nh >= 1, KS_ERR_ARGUMENT,
               lv + " and level " + std::to_string(l + 1) + " have the same extents " + mg_dims_text(L.dims) + " (at least one axis must be halved per level)");
    L.scale = std::ldexp(1.0, -nh);
    const double lam = lambda_max[l];
    KS_REQUIRE(std::isfinite(lam) && lam > 0.0, KS_ERR_ARGUMENT, lv + ": lambda_max = " + std::to_string(lam) + " (must be positive and finite)");
    const double lo = lam / ratio, thc = (lam + lo) / 2.0, del = (lam - lo) / 2.0;
    KS_REQUIRE(std::isfinite(thc) && del > 0.0 && std::isfinite(1.0 / thc) && std::isfinite(1.0 / del), KS_ERR_ARGUMENT,
               lv + ": lambda_max = " + std::to_string(lam) + " and ratio = " + std::to_string(ratio) + " leave no interval to smooth on");
    const double sig = thc / del;
    double rho = 1.0 / sig;
    L.a.assign((size_t)degree, 0.0);
    L.b.assign((size_t)degree, 0.0);
    L.b[0] = 1.0 / thc;
    for (int j = 1; j < degree; ++j) {
      const double rho_new = 1.0 / (2.0 * sig - rho);
      L.a[j] = rho_new * rho;
      L.b[j] = (2.0 * rho_new) / del;
      rho = rho_new;
    }
    if (inv_diag && inv_diag[l]) {
      const double* d = inv_diag[l];
      for (int64_t i = 0; i < L.rows; ++i)
        KS_REQUIRE(std::isfinite(d[i]) && d[i] > 0.0, KS_ERR_ARGUMENT,
                   lv + ": inv_diag entry " + std::to_string(i) + " = " + std::to_string(d[i]) + " (must be positive and finite)");
    }
  }
  return P;
}

// the pair of levels of one transfer, checked like a link of the chain: halved[] and s
struct MgPair {
  int64_t f[3], c[3];
  int h[3];
  double scale;
};

inline MgPair mg_pair(const int64_t* fine, const int64_t* coarse, const std::string& who) {
  KS_REQUIRE(fine && coarse, KS_ERR_ARGUMENT, who + ": null dims");
  int64_t both[6] = {fine[0], fine[1], fine[2], coarse[0], coarse[1], coarse[2]};
  const double lam = 1.0;
  const MgPlan P = mg_plan(1, both, &lam, 1, 2.0, nullptr, who);
  MgPair g;
  for (int a = 0; a < 3; ++a) {
    g.f[a] = fine[a];
    g.c[a] = coarse[a];
    g.h[a] = P.levels[0].halved[a];
  }
  g.scale = P.levels[0].scale;
  return g;
}

// rc[I] = s * sum over the aggregate of fl(b[i] - t[i]), the terms added to +0.0 in ascending fine row order
inline void mg_restrict_host(const MgPair& g, int ncomp, const double* b, const double* t, double* rc) {
  for (int64_t K = 0; K < g.c[2]; ++K)
    for (int64_t J = 0; J < g.c[1]; ++J)
      for (int64_t I = 0; I < g.c[0]; ++I)
        for (int c = 0; c < ncomp; ++c) {
          volatile double acc = 0.0;   // (volatile: every partial sum is rounded to a double in this order)
          for (int64_t k = K << g.h[2]; k < g.f[2] && k <= (K << g.h[2]) + g.h[2]; ++k)
            for (int64_t j = J << g.h[1]; j < g.f[1] && j <= (J << g.h[1]) + g.h[1]; ++j)
              for (int64_t i = I << g.h[0]; i < g.f[0] && i <= (I << g.h[0]) + g.h[0]; ++i) {
                const int64_t r = (i + g.f[0] * (j + g.f[1] * k)) * ncomp + c;
                const double term = b[r] - t[r];
                acc = acc + term;
              }
          rc[(I + g.c[0] * (J + g.c[1] * K)) * ncomp + c] = g.scale * acc;
        }
}

// x[i] += ec[aggregate of i]
inline void mg_prolong_add_host(const MgPair& g, int ncomp, const double* ec, double* x) {
  for (int64_t k = 0; k < g.f[2]; ++k)
    for (int64_t j = 0; j < g.f[1]; ++j)
      for (int64_t i = 0; i < g.f[0]; ++i) {
        const int64_t r = i + g.f[0] * (j + g.f[1] * k);
        const int64_t R = (i >> g.h[0]) + g.c[0] * ((j >> g.h[1]) + g.c[1] * (k >> g.h[2]));
        for (int c = 0; c < ncomp; ++c) x[r * ncomp + c] = x[r * ncomp + c] + ec[R * ncomp + c];
      }
}
