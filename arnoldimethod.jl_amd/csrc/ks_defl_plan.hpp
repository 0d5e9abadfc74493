// IN-CHAIN DEFLATION, the plan of a batch: which leading locked columns a Newton chain is projected against.  Host only, no HIP
// (tests/defl_plan_check.cpp builds this header with a plain host compiler under the sanitizers; tests/test_defl_plan_cpu.py holds it
// to tests/sstep_model.py: defl_plan case by case).  HipBackend::defl_plan (ks_backend.hpp) adds the switches and the workspace's
// guards and says why these columns are the ones that matter.
//
// The locked columns are the leading decoupled block of H: columns 0 .. nl-1, nl = the LAST zero sub-diagonal entry H(j, j-1) with
// 1 <= j <= j0 - 2.  A restart leaves that block QUASI-TRIANGULAR (1 x 1 and 2 x 2 diagonal blocks of the real Schur form), and its
// eigenvalues are read off those blocks.  A leading block with two consecutive non-zero sub-diagonal entries is a general Hessenberg
// matrix -- a caller's own H, or an accidental zero inside the active part -- whose diagonal blocks say nothing about its
// eigenvalues: no plan (0 columns) instead of numbers that would drive the Ritz classification, the shift exclusion and the growth
// test.
// Deflated: the LEADING locked columns whose eigenvalue exceeds `ratio` times the largest finite Ritz value outside the locked set
// (1e-6 relative match) and whose growth over the block, (|lambda| / rest)^max(1, steps - 1), exceeds 1e3; a 2 x 2 block is taken
// whole or not at all; at most nmax columns.  `ex` receives the eigenvalues of the deflated columns.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <vector>

// H: column-major, leading dimension ldh, at least j0 - 1 rows and columns valid.  T = double or std::complex<double>.
template <class T>
inline int defl_plan_columns(const T* H, int ldh, int j0, const std::complex<double>* ritz, int nritz, double ratio, int steps, int nmax,
                             std::vector<std::complex<double>>& ex, int* locked = nullptr, double* rest_out = nullptr) {
  using C = std::complex<double>;
  ex.clear();
  if (locked) *locked = 0;       // diagnostics (KS_DEFLATE_DEBUG): locked columns found, largest Ritz value outside them
  if (rest_out) *rest_out = 0.0;
  if (!H || ldh < 1 || !ritz || nritz <= 0) return 0;
  auto h = [&](int i, int j) -> const T& { return H[i + (size_t)j * ldh]; };
  int nl = 0;
  for (int j = 1; j <= j0 - 2; ++j)
    if (h(j, j - 1) == T(0)) nl = j;
  if (nl == 0) return 0;
  for (int j = 1; j + 1 < nl; ++j)
    if (h(j, j - 1) != T(0) && h(j + 1, j) != T(0)) return 0;   // not quasi-triangular: no eigenvalues to read off
  if (locked) *locked = nl;
  std::vector<C> lam(nl);
  std::vector<int> width(nl, 1);
  for (int j = 0; j < nl;) {
    if (j + 1 < nl && h(j + 1, j) != T(0)) {   // 2 x 2 block of the real Schur form
      const C a = C(h(j, j)), b = C(h(j, j + 1)), c = C(h(j + 1, j)), d = C(h(j + 1, j + 1));
      const C tr2 = 0.5 * (a + d), disc = std::sqrt(tr2 * tr2 - (a * d - b * c));
      lam[j] = tr2 + disc; lam[j + 1] = tr2 - disc;
      width[j] = 2; width[j + 1] = 0;
      j += 2;
    } else {
      lam[j] = C(h(j, j));
      ++j;
    }
  }
  double rest = 0.0;
  for (int q = 0; q < nritz; ++q) {
    const C z = ritz[q];
    if (!std::isfinite(std::abs(z))) continue;
    bool is_locked = false;
    for (int j = 0; j < nl; ++j) is_locked = is_locked || std::abs(z - lam[j]) <= 1e-6 * std::max(1.0, std::abs(lam[j]));
    if (!is_locked) rest = std::max(rest, std::abs(z));
  }
  if (rest_out) *rest_out = rest;
  if (!(rest > 0.0)) return 0;
  int nd = 0;
  for (int j = 0; j < nl;) {
    const int w = width[j] == 2 ? 2 : 1;
    const double mag = w == 2 ? std::max(std::abs(lam[j]), std::abs(lam[j + 1])) : std::abs(lam[j]);
    const double growth = std::pow(mag / rest, std::max(1, steps - 1));
    if (!(mag > ratio * rest) || !(growth > 1e3) || nd + w > nmax) break;
    for (int q = 0; q < w; ++q) ex.push_back(lam[j + q]);
    nd += w;
    j += w;
  }
  return nd;
}
