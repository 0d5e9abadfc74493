// Tridiagonal shift-invert  y = (T - sigma I)^-1 x, factored ONCE: partition, factors and the host apply.  Pure host arithmetic,
// no HIP header and no hip* call -- TridiagSolveOp (ks_tridiag.hpp) uploads the plan made here and walks the same arrays in the
// same order on the device; ks_host_tridiag_solve / ks_host_tridiag_info (include/kschur.h) run it without a device.
//
// Recursive separator elimination.  Level 0 is M = T - sigma I.  The rows of a level are split into blocks of at most m rows with
// ONE separator row after each block (block, separator, block, ...; the last row is a separator or the end of a tail block).
// Per block p (tridiagonal sub-matrix M_p) the plan holds a partially pivoted LU (multiplier, pivot flag, reciprocal of the U
// diagonal and the two upper bands of U per row) and the two spikes  w_p = M_p^-1 e_first dl[first],  v_p = M_p^-1 e_last du[last].
// With g_p = M_p^-1 f_p the separators satisfy a tridiagonal Schur system (one row per separator), which is fixed as well and
// becomes the next level.  A level of at most 2 m rows is the DIRECT level: one block, no separator, the same pivoted LU walked
// by one lane.  Then  x_p = g_p - w_p z_left - v_p z_right  on the way back, separators copy z.
//
// Partition rule.  A block is accepted when  growth = max|M_p^-1 [e_first e_last]| * ||M_p||_inf  <= kGrowthLimit (1e6; a
// singular block has infinite growth).  The planner takes the longest admissible block at every position, longest first, and
// backtracks when a choice leaves no admissible continuation; positions proven hopeless are remembered, so every (position,
// length) pair is factored at most once: at most n m block factorisations per level, whatever the matrix.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <type_traits>
#include <vector>

#include "ks_host_defs.hpp"

namespace {
namespace td {

constexpr int kMaxLevels = 8;            // ks_operator_tridiag_info reports at most this many level sizes
constexpr int kDefaultBlockRows = 64;    // block_rows = 0
constexpr int kMinBlockRows = 2, kMaxBlockRows = 64;
constexpr double kGrowthLimit = 1e6;     // admissible block: max|M_p^-1 [e_first e_last]| ||M_p|| at most this
constexpr double kResidualLimit = 1e-10; // normwise backward error of the check solve at upload (extras.sparse_shift_invert's residual_limit)

using cplx = std::complex<double>;

// ---- element arithmetic, spelled out so that host and device perform the same operations in the same order -------------------
inline double abs1(double a) { return std::fabs(a); }
inline double abs1(const cplx& a) { return std::fabs(a.real()) + std::fabs(a.imag()); }
inline bool is_finite(double a) { return std::isfinite(a); }
inline bool is_finite(const cplx& a) { return std::isfinite(a.real()) && std::isfinite(a.imag()); }
inline bool is_zero(double a) { return a == 0.0; }
inline bool is_zero(const cplx& a) { return a.real() == 0.0 && a.imag() == 0.0; }
inline double mul(double a, double b) { return a * b; }
inline cplx mul(const cplx& a, const cplx& b) { return cplx(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
// c - a b
inline double nmsub(double a, double b, double c) { return c - a * b; }
inline cplx nmsub(const cplx& a, const cplx& b, const cplx& c) {
  return cplx((c.real() + a.imag() * b.imag()) - a.real() * b.real(), (c.imag() - a.imag() * b.real()) - a.real() * b.imag());
}
inline double neg(double a) { return -a; }
inline cplx neg(const cplx& a) { return cplx(-a.real(), -a.imag()); }

// One level.  Factor arrays are BLOCK-INTERLEAVED: entry i of block p lives at [i * nblocks + p], so the lanes of a wavefront (one
// block each) read neighbouring addresses at every step of the walk.  Spikes are in SLOT order [p * (cap + 1) + i] (slot len[p] of
// a block is its separator), the order in which the streaming pass back visits the rows.
template <class T> struct Level {
  int64_t n = 0;        // rows of this level's system
  int cap = 0;          // longest block of the level: block_rows, or n at the direct level
  bool direct = false;  // one block, no separator: solved outright
  int64_t nblocks = 0, nsep = 0;
  std::vector<int32_t> start, len;   // rows [start[p], start[p] + len[p]) of block p
  std::vector<T> mult, inv, u1, u2;  // per row of a block: multiplier, 1 / U diagonal, first and second upper band of U
  std::vector<uint8_t> flag;         // 1: rows i and i + 1 were interchanged at step i
  std::vector<T> w, v;               // spikes (not at the direct level)
  // right-hand side of the NEXT level, formed from this level's g:  f'[j] = g[sep[j]] - sdl[j] g[sep[j] - 1] - sdu[j] g[sep[j] + 1]
  std::vector<int32_t> sep;
  std::vector<T> sdl, sdu;
  int pitch() const { return (cap + 1) | 1; }  // LDS row pitch of the device walk in elements: odd, so lanes striding by it hit distinct banks
};

template <class T> struct Plan {
  int64_t n = 0;
  int block_rows = 0;
  std::vector<Level<T>> levels;
  int64_t shortened = 0;   // blocks (all levels) shorter than the default split would have made them
  double max_growth = 0.0; // largest growth among the accepted blocks
  double residual = 0.0;   // backward error of the check solve
  double norm1 = 0.0;      // ||M||_1
};

// ---- one block: pivoted LU (LAPACK's gttrf recurrence), spikes, growth ----------------------------------------------------------
template <class T> struct BlockWork {
  std::vector<T> mult, dd, u1, u2, inv, w, v;
  std::vector<uint8_t> flag;
  double growth = 0.0;
  explicit BlockWork(int cap) : mult(cap), dd(cap), u1(cap), u2(cap), inv(cap), w(cap), v(cap), flag(cap) {}
};

// forward and back substitution of one block on f[0..L): THE walk -- the device runs exactly these steps per lane
template <class T>
inline void walk_block(int L, const T* mult, const uint8_t* flag, const T* inv, const T* u1, const T* u2, int64_t stride, T* f) {
  T cur = f[0];
  for (int i = 0; i + 1 < L; ++i) {
    const T nxt = f[i + 1];
    const bool sw = flag[i * stride] != 0;
    const T t = sw ? nxt : cur, o = sw ? cur : nxt;
    f[i] = t;
    cur = nmsub(mult[i * stride], t, o);
  }
  f[L - 1] = cur;
  T xp1 = T(0), xp2 = T(0);
  for (int i = L - 1; i >= 0; --i) {
    const T xi = mul(nmsub(u2[i * stride], xp2, nmsub(u1[i * stride], xp1, f[i])), inv[i * stride]);
    f[i] = xi;
    xp2 = xp1;
    xp1 = xi;
  }
}

// Factor rows [r0, r0 + L) of the level (a: sub-, b: main, c: super-diagonal, all of length n with a[0] = c[n-1] = 0).
// false: an exactly zero pivot.  `spikes`: also the two spikes and the growth.
template <class T> bool factor_block(const T* a, const T* b, const T* c, int64_t r0, int L, bool spikes, BlockWork<T>& W) {
  double norm = 0.0;
  for (int i = 0; i < L; ++i) {
    W.dd[i] = b[r0 + i];
    W.u1[i] = i + 1 < L ? c[r0 + i] : T(0);
    W.u2[i] = T(0);
    W.mult[i] = T(0);
    W.flag[i] = 0;
    norm = std::max(norm, (i > 0 ? abs1(a[r0 + i]) : 0.0) + abs1(b[r0 + i]) + (i + 1 < L ? abs1(c[r0 + i]) : 0.0));
  }
  for (int i = 0; i + 1 < L; ++i) {
    const T sub = a[r0 + i + 1];
    if (abs1(W.dd[i]) >= abs1(sub)) {
      if (is_zero(W.dd[i])) return false;  // (the sub-diagonal entry is zero as well)
      const T fact = sub / W.dd[i];
      W.mult[i] = fact;
      W.dd[i + 1] = nmsub(fact, W.u1[i], W.dd[i + 1]);
    } else {
      const T fact = W.dd[i] / sub;
      W.dd[i] = sub;
      W.mult[i] = fact;
      const T temp = W.u1[i];
      W.u1[i] = W.dd[i + 1];
      W.dd[i + 1] = nmsub(fact, W.dd[i + 1], temp);
      if (i + 2 < L) {
        W.u2[i] = W.u1[i + 1];
        W.u1[i + 1] = neg(mul(fact, W.u1[i + 1]));
      }
      W.flag[i] = 1;
    }
  }
  for (int i = 0; i < L; ++i) {
    if (is_zero(W.dd[i]) || !is_finite(W.dd[i])) return false;
    W.inv[i] = T(1) / W.dd[i];
    if (!is_finite(W.inv[i])) return false;
  }
  if (!spikes) return true;
  for (int i = 0; i < L; ++i) W.w[i] = W.v[i] = T(0);
  W.w[0] = T(1);
  W.v[L - 1] = T(1);
  walk_block<T>(L, W.mult.data(), W.flag.data(), W.inv.data(), W.u1.data(), W.u2.data(), 1, W.w.data());
  if (L > 1) walk_block<T>(L, W.mult.data(), W.flag.data(), W.inv.data(), W.u1.data(), W.u2.data(), 1, W.v.data());
  else W.v[0] = W.w[0];
  double big = 0.0;
  for (int i = 0; i < L; ++i) big = std::max(big, std::max(abs1(W.w[i]), abs1(W.v[i])));
  W.growth = big * norm;
  if (!(W.growth <= std::numeric_limits<double>::max())) return false;  // (NaN or infinite)
  const T cl = a[r0], cr = c[r0 + L - 1];  // couplings to the separators on the left and on the right (zero at the ends)
  for (int i = 0; i < L; ++i) {
    W.w[i] = mul(W.w[i], cl);
    W.v[i] = mul(W.v[i], cr);
  }
  return true;
}

// ---- one level: partition, then factors ------------------------------------------------------------------------------------------
template <class T>
void plan_level(int level, const std::vector<T>& a, const std::vector<T>& b, const std::vector<T>& c, int m, Plan<T>& P, Level<T>& V) {
  const int64_t n = (int64_t)b.size();
  V.n = n;
  if (n <= 2 * (int64_t)m) {  // the direct level
    V.direct = true;
    V.cap = (int)n;
    V.nblocks = 1;
    V.start = {0};
    V.len = {(int32_t)n};
    BlockWork<T> W((int)n);
    KS_REQUIRE(factor_block<T>(a.data(), b.data(), c.data(), 0, (int)n, false, W), KS_ERR_ARGUMENT,
               "tridiagonal solve: exactly zero pivot in the direct solve of level " + std::to_string(level) + " (" + std::to_string(n) +
                   " rows): T - sigma I is singular to working precision");
    V.mult = W.mult; V.inv = W.inv; V.u1 = W.u1; V.u2 = W.u2; V.flag = W.flag;
    return;
  }
  V.cap = m;
  BlockWork<T> W(m);
  // depth-first, longest block first; dead[r]: no admissible partition of rows [r, n) starts with a block at r
  std::vector<uint8_t> dead((size_t)n + 1, 0);
  struct Choice { int64_t pos; int len; };
  std::vector<Choice> path;
  int64_t pos = 0, deepest = 0;
  int first_try = (int)std::min<int64_t>(m, n);
  bool done = false;
  while (!done) {
    bool advanced = false;
    for (int L = first_try; L >= 1; --L) {
      const int64_t end = pos + L;  // end == n: tail block; end == n - 1: the last row is a separator; else a block follows at end + 1
      if (end < n - 1 && dead[end + 1]) continue;
      if (!factor_block<T>(a.data(), b.data(), c.data(), pos, L, true, W) || !(W.growth <= kGrowthLimit)) continue;
      path.push_back({pos, L});
      advanced = true;
      if (end >= n - 1) { done = true; break; }
      pos = end + 1;
      first_try = (int)std::min<int64_t>(m, n - pos);
      break;
    }
    if (advanced) continue;
    dead[pos] = 1;
    deepest = std::max(deepest, pos);
    KS_REQUIRE(!path.empty(), KS_ERR_ARGUMENT,
               "tridiagonal solve: no admissible partition at level " + std::to_string(level) + ": every block starting at row " +
                   std::to_string(deepest) + " of its " + std::to_string(n) + " rows is singular or grows beyond 1e6 (try another block_rows)");
    pos = path.back().pos;
    first_try = path.back().len - 1;
    path.pop_back();
  }
  const int64_t nb = (int64_t)path.size();
  const int slot = m + 1;
  V.nblocks = nb;
  V.start.resize(nb);
  V.len.resize(nb);
  V.mult.assign((size_t)nb * m, T(0)); V.inv.assign((size_t)nb * m, T(0)); V.u1.assign((size_t)nb * m, T(0)); V.u2.assign((size_t)nb * m, T(0));
  V.flag.assign((size_t)nb * m, 0);
  V.w.assign((size_t)nb * slot, T(0));
  V.v.assign((size_t)nb * slot, T(0));
  for (int64_t p = 0; p < nb; ++p) {
    const int64_t r0 = path[p].pos;
    const int L = path[p].len;
    V.start[p] = (int32_t)r0;
    V.len[p] = L;
    if (L < std::min<int64_t>(m, n - r0)) P.shortened++;
    factor_block<T>(a.data(), b.data(), c.data(), r0, L, true, W);
    P.max_growth = std::max(P.max_growth, W.growth);
    for (int i = 0; i < L; ++i) {
      const size_t q = (size_t)i * nb + p;
      V.mult[q] = W.mult[i]; V.inv[q] = W.inv[i]; V.u1[q] = W.u1[i]; V.u2[q] = W.u2[i]; V.flag[q] = W.flag[i];
      V.w[(size_t)p * slot + i] = W.w[i];
      V.v[(size_t)p * slot + i] = W.v[i];
    }
    if (r0 + L < n) {
      V.sep.push_back((int32_t)(r0 + L));
      V.sdl.push_back(a[r0 + L]);
      V.sdu.push_back(c[r0 + L]);
    }
  }
  V.nsep = (int64_t)V.sep.size();
}

// the Schur system of the separators of level V (a, b, c: V's own diagonals)
template <class T>
void schur_system(const Level<T>& V, const std::vector<T>& a, const std::vector<T>& b, const std::vector<T>& c, std::vector<T>& a1,
                  std::vector<T>& b1, std::vector<T>& c1) {
  const int64_t q = V.nsep;
  const int slot = V.cap + 1;
  a1.assign(q, T(0)); b1.assign(q, T(0)); c1.assign(q, T(0));
  for (int64_t j = 0; j < q; ++j) {
    const int64_t s = V.sep[j];
    const size_t last = (size_t)j * slot + (V.len[j] - 1);
    const bool right = j + 1 < V.nblocks;
    const T wf = right ? V.w[(size_t)(j + 1) * slot] : T(0), vf = right ? V.v[(size_t)(j + 1) * slot] : T(0);
    b1[j] = nmsub(c[s], wf, nmsub(a[s], V.v[last], b[s]));
    if (j > 0) a1[j] = neg(mul(a[s], V.w[last]));
    if (j + 1 < q) c1[j] = neg(mul(c[s], vf));
  }
}

// ---- host apply: the arrays the device reads, in the order the device reads them ------------------------------------------------
template <class T> struct Scratch {
  std::vector<std::vector<T>> g;  // g[l]: right-hand side, then solution, of level l >= 1
  std::vector<T> buf;
  explicit Scratch(const Plan<T>& P) : g(P.levels.size()) {
    int cap = 1;
    for (size_t l = 0; l < P.levels.size(); ++l) {
      if (l > 0) g[l].assign((size_t)P.levels[l].n, T(0));
      cap = std::max(cap, P.levels[l].cap + 1);
    }
    buf.assign(cap, T(0));
  }
};

template <class T> void host_apply(const Plan<T>& P, const T* x, T* y, Scratch<T>& S) {
  const int nl = (int)P.levels.size();
  for (int l = 0; l < nl; ++l) {  // down
    const Level<T>& V = P.levels[l];
    T* g = l == 0 ? y : S.g[l].data();
    const Level<T>* B = l > 0 ? &P.levels[l - 1] : nullptr;
    const T* gb = l == 0 ? nullptr : (l == 1 ? y : S.g[l - 1].data());
    auto rhs = [&](int64_t row) -> T {
      if (!B) return x[row];
      const int64_t s = B->sep[row];
      const T nxt = s + 1 < B->n ? gb[s + 1] : T(0);
      return nmsub(B->sdu[row], nxt, nmsub(B->sdl[row], gb[s - 1], gb[s]));
    };
    for (int64_t p = 0; p < V.nblocks; ++p) {
      const int L = V.len[p];
      const int64_t r0 = V.start[p];
      const int rows = (int)std::min<int64_t>(L + 1, V.n - r0);  // with the separator slot
      for (int i = 0; i < rows; ++i) S.buf[i] = rhs(r0 + i);
      walk_block<T>(L, V.mult.data() + p, V.flag.data() + p, V.inv.data() + p, V.u1.data() + p, V.u2.data() + p, V.nblocks, S.buf.data());
      for (int i = 0; i < rows; ++i) g[r0 + i] = S.buf[i];
    }
  }
  for (int l = nl - 2; l >= 0; --l) {  // up
    const Level<T>& V = P.levels[l];
    T* g = l == 0 ? y : S.g[l].data();
    const T* z = S.g[l + 1].data();
    const int slot = V.cap + 1;
    for (int64_t p = 0; p < V.nblocks; ++p) {
      const T zl = p > 0 ? z[p - 1] : T(0), zr = p < V.nsep ? z[p] : T(0);
      const int64_t r0 = V.start[p];
      for (int i = 0; i < V.len[p]; ++i)
        g[r0 + i] = nmsub(V.v[(size_t)p * slot + i], zr, nmsub(V.w[(size_t)p * slot + i], zl, g[r0 + i]));
      if (p < V.nsep) g[r0 + V.len[p]] = zr;
    }
  }
}

// ---- the whole plan ----------------------------------------------------------------------------------------------------------------
// dl, du: n - 1 entries, d: n entries; sigma is subtracted from d.  block_rows: 0 (default) or 2...64.
template <class T> Plan<T> build_plan(int64_t n, const T* dl, const T* d, const T* du, T sigma, int block_rows) {
  KS_REQUIRE(n >= 1 && n < (int64_t)2147483647, KS_ERR_ARGUMENT, "tridiagonal solve: n must be in [1, 2^31)");
  KS_REQUIRE(block_rows == 0 || (block_rows >= kMinBlockRows && block_rows <= kMaxBlockRows), KS_ERR_ARGUMENT,
             "tridiagonal solve: block_rows must be 0 (default) or in [2, 64]");
  KS_REQUIRE(d && (n == 1 || (dl && du)), KS_ERR_ARGUMENT, "tridiagonal solve: null diagonal");
  KS_REQUIRE(is_finite(sigma), KS_ERR_ARGUMENT, "tridiagonal solve: sigma is not finite");
  const int m = block_rows ? block_rows : kDefaultBlockRows;
  Plan<T> P;
  P.n = n;
  P.block_rows = m;
  std::vector<T> a((size_t)n, T(0)), b((size_t)n), c((size_t)n, T(0));
  for (int64_t i = 0; i < n; ++i) {
    b[i] = d[i] - sigma;
    if (i > 0) a[i] = dl[i - 1];
    if (i + 1 < n) c[i] = du[i];
    KS_REQUIRE(is_finite(a[i]) && is_finite(b[i]) && is_finite(c[i]), KS_ERR_ARGUMENT,
               "tridiagonal solve: non-finite entry in row " + std::to_string(i));
  }
  for (int64_t j = 0; j < n; ++j)
    P.norm1 = std::max(P.norm1, std::abs(b[j]) + (j > 0 ? std::abs(c[j - 1]) : 0.0) + (j + 1 < n ? std::abs(a[j + 1]) : 0.0));
  const std::vector<T> a0 = a, b0 = b, c0 = c;
  for (int level = 0;; ++level) {
    KS_REQUIRE(level < kMaxLevels, KS_ERR_ARGUMENT, "tridiagonal solve: more than 8 levels (use a larger block_rows)");
    P.levels.emplace_back();
    plan_level<T>(level, a, b, c, m, P, P.levels.back());
    if (P.levels.back().direct) break;
    std::vector<T> a1, b1, c1;
    schur_system<T>(P.levels.back(), a, b, c, a1, b1, c1);
    for (size_t j = 0; j < b1.size(); ++j)
      KS_REQUIRE(is_finite(a1[j]) && is_finite(b1[j]) && is_finite(c1[j]), KS_ERR_ARGUMENT,
                 "tridiagonal solve: the reduced system of level " + std::to_string(level + 1) + " is not finite in row " + std::to_string(j));
    a.swap(a1); b.swap(b1); c.swap(c1);
  }
  // check solve: b_i = cos(0.7 i + 0.3), eta = ||M x - b||_2 / (||M||_1 ||x||_2 + ||b||_2)
  {
    std::vector<T> rhs((size_t)n), x((size_t)n);
    for (int64_t i = 0; i < n; ++i) rhs[i] = T(std::cos(0.7 * (double)i + 0.3));
    Scratch<T> S(P);
    host_apply<T>(P, rhs.data(), x.data(), S);
    double rr = 0.0, xx = 0.0, bb = 0.0;
    bool finite = true;
    for (int64_t i = 0; i < n; ++i) {
      T r = mul(b0[i], x[i]) - rhs[i];
      if (i > 0) r += mul(a0[i], x[i - 1]);
      if (i + 1 < n) r += mul(c0[i], x[i + 1]);
      finite = finite && is_finite(x[i]);
      rr += std::norm(r); xx += std::norm(x[i]); bb += std::norm(rhs[i]);
    }
    P.residual = finite ? std::sqrt(rr) / (P.norm1 * std::sqrt(xx) + std::sqrt(bb)) : std::numeric_limits<double>::infinity();
    char eta[32];
    std::snprintf(eta, sizeof eta, "%.3g", P.residual);
    KS_REQUIRE(P.residual <= kResidualLimit, KS_ERR_ARGUMENT,
               std::string("tridiagonal solve: the check solve has backward error ") + eta + " (> 1e-10): T - sigma I is singular or too ill-conditioned for this factorisation");
  }
  return P;
}

// plan, report, and the host apply on nrhs columns: what ks_host_tridiag_solve / ks_host_tridiag_info export
template <class H>
void host_solve(int64_t n, const void* dl, const void* d, const void* du, double sre, double sim, int block_rows, int nrhs, const void* b,
                  int64_t ldb, void* x, int64_t ldx, int* levels, int64_t* level_rows, int64_t* shortened_blocks, double* max_growth,
                  double* residual) {
  H sigma;
  if constexpr (std::is_same<H, double>::value) sigma = sre;
  else sigma = H(sre, sim);
  const Plan<H> P = build_plan<H>(n, static_cast<const H*>(dl), static_cast<const H*>(d), static_cast<const H*>(du), sigma, block_rows);
  if (levels) *levels = (int)P.levels.size();
  for (int l = 0; level_rows && l < kMaxLevels; ++l) level_rows[l] = l < (int)P.levels.size() ? P.levels[l].n : 0;
  if (shortened_blocks) *shortened_blocks = P.shortened;
  if (max_growth) *max_growth = P.max_growth;
  if (residual) *residual = P.residual;
  Scratch<H> S(P);
  for (int k = 0; k < nrhs; ++k) host_apply<H>(P, static_cast<const H*>(b) + (int64_t)k * ldb, static_cast<H*>(x) + (int64_t)k * ldx, S);
}

}  // namespace td
}  // namespace
