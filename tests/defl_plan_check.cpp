// Stand-alone host check of csrc/ks_defl_plan.hpp, built by tests/test_defl_plan_cpu.py with the host compiler under
// -fsanitize=address,undefined.  Reads cases from standard input, runs defl_plan_columns on each and prints the plan; the Python test
// compares every line with tests/sstep_model.py: defl_plan.  Each H sits on the heap at exactly the (j0 - 1) x (j0 - 1) entries the
// plan may read (leading dimension j0 - 1), so a read past them is reported.
//
//   input, per case:   <r|c> <j0> <steps> <nmax> <ratio> <nritz>   then (j0 - 1)^2 entries of H, column by column (re [im]), then
//                      nritz Ritz values (re im; "inf" / "nan" allowed)
//   output, per case:  <nd> <number of excluded eigenvalues> then those (re im), %.17g
// A few fixed cases run first.  Prints DEFL_PLAN_CHECK_OK and exits 0 when everything holds and the input was well formed.
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../arnoldimethod.jl_amd/csrc/ks_defl_plan.hpp"

namespace {

int failures = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond);         \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

using C = std::complex<double>;

bool read_double(double& x) {
  std::string tok;
  if (!(std::cin >> tok)) return false;
  char* end = nullptr;
  x = std::strtod(tok.c_str(), &end);
  return end && *end == '\0';
}

template <class T> bool read_entry(T& x);
template <> bool read_entry<double>(double& x) { return read_double(x); }
template <> bool read_entry<C>(C& x) {
  double re, im;
  if (!read_double(re) || !read_double(im)) return false;
  x = C(re, im);
  return true;
}

template <class T> bool run_case(int j0, int steps, int nmax, double ratio, int nritz) {
  const int m = j0 - 1 > 0 ? j0 - 1 : 0;
  std::vector<T> H((size_t)m * m);
  for (auto& x : H)
    if (!read_entry<T>(x)) return false;
  std::vector<C> ritz((size_t)nritz);
  for (auto& z : ritz)
    if (!read_entry<C>(z)) return false;
  std::vector<C> ex;
  const int nd = defl_plan_columns<T>(m ? H.data() : nullptr, m > 0 ? m : 1, j0, nritz ? ritz.data() : nullptr, nritz, ratio, steps, nmax, ex);
  CHECK(nd >= 0 && nd <= nmax && (int)ex.size() == nd);
  std::printf("%d %d", nd, (int)ex.size());
  for (const C& z : ex) std::printf(" %.17g %.17g", z.real(), z.imag());
  std::printf("\n");
  return true;
}

void fixed_cases() {
  std::vector<C> ex(3, C(1.0, 1.0));
  const C ritz[3] = {C(50.0), C(1.0), C(0.5, 0.5)};
  // no H, no Ritz values, nothing locked: no plan, and `ex` comes back empty
  CHECK(defl_plan_columns<double>(nullptr, 1, 5, ritz, 3, 1.5, 10, 16, ex) == 0 && ex.empty());
  std::vector<double> H(16, 0.0);   // 4 x 4
  H[0] = 50.0;
  H[1 + 4 * 1] = 1.0; H[2 + 4 * 1] = 0.3; H[2 + 4 * 2] = 0.7; H[3 + 4 * 2] = 0.2; H[3 + 4 * 3] = 0.1;
  CHECK(defl_plan_columns<double>(H.data(), 4, 5, nullptr, 0, 1.5, 10, 16, ex) == 0);
  CHECK(defl_plan_columns<double>(H.data(), 4, 5, ritz, 3, 1.5, 10, 16, ex) == 1 && ex.size() == 1 && ex[0] == C(50.0));
  CHECK(defl_plan_columns<double>(H.data(), 4, 5, ritz, 3, 1.5, 10, 0, ex) == 0 && ex.empty());        // no room
  CHECK(defl_plan_columns<double>(H.data(), 4, 2, ritz, 3, 1.5, 10, 16, ex) == 0);                      // j0 too small to lock anything
  H[1] = 0.4;                                                                                             // H(1, 0): nothing decoupled
  CHECK(defl_plan_columns<double>(H.data(), 4, 5, ritz, 3, 1.5, 10, 16, ex) == 0);
  const C inf[2] = {C(std::numeric_limits<double>::infinity(), 0.0), C(std::nan(""), 0.0)};
  H[1] = 0.0;
  CHECK(defl_plan_columns<double>(H.data(), 4, 5, inf, 2, 1.5, 10, 16, ex) == 0);                       // no finite Ritz value
}

}  // namespace

int main() {
  fixed_cases();
  std::string kind;
  int ncases = 0;
  while (std::cin >> kind) {
    double j0, steps, nmax, ratio, nritz;
    if (!read_double(j0) || !read_double(steps) || !read_double(nmax) || !read_double(ratio) || !read_double(nritz) || (kind != "r" && kind != "c")) {
      std::printf("malformed header of case %d\n", ncases);
      return 2;
    }
    const bool ok = kind == "r" ? run_case<double>((int)j0, (int)steps, (int)nmax, ratio, (int)nritz) : run_case<C>((int)j0, (int)steps, (int)nmax, ratio, (int)nritz);
    if (!ok) {
      std::printf("malformed body of case %d\n", ncases);
      return 2;
    }
    ++ncases;
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("DEFL_PLAN_CHECK_OK %d\n", ncases);
  return 0;
}
