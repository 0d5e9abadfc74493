// BiCGStab(2) solve  y ~ (A - theta I)^-1 x  for ANY device operator A that can be enqueued ahead (ks_operator_bicgstab,
// include/kschur.h): shift-invert for operators that are not Hermitian -- a convection term, a complex shift -- and have nothing to
// factor, the inner iterative solver of the reference's "LinearMap around a solve" (docs/src/index.md:234-259) where ks_operator_cg
// and ks_operator_minres (ks_cg.hpp, ks_minres.hpp) need a Hermitian operator.  Part of the ONE translation unit of
// libkschur_hip.so: included by ks_hip.hip after ks_minres.hpp; it shares block_range, cg_put, cg_owns_tail, the launch shape
// (cg_blocks), the two-slot record protocol and the chunked host loop with them.
//
// A is BORROWED like a product's factors.  The solver owns six vectors r0, r1, r2, u0, u1, u2, allocated like CgOp's (a multiple of
// 64 elements, zero-filled once; every kernel writes rows < n_local only).  rt = b is the caller's input: read, never copied, never
// written.  <a, c> = a^H c.  Bytes per row in Float64 (ComplexF64: twice):
//
//   init:  y = 0, r0 = b, rho1 = ||b||^2, rho0 = 1, alpha = 0, omega = 1        k_bs_init (24) + k_bs_start (one workgroup)
//   k = 1, 2, ...                                                               rho0 <- -omega rho0
//     1   beta = alpha rho1 / rho0;  u0 = r0 - beta u0                          k_bs_u0     reads r0, u0, writes u0            24
//         u1 = (A - theta) u0                                                   product
//     2   gamma = <rt, u1>                                                      k_bs_dot    reads rt, u1                       16
//     3   alpha = rho1 / gamma;  r0 -= alpha u1;  y += alpha u0;  ||r0||^2       k_bs_step1  reads r0, u1, y, u0, writes r0, y  48
//         stage 1 test;  r1 = (A - theta) r0                                    product
//     4   rho1 = <rt, r1>                                                       k_bs_dot                                       16
//     5   beta = alpha rho1 / rho0;  u0 = r0 - beta u0;  u1 = r1 - beta u1      k_bs_dir2   reads r0, u0, r1, u1, writes u0, u1 48
//         u2 = (A - theta) u1                                                   product
//     6   gamma = <rt, u2>                                                      k_bs_dot                                       16
//     7   alpha = rho1 / gamma;  r0 -= alpha u1;  r1 -= alpha u2;  y += alpha u0;  ||r0||^2
//                                                                               k_bs_step2  reads r0, u1, r1, u2, y, u0, writes r0, r1, y  72
//         stage 2 test;  r2 = (A - theta) r1                                    product
//     8   <r1,r1>, <r2,r2>, <r1,r2>, <r1,r0>, <r2,r0>                           k_bs_mr_sums reads r0, r1, r2                  24
//     9   G g = h;  y += g1 r0 + g2 r1;  r0 -= g1 r1 + g2 r2;  u0 -= g1 u1 + g2 u2;  omega = g2;  <rt, r0>, ||r0||^2
//                                                                               k_bs_mr     reads y, r0, r1, r2, u0, u1, u2, rt, writes y, r0, u0  88
//     10  stage 3 test, the record of iteration k                               k_bs_close (one workgroup)
//
// 352 bytes per row and iteration beside the four products: 88 per product (conjugate gradients 80, MINRES 112).  The first
// iteration reads no u0: beta is exactly zero there and the buffer may hold what a failed solve left behind.
//
// SCALARS.  Every kernel writes its per-workgroup partial sums into rows of its own in part[row][workgroup] (BsRows,
// ks_bicgstab_plan.hpp).  A kernel of iteration k reads the record of iteration k - 1 (slot (k - 1) & 1) and the rows that EARLIER
// launches of iteration k wrote, adds each row in one fixed order (bs_sums: cg_sum's order, several rows behind one barrier pair) and
// runs the chain bs_iter itself as far as it needs: identical inputs, identical code, identical coefficients in every workgroup
// and in every run.  From the same chain every kernel derives "a stage of this iteration has already ended the solve" or "a step
// of it broke" and returns at entry -- nothing is read that a sibling workgroup of the same launch may be writing, and no kernel
// reads a row it writes.  A returning kernel leaves its rows stale; the chain of every later kernel stops before it reads them.
// k_bs_close, one workgroup, runs the whole chain and writes the record of iteration k into slot k & 1 (a finished or failed solve:
// the record it found, carried forward).  Scalars are complex for ComplexF64 -- the kernels are templates on the scalar type (double
// or BsZ), and a complex inner product is two rows.
//
// THE HOST enqueues check_every iterations, copies both slots into pinned memory and waits for an event behind that copy; it goes on
// until done, fail or maxit.  After done or fail only the products of the rest of a chunk still run, into u1, r1, u2 and r2, which
// nothing reads again; y and the iteration count do not depend on check_every.
#pragma once

namespace ksd {

// p + a x on a 16-byte pack: two Float64 elements, or one ComplexF64 element
__device__ __forceinline__ double2 bs_axpy(double a, double2 x, double2 p) { return make_double2(fma(a, x.x, p.x), fma(a, x.y, p.y)); }
__device__ __forceinline__ double2 bs_axpy(BsZ a, double2 x, double2 p) {
  return make_double2(fma(a.re, x.x, fma(-a.im, x.y, p.x)), fma(a.re, x.y, fma(a.im, x.x, p.y)));
}
// acc += a^H c on a pack.  The imaginary part is the difference of two products rounded on their own (mul_nc: no contraction), so
// that <a, s a> with a real s has no imaginary part at all: <rt, (A - theta) u> of a real multiple of the identity is exactly real,
// and with k_bs_init summing ||b||^2 by the same operations, gamma = <b, 2 b> is exactly 2 <b, b> in both types.
__device__ __forceinline__ void bs_dot(double& acc, double2 a, double2 c) { acc = fma(a.x, c.x, fma(a.y, c.y, acc)); }
__device__ __forceinline__ void bs_dot(BsZ& acc, double2 a, double2 c) {
  acc.re = fma(a.x, c.x, fma(a.y, c.y, acc.re));
  acc.im += mul_nc(a.x, c.y) - mul_nc(a.y, c.x);
}

using BsRed = double[kBsMaxRows][kBlock / 64];

// sums of rows [0, N) of part[row][workgroup], each in cg_sum's fixed order, behind ONE barrier pair; the same values in every
// thread of every workgroup that asks (all 256 threads call it)
template <int N>
__device__ __forceinline__ void bs_sums(const double* __restrict__ part, int nb, BsRed& red, double* out) {
  if constexpr (N > 0) {
    double s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = 0.0;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
#pragma unroll
      for (int j = 0; j < N; ++j) s[j] += part[(int64_t)j * nb + b];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = wave_sum(s[j]);
    __syncthreads();   // (red may still be read from an earlier sum)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < N; ++j) red[j][threadIdx.x >> 6] = s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = (red[j][0] + red[j][1]) + (red[j][2] + red[j][3]);
  }
}

// a scalar accumulator -> its row (pair) of this workgroup
__device__ __forceinline__ void bs_put(double acc, double* __restrict__ part, int row, int nb, double* red) { cg_put(acc, part + (int64_t)row * nb, red); }
__device__ __forceinline__ void bs_put(BsZ acc, double* __restrict__ part, int row, int nb, double* red) {
  cg_put(acc.re, part + (int64_t)row * nb, red);
  cg_put(acc.im, part + (int64_t)(row + 1) * nb, red);
}

// the entry of every kernel of iteration k: false -> return (the solve has ended or broken, before this iteration or inside it)
template <class S, int LEVEL>
__device__ __forceinline__ bool bs_enter(const BsRecord* __restrict__ rec, int k, const double* __restrict__ part, int nb, double tol, BsRed& red,
                                         BsIter<S>& it) {
  const BsRecord was = rec[(k - 1) & 1];
  if (was.done || was.fail) return false;
  double sums[kBsMaxRows];
  bs_sums<BsRows<S>::upto(LEVEL)>(part, nb, red, sums);
  it = bs_iter<S, LEVEL>(was, tol, sums);
  return !(it.ended || it.fail);
}

// y = 0, r0 = b, row NN of this workgroup = sum b^2 (k_bs_start takes rho1 = <b, b> from it: no imaginary part)
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_init(const double* __restrict__ b, double* __restrict__ y, double* __restrict__ r0, int64_t nd, double* __restrict__ part, int nb) {
  using R = BsRows<S>;
  __shared__ BsRed red;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 v = ld_pack(b + 2 * i);
    st_pack_nt(y + 2 * i, make_double2(0.0, 0.0));
    st_pack(r0 + 2 * i, v);
    bs_dot(acc, v, v);   // (the operations of k_bs_dot's real part, in its order)
  }
  if (cg_owns_tail(nd)) {
    const double v = b[nd - 1];
    y[nd - 1] = 0.0;
    r0[nd - 1] = v;
    acc = fma(v, v, acc);
  }
  cg_put(acc, part + (int64_t)R::NN * nb, red[0]);
}

// ONE workgroup: beta1 from the partial sums of k_bs_init, the record of iteration 0 into slot 0.  ||b|| == 0: done, y = 0 stands;
// not finite: fail.
template <class S>
__global__ void __launch_bounds__(kBlock) k_bs_start(const double* __restrict__ part, int nb, BsRecord* __restrict__ rec) {
  using R = BsRows<S>;
  __shared__ BsRed red;
  const double bb = cg_sum(part + (int64_t)R::NN * nb, nb, red[0]);
  if (threadIdx.x == 0) {
    BsRecord r{};
    r.iteration = 0;
    r.done = bb == 0.0 ? 1 : 0;
    r.fail = cg_finite(bb) ? 0 : 6;
    r.stage = 0;
    r.beta1 = sqrt(bb);
    r.rr = bb;
    r.rho0[0] = 1.0;
    r.omega[0] = 1.0;
    r.rho1[0] = bb;
    rec[0] = r;
  }
}

// 1: u0 = r0 - beta u0 (k == 1: u0 = r0, the old u0 is not read)
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_u0(double* __restrict__ u0, const double* __restrict__ r0, int64_t nd, const double* __restrict__ part, int nb, double tol,
            const BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 0>(rec, k, part, nb, tol, red, it)) return;
  const S mb = bs_neg(it.beta_1);
  const bool first = k == 1;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    double2 u = ld_pack(r0 + 2 * i);
    if (!first) u = bs_axpy(mb, ld_pack(u0 + 2 * i), u);
    st_pack(u0 + 2 * i, u);   // (cacheable: the next product gathers exactly this vector)
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const int64_t i = nd - 1;
      u0[i] = first ? r0[i] : fma(mb, u0[i], r0[i]);
    }
  }
}

// 2, 4, 6: row `row` = <rt, v>.  LEVEL is what the chain must have passed for v to be this iteration's vector.
template <class S, int LEVEL>
__global__ void __launch_bounds__(kBlock)
    k_bs_dot(const double* __restrict__ rt, const double* __restrict__ v, int64_t nd, double* __restrict__ part, int row, int nb, double tol,
             const BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, LEVEL>(rec, k, part, nb, tol, red, it)) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  S acc = bs_real<S>(0.0);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) bs_dot(acc, ld_pack(rt + 2 * i), ld_pack(v + 2 * i));
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) acc = fma(rt[nd - 1], v[nd - 1], acc);
  }
  bs_put(acc, part, row, nb, red[0]);
}

// 3: r0 -= alpha u1, y += alpha u0, row N1 = ||r0||^2
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_step1(double* __restrict__ r0, const double* __restrict__ u1, double* __restrict__ y, const double* __restrict__ u0, int64_t nd,
               double* __restrict__ part, int nb, double tol, const BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 1>(rec, k, part, nb, tol, red, it)) return;
  const S a = it.alpha_1, ma = bs_neg(a);
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 r = bs_axpy(ma, ld_pack(u1 + 2 * i), ld_pack(r0 + 2 * i));
    const double2 yv = bs_axpy(a, ld_pack(u0 + 2 * i), ld_pack(y + 2 * i));
    st_pack(r0 + 2 * i, r);   // (cacheable: the next product gathers exactly this vector)
    st_pack_nt(y + 2 * i, yv);
    acc += nrm2_pack(r);
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const int64_t i = nd - 1;
      const double r = fma(ma, u1[i], r0[i]);
      r0[i] = r;
      y[i] = fma(a, u0[i], y[i]);
      acc = fma(r, r, acc);
    }
  }
  cg_put(acc, part + (int64_t)BsRows<S>::N1 * nb, red[0]);
}

// 5: u0 = r0 - beta u0, u1 = r1 - beta u1
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_dir2(double* __restrict__ u0, double* __restrict__ u1, const double* __restrict__ r0, const double* __restrict__ r1, int64_t nd,
              const double* __restrict__ part, int nb, double tol, const BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 3>(rec, k, part, nb, tol, red, it)) return;
  const S mb = bs_neg(it.beta_2);
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 a = bs_axpy(mb, ld_pack(u0 + 2 * i), ld_pack(r0 + 2 * i));
    const double2 c = bs_axpy(mb, ld_pack(u1 + 2 * i), ld_pack(r1 + 2 * i));
    st_pack(u0 + 2 * i, a);
    st_pack(u1 + 2 * i, c);   // (cacheable: the next product gathers exactly this vector)
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const int64_t i = nd - 1;
      u0[i] = fma(mb, u0[i], r0[i]);
      u1[i] = fma(mb, u1[i], r1[i]);
    }
  }
}

// 7: r0 -= alpha u1, r1 -= alpha u2, y += alpha u0, row N2 = ||r0||^2
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_step2(double* __restrict__ r0, double* __restrict__ r1, double* __restrict__ y, const double* __restrict__ u0,
               const double* __restrict__ u1, const double* __restrict__ u2, int64_t nd, double* __restrict__ part, int nb, double tol,
               const BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 4>(rec, k, part, nb, tol, red, it)) return;
  const S a = it.alpha_2, ma = bs_neg(a);
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double acc = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 r = bs_axpy(ma, ld_pack(u1 + 2 * i), ld_pack(r0 + 2 * i));
    const double2 q = bs_axpy(ma, ld_pack(u2 + 2 * i), ld_pack(r1 + 2 * i));
    const double2 yv = bs_axpy(a, ld_pack(u0 + 2 * i), ld_pack(y + 2 * i));
    st_pack(r0 + 2 * i, r);
    st_pack(r1 + 2 * i, q);   // (cacheable: the next product gathers exactly this vector)
    st_pack_nt(y + 2 * i, yv);
    acc += nrm2_pack(r);
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const int64_t i = nd - 1;
      const double r = fma(ma, u1[i], r0[i]);
      r0[i] = r;
      r1[i] = fma(ma, u2[i], r1[i]);
      y[i] = fma(a, u0[i], y[i]);
      acc = fma(r, r, acc);
    }
  }
  cg_put(acc, part + (int64_t)BsRows<S>::N2 * nb, red[0]);
}

// 8: the five sums of the minimal-residual step, rows M11 ... H2
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_mr_sums(const double* __restrict__ r0, const double* __restrict__ r1, const double* __restrict__ r2, int64_t nd,
                 double* __restrict__ part, int nb, double tol, const BsRecord* __restrict__ rec, int k) {
  using R = BsRows<S>;
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 5>(rec, k, part, nb, tol, red, it)) return;
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  double m11 = 0.0, m22 = 0.0;
  S m12 = bs_real<S>(0.0), h1 = m12, h2 = m12;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 a = ld_pack(r0 + 2 * i), b = ld_pack(r1 + 2 * i), c = ld_pack(r2 + 2 * i);
    m11 += nrm2_pack(b);
    m22 += nrm2_pack(c);
    bs_dot(m12, b, c);
    bs_dot(h1, b, a);
    bs_dot(h2, c, a);
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const double a = r0[nd - 1], b = r1[nd - 1], c = r2[nd - 1];
      m11 = fma(b, b, m11);
      m22 = fma(c, c, m22);
      m12 = fma(b, c, m12);
      h1 = fma(b, a, h1);
      h2 = fma(c, a, h2);
    }
  }
  cg_put(m11, part + (int64_t)R::M11 * nb, red[0]);
  cg_put(m22, part + (int64_t)R::M22 * nb, red[0]);
  bs_put(m12, part, R::M12, nb, red[0]);
  bs_put(h1, part, R::H1, nb, red[0]);
  bs_put(h2, part, R::H2, nb, red[0]);
}

// 9: y += g1 r0 + g2 r1;  r0 -= g1 r1 + g2 r2;  u0 -= g1 u1 + g2 u2;  rows RHO = <rt, r0>, NN = ||r0||^2 of the new r0.  Every vector
// is read and written at the same index by the same thread.
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_mr(double* __restrict__ y, double* __restrict__ r0, const double* __restrict__ r1, const double* __restrict__ r2,
            double* __restrict__ u0, const double* __restrict__ u1, const double* __restrict__ u2, const double* __restrict__ rt, int64_t nd,
            double* __restrict__ part, int nb, double tol, const BsRecord* __restrict__ rec, int k) {
  using R = BsRows<S>;
  __shared__ BsRed red;
  BsIter<S> it;
  if (!bs_enter<S, 6>(rec, k, part, nb, tol, red, it)) return;
  const S g1 = it.g1, g2 = it.g2, mg1 = bs_neg(g1), mg2 = bs_neg(g2);
  int64_t pb, pe;
  block_range(nd / 2, blockIdx.x, gridDim.x, pb, pe);
  S rho = bs_real<S>(0.0);
  double nn = 0.0;
  for (int64_t i = pb + threadIdx.x; i < pe; i += kBlock) {
    const double2 a = ld_pack(r0 + 2 * i);
    const double2 b = ld_pack_nt(r1 + 2 * i), c = ld_pack_nt(r2 + 2 * i);      // (their last use: the next products overwrite them)
    const double2 p = ld_pack_nt(u1 + 2 * i), q = ld_pack_nt(u2 + 2 * i);
    const double2 yv = bs_axpy(g2, b, bs_axpy(g1, a, ld_pack(y + 2 * i)));
    const double2 r = bs_axpy(mg2, c, bs_axpy(mg1, b, a));
    const double2 u = bs_axpy(mg2, q, bs_axpy(mg1, p, ld_pack(u0 + 2 * i)));
    st_pack_nt(y + 2 * i, yv);
    st_pack(r0 + 2 * i, r);
    st_pack(u0 + 2 * i, u);
    bs_dot(rho, ld_pack(rt + 2 * i), r);
    nn += nrm2_pack(r);
  }
  if constexpr (sizeof(S) == 8) {
    if (cg_owns_tail(nd)) {
      const int64_t i = nd - 1;
      const double a = r0[i], b = r1[i], c = r2[i];
      y[i] = fma(g2, b, fma(g1, a, y[i]));
      const double r = fma(mg2, c, fma(mg1, b, a));
      r0[i] = r;
      u0[i] = fma(mg2, u2[i], fma(mg1, u1[i], u0[i]));
      rho = fma(rt[i], r, rho);
      nn = fma(r, r, nn);
    }
  }
  bs_put(rho, part, R::RHO, nb, red[0]);
  cg_put(nn, part + (int64_t)R::NN * nb, red[0]);
}

// 10, ONE workgroup: the whole chain of iteration k, its record into slot k & 1
template <class S>
__global__ void __launch_bounds__(kBlock)
    k_bs_close(const double* __restrict__ part, int nb, double tol, BsRecord* __restrict__ rec, int k) {
  __shared__ BsRed red;
  const BsRecord was = rec[(k - 1) & 1];
  BsRecord* out = rec + (k & 1);
  if (was.done || was.fail) {
    if (threadIdx.x == 0) *out = was;
    return;
  }
  double sums[kBsMaxRows];
  bs_sums<BsRows<S>::COUNT>(part, nb, red, sums);
  const BsIter<S> it = bs_iter<S, 7>(was, tol, sums);
  if (threadIdx.x == 0) {
    BsRecord r = was;
    r.iteration = k;
    r.done = it.ended ? 1 : 0;
    r.fail = it.fail;
    r.stage = it.ended ? it.ended : it.fail == 0 ? 3 : it.fail <= 2 ? 1 : it.fail <= 4 ? 2 : 3;
    r.rr = it.rr;
    bs_store(r.rho0, it.rho0);
    bs_store(r.alpha, it.alpha);
    bs_store(r.omega, it.omega);
    bs_store(r.rho1, it.rho1);
    bs_store(r.bad, it.bad);
    *out = r;
  }
}

}  // namespace ksd

namespace {

struct BicgstabOp : ks_operator {
  ks_operator* A = nullptr;
  double theta_re = 0.0, theta_im = 0.0, tol = 0.0;
  int maxit = 0, check_every = kCgDefaultCheckEvery;
  void* vec[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // r0, r1, r2, u0, u1, u2
  double* part = nullptr;                                                  // [BsRows::COUNT][nb]
  BsRecord* rec = nullptr;                                                 // device, two slots
  BsRecord* rec_h = nullptr;                                               // pinned copy of both
  hipEvent_t ev = nullptr;
  int nb = 1;
  int64_t applications = 0, iterations = 0;
  int last_iterations = 0, last_stage = 0;
  double last_relres = 0.0, worst_relres = 0.0;
  ~BicgstabOp() override {
    for (void* p : vec) (void)hipFree(p);
    (void)hipFree(part); (void)hipFree(rec);
    (void)hipHostFree(rec_h);
    if (ev) (void)hipEventDestroy(ev);
  }
  void product(const double* x, double* y, int64_t ld, const DevState* st) {
    A->in_scale = 1.0;
    if (theta_re == 0.0 && theta_im == 0.0) A->apply(x, y, st);
    else A->apply_shifted(x, y, theta_re, theta_im, 1.0, ld, st);
  }
  // (the profile classes tell the kernels apart: dots = the three k_bs_dot, axpy = k_bs_u0, rotate = k_bs_step1 and k_bs_dir2,
  // fin = k_bs_step2, scale = k_bs_mr_sums, fused = k_bs_mr with k_bs_close)
  template <class S>
  void solve(const double* b, double* y, const DevState* st) {
    using R = BsRows<S>;
    hipStream_t s = ctx->stream;
    const int64_t nd = n_local * (dtype == KS_F64 ? 1 : 2), ld = round_up(n_local, 64);
    const double B = 8.0 * (double)nd;
    double* v[6];
    for (int t = 0; t < 6; ++t) v[t] = static_cast<double*>(vec[t]);
    double *r0 = v[0], *r1 = v[1], *r2 = v[2], *u0 = v[3], *u1 = v[4], *u2 = v[5];
    ksd::k_bs_init<S><<<nb, kBlock, 0, s>>>(b, y, r0, nd, part, nb);
    ksd::k_bs_start<S><<<1, kBlock, 0, s>>>(part, nb, rec);
    KS_HIP(hipGetLastError());
    ++applications;
    const int every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
    int k = 0;
    BsRecord rd{};
    for (;;) {
      const int upto = std::min(maxit, k + every);
      while (k < upto) {
        ++k;
        {
          ProfScope ps(ctx, KSP_AXPY, 3.0 * B);
          ksd::k_bs_u0<S><<<nb, kBlock, 0, s>>>(u0, r0, nd, part, nb, tol, rec, k);
        }
        product(u0, u1, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_bs_dot<S, 0><<<nb, kBlock, 0, s>>>(b, u1, nd, part, R::G1, nb, tol, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_ROTATE, 6.0 * B);
          ksd::k_bs_step1<S><<<nb, kBlock, 0, s>>>(r0, u1, y, u0, nd, part, nb, tol, rec, k);
        }
        product(r0, r1, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_bs_dot<S, 2><<<nb, kBlock, 0, s>>>(b, r1, nd, part, R::R2, nb, tol, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_ROTATE, 6.0 * B);
          ksd::k_bs_dir2<S><<<nb, kBlock, 0, s>>>(u0, u1, r0, r1, nd, part, nb, tol, rec, k);
        }
        product(u1, u2, ld, st);
        {
          ProfScope ps(ctx, KSP_DOTS, 2.0 * B);
          ksd::k_bs_dot<S, 3><<<nb, kBlock, 0, s>>>(b, u2, nd, part, R::G2, nb, tol, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_FIN, 9.0 * B);
          ksd::k_bs_step2<S><<<nb, kBlock, 0, s>>>(r0, r1, y, u0, u1, u2, nd, part, nb, tol, rec, k);
        }
        product(r1, r2, ld, st);
        {
          ProfScope ps(ctx, KSP_SCALE, 3.0 * B);
          ksd::k_bs_mr_sums<S><<<nb, kBlock, 0, s>>>(r0, r1, r2, nd, part, nb, tol, rec, k);
        }
        {
          ProfScope ps(ctx, KSP_FUSED, 11.0 * B);
          ksd::k_bs_mr<S><<<nb, kBlock, 0, s>>>(y, r0, r1, r2, u0, u1, u2, b, nd, part, nb, tol, rec, k);
          ksd::k_bs_close<S><<<1, kBlock, 0, s>>>(part, nb, tol, rec, k);
        }
        KS_HIP(hipGetLastError());
      }
      KS_HIP(hipMemcpyAsync(rec_h, rec, 2 * sizeof(BsRecord), hipMemcpyDeviceToHost, s));
      KS_HIP(hipEventRecord(ev, s));
      KS_HIP(hipEventSynchronize(ev));
      rd = rec_h[k & 1];
      if (rd.done || rd.fail || k >= maxit) break;
    }
    last_iterations = rd.iteration;
    last_stage = rd.stage;
    iterations += rd.iteration;
    last_relres = rd.beta1 > 0.0 ? std::sqrt(rd.rr) / rd.beta1 : 0.0;
    if (!(last_relres <= worst_relres)) worst_relres = last_relres;   // (a NaN sticks)
    auto sci = [](double x) { char buf[40]; std::snprintf(buf, sizeof buf, "%.6g", x); return std::string(buf); };
    auto val = [&](const double* z) { return dtype == KS_F64 ? sci(z[0]) : "(" + sci(z[0]) + ", " + sci(z[1]) + ")"; };
    if (rd.fail) {
      if (rd.iteration == 0) throw KsError{KS_ERR_OPERATOR, "ks_operator_bicgstab: the right-hand side is not finite"};
      const char* what = rd.fail == 5 ? "det G = " : (rd.fail == 1 || rd.fail == 3) ? "rho = " : "gamma = ";
      throw KsError{KS_ERR_OPERATOR, std::string("ks_operator_bicgstab: breakdown: ") + what + (rd.fail == 5 ? sci(rd.bad[0]) : val(rd.bad)) + " in stage " +
                                         std::to_string(rd.stage) + " at iteration " + std::to_string(rd.iteration) + " [rho1 = " + val(rd.rho1) +
                                         ", alpha = " + val(rd.alpha) + ", omega = " + val(rd.omega) + "]" +
                                         " (the shift is an eigenvalue, the shadow residual has lost the Krylov space, or the operator returned values that are not finite)"};
    }
    if (!rd.done)
      throw KsError{KS_ERR_OPERATOR, "ks_operator_bicgstab: did not converge: relative residual " + sci(last_relres) + " after " + std::to_string(maxit) + " iterations"};
  }
  void apply(const void* x, void* y, const DevState* st) override {
    KS_REQUIRE(x != y, KS_ERR_ARGUMENT, "BiCGStab(2): the solve needs distinct x and y");
    auto aligned = [](const void* v) { return (reinterpret_cast<uintptr_t>(v) & 15u) == 0; };
    KS_REQUIRE(aligned(x) && aligned(y), KS_ERR_ARGUMENT, "BiCGStab(2): a vector is not 16-byte aligned");
    if (n_local <= 0) return;
    if (dtype == KS_F64) solve<double>(static_cast<const double*>(x), static_cast<double*>(y), st);
    else solve<BsZ>(static_cast<const double*>(x), static_cast<double*>(y), st);
  }
};

inline ks_operator* make_bicgstab(ks_ctx* ctx, ks_operator* A, double shift_re, double shift_im, double tol, int maxit, int check_every) {
  auto op = std::make_unique<BicgstabOp>();
  op->ctx = ctx;
  KS_REQUIRE(A->ctx == ctx, KS_ERR_ARGUMENT, "ks_operator_bicgstab: the operator lives on another context");
  KS_REQUIRE(A->dtype == KS_F64 || A->dtype == KS_C64, KS_ERR_ARGUMENT, "ks_operator_bicgstab: the operator is neither Float64 nor ComplexF64");
  KS_REQUIRE(A->async_capable, KS_ERR_ARGUMENT,
             "ks_operator_bicgstab: the operator cannot be enqueued ahead (a host callback, a conjugate-gradient, MINRES or BiCGStab solve, or a product or filter of one)");
  KS_REQUIRE(std::isfinite(tol) && tol > 0.0 && tol < 1.0, KS_ERR_ARGUMENT, "ks_operator_bicgstab: tol = " + std::to_string(tol) + " (must lie in (0, 1))");
  KS_REQUIRE(maxit >= 1, KS_ERR_ARGUMENT, "ks_operator_bicgstab: maxit = " + std::to_string(maxit) + " (must be at least 1)");
  KS_REQUIRE(check_every >= 0, KS_ERR_ARGUMENT, "ks_operator_bicgstab: check_every = " + std::to_string(check_every) + " (must not be negative; 0: the library default)");
  KS_REQUIRE(std::isfinite(shift_re) && std::isfinite(shift_im), KS_ERR_ARGUMENT, "ks_operator_bicgstab: shift is not finite");
  KS_REQUIRE(shift_im == 0.0 || A->dtype == KS_C64, KS_ERR_ARGUMENT,
             "ks_operator_bicgstab: an imaginary shift on a Float64 operator (build the operator in ComplexF64: the solve runs in the operator's type)");
  op->A = A;
  op->theta_re = shift_re;
  op->theta_im = shift_im;
  op->tol = tol;
  op->maxit = maxit;
  op->check_every = check_every > 0 ? check_every : kCgDefaultCheckEvery;
  op->n_local = A->n_local;
  op->dtype = A->dtype;
  op->async_capable = false;   // the host reads the record between chunks: one step per batch, like a host callback
  op->nnz = A->nnz;
  const int64_t nd = op->n_local * (op->dtype == KS_F64 ? 1 : 2);
  op->nb = CgOp::cg_blocks(ctx, nd);
  const size_t bytes = (size_t)std::max<int64_t>(round_up(op->n_local, 64), 64) * (op->dtype == KS_F64 ? 8 : 16);
  for (int t = 0; t < 6; ++t) {
    KS_HIP(hipMalloc(&op->vec[t], bytes));
    KS_HIP(hipMemset(op->vec[t], 0, bytes));
  }
  const size_t part_bytes = (size_t)kBsMaxRows * op->nb * sizeof(double);
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->part), part_bytes));
  KS_HIP(hipMemset(op->part, 0, part_bytes));
  KS_HIP(hipMalloc(reinterpret_cast<void**>(&op->rec), 2 * sizeof(BsRecord)));
  KS_HIP(hipMemset(op->rec, 0, 2 * sizeof(BsRecord)));
  KS_HIP(hipHostMalloc(reinterpret_cast<void**>(&op->rec_h), 2 * sizeof(BsRecord)));
  KS_HIP(hipEventCreateWithFlags(&op->ev, hipEventDisableTiming));
  return op.release();
}

}  // namespace
