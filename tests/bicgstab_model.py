"""The BiCGStab(2) recurrence of `ks_operator_bicgstab` (csrc/ks_bicgstab.hpp, csrc/ks_bicgstab_plan.hpp) in numpy, step for step:
Float64 with a real shift, ComplexF64 with a complex one.  Plain numpy: no device, no library.  The device differs from this model
in the order of its sums and in the fused multiply-adds of its updates (tests/test_bicgstab_model_cpu.py records what summation
order alone does to the iteration count).  <a, c> = a^H c; rt = b is the shadow residual, read only.

    init:  y = 0, r0 = b, u0 = 0, rho0 = 1, alpha = 0, omega = 1, beta1 = ||b||     beta1 == 0 -> done, 0 iterations; not finite -> fail
    k = 1, 2, ... (one iteration = 4 products):
      rho0 <- -omega rho0
      step 1:  rho1 = <rt, r0>; beta = alpha rho1 / rho0; rho0 <- rho1; u0 <- r0 - beta u0
               u1 = (A - theta) u0; gamma = <rt, u1>; alpha = rho0 / gamma; r0 <- r0 - alpha u1; y <- y + alpha u0
               stage 1: ||r0|| <= tol beta1 -> done
               r1 = (A - theta) r0
      step 2:  rho1 = <rt, r1>; beta = alpha rho1 / rho0; rho0 <- rho1; u0 <- r0 - beta u0; u1 <- r1 - beta u1
               u2 = (A - theta) u1; gamma = <rt, u2>; alpha = rho0 / gamma; r0 <- r0 - alpha u1; r1 <- r1 - alpha u2; y <- y + alpha u0
               stage 2: ||r0|| <= tol beta1 -> done
               r2 = (A - theta) r1
      MR:      G = [<r1,r1> <r1,r2>; <r2,r1> <r2,r2>], h = [<r1,r0>; <r2,r0>], G g = h (Cramer's rule)
               y <- y + g1 r0 + g2 r1; r0 <- r0 - g1 r1 - g2 r2; u0 <- u0 - g1 u1 - g2 u2; omega = g2
               stage 3: ||r0|| <= tol beta1 -> done

Breakdown: rho0 (the divisor of beta), gamma or det G zero or not finite, or a quotient that is not finite, while the residual
test has not passed.  `late_stage_tests=True` evaluates a stage's test only after the scalars of the following stage exist (as a
device kernel that derives "already finished" from partial sums does): the record must not depend on it."""
import numpy as np


class Breakdown(RuntimeError):
    pass


class NotFinite(RuntimeError):
    pass


class DidNotConverge(RuntimeError):
    pass


def _finite(z):
    return bool(np.isfinite(np.real(z)) and np.isfinite(np.imag(z)))


def _np(*z):
    """numpy scalars (no Python exception on a zero divisor or an overflow): complex128 if any argument is complex"""
    t = np.complex128 if any(isinstance(v, (complex, np.complexfloating)) for v in z) else np.float64
    return [t(v) for v in z]


def bicg_coef(rho0, rho1, alpha, gamma):
    """(beta, alpha', fail): bs_coef of csrc/ks_bicgstab_plan.hpp.  fail 1: rho0 zero or not finite, or beta not finite;
    fail 2: gamma zero or not finite, or alpha' not finite.  A failed step returns zeros."""
    rho0, rho1, alpha, gamma = _np(rho0, rho1, alpha, gamma)
    with np.errstate(all="ignore"):
        if rho0 == 0 or not _finite(rho0):
            return 0.0, 0.0, 1
        beta = alpha * rho1 / rho0
        if not _finite(beta):
            return 0.0, 0.0, 1
        if gamma == 0 or not _finite(gamma):
            return beta, 0.0, 2
        a = rho1 / gamma
        if not _finite(a):
            return beta, 0.0, 2
    return beta, a, 0


def mr_solve(g11, g22, g12, h1, h2):
    """(g1, g2, det, fail): the Hermitian 2 x 2 system [g11 g12; conj(g12) g22] g = h by Cramer's rule (bs_mr of the plan header)."""
    g12, h1, h2 = _np(g12, h1, h2)
    g11, g22 = np.float64(g11), np.float64(g22)
    with np.errstate(all="ignore"):
        det = g11 * g22 - (g12.real * g12.real + g12.imag * g12.imag)
        if det == 0 or not np.isfinite(det):
            return 0.0, 0.0, float(det), 1
        g1 = (g22 * h1 - g12 * h2) / det
        g2 = (g11 * h2 - np.conj(g12) * h1) / det
        if not (_finite(g1) and _finite(g2)):
            return 0.0, 0.0, float(det), 1
    return g1, g2, float(det), 0


def solve(A, b, shift=0.0, tol=1e-13, maxit=10000, late_stage_tests=False):
    """(y, iterations, stage, relres): `stage` 1, 2 or 3 is where the last iteration ended (0: b = 0), relres[k] = ||r0|| / beta1 of
    the recurrence after iteration k (at the stage it ended).  `A`: anything with `A @ v`."""
    b = np.asarray(b)
    cplx = b.dtype.kind == "c"
    sc = (lambda z: complex(z)) if cplx else (lambda z: float(np.real(z)))
    dot = lambda a, c: sc(np.vdot(a, c))
    nrm = lambda v: float(np.sqrt(np.vdot(v, v).real))
    mul = (lambda v: A @ v - shift * v) if shift != 0 else (lambda v: A @ v)
    y = np.zeros_like(b)
    beta1 = nrm(b)
    if not np.isfinite(beta1):
        raise NotFinite("the right-hand side is not finite")
    if beta1 == 0.0:
        return y, 0, 0, [0.0]
    stop = tol * beta1
    rt = b
    r0 = b.copy()
    u0 = np.zeros_like(b)
    u1 = r1 = None
    rho0, alpha, omega = sc(1.0), sc(0.0), sc(1.0)
    relres = [1.0]
    rho1 = dot(rt, r0)
    for k in range(1, maxit + 1):
        rho0 = -omega * rho0
        # ---- BiCG step 1
        beta, _, fail = bicg_coef(rho0, rho1, alpha, sc(1.0))
        if fail:
            raise Breakdown("rho = %s at iteration %d" % (rho0, k))
        beta = sc(beta)
        rho0 = rho1
        u0 = r0 - beta * u0 if k > 1 else r0.copy()
        u1 = mul(u0)
        gamma = dot(rt, u1)
        _, alpha, fail = bicg_coef(sc(1.0), rho0, sc(0.0), gamma)
        if fail:
            raise Breakdown("gamma = %s at iteration %d" % (gamma, k))
        alpha = sc(alpha)
        r0 = r0 - alpha * u1
        y = y + alpha * u0
        n1 = nrm(r0)
        if not late_stage_tests and n1 <= stop:
            relres.append(n1 / beta1)
            return y, k, 1, relres
        r1 = mul(r0)
        # ---- BiCG step 2
        rho1 = dot(rt, r1)
        if late_stage_tests and n1 <= stop:
            relres.append(n1 / beta1)
            return y, k, 1, relres
        beta, _, fail = bicg_coef(rho0, rho1, alpha, sc(1.0))
        if fail:
            raise Breakdown("rho = %s at iteration %d" % (rho0, k))
        beta = sc(beta)
        rho0 = rho1
        u0 = r0 - beta * u0
        u1 = r1 - beta * u1
        u2 = mul(u1)
        gamma = dot(rt, u2)
        _, alpha, fail = bicg_coef(sc(1.0), rho0, sc(0.0), gamma)
        if fail:
            raise Breakdown("gamma = %s at iteration %d" % (gamma, k))
        alpha = sc(alpha)
        r0 = r0 - alpha * u1
        r1 = r1 - alpha * u2
        y = y + alpha * u0
        n2 = nrm(r0)
        if not late_stage_tests and n2 <= stop:
            relres.append(n2 / beta1)
            return y, k, 2, relres
        r2 = mul(r1)
        # ---- the two-dimensional minimal-residual step
        g11, g22 = float(np.vdot(r1, r1).real), float(np.vdot(r2, r2).real)
        g12, h1, h2 = dot(r1, r2), dot(r1, r0), dot(r2, r0)
        if late_stage_tests and n2 <= stop:
            relres.append(n2 / beta1)
            return y, k, 2, relres
        g1, g2, det, fail = mr_solve(g11, g22, g12, h1, h2)
        if fail:
            raise Breakdown("det G = %g at iteration %d" % (det, k))
        g1, g2 = sc(g1), sc(g2)
        y = y + g1 * r0 + g2 * r1
        r0 = r0 - g1 * r1 - g2 * r2
        u0 = u0 - g1 * u1 - g2 * u2
        omega = g2
        rho1 = dot(rt, r0)
        n3 = nrm(r0)
        relres.append(n3 / beta1)
        if n3 <= stop:
            return y, k, 3, relres
    raise DidNotConverge("relative residual %g after %d iterations" % (relres[-1], maxit))
