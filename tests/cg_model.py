"""The conjugate-gradient recurrence of `ks_operator_cg` (csrc/ks_cg.hpp, csrc/ks_cg_plan.hpp) in numpy, step for step: Float64 and
ComplexF64, with a shift.  Plain numpy: no device, no library.  The device differs from this model only in the order of its sums
(and in the fused multiply-adds of its updates), so its iteration count lies within one of the model's.

    init:  y = 0, r = p = b, rho = rho0 = ||b||^2;  rho0 == 0 -> done, 0 iterations, y = 0
    k = 1, 2, ...:
      q = (A - shift) p;  pq = Re p^H q;  alpha = rho / pq;  r -= alpha q;  rho' = ||r||^2;  y += alpha p
      done if rho' <= tol^2 rho0, else beta = rho' / rho, p = r + beta p, rho = rho'
      fail when pq is not finite or pq <= 0."""
import numpy as np


class NotPositiveDefinite(RuntimeError):
    pass


class DidNotConverge(RuntimeError):
    pass


def cg_step(rho, pq, rho_new, stop):
    """(alpha, beta, done, fail): cg_step of csrc/ks_cg_plan.hpp."""
    if not np.isfinite(pq) or not pq > 0.0:
        return 0.0, 0.0, False, True
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.float64(rho) / np.float64(pq)
    if not np.isfinite(alpha) or not np.isfinite(rho_new):
        return 0.0, 0.0, False, True
    if rho_new <= stop:
        return float(alpha), 0.0, True, False
    with np.errstate(over="ignore", divide="ignore"):
        beta = np.float64(rho_new) / np.float64(rho)
    return float(alpha), float(beta), False, False


def solve(A, b, shift=0.0, tol=1e-13, maxit=1000):
    """(y, iterations, relres) with relres[k] = sqrt(rho_k / rho0) after k iterations (relres[0] = 1).  `A`: anything with `A @ p`."""
    b = np.asarray(b)
    y = np.zeros_like(b)
    r, p = b.copy(), b.copy()
    rho0 = rho = float(np.vdot(b, b).real)
    if rho0 == 0.0:
        return y, 0, [0.0]
    relres = [1.0]
    for k in range(1, maxit + 1):
        q = A @ p - shift * p if shift != 0.0 else A @ p
        pq = float(np.vdot(p, q).real)
        alpha, _, _, fail = cg_step(rho, pq, 0.0, 0.0)
        if fail:
            raise NotPositiveDefinite("p^H (A - theta) p = %g at iteration %d" % (pq, k))
        r = r - alpha * q
        rho_new = float(np.vdot(r, r).real)
        alpha, beta, done, fail = cg_step(rho, pq, rho_new, tol * tol * rho0)
        if fail:
            raise NotPositiveDefinite("the residual is not finite at iteration %d" % k)
        y = y + alpha * p
        relres.append(float(np.sqrt(rho_new / rho0)))
        if done:
            return y, k, relres
        p = r + beta * p
        rho = rho_new
    raise DidNotConverge("relative residual %g after %d iterations" % (relres[-1], maxit))
