"""The preconditioned conjugate-gradient recurrence of `ks_operator_pcg` (csrc/ks_pcg.hpp, csrc/ks_pcg_plan.hpp) in numpy, step for
step: Float64 and ComplexF64, with a shift.  Plain numpy: no device, no library.  The device differs from this model only in the
order of its sums (and in the fused multiply-adds of its updates).

    init:  y = 0, r = b, rho0 = ||b||^2;  rho0 == 0 -> done, 0 iterations, y = 0;  z = M r;  tau = Re r^H z;  p = z
    k = 1, 2, ...:
      q = (A - shift) p;  pq = Re p^H q;  alpha = tau / pq;  r -= alpha q;  rho' = ||r||^2;  y += alpha p
      done if rho' <= tol^2 rho0, else z = M r, tau' = Re r^H z, beta = tau' / tau, p = z + beta p, tau = tau'
      fail when pq, tau or tau' is not finite or <= 0, or rho' is not finite.

`M`: a callable r -> z, or anything with `M @ r`.  `order`: a permutation of the rows in which every inner product is summed (None:
numpy's own order) -- what tests/pcg_cases.py measures the spread of the iteration count with."""
import numpy as np

FAIL_CURVATURE, FAIL_PRECONDITIONER, FAIL_RESIDUAL = 2, 3, 4


class NotPositiveDefinite(RuntimeError):
    pass


class PreconditionerNotPositiveDefinite(RuntimeError):
    pass


class DidNotConverge(RuntimeError):
    pass


def pcg_step(tau, pq, rho_new, stop, tau_new):
    """(alpha, beta, done, fail): pcg_step and pcg_beta of csrc/ks_pcg_plan.hpp as ks_host_pcg_step combines them."""
    if not np.isfinite(pq) or not pq > 0.0:
        return 0.0, 0.0, False, FAIL_CURVATURE
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.float64(tau) / np.float64(pq)
    if not np.isfinite(alpha):
        return 0.0, 0.0, False, FAIL_CURVATURE
    if not np.isfinite(rho_new):
        return 0.0, 0.0, False, FAIL_RESIDUAL
    if rho_new <= stop:
        return float(alpha), 0.0, True, 0
    if not np.isfinite(tau_new) or not tau_new > 0.0:
        return float(alpha), 0.0, False, FAIL_PRECONDITIONER
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        beta = np.float64(tau_new) / np.float64(tau)
    if not np.isfinite(beta):
        return float(alpha), 0.0, False, FAIL_PRECONDITIONER
    return float(alpha), float(beta), False, 0


def _dot(a, b, order):
    if order is None:
        return float(np.vdot(a, b).real)
    return float(np.sum((np.conj(a) * b).real[order]))


def solve(A, M, b, shift=0.0, tol=1e-13, maxit=1000, order=None):
    """(y, iterations, relres) with relres[k] = sqrt(rho_k / rho0) after k iterations (relres[0] = 1)."""
    apply_m = M if callable(M) else (lambda r: M @ r)
    b = np.asarray(b)
    y = np.zeros_like(b)
    r = b.copy()
    rho0 = _dot(b, b, order)
    if rho0 == 0.0:
        return y, 0, [0.0]
    z = apply_m(r)
    tau = _dot(r, z, order)
    if not np.isfinite(tau) or not tau > 0.0:
        raise PreconditionerNotPositiveDefinite("r^H M r = %g at iteration 0" % tau)
    p = z.copy()
    relres = [1.0]
    for k in range(1, maxit + 1):
        q = A @ p - shift * p if shift != 0.0 else A @ p
        pq = _dot(p, q, order)
        alpha, _, _, fail = pcg_step(tau, pq, 0.0, 0.0, 1.0)
        if fail:
            raise NotPositiveDefinite("p^H (A - theta) p = %g at iteration %d" % (pq, k))
        r = r - alpha * q
        rho_new = _dot(r, r, order)
        z = apply_m(r)
        tau_new = _dot(r, z, order)
        alpha, beta, done, fail = pcg_step(tau, pq, rho_new, tol * tol * rho0, tau_new)
        if fail == FAIL_PRECONDITIONER:
            raise PreconditionerNotPositiveDefinite("r^H M r = %g at iteration %d" % (tau_new, k))
        if fail:
            raise NotPositiveDefinite("the residual is not finite at iteration %d" % k)
        y = y + alpha * p
        relres.append(float(np.sqrt(rho_new / rho0)))
        if done:
            return y, k, relres
        p = z + beta * p
        tau = tau_new
    raise DidNotConverge("relative residual %g after %d iterations" % (relres[-1], maxit))
