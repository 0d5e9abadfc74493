"""The MINRES recurrence of `ks_operator_minres` (csrc/ks_minres.hpp, csrc/ks_minres_plan.hpp) in numpy, step for step: Float64 and
ComplexF64, with a shift anywhere on the real axis.  Plain numpy: no device, no library.  The device differs from this model in the
order of its sums and in the fused multiply-adds of its updates; unlike conjugate gradients on a well-conditioned matrix that moves
the iteration count of an indefinite solve by several per cent (tests/test_minres_model_cpu.py records by how much).

    init:  y = 0, beta1 = ||b||, v = b / beta1, v_ = 0, w_ = w__ = 0, beta = 0, (c, s) = (c_, s_) = (1, 0), phibar = beta1
           beta1 == 0 -> done, 0 iterations, y = 0;  beta1 not finite -> fail
    k = 1, 2, ...:
      q = (A - shift) v;  alpha = Re v^H q;  r = q - beta v_ - alpha v;  beta' = ||r||
      eps = s_ beta;  dbar = c_ beta;  delta = c dbar + s alpha;  gbar = -s dbar + c alpha
      gamma = hypot(gbar, beta');  gamma == 0 or not finite -> fail ("singular")
      c' = gbar / gamma;  s' = beta' / gamma;  phi = c' phibar;  phibar <- -s' phibar
      w = (v - eps w__ - delta w_) / gamma;  y += phi w
      done if |phibar| <= tol beta1
      else v_ <- v, v <- r / beta', beta <- beta', (c_, s_) <- (c, s), (c, s) <- (c', s'), w__ <- w_, w_ <- w

|phibar| is the residual norm of the recurrence; it never increases (|s'| <= 1), which `solve` asserts."""
import numpy as np


class Singular(RuntimeError):
    pass


class NotFinite(RuntimeError):
    pass


class DidNotConverge(RuntimeError):
    pass


def minres_step(alpha, beta, beta_new, c, s, c_prev, s_prev, phibar, stop):
    """(eps, delta, gamma, c', s', phi, phibar', done, fail): mr_step of csrc/ks_minres_plan.hpp with numpy's hypot."""
    f = np.float64
    alpha, beta, beta_new, c, s, c_prev, s_prev, phibar = map(f, (alpha, beta, beta_new, c, s, c_prev, s_prev, phibar))
    with np.errstate(all="ignore"):
        eps = s_prev * beta
        dbar = c_prev * beta
        delta = c * dbar + s * alpha
        gbar = -s * dbar + c * alpha
        if not (np.isfinite(alpha) and np.isfinite(beta_new) and np.isfinite(gbar)):
            return 0.0, 0.0, float("nan"), 0.0, 0.0, 0.0, 0.0, False, True
        gamma = np.hypot(gbar, beta_new)
        if gamma == 0.0 or not np.isfinite(gamma):
            return 0.0, 0.0, float(gamma), 0.0, 0.0, 0.0, 0.0, False, True
        c_new, s_new = gbar / gamma, beta_new / gamma
        phi = c_new * phibar
        phibar_new = -(s_new * phibar)
    return float(eps), float(delta), float(gamma), float(c_new), float(s_new), float(phi), float(phibar_new), bool(abs(phibar_new) <= stop), False


def solve(A, b, shift=0.0, tol=1e-13, maxit=10000):
    """(y, iterations, relres) with relres[k] = |phibar_k| / beta1 after k iterations (relres[0] = 1).  `A`: anything with `A @ v`."""
    b = np.asarray(b)
    y = np.zeros_like(b)
    beta1 = float(np.sqrt(np.vdot(b, b).real))
    if not np.isfinite(beta1):
        raise NotFinite("the right-hand side is not finite")
    if beta1 == 0.0:
        return y, 0, [0.0]
    v = b / beta1
    vm = np.zeros_like(b)
    wm, wmm = np.zeros_like(b), np.zeros_like(b)
    beta, c, s, c_prev, s_prev, phibar = 0.0, 1.0, 0.0, 1.0, 0.0, beta1
    relres = [1.0]
    for k in range(1, maxit + 1):
        q = A @ v - shift * v if shift != 0.0 else A @ v
        alpha = float(np.vdot(v, q).real)
        r = q - beta * vm - alpha * v
        beta_new = float(np.sqrt(np.vdot(r, r).real))
        eps, delta, gamma, c_new, s_new, phi, phibar_new, done, fail = minres_step(alpha, beta, beta_new, c, s, c_prev, s_prev, phibar, tol * beta1)
        if fail:
            raise Singular("gamma = %g at iteration %d" % (gamma, k))
        assert abs(phibar_new) <= abs(phibar), (k, phibar, phibar_new)      # monotone: |s'| <= 1
        w = (v - eps * wmm - delta * wm) / gamma
        y = y + phi * w
        phibar = phibar_new
        relres.append(abs(phibar) / beta1)
        if done:
            return y, k, relres
        vm, v = v, r / beta_new
        beta = beta_new
        c_prev, s_prev, c, s = c, s, c_new, s_new
        wmm, wm = wm, w
    raise DidNotConverge("relative residual %g after %d iterations" % (relres[-1], maxit))
