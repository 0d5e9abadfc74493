"""Shared by tests/test_tridiag_pencil_cpu.py and tests/test_gpu_tridiag_pencil.py: the seeded tridiagonal PENCILS (K, M) of the
fused operator y = (K - sigma M)^-1 M x (`ks_operator_tridiag_pencil`, csrc/ks_tridiag.hpp), built on the stiffness families of
tests/tridiag_cases.py with two mass matrices:

  fem    the consistent mass of linear elements: mdl = mdu = 1/6, md = 4/6
  rand   standard normal on all three diagonals, default_rng(2000 + n + (7 if cplx else 0)), complex when cplx

Families (K, M, dtype, sigma): (a, fem, f64, 1.0), (a, fem, f64, 0.0), (b, fem, c128, 1.7+0.1i), (d, rand, f64, 0.25),
(d, rand, c128, 0.25+0.5i).  The Float64 twin of family b is left out on purpose: with the fem mass at n = 70 000 the host
planner's own solve reaches eta = 9.6e-15, 68 % of the bound.

The backward error is that of the system the operator solves, (K - sigma M) y = M b, in the norm of tridiag_cases.eta.
"""
import numpy as np

from tridiag_cases import ETA_BOUND, default_levels, eta, family, matvec, rhs  # noqa: F401  (re-exported)

# (K family, mass, complex, sigma)
FAMILIES = [("a", "fem", False, 1.0), ("a", "fem", False, 0.0), ("b", "fem", True, 1.7 + 0.1j), ("d", "rand", False, 0.25),
            ("d", "rand", True, 0.25 + 0.5j)]
IDS = [f"{k}-{m}-{'c128' if c else 'f64'}-{s}" for k, m, c, s in FAMILIES]
SIZES = [(n, 4) for n in (1, 2, 5, 6, 11, 25, 26, 341, 400, 700)] + [(n, 0) for n in (64, 65, 66, 131, 4226, 8449, 70000)]


def mass(name, n, cplx=False):
    """-> (mdl, md, mdu)"""
    m = max(n - 1, 0)
    if name == "fem":
        return np.full(m, 1.0 / 6.0), np.full(n, 4.0 / 6.0), np.full(m, 1.0 / 6.0)
    if name == "identity":
        dt = complex if cplx else float
        return np.zeros(m, dtype=dt), np.ones(n, dtype=dt), np.zeros(m, dtype=dt)
    assert name == "rand"
    rng = np.random.default_rng(2000 + n + (7 if cplx else 0))

    def normal(k):
        x = rng.standard_normal(k)
        return (x + 1j * rng.standard_normal(k)) if cplx else x

    mdl, mdu, md = normal(m), normal(m), normal(n)
    return mdl, md, mdu


def pencil(kname, mname, n, cplx, sigma):
    """-> (K, M, sigma): K and M as (dl, d, du) triples; K is the family of tridiag_cases WITHOUT its shift applied."""
    kdl, kd, kdu, _ = family(kname, n, cplx, sigma if kname == "a" else None)
    return (kdl, kd, kdu), mass(mname, n, cplx), sigma


def shifted(K, M, sigma):
    """T = K - sigma M as a (dl, d, du) triple"""
    return tuple(np.asarray(k) - sigma * np.asarray(m) for k, m in zip(K, M))


def pencil_eta(K, M, sigma, y, b):
    """normwise backward error of (K - sigma M) y = M b"""
    return eta(*shifted(K, M, sigma), 0.0, y, matvec(*M, 0.0, np.asarray(b, dtype=np.result_type(y, b))))
