"""Cases and the independent reference assembly shared by tests/test_grid_var_periodic_cpu.py and tests/test_gpu_grid_var_periodic.py
(the matrix-free variable-coefficient grid operator with periodic axes, `ks_operator_grid_var_periodic`, csrc/ks_grid_var.hpp).
Shapes, taps, potential and vector are those of tests/grid_cases.py, the periodic cases and wrap values those of
tests/grid_periodic_cases.py, the coefficients those of tests/grid_var_cases.py.  Plain numpy / scipy: no device, no library."""
import numpy as np
import scipy.sparse as sp

import grid_cases as gc
import grid_periodic_cases as gp
import grid_var_cases as vc

# The edges of the tiles ComplexF64 takes (32 x 16 and 512 x 1, csrc/ks_grid_var.hpp) along their periodic axis; a single partial
# tile in y (the +y wrap neighbour is the LDS slot of an owned point); a partial wide tile with a z wrap across two z-ranges.
CASES_C64_TILE = ([((5, k, 2), gp.Y) for k in (15, 16, 17, 33)] + [((k, 1, 2), gp.X) for k in (511, 512, 513, 1025)]
                  + [((513,), (True,)), ((1025,), (True,))] + [((5, 15, 3), gp.ALL), ((511, 1, 9), (True, False, True))])
# gp.GROUPS: every axis at 3, t - 1, t, t + 1, 2 t + 1 of the Float64 tiles and of the 8-plane z-range, partial single tiles included
GROUPS = dict(gp.GROUPS, c64tile=CASES_C64_TILE)


def assemble(shape, per, t, c, w=None, v=None):
    """The definition of the operator, assembled independently of the library: vc.assemble extended with the wrap links.  Per
    direction an index mask for "interior", one for "wrapped" with the wrap image's index, and on REAL arrays hre * (c + c[s]),
    him * (c + c[s]) -- h = 0.5 tap for an interior link, 0.5 wrap value for a wrapped one (w = None: the taps); the diagonal is
    centre + potential, one numpy addition.  The rows are then sorted into ascending columns (extents >= 3 on periodic axes make
    the columns of a row distinct).  Returns CSR."""
    ndim = len(shape)
    n = gc.size(shape)
    ext = list(shape) + [1] * (3 - ndim)
    pr = list(per) + [False] * (3 - ndim)
    assert all(m >= 3 for m, p in zip(ext, pr) if p)
    cplx = any(a is not None and np.dtype(np.asarray(a).dtype).kind == "c" for a in (t, w, v))
    t7 = np.zeros(7, dtype=np.complex128)
    t7[3 - ndim : 4 + ndim] = t
    w7 = t7.copy()                     # the wrap value of slot k (slot 3 is never used)
    if w is not None:
        w6 = np.zeros(6, dtype=np.complex128)
        w6[3 - ndim : 3 + ndim] = w
        w7[:3], w7[4:] = w6[:3], w6[3:]
    idx = np.arange(n)
    stride = (1, ext[0], ext[0] * ext[1])
    pos = (idx % ext[0], (idx // ext[0]) % ext[1], idx // (ext[0] * ext[1]))
    rows, cols, vre, vim = [], [], [], []

    def put(mask, s, hre, him):
        r = idx[mask]
        m = c[r] + c[s]
        rows.append(r), cols.append(s), vre.append(hre * m), vim.append(him * m)

    for k, (ok, off) in enumerate(vc.links(shape)):
        if k == 3:
            d = np.full(n, t7[3]) if v is None else np.add(t7[3], np.asarray(v, dtype=np.complex128).ravel())
            rows.append(idx), cols.append(idx), vre.append(d.real.copy()), vim.append(d.imag.copy())
            continue
        a, sign = (2 - k, -1) if k < 3 else (k - 4, 1)
        put(ok, idx[ok] + off, 0.5 * t7[k].real, 0.5 * t7[k].imag)
        if pr[a]:
            edge = pos[a] == (0 if sign < 0 else ext[a] - 1)
            put(edge, idx[edge] - sign * (ext[a] - 1) * stride[a], 0.5 * w7[k].real, 0.5 * w7[k].imag)
    rows, cols, vre, vim = (np.concatenate(x) for x in (rows, cols, vre, vim))
    order = np.lexsort((cols, rows))
    rows, cols, vre, vim = rows[order], cols[order], vre[order], vim[order]
    assert np.all((np.diff(rows) > 0) | (np.diff(cols) > 0))      # distinct columns within a row
    data = vre
    if cplx:      # (the two parts are stored, not combined by arithmetic)
        data = np.empty(rows.size, dtype=np.complex128)
        data.real, data.imag = vre, vim
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return sp.csr_matrix((data, cols.astype(np.int32), indptr), shape=(n, n))


# ------------------------------------------------------------------------------------------------ the two whole-solve problems
SOLVE_SHAPE = (12, 10, 9)
SOLVE_THETA = (0.7, 1.1, 1.9)
# The strength of the harmonic potential gc.harmonic added to the diffusion operator on the torus.  With strength 1 (the open solve
# case of tests/test_gpu_grid_var.py) the lowest five eigenvalues of the real torus are 1.202, 1.933, 1.944, 1.981, 2.464 -- the
# second and third 0.011 apart, closer than the 0.03 that tests/test_grid_var_cpu.py asks of its solve case -- so the strength was
# changed to 0.25: real torus 0.552, 0.956, 1.040, 1.096, 1.192 (smallest gap 0.056), Bloch problem at SOLVE_THETA 0.601, 0.923,
# 0.997, 1.033, 1.293 (0.036).  tests/test_grid_var_periodic_cpu.py checks the criterion on the dense matrices.
SOLVE_POTENTIAL_STRENGTH = 0.25


def solve_potential():
    return SOLVE_POTENTIAL_STRENGTH * gc.harmonic(SOLVE_SHAPE)
