"""Guards the REFERENCE of tests/test_gpu_headline_forms.py (tests/headline_forms_cases.py): for every case the device tests use,
h = V^H w, w' = w - V h, c = V^H w' and w'' = w' - V c come out bit-identical under different chunkings and orders of the sums
(so a kernel's grid, trip count and staging depth cannot show in them), one entry of each inner product is confirmed in rational
arithmetic, the DGKS decision is far from its threshold, and the shapes reach the kernel forms they are there for.  No device."""
from fractions import Fraction

import numpy as np
import pytest

import headline_forms_cases as hc

# (shape, columns) of every device case: the fused step on both shapes, the eager sequence on the small one
CASES = ([(hc.SMALL, j) for j in hc.J_FUSED] + [(hc.LARGE, j) for j in hc.J_FUSED_LARGE] + [(hc.SMALL, j) for j in hc.J_EAGER])
ORDERS = [dict(row_chunk=1000, col_chunk=7, reverse=False), dict(row_chunk=4099, col_chunk=3, reverse=True),
          dict(row_chunk=64, col_chunk=40, reverse=True)]


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("which", hc.VECTORS)
@pytest.mark.parametrize("shape,j", CASES)
def test_projections_do_not_depend_on_summation_order(shape, j, which, dtype):
    V = hc.basis_for(shape, j, dtype)[:, :j]
    w = hc.start_vector(shape, j, dtype, which)
    ref = hc.projections(V, w)
    for order in ORDERS[: 2 if shape == hc.LARGE else 3]:
        got = hc.projections(V, w, **order)
        for name, a, b in zip(("h", "w'", "c", "w''"), ref, got):
            assert np.array_equal(a, b), (name, order)
    # the correction is there to be found: V^H V != I from three columns on
    if j >= 3:
        assert np.count_nonzero(ref[2]) >= (2 * (j // 3) if which == "a" else 1), np.count_nonzero(ref[2])
    st = hc.step(shape, j, dtype, which)
    ratio = st.wnorm1 / st.rnorm
    # far from eta = 0.707 on either side: no rounding of the norms can flip the decision
    assert (ratio > 0.9 and not st.reorth) if which == "a" else (ratio < 0.5 and st.reorth), ratio
    # no breakdown (src/expansion.jl:99), again far from the threshold
    assert st.ok and (not st.reorth or st.beta > 0.9 * st.wnorm1), st.beta / st.wnorm1


@pytest.mark.parametrize("dtype", hc.DTYPES)
@pytest.mark.parametrize("which", hc.VECTORS)
@pytest.mark.parametrize("shape,j", [(hc.SMALL, 64), (hc.SMALL, 41), (hc.LARGE, 64)])
def test_inner_products_equal_rational_arithmetic(shape, j, which, dtype):
    V = hc.basis_for(shape, j, dtype)[:, :j]
    w = hc.start_vector(shape, j, dtype, which)
    h, w1, c, _ = hc.projections(V, w)
    col = max(c for c in range(j) if c % 3 == 2)      # a column with the 1/4 admixture
    for vec, got in ((w, h), (w1, c)):
        re, im = hc.exact_dot(V, vec, col)
        assert Fraction(float(np.real(got[col]))) == re and Fraction(float(np.imag(got[col]))) == im


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_gemv_references_do_not_depend_on_summation_order(dtype):
    for j in hc.J_GEMV:
        V = hc.basis(hc.SMALL, hc.MAXDIM_EAGER, dtype)[:, :j]
        w, g, h, wg = hc.gemv_case(j, dtype)
        for rc, cc, rev in ((1000, 7, False), (64, 40, True)):
            assert np.array_equal(h, hc._cdot(V, w, rc, rev)) and np.array_equal(wg, w - hc._vh(V, g, cc, rev)), j


def test_basis_is_what_the_docstring_says():
    for dtype in hc.DTYPES:
        V = hc.basis(hc.SMALL, 64, dtype)
        n0, tail = hc.SMALL
        assert V.shape == (n0 + tail, 64) and not V[n0:].any()
        G = V.conj().T @ V
        off = G - np.diag(np.diag(G))
        assert np.count_nonzero(off) == 2 * len(range(2, 64, 3))      # one neighbour pair per third column
        assert np.allclose(np.diag(G)[[0, 1, 3]], 1.0) and np.isclose(G[2, 2].real, 1.0 + 1.0 / 16)
        if hc.is_complex(dtype):
            assert not np.imag(V[:, 0::2]).any() and not np.real(V[:, 1::2]).any()


@pytest.mark.parametrize("dtype", hc.DTYPES)
def test_shapes_reach_the_forms_they_are_there_for(dtype):
    """The coverage condition of the device tests, from n, the cap and U alone."""
    for U, WB in hc.FUSED_UWB:
        assert hc.ring_wrap_covered(hc.nrows(hc.LARGE), dtype, 3, U, WB), (U, WB)
        # (ComplexF64 columns are padded to whole 64-pack units: 16512 packs are exactly 129 tiles of 128 -- the small shape has
        # no partial last tile at U = 2 there, the large one has)
        if not (hc.is_complex(dtype) and U == 2):
            assert hc.ring_wrap_covered(hc.nrows(hc.SMALL), dtype, 1, U, WB), (U, WB)
    tiles = {U: hc.fused_tiles(hc.nrows(hc.SMALL), dtype, 1, U)[0][0] for U in (4, 2)}
    assert tiles == ({4: 65, 2: 129} if hc.is_complex(dtype) else {4: 33, 2: 65})
    # k_axpy<D, 8>: main loop of 8 x 256 packs plus the one-pack remainder loop
    ppb = hc.axpy_packs_per_workgroup(hc.nrows(hc.SMALL), dtype, 1)
    assert ppb >= 3072 and ppb % (8 * hc.KBLOCK) != 0
    # rotations: at least three trips of every kernel's row loop, the last one partial
    for kind, (trips, partial) in hc.rot_trips(hc.ROT_ROWS[np.dtype(dtype)], dtype).items():
        assert trips >= 3 and partial, kind


def test_integer_rotation_reference_is_exact():
    rng = np.random.default_rng(3)
    for dtype in hc.DTYPES:
        V, Q = hc.small_ints(rng, dtype, 50, 100), hc.small_ints(rng, dtype, 100, 17)
        want = hc.int_product(V, Q)
        assert np.array_equal(want, V @ Q) and np.abs(want).max() < 2 ** 20
