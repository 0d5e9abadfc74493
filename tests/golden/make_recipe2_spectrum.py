"""Records scipy.linalg.eigvals(A, B) of the two dense pencils of tests/test_gpu_operator_product.py (recipe 2 end to end: the 30 x 35
grid, A the 2-D Laplacian (+ i diag), B the consistent mass) under tests/golden/: the QZ iteration takes 5 s (Float64) and 17 s
(ComplexF64), too long for a test that runs with every suite.  The test checks the record against the matrices through the trace.
Run from the repo root:   python tests/golden/make_recipe2_spectrum.py
"""
import os
import sys

import numpy as np
import scipy.linalg as sla

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(OUT, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_operator_product as t  # noqa: E402

if __name__ == "__main__":
    for cplx, name in ((False, "f64"), (True, "c128")):
        _, A, B, _ = t._recipe2_problem(cplx)
        lam = sla.eigvals(A.toarray(), B.toarray())
        np.save(os.path.join(OUT, f"recipe2_pencil_eigvals_{name}.npy"), lam)
        print(name, lam.shape, lam.dtype)
