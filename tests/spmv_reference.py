"""Plain numpy references of the stored-matrix product mul!(y, A, x) (src/expansion.jl:121) and of the Newton step
y = sigma (A x - theta x) the s-step expansion makes of it.  No device, no library.

seq_matvec: the BITS the layouts promise -- every product rounded on its own, the products of a row added to +0.0 in stored
order (csrc/ks_kernels.hpp: mul_nc, add_).  hp_shifted: the shifted product in extended precision together with the scale
and the row lengths of its forward-error bound."""
import numpy as np

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not an extended format here: no high-precision reference"

EPS = float(np.finfo(np.float64).eps)


def _by_position(A):
    """Yields (rows, entry positions) for k = 0, 1, ...: the rows that have a k-th stored entry, and where it is stored."""
    ptr = A.indptr.astype(np.int64)
    length = np.diff(ptr)
    rows = np.argsort(-length, kind="stable")       # longest rows first: the rows still running are a prefix
    sorted_len = length[rows]
    k = 0
    while True:
        live = int(np.searchsorted(-sorted_len, -k, side="left"))   # rows with length > k
        if live == 0:
            return
        r = rows[:live]
        yield r, ptr[r] + k
        k += 1


def seq_matvec(A, x):
    """y = A x for a scipy CSR matrix with the library's rounding: per row s = +0.0, then s = fl(s + fl(a_k x_k)) in stored order.
    Complex: a product is (fl(fl(ar br) - fl(ai bi)), fl(fl(ar bi) + fl(ai br))), the sum componentwise.  Every multiply and add
    is a numpy call of its own on real arrays, so nothing can be contracted."""
    n = A.shape[0]
    idx, val = A.indices, A.data
    cplx = np.iscomplexobj(val) or np.iscomplexobj(x)
    if not cplx:
        a, xv = np.ascontiguousarray(val, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64)
        s = np.zeros(n, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for r, p in _by_position(A):
                prod = np.multiply(a[p], xv[idx[p]])
                s[r] = np.add(s[r], prod)
        return s
    val = np.asarray(val, dtype=np.complex128)
    x = np.asarray(x, dtype=np.complex128)
    ar, ai = np.ascontiguousarray(val.real), np.ascontiguousarray(val.imag)
    xr, xi = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    sr, si = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, p in _by_position(A):
            c = idx[p]
            p1, p2 = np.multiply(ar[p], xr[c]), np.multiply(ai[p], xi[c])
            p3, p4 = np.multiply(ar[p], xi[c]), np.multiply(ai[p], xr[c])
            sr[r] = np.add(sr[r], np.subtract(p1, p2))
            si[r] = np.add(si[r], np.add(p3, p4))
    out = np.empty(n, dtype=np.complex128)
    out.real, out.imag = sr, si
    return out


def seq_matvec_loop(A, x):
    """seq_matvec as the naive double loop over Python scalars (small matrices: the check of the vectorised form)."""
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data) or np.iscomplexobj(x)
    out = np.zeros(n, dtype=np.complex128 if cplx else np.float64)
    for i in range(n):
        if cplx:
            sr, si = 0.0, 0.0
            for p in range(A.indptr[i], A.indptr[i + 1]):
                a, b = complex(A.data[p]), complex(x[A.indices[p]])
                p1, p2, p3, p4 = a.real * b.real, a.imag * b.imag, a.real * b.imag, a.imag * b.real
                sr, si = sr + (p1 - p2), si + (p3 + p4)
            out[i] = complex(sr, si)
        else:
            s = 0.0
            for p in range(A.indptr[i], A.indptr[i + 1]):
                s = s + float(A.data[p]) * float(x[A.indices[p]])   # (Python floats: two roundings, never fused)
            out[i] = s
    return out


def abs_matvec(A, x):
    """(sum_j |a_ij| |x_j|, row lengths) in extended precision."""
    hp = np.longdouble
    n = A.shape[0]
    aa, ax = np.abs(A.data).astype(hp), np.abs(x).astype(hp)
    w = np.zeros(n, dtype=hp)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, p in _by_position(A):
            w[r] += aa[p] * ax[A.indices[p]]
    return w, np.diff(A.indptr).astype(np.int64)


def hp_shifted(A, x, theta, sigma):
    """(y, w, L): y = sigma (A x - theta x) in np.longdouble / np.clongdouble, the componentwise scale
    w_i = |sigma| (sum_j |a_ij| |x_j| + |theta| |x_i|) of its forward error, and the row lengths L_i.  The operation sequence
    `L products, L adds, theta x, the subtraction, the scaling` is off by at most (L_i + 3) eps w_i in Float64, fused
    multiply-adds or not."""
    cplx = np.iscomplexobj(A.data) or np.iscomplexobj(x) or np.iscomplexobj(theta)
    hp = np.clongdouble if cplx else np.longdouble
    n = A.shape[0]
    a, xv = A.data.astype(hp), np.asarray(x).astype(hp)
    s = np.zeros(n, dtype=hp)
    with np.errstate(invalid="ignore", over="ignore"):
        for r, p in _by_position(A):
            s[r] += a[p] * xv[A.indices[p]]
        th = hp(theta) if cplx else np.longdouble(np.real(theta))
        y = np.longdouble(sigma) * (s - th * xv)
        w, L = abs_matvec(A, x)
        w = np.abs(np.longdouble(sigma)) * (w + np.abs(th) * np.abs(xv))
    return y, w, L
