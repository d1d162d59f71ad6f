"""NumPy restatement of the contract of symgpu_matvec_apply (include/symgpu.h f7), term by term in the stated order, O(T 2^n):
    y[b] = sum over the groups g of equal X-part, in ascending x_g, of  D_g(b) v[b ^ x_g]
    D_g(b) = sum over the terms k of g, in operator order, of  c_k (-i)^{Y_k} (-1)^{|b & z_k|}
every sum started from its first addend, every complex product the plain four-multiplication one.  Test infrastructure only."""
import numpy as np

from _sparse_oracle import bits_to_int, times_minus_i_pow, _parity


def _complex(re, im):
    """re + i im without arithmetic (signed zeros survive)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def terms_of(symp_matrix, coeff_vec):
    """(x int64[T], z int64[T], (Re c', Im c') float64[T] each) of an operator as given (not cleaned)."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    x, z = bits_to_int(symp[:, :n]), bits_to_int(symp[:, n:])
    y = np.sum(symp[:, :n] & symp[:, n:], axis=1)
    return x, z, times_minus_i_pow(np.asarray(coeff_vec, dtype=np.complex128), y)


def groups_of(x):
    """[(x_g, term indices in operator order)] in ascending x_g."""
    order = np.argsort(x, kind='stable')
    xs = x[order]
    cuts = np.flatnonzero(np.diff(xs)) + 1
    return [(int(x[idx[0]]), idx) for idx in np.split(order, cuts)] if len(x) else []


def group_sum(z, c, idx, b):
    """D_g(b) for all rows b: the terms idx added in order from the first one, real and imaginary parts apart."""
    re = im = None
    for k in idx:
        sign = np.where(_parity(b & z[k]), -1.0, 1.0)
        tr, ti = sign * c[0][k], sign * c[1][k]
        re, im = (tr, ti) if re is None else (re + tr, im + ti)
    return re, im


def matvec(symp_matrix, coeff_vec, v):
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    assert v.shape[0] == 1 << n
    x, z, c = terms_of(symp, coeff_vec)
    b = np.arange(1 << n, dtype=np.int64)
    acc_re = acc_im = None
    for xg, idx in groups_of(x):
        dr, di = group_sum(z, c, idx, b)
        w = v[b ^ xg]
        pr, pi = dr * w.real - di * w.imag, dr * w.imag + di * w.real
        acc_re, acc_im = (pr, pi) if acc_re is None else (acc_re + pr, acc_im + pi)
    if acc_re is None:
        return np.zeros(1 << n, dtype=np.complex128)
    return _complex(acc_re, acc_im)


def diagonal(symp_matrix, coeff_vec):
    """D_0(b) of an operator without X-parts (a number operator), complex128[2^n]."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    assert not symp[:, :n].any()
    x, z, c = terms_of(symp, coeff_vec)
    re, im = group_sum(z, c, np.arange(len(x)), np.arange(1 << n, dtype=np.int64))
    return _complex(re, im)


def error_bound(symp_matrix, coeff_vec, v):
    """The a-priori bound of |y - y_oracle|_inf for Gaussian inputs: 8 (T + G + 3) 2^-53 sum|c| max|v| — T + G additions and one complex
    product per group, two roundings each, on either side."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    T = symp.shape[0]
    G = len(np.unique(bits_to_int(symp[:, :n]))) if T else 0
    return 8 * (T + G + 3) * 2.0 ** -53 * np.abs(np.asarray(coeff_vec)).sum() * np.abs(np.asarray(v)).max()
