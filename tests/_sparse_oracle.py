"""NumPy restatement of ``PauliwordOp.to_sparse_matrix``'s contract (test helper; no scipy, no GPU).

Entry (b, b ^ x_k) of the ``2^n x 2^n`` matrix is the sum, over the terms k in operator order, of ``c_k (-i)^{Y_k} (-1)^{|b & z_k|}``,
with x_k, z_k the term's X and Z bits read with qubit 0 as the most significant bit and Y_k = |x_k & z_k|.  The phase is applied as an
exact component swap, each entry starts from its first term and adds the others one by one.  The result is canonical CSR: columns
ascending within a row, no duplicates, no entry whose two components are both +-0 (NaN and inf are kept).
"""
import numpy as np


def bits_to_int(block):
    """bool[T, n] -> int64[T], column 0 the most significant bit."""
    block = np.asarray(block, dtype=np.int64)
    n = block.shape[1]
    return block @ (np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64)) if n else np.zeros(block.shape[0], np.int64)


def times_minus_i_pow(c, y):
    """c (-i)^y componentwise, exactly: (re, im) -> (im, -re) per factor."""
    re, im = c.real.copy(), c.imag.copy()
    out_re, out_im = re.copy(), im.copy()
    k = np.asarray(y) % 4
    out_re[k == 1], out_im[k == 1] = im[k == 1], -re[k == 1]
    out_re[k == 2], out_im[k == 2] = -re[k == 2], -im[k == 2]
    out_re[k == 3], out_im[k == 3] = -im[k == 3], re[k == 3]
    return out_re, out_im


_PARITY16 = np.array([bin(i).count('1') & 1 for i in range(1 << 16)], dtype=bool)


def _parity(v):
    """Parity of the set bits of non-negative int64 values below 2^32."""
    return _PARITY16[v & 0xFFFF] ^ _PARITY16[(v >> 16) & 0xFFFF]


def to_csr(symp_matrix, coeff_vec):
    """(data complex128, indices int64, indptr int64) of the operator's matrix."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    side = 1 << n
    x = bits_to_int(symp[:, :n])
    z = bits_to_int(symp[:, n:])
    y = np.sum(symp[:, :n] & symp[:, n:], axis=1)
    cre, cim = times_minus_i_pow(np.asarray(coeff_vec, dtype=np.complex128), y)
    xs = np.unique(x)
    D = len(xs)
    b = np.arange(side, dtype=np.int64)
    val_re = np.zeros((side, D))
    val_im = np.zeros((side, D))
    started = np.zeros(D, dtype=bool)
    gid = np.searchsorted(xs, x)
    for k in range(len(x)):                                   # operator order
        neg = _parity(b & z[k])
        vr = np.where(neg, -cre[k], cre[k])
        vi = np.where(neg, -cim[k], cim[k])
        d = gid[k]
        first = not started[d]
        val_re[:, d] = vr if first else val_re[:, d] + vr
        val_im[:, d] = vi if first else val_im[:, d] + vi
        started[d] = True
    cols = b[:, None] ^ xs[None, :]                           # [row, group]
    order = np.argsort(cols, axis=1, kind='stable')
    cols = np.take_along_axis(cols, order, axis=1)
    val_re = np.take_along_axis(val_re, order, axis=1)
    val_im = np.take_along_axis(val_im, order, axis=1)
    keep = ~((val_re == 0) & (val_im == 0))
    data = np.empty(int(keep.sum()), dtype=np.complex128)
    data.real = val_re[keep]
    data.imag = val_im[keep]
    indices = cols[keep].astype(np.int64)
    indptr = np.zeros(side + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return data, indices, indptr


def to_dense(symp_matrix, coeff_vec):
    data, indices, indptr = to_csr(symp_matrix, coeff_vec)
    side = len(indptr) - 1
    out = np.zeros((side, side), dtype=np.complex128)
    rows = np.repeat(np.arange(side), np.diff(indptr))
    out[rows, indices] = data
    return out


_PAULI = {
    (0, 0): np.eye(2, dtype=np.complex128),
    (1, 0): np.array([[0, 1], [1, 0]], dtype=np.complex128),
    (1, 1): np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    (0, 1): np.array([[1, 0], [0, -1]], dtype=np.complex128),
}


def kron_dense(symp_matrix, coeff_vec):
    """The definition itself: sum_k c_k P_0 x P_1 x ... x P_{n-1} with Y = [[0, -i], [i, 0]]."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    out = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for row, c in zip(symp, np.asarray(coeff_vec, dtype=np.complex128)):
        m = np.ones((1, 1), dtype=np.complex128)
        for q in range(n):
            m = np.kron(m, _PAULI[(int(row[q]), int(row[n + q]))])
        out += c * m
    return out
