"""NumPy restatement of ``PauliwordOp.from_matrix``'s contract (test helper; no scipy, no GPU).

For a ``2^n x 2^n`` matrix M, with qubit 0 the most significant bit of a row / column index b and of a term's X and Z parts x, z:

    d_x[b]  = M[b, b ^ x]
    c(x, z) = i^{|x & z| mod 4} 2^-n WHT(d_x)[z],        WHT(d)[z] = sum_b (-1)^{|b & z|} d[b]

with the PINNED arithmetic of the contract: the radix-2 butterfly, stage s = 0 .. n-1 combining the two elements whose indices differ in
bit s (a' = a + b, b' = a - b, a the element whose bit is clear), per component in IEEE double; then one multiplication by 2^-n (exact)
and i^k as a component swap / negation (exact).  Every device form performs these additions in this order, so it agrees with this file
bit for bit on any input.  Coefficients whose two components are both +-0 are dropped (NaN and inf are kept); the rest are listed in
ascending (x, z) order, x the high part.
"""
import numpy as np


def wht_pinned(re, im):
    """The butterfly over the last axis (length 2^n) of two float64 arrays, in place; returns them."""
    size = re.shape[-1]
    n = size.bit_length() - 1
    assert size == 1 << n
    lead = re.shape[:-1]
    for s in range(n):
        for v in (re, im):
            w = v.reshape(lead + (size >> (s + 1), 2, 1 << s))
            a, b = w[..., 0, :].copy(), w[..., 1, :].copy()
            w[..., 0, :] = a + b
            w[..., 1, :] = a - b
    return re, im


_POPCOUNT16 = np.array([bin(i).count('1') for i in range(1 << 16)], dtype=np.int64)


def popcount(v):
    v = np.asarray(v, dtype=np.int64)
    return _POPCOUNT16[v & 0xFFFF] + _POPCOUNT16[(v >> 16) & 0xFFFF]


def times_i_pow(re, im, k):
    """(re + i im) i^k componentwise, exactly: k = 1: (-im, re), 2: (-re, -im), 3: (im, -re)."""
    k = np.asarray(k) % 4
    out_re = np.where(k == 0, re, np.where(k == 1, -im, np.where(k == 2, -re, im)))
    out_im = np.where(k == 0, im, np.where(k == 1, re, np.where(k == 2, -im, -re)))
    return out_re, out_im


def diagonals(matrix, xs):
    """complex128[D, 2^n]: row j is d_x for x = xs[j]."""
    m = np.asarray(matrix, dtype=np.complex128)
    b = np.arange(m.shape[0], dtype=np.int64)
    return m[b[None, :], b[None, :] ^ np.asarray(xs, dtype=np.int64)[:, None]]


def coefficients_of_diagonals(diag, xs, n):
    """complex128[D, 2^n]: entry (j, z) = c(xs[j], z), zeros included."""
    diag = np.asarray(diag, dtype=np.complex128)
    xs = np.asarray(xs, dtype=np.int64)
    re, im = wht_pinned(diag.real.copy(), diag.imag.copy())
    scale = 2.0 ** -n
    re *= scale
    im *= scale
    z = np.arange(1 << n, dtype=np.int64)
    re, im = times_i_pow(re, im, popcount(xs[:, None] & z[None, :]))
    out = np.empty(re.shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def decompose_diagonals(diag, xs, n):
    """(x int64[T], z int64[T], coeff complex128[T]) of the kept coefficients, ascending (x, z); ``xs`` ascending."""
    xs = np.asarray(xs, dtype=np.int64)
    assert np.all(np.diff(xs) > 0)
    c = coefficients_of_diagonals(diag, xs, n)
    keep = ~((c.real == 0) & (c.imag == 0))
    j, z = np.nonzero(keep)
    return xs[j], z.astype(np.int64), c[keep]


def decompose(matrix, n, xs=None):
    """The decomposition of a dense ``2^n x 2^n`` matrix over all diagonals (or the ascending ``xs``)."""
    xs = np.arange(1 << n, dtype=np.int64) if xs is None else np.asarray(xs, dtype=np.int64)
    return decompose_diagonals(diagonals(matrix, xs), xs, n)


def symp_of(x, z, n):
    """bool[T, 2n] = [X | Z] of terms given as n-bit integers, qubit 0 the most significant bit."""
    shifts = np.arange(n - 1, -1, -1, dtype=np.int64)
    x, z = np.asarray(x, dtype=np.int64), np.asarray(z, dtype=np.int64)
    return np.hstack([(x[:, None] >> shifts) & 1, (z[:, None] >> shifts) & 1]).astype(bool)


def xz_of(symp_matrix):
    """(x, z) int64[T] of a bool[T, 2n] symplectic matrix."""
    symp = np.asarray(symp_matrix, dtype=np.int64)
    n = symp.shape[1] // 2
    w = np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64)
    return symp[:, :n] @ w, symp[:, n:] @ w


def bits_equal(a, b):
    """Same shape and the same bits in every component (so -0.0 differs from +0.0)."""
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the reference's answers (tests/golden/from_matrix.npz, tools/gen_golden_from_matrix.py) ---------------------------------------------
def golden_cases():
    """[(tag, layout, kind, n, dense matrix, (data, indices, indptr) or None, reference symp, reference coeff)], loaded once."""
    global _GOLDEN
    if _GOLDEN is None:
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'from_matrix.npz'))
        _GOLDEN = []
        for k in range(int(g['n_cases'])):
            t = f'{k:02d}'
            layout, kind, n = str(g[f'{t}/layout']), str(g[f'{t}/kind']), int(g[f'{t}/n'])
            side = 1 << n
            if layout == 'dense':
                dense, csr = g[f'{t}/matrix'], None
            else:
                csr = (g[f'{t}/data'], g[f'{t}/indices'], g[f'{t}/indptr'])
                dense = np.zeros((side, side), dtype=np.complex128)
                dense[np.repeat(np.arange(side), np.diff(csr[2])), csr[1]] = csr[0]
            _GOLDEN.append((t, layout, kind, n, dense, csr, g[f'{t}/symp'], g[f'{t}/coeff']))
    return _GOLDEN


_GOLDEN = None


def reference_bound(n, matrix):
    """Per component: the reference adds 2^n exact terms one by one, the butterfly has n levels -> (2^n + n) 2^-53 max|M|."""
    return (2.0 ** n + n) * 2.0 ** -53 * float(np.max(np.abs(matrix)))


def assert_matches_reference(x, z, coeff, ref_symp, ref_coeff, kind, n, matrix):
    """A decomposition against the reference's, as sets keyed by (x, z).  Dyadic inputs: identical term sets and equal coefficients with
    no tolerance (`==` per component: the reference forms its coefficients as complex products, which leave -0.0 in a zero component
    where the exact swap leaves +0.0, so the SIGN of a zero component is the one thing not compared).  Gaussian inputs: every component
    within `reference_bound`; a term that only one side lists has both components within that bound of zero."""
    got = {(int(a), int(b)): complex(c) for a, b, c in zip(x, z, coeff)}
    rx, rz = xz_of(ref_symp)
    ref = {(int(a), int(b)): complex(c) for a, b, c in zip(rx, rz, ref_coeff)}
    assert len(got) == len(coeff) and len(ref) == len(ref_coeff), 'a term listed twice'
    if kind == 'dyadic':
        assert set(got) == set(ref), f'term sets differ: {sorted(set(got) ^ set(ref))[:8]}'
        bad = [q for q in got if got[q].real != ref[q].real or got[q].imag != ref[q].imag]
        assert not bad, f'{len(bad)} coefficients differ, e.g. {bad[0]}: {got[bad[0]]!r} != {ref[bad[0]]!r}'
        return
    bound = reference_bound(n, matrix)
    for q in set(got) | set(ref):
        a, b = got.get(q, 0j), ref.get(q, 0j)
        assert abs(a.real - b.real) <= bound and abs(a.imag - b.imag) <= bound, f'term {q}: {a!r} vs {b!r}, bound {bound:.3g}'
