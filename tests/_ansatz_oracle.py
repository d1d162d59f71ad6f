"""NumPy restatement of the contract of csrc/ansatz.hip (include/symgpu.h f8): |psi(theta)> = prod_k exp(i theta_k P_k) |ref>, rotation 0
first, qubit 0 the MOST significant bit of a basis index b, (P v)[b] = (-i)^Y (-1)^{|b & z|} v[b ^ x].  `rotate` is the arithmetic
contract component by component (every product and sum rounded once, as NumPy's elementwise operations are), so the device state is
compared bit for bit; the gradients are restated by OTHER means than the device uses: parameter shift for the ansatz parameters, dense
i [H, P] for the pool.  Test infrastructure only."""
import numpy as np

from _sparse_oracle import bits_to_int, _parity
from _matvec_oracle import _complex, matvec


def gens_of(symp_matrix):
    """(x, z, Y) int64[K] of the rows of a bool[K, 2n] matrix."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    symp = symp.reshape(-1, 2 * n)
    return bits_to_int(symp[:, :n]), bits_to_int(symp[:, n:]), np.sum(symp[:, :n] & symp[:, n:], axis=1).astype(np.int64)


def apply_pauli(x, z, y, v):
    """P v, exactly (a permutation, sign changes and component swaps)."""
    v = np.asarray(v, dtype=np.complex128)
    b = np.arange(v.shape[0], dtype=np.int64)
    sign = np.where(_parity(b & int(z)), -1.0, 1.0)
    p = v[b ^ int(x)]
    re, im = sign * p.real, sign * p.imag
    return [_complex(re, im), _complex(im, -re), _complex(-re, -im), _complex(-im, re)][int(y) % 4]     # (-i)^Y


def rotate(x, z, y, c, s, v):
    """(c + i s P) v with the device's arithmetic: w = i s (-i)^Y sigma is +-s or +-i s, psi'[b] = (c a.re + (w o p).re, c a.im + (w o p).im)."""
    v = np.asarray(v, dtype=np.complex128)
    b = np.arange(v.shape[0], dtype=np.int64)
    y = int(y) % 4
    neg = _parity(b & int(z)).astype(bool) ^ bool(y >> 1)
    ss = np.where(neg, -float(s), float(s))
    p = v[b ^ int(x)]
    if y & 1:
        wr, wi = ss * p.real, ss * p.imag
    else:
        wr, wi = -(ss * p.imag), ss * p.real
    return _complex(float(c) * v.real + wr, float(c) * v.imag + wi)


def state(symp_matrix, theta, ref, k_begin=0, k_end=None, inverse=False):
    """Rotations k_begin .. k_end-1 on ref; inverse: the inverse rotations from k_end-1 down to k_begin."""
    x, z, y = gens_of(symp_matrix)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    k_end = len(x) if k_end is None else k_end
    c, s = np.cos(theta), np.sin(theta)
    v = np.array(ref, dtype=np.complex128).reshape(-1)
    order = range(k_end - 1, k_begin - 1, -1) if inverse else range(k_begin, k_end)
    for k in order:
        v = rotate(x[k], z[k], y[k], c[k], -s[k] if inverse else s[k], v)
    return v


def energy(h_symp, h_coeff, v):
    """Re <v| H |v> with H v from the matvec oracle."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    return float(np.vdot(v, matvec(h_symp, h_coeff, v)).real)


def energy_at(h_symp, h_coeff, symp_matrix, theta, ref):
    return energy(h_symp, h_coeff, state(symp_matrix, theta, ref))


def grad_shift(h_symp, h_coeff, symp_matrix, theta, ref):
    """dE/dtheta_k by the parameter shift rule: E(theta + pi/4 e_k) - E(theta - pi/4 e_k)."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    out = np.zeros(theta.shape[0])
    for k in range(theta.shape[0]):
        up, dn = theta.copy(), theta.copy()
        up[k] += np.pi / 4
        dn[k] -= np.pi / 4
        out[k] = energy_at(h_symp, h_coeff, symp_matrix, up, ref) - energy_at(h_symp, h_coeff, symp_matrix, dn, ref)
    return out


def _phases(x, z, y, n):
    """ph[b] = P[b, b ^ x], the one entry of row b."""
    return apply_pauli(0, z, y, np.ones(1 << n, dtype=np.complex128))


def dense_pauli(x, z, y, n):
    """The 2^n x 2^n matrix of one Pauli string."""
    b = np.arange(1 << n, dtype=np.int64)
    P = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    P[b, b ^ int(x)] = _phases(x, z, y, n)
    return P


def dense_operator(h_symp, h_coeff):
    """sum_k c_k P_k as a dense matrix, the terms added in operator order."""
    h_symp = np.asarray(h_symp, dtype=bool)
    n = h_symp.shape[1] // 2
    x, z, y = gens_of(h_symp)
    b = np.arange(1 << n, dtype=np.int64)
    H = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for k in range(len(x)):
        H[b, b ^ int(x[k])] += complex(h_coeff[k]) * _phases(x[k], z[k], y[k], n)
    return H


def pool_grad(h_dense, pool_symp, v):
    """<v| i [H, P_j] |v> for every pool row from the two dense products of the commutator, each built from the dense H and the signed
    permutation P: (H P)[:, c] = H[:, c ^ x] ph[c ^ x] and (P H)[b, :] = ph[b] H[b ^ x, :].  The permuted copies of H are gathered
    row-wise (from H and from a contiguous H^T) and taken straight into the quadratic form, so a pool of 96 on 10 qubits takes about a second."""
    pool_symp = np.asarray(pool_symp, dtype=bool)
    n = pool_symp.shape[1] // 2
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    x, z, y = gens_of(pool_symp)
    b = np.arange(1 << n, dtype=np.int64)
    h_dense = np.ascontiguousarray(h_dense)
    h_t = np.ascontiguousarray(h_dense.T)
    cols, rows = np.empty_like(h_dense), np.empty_like(h_dense)
    out = np.zeros(len(x))
    for j in range(len(x)):
        ph, partner = _phases(x[j], z[j], y[j], n), b ^ int(x[j])
        np.take(h_t, partner, axis=0, out=cols)                  # cols.T = H[:, c ^ x]
        np.take(h_dense, partner, axis=0, out=rows)              # rows = H[b ^ x, :]
        hp_v = (ph[partner] * v) @ cols                          # (H P) v
        ph_v = ph * (rows @ v)                                   # (P H) v
        out[j] = (1j * np.vdot(v, hp_v - ph_v)).real
    return out


LOW_BITS, TILE_BITS, PAD_BITS = 4, 12, 10


def plan_runs(symp_matrix):
    """The cut rule of the tiled form: [(k0, k1, S, tiled)] over the generators in order.  A run's tile bits S start as the LOW_BITS lowest
    index bits and grow by each X-part while |S| <= min(n, TILE_BITS); x = 0 joins an open run; a generator that does not fit closes the
    run and opens the next one, or takes a direct pass (S = 0, adjacent ones merged) when LOW_BITS and its own X-part exceed the budget.
    A closed run of fewer than min(n, PAD_BITS) bits takes the lowest free bits up to that number."""
    symp = np.asarray(symp_matrix, dtype=bool)
    n = symp.shape[1] // 2
    xs = gens_of(symp)[0]
    cap, pad, low = min(n, TILE_BITS), min(n, PAD_BITS), (1 << min(n, LOW_BITS)) - 1
    count = lambda v: bin(v).count('1')
    segs, run = [], None                                   # run = [k0, S]

    def close(k):
        nonlocal run
        if run is not None:
            S, bit = run[1], 0
            while count(S) < pad:
                S, bit = S | (1 << bit), bit + 1
            segs.append((run[0], k, S, True))
            run = None

    for k, x in enumerate(int(v) for v in xs):
        if run is not None and count(run[1] | x) <= cap:
            run[1] |= x
            continue
        close(k)
        if count(low | x) <= cap:
            run = [k, low | x]
        elif segs and not segs[-1][3] and segs[-1][1] == k:
            segs[-1] = (segs[-1][0], k + 1, 0, False)
        else:
            segs.append((k, k + 1, 0, False))
    close(len(xs))
    return segs


def bound(n, K, T, coeff):
    """R = (16 K + 4 T + 2^n + 64) 2^-53 sum|c|: each of K rotations perturbs the unit state by a few roundoffs, the product with H by
    T u sum|c|, a 2^n-term sum in any order by 2^n u times the norms, every quantity bounded by |H| <= sum|c|."""
    return (16 * K + 4 * T + (1 << n) + 64) * 2.0 ** -53 * float(np.abs(np.asarray(coeff)).sum())
