"""NumPy restatement of the ORDER of the statevector reductions as include/symgpu.h states it (f7 symgpu_lanczos_step / symgpu_vec_combine,
f8 symgpu_ansatz_energy_grad / symgpu_pool_gradient), written from the header's words:
  the units (elements, or slots for the sweep) are cut into chunks of C = max(256, count / 1024) consecutive units; thread t of 256 adds
  the terms of units t, t + 256, ... of its chunk to 0 in ascending order; the 256 thread sums are folded by halving (s[t] += s[t + 128],
  then 64, ... 1); one launch adds the chunk sums to 0 in ascending chunk order.
Every device operation in these sums is one separately rounded product, sum or difference, as NumPy's elementwise operations are, so the
device's scalars are compared for equality.  The product H v is taken from tests/_matvec_oracle.py; for an H of ONE string with a
power-of-two coefficient it is exact, which is what the GPU tests feed.  The module also holds the inputs (strings, seeds) that the CPU
tests of this oracle and the GPU tests share.  Test infrastructure only."""
import numpy as np

import _ansatz_oracle as ao
import _matvec_oracle as mo
from _matvec_oracle import _complex

WG = 256


def chunk_of(count):
    """C = max(256, count / 1024)."""
    return max(WG, int(count) >> 10)


def fold_halving(acc):
    """s[t] += s[t + h] for t < h, h = 128, 64, ... 1, on every row of float64[chunks, 256]; the chunk sums."""
    h = WG // 2
    while h:
        acc = acc[:, :h] + acc[:, h:2 * h]
        h >>= 1
    return acc[:, 0]


def fold_ascending(acc):
    """NOT the contract: the 256 thread sums added to 0 one after the other.  For the tests that show that the inputs tell the orders apart."""
    total = np.zeros(acc.shape[0])
    for t in range(WG):
        total = total + acc[:, t]
    return total


def two_level(terms, chunk, fold):
    """The two-level sum of float64[count] with chunks of `chunk` units and `fold` over the 256 thread sums of a chunk.  Units past the
    end add nothing (a thread skips them): they are padded with zeros, which changes no value."""
    t = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1)
    count = t.shape[0]
    chunks, strides = -(-count // chunk), -(-chunk // WG)
    flat = np.zeros(chunks * chunk)
    flat[:count] = t
    padded = np.zeros((chunks, strides * WG))
    padded[:, :chunk] = flat.reshape(chunks, chunk)
    padded = padded.reshape(chunks, strides, WG)                     # unit s * 256 + t of a chunk belongs to thread t
    acc = np.zeros((chunks, WG))
    for s in range(strides):
        acc = acc + padded[:, s, :]
    total = 0.0
    for c in fold(acc):
        total = total + float(c)
    return total


def ordered_sum(terms):
    """The sum of float64[count], in unit order, as the header orders it."""
    return two_level(terms, chunk_of(np.size(terms)), fold_halving)


def ordered_sum_complex(re, im):
    return ordered_sum(re), ordered_sum(im)


# the same terms in three orders that the header does NOT state: name -> function of the term vector
OTHER_ORDERS = {
    'chunks of 256 at every size': lambda t: two_level(t, WG, fold_halving),
    'thread sums added in ascending order': lambda t: two_level(t, chunk_of(np.size(t)), fold_ascending),
    'np.sum': lambda t: float(np.sum(t)),
}


# ---- the terms -------------------------------------------------------------------------------------------------------------------------
def dot_terms(a, c):
    """(re, im) terms of conj(a[b]) c[b]: re = a.re c.re + a.im c.im, im = a.re c.im - a.im c.re."""
    return a.real * c.real + a.imag * c.imag, a.real * c.imag - a.imag * c.real


def im_terms(lam, q):
    """Im conj(lam[b]) q[b] = lam.re q.im - lam.im q.re per element."""
    return lam.real * q.imag - lam.imag * q.real


def slot_elements(x, n):
    """(b0, b1) of the slots t < 2^(n-1): b0 = t with a clear bit inserted at the top set bit of x (at bit n-1 for x = 0), b1 = b0 ^ x
    (b0 | 2^(n-1) for x = 0)."""
    x = int(x)
    t = np.arange(1 << (n - 1), dtype=np.int64)
    h = x.bit_length() - 1 if x else n - 1
    b0 = ((t >> h) << (h + 1)) | (t & ((1 << h) - 1))
    return b0, (b0 ^ x if x else b0 | (1 << h))


def slot_units(x, n, term):
    """A slot's unit: term of b0 + term of b1."""
    b0, b1 = slot_elements(x, n)
    return term[b0] + term[b1]


def energy_terms(h_symp, h_coeff, psi):
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    return dot_terms(psi, mo.matvec(h_symp, h_coeff, psi))[0]


def energy_ordered(h_symp, h_coeff, psi):
    """Re <psi| H |psi>, one term per element."""
    return ordered_sum(energy_terms(h_symp, h_coeff, psi))


def sweep_units(h_symp, h_coeff, symp_matrix, theta, ref):
    """[(k, units of t_k)] for k = K-1 .. 0, the units from the values before U_k^+ is applied to psi and lambda."""
    n = np.asarray(symp_matrix).shape[1] // 2
    x, z, y = ao.gens_of(symp_matrix)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    c, s = np.cos(theta), np.sin(theta)
    psi = ao.state(symp_matrix, theta, ref)
    lam = mo.matvec(h_symp, h_coeff, psi)
    for k in range(len(x) - 1, -1, -1):
        yield k, slot_units(x[k], n, im_terms(lam, ao.apply_pauli(x[k], z[k], y[k], psi)))
        psi, lam = ao.rotate(x[k], z[k], y[k], c[k], -s[k], psi), ao.rotate(x[k], z[k], y[k], c[k], -s[k], lam)


def sweep_grad_ordered(h_symp, h_coeff, symp_matrix, theta, ref, total=ordered_sum):
    """dE/dtheta_k by the reverse sweep: g_k = -2 t_k, t_k summed over the slots."""
    out = np.zeros(np.asarray(symp_matrix).shape[0])
    for k, units in sweep_units(h_symp, h_coeff, symp_matrix, theta, ref):
        out[k] = -2.0 * total(units)
    return out


def pool_terms(h_symp, h_coeff, pool_symp, psi):
    """[terms of row j] of the pool, one term per element, phi = H psi taken once."""
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    phi = mo.matvec(h_symp, h_coeff, psi)
    x, z, y = ao.gens_of(pool_symp)
    for j in range(len(x)):
        yield im_terms(phi, ao.apply_pauli(x[j], z[j], y[j], psi))


def pool_grad_ordered(h_symp, h_coeff, pool_symp, psi, total=ordered_sum):
    """<psi| i [H, P_j] |psi> = -2 sum_b Im conj(phi[b]) (P_j psi)[b] for every pool row."""
    return np.array([-2.0 * total(t) for t in pool_terms(h_symp, h_coeff, pool_symp, psi)], dtype=np.float64)


def norm_ordered(wr, wi):
    """|w| = sqrt(<w, w>), the products w.re w.re + w.im w.im summed in the order above."""
    return float(np.sqrt(ordered_sum(wr * wr + wi * wi)))


def lanczos_step_ordered(h_symp, h_coeff, keep, V, j):
    """(alpha, beta, v_next) of one step on the slots V[0 .. j] (complex128 [>= j + 1, 2^n]); keep: bool[2^n] or None.  Classical
    Gram-Schmidt done twice: all j + 1 inner products of a pass from the same w, then w = ((w - h_0 v_0) - h_1 v_1) - ... in basis order,
    every complex product the plain four-multiplication one.  v_next is None unless beta > 0."""
    V = np.asarray(V, dtype=np.complex128)
    w = mo.matvec(h_symp, h_coeff, V[j])
    if keep is not None:
        w = np.where(np.asarray(keep, dtype=bool), w, 0.0)
    wr, wi = w.real.copy(), w.imag.copy()
    alpha = None
    for sweep in range(2):
        hs = [ordered_sum_complex(*dot_terms(V[i], _complex(wr, wi))) for i in range(j + 1)]
        if sweep == 0:
            alpha = hs[j][0]
        for i, (hr, hi) in enumerate(hs):
            vr, vi = V[i].real, V[i].imag
            wr, wi = wr - (hr * vr - hi * vi), wi - (hr * vi + hi * vr)
    beta = norm_ordered(wr, wi)
    return alpha, beta, (_complex(wr / beta, wi / beta) if beta > 0.0 else None)


def combine_ordered(V, s, normalise=False):
    """s_0 v_0 + s_1 v_1 + ... from the first product, in basis order; with `normalise` divided by its norm (a zero vector stays)."""
    V = np.asarray(V, dtype=np.complex128)
    s = np.asarray(s, dtype=np.float64)
    re, im = s[0] * V[0].real, s[0] * V[0].imag
    for j in range(1, len(s)):
        re, im = re + s[j] * V[j].real, im + s[j] * V[j].imag
    if normalise:
        beta = norm_ordered(re, im)
        if beta > 0.0:
            re, im = re / beta, im / beta
    return _complex(re, im)


# ---- the shared inputs -----------------------------------------------------------------------------------------------------------------
def symp_of(strings):
    n = len(strings[0])
    out = np.zeros((len(strings), 2 * n), dtype=bool)
    for r, s in enumerate(strings):
        for q, ch in enumerate(s):
            out[r, q], out[r, n + q] = ch in 'XY', ch in 'ZY'
    return out


def on_qubits(n, letters):
    """The string with the given {qubit: letter}, I elsewhere."""
    return ''.join(letters.get(q, 'I') for q in range(n))


def anticommute(a, b):
    return sum(1 for p, q in zip(a, b) if 'I' not in (p, q) and p != q) % 2 == 1


def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


def unit(v):
    return v / np.linalg.norm(v)


H_COEFF = np.array([0.5])
SWEEP_SIZES = [1, 5, 9, 10, 19, 20, 21]              # slots: 1, 16, 256, 512, 2^18, 2^19, 2^20
ELEMENT_SIZES = [4, 8, 9, 18, 19, 20]                # elements: 16, 256, 512, 2^18, 2^19, 2^20
LARGE_SWEEP, LARGE_ELEMENT = [20, 21], [19, 20]      # the first sizes with more than one unit per thread
MIN_GRADIENT = 1e-3


def h_string(n):
    """One string with X, Y and Z letters (as far as there is room) that touches qubit 0 and qubit n-1."""
    return {1: 'Y', 2: 'XZ'}.get(n) or on_qubits(n, {0: 'X', 1: 'Y', n - 1: 'Z'})


def masked_h_string(n):
    """A Z-string (it conserves the particle number) on qubits 0, 1 and n-1."""
    return on_qubits(n, {0: 'Z', 1: 'Z', n - 1: 'Z'})


def generators(n):
    """The K generators of the size, none commuting with h_string(n):
      0: X-part on qubit 0 (the partner is 2^(n-1) away) and Y on qubit n-1;
      1: X-part on the lowest qubits only;
      2: 13 or more X/Y positions from qubit 0 down, so that from n = 14 on it takes a direct pass between two tiled runs;
      3: diagonal, Z on qubits 0 and n-1.
    n = 21 keeps 0 and 3 (K = 2); n = 1 has the single-letter strings."""
    if n == 1:
        return ['X', 'Z', 'X', 'Z']
    h = h_string(n)
    first = on_qubits(n, {0: 'X', n - 1: 'Y'})
    low = on_qubits(n, {n - 2: 'Y', n - 1: 'X'}) if n >= 4 else on_qubits(n, {n - 1: 'X'})
    body = {q: 'XY'[q % 2] for q in range(1, min(n, 14))}
    wide = next(s for s in (on_qubits(n, {0: ch, **body}) for ch in 'XY') if anticommute(s, h))
    diagonal = on_qubits(n, {0: 'Z', n - 1: 'Z'})
    out = [first, diagonal] if n == 21 else [first, low, wide, diagonal]
    assert all(anticommute(s, h) for s in out)
    return out


# Seeds chosen on the CPU (tests/test_reduction_oracle.py holds the conditions): every component of the ordered gradient is at least
# MIN_GRADIENT in magnitude — for a normalised Gaussian state a Pauli expectation is of order 2^(-n/2), which is 1e-3 at n = 20 — and at
# the large sizes the three other orders give other values than the stated one.
SWEEP_SEEDS = {1: 1, 5: 1, 9: 4, 10: 1, 19: 110, 20: 3078, 21: 349}
POOL_SEEDS = {4: 1, 8: 1, 9: 4, 18: 13, 19: 66, 20: 5027}
LANCZOS_SEEDS = {4: 504, 8: 508, 9: 509, 18: 518, 19: 520, 20: 520}


def gaussian_inputs(n, seed):
    """(h_symp, h_coeff, gens, theta, ref): theta uniform in (-pi, pi), ref a normalised Gaussian vector."""
    rng = np.random.default_rng(seed)
    gens = symp_of(generators(n))
    theta = rng.uniform(-np.pi, np.pi, gens.shape[0])
    return symp_of([h_string(n)]), H_COEFF, gens, theta, unit(gaussian(rng, 1 << n))


def sweep_inputs(n):
    return gaussian_inputs(n, SWEEP_SEEDS[n])


def pool_inputs(n):
    """(h_symp, h_coeff, pool, psi): the pool is the size's generators, psi the state they prepare."""
    h_symp, h_coeff, gens, theta, ref = gaussian_inputs(n, POOL_SEEDS[n])
    return h_symp, h_coeff, gens, ao.state(gens, theta, ref)


def lanczos_start(n, keep=None):
    """v_0: a normalised Gaussian vector, zero outside `keep`."""
    v = gaussian(np.random.default_rng(LANCZOS_SEEDS[n]), 1 << n)
    return unit(v if keep is None else np.where(keep, v, 0.0))


def particle_sector(n):
    """bool[2^n]: the basis states of n // 2 particles."""
    b = np.arange(1 << n, dtype=np.int64)
    weight = np.zeros(1 << n, dtype=np.int64)
    for q in range(n):
        weight += (b >> q) & 1
    return weight == n // 2


# ---- the dyadic inputs: every partial sum in any order is exact ------------------------------------------------------------------------
AMP_SCALE, COEFF_SCALE = 16, 8                       # amplitudes are integers in [-8, 8] over 16, coefficients integers over 8


def dyadic_vector(n, seed=77):
    rng = np.random.default_rng(seed + n)
    return (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / float(AMP_SCALE)


def dyadic_operator(n):
    """(h_symp, h_coeff) of 12 terms with real dyadic coefficients: terms 2 and 3 share an X-part, the last two cancel."""
    terms = [({0: 'X', 1: 'Y', n - 1: 'Z'}, 0.5), ({0: 'Z', n - 1: 'Z'}, -0.75), ({0: 'X', 2: 'Z'}, 1.25), ({0: 'Y'}, 0.375),
             ({n - 1: 'X'}, -1.5), ({n - 2: 'Y', n - 1: 'X'}, 0.625), ({3: 'Z'}, 2.0), ({5: 'X', 6: 'X', 7: 'Y', 8: 'Y'}, -0.125),
             ({5: 'Y', 6: 'Y', 7: 'X', 8: 'X'}, 0.125), ({1: 'Z', 2: 'Z'}, 3.5), ({0: 'X', n - 1: 'X'}, 0.25), ({0: 'X', n - 1: 'X'}, -0.25)]
    return symp_of([on_qubits(n, letters) for letters, _ in terms]), np.array([c for _, c in terms])


def dyadic_pool(n):
    return symp_of([on_qubits(n, {0: 'X', n - 1: 'Y'}), on_qubits(n, {n - 2: 'Y', n - 1: 'X'}), on_qubits(n, {0: 'Z', n - 1: 'Z'}),
                    on_qubits(n, {0: 'Y', 2: 'X', 5: 'Z'}), on_qubits(n, {1: 'X'}), on_qubits(n, {q: 'XY'[q % 2] for q in range(14)})])


def _pauli_int(x, z, y, re, im):
    """P v on Gaussian integers (int64 re, im): a permutation, sign changes and component swaps."""
    b = np.arange(re.shape[0], dtype=np.int64)
    sign = 1 - 2 * ao._parity(b & int(z)).astype(np.int64)
    pr, pi = sign * re[b ^ int(x)], sign * im[b ^ int(x)]
    return [(pr, pi), (pi, -pr), (-pr, -pi), (-pi, pr)][int(y) % 4]


def integer_results(h_symp, h_coeff, pool_symp, v):
    """(<v|H|v>, [<v| i [H, P_j] |v>]) of the dyadic inputs from integer arithmetic: amplitudes times 16 and coefficients times 8 are
    integers, every sum is an int64 far below 2^63 (asserted), and the one division by 16 * 16 * 8 is by a power of two."""
    re, im = np.rint(v.real * AMP_SCALE).astype(np.int64), np.rint(v.imag * AMP_SCALE).astype(np.int64)
    ci = np.rint(np.asarray(h_coeff) * COEFF_SCALE).astype(np.int64)
    assert np.array_equal(re / AMP_SCALE, v.real) and np.array_equal(im / AMP_SCALE, v.imag) and np.array_equal(ci / COEFF_SCALE, h_coeff)
    assert int(np.abs(ci).sum()) * 8 * 8 * 2 * v.shape[0] < 2 ** 52            # every sum of terms, in any order, is an exact double too
    x, z, y = ao.gens_of(h_symp)
    wr, wi = np.zeros_like(re), np.zeros_like(im)
    for k in range(len(x)):
        pr, pi = _pauli_int(x[k], z[k], y[k], re, im)
        wr, wi = wr + int(ci[k]) * pr, wi + int(ci[k]) * pi
    scale = float(AMP_SCALE * AMP_SCALE * COEFF_SCALE)
    energy = int(np.sum(re * wr + im * wi)) / scale
    px, pz, py = ao.gens_of(pool_symp)
    grad = []
    for j in range(len(px)):
        qr, qi = _pauli_int(px[j], pz[j], py[j], re, im)
        grad.append(-2 * int(np.sum(wr * qi - wi * qr)) / scale)
    return energy, np.array(grad)
