"""Product states with dyadic factors: vectors of 2^n amplitudes every property of which has a closed form, so that the dense-statevector
kernels can be held to EXACT answers at 27 and 28 qubits, where no NumPy oracle over the whole vector is affordable.

    psi = (x)_q (a_q |0> + b_q |1>),   qubit 0 the most significant bit of the index (qubit q at bit n-1-q),
    (a_q, b_q) = (i^p, i^r 2^-e),  e in {0, 1}

with a_q != b_q for every qubit (one wrong index bit changes the value), neighbouring qubits with different pairs, and at most MAX_HALF
qubits with e = 1.  An amplitude is then i^P 2^-k with P the sum of the chosen phase exponents and k <= MAX_HALF the number of chosen
halves: it is formed here in INTEGERS, so nothing below rounds.

Exactness.  With m <= MAX_HALF half-magnitude qubits an amplitude is a multiple of 2^-m of magnitude at most 1, a product of two a
multiple of 2^-2m, and a sum over the whole vector is below 2^n times the largest addend.  Operator and Chebyshev coefficients are integers
over 8, the centre an integer over 8, the half-width a power of two.  `assert_exact_budget` holds n + 2m + (bits of the coefficient sums)
to 52: every partial sum, in ANY order and with or without fused multiply-adds, is then an exact double, and the device must be EQUAL to
the closed form (compared with ==, so that the sign of a zero does not matter).

tests/test_large_vectors.py proves every closed form here against the project's oracles at 8 .. 12 qubits, where psi is materialised.
Test infrastructure only."""
import numpy as np

MAX_HALF = 8
SEEDS = (1, 3)                  # the two assignments in use: 1 has a half-magnitude qubit among the top three, 3 none among the top five
LOW_BITS = 14                   # the low-qubit vector of an upload piece: 2^14 amplitudes
PIECE_BITS = 24                 # an upload piece: 2^24 amplitudes, 256 MiB
UNITS = np.array([1, 1j, -1, -1j], dtype=np.complex128)             # i^p by p mod 4
RADIX_BITS = 4                  # the radix-16 sum tree of csrc/sample.hip
SQRT_HALF = float.fromhex('0x1.6a09e667f3bcdp-1')


# ---- the factor lists -----------------------------------------------------------------------------------------------------------------------
def factors(n, seed):
    """(phase int64[n, 2], half int64[n]): a_q = i^phase[q, 0], b_q = i^phase[q, 1] 2^-half[q].  Seeded; the rules of the module docstring
    are enforced while drawing and asserted at the end."""
    rng = np.random.default_rng(990000 + seed)
    phase, half = np.zeros((n, 2), dtype=np.int64), np.zeros(n, dtype=np.int64)
    for q in range(n):
        while True:
            p, r, e = int(rng.integers(4)), int(rng.integers(4)), int(rng.integers(2))
            if e and half.sum() >= MAX_HALF:
                e = 0
            if e == 0 and p == r:
                continue                                            # a_q == b_q
            if q and (p, r, e) == (phase[q - 1, 0], phase[q - 1, 1], half[q - 1]):
                continue                                            # the neighbour's pair
            phase[q], half[q] = (p, r), e
            break
    assert half.sum() <= MAX_HALF and all(half[q] or phase[q, 0] != phase[q, 1] for q in range(n))
    assert all((*phase[q], half[q]) != (*phase[q - 1], half[q - 1]) for q in range(1, n))
    return phase, half


def factor_values(n, seed):
    """complex128[n, 2]: (a_q, b_q)."""
    phase, half = factors(n, seed)
    return np.stack([UNITS[phase[:, 0]], UNITS[phase[:, 1]] * 2.0 ** -half], axis=1)


def _product(phase, half, idx):
    """i^P 2^-k over the qubits of `phase` / `half`, the LAST of them at bit 0 of idx."""
    idx = np.asarray(idx, dtype=np.int64)
    w = phase.shape[0]
    p, k = np.zeros(idx.shape, dtype=np.int64), np.zeros(idx.shape, dtype=np.int64)
    for q in range(w):
        bit = (idx >> (w - 1 - q)) & 1
        p += np.where(bit == 1, phase[q, 1], phase[q, 0])
        k += bit * half[q]
    return UNITS[p & 3] * np.ldexp(1.0, -k)


def amplitudes(n, seed, idx):
    """psi[idx] for any int64 index array, without the vector."""
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < 1 << n)
    return _product(*factors(n, seed), idx)


def pieces(n, seed):
    """(first element, complex128 piece) over the vector in order: pieces of 2^min(n, 24) amplitudes, each the outer product of the
    high-qubit factor vector and the low-qubit vector of 2^min(n, 14) amplitudes."""
    phase, half = factors(n, seed)
    low, piece = min(n, LOW_BITS), min(n, PIECE_BITS)
    lo = _product(phase[n - low:], half[n - low:], np.arange(1 << low, dtype=np.int64))
    hi_count = 1 << (piece - low)
    for j in range(1 << (n - piece)):
        hi = _product(phase[:n - low], half[:n - low], j * hi_count + np.arange(hi_count, dtype=np.int64)) if n > low else np.ones(1, dtype=np.complex128)
        yield j << piece, np.multiply.outer(hi, lo).reshape(-1)


def materialise(n, seed):
    """The whole vector on the host (small n only)."""
    assert n <= PIECE_BITS
    return np.concatenate([p for _, p in pieces(n, seed)])


def upload(n, seed):
    """psi as a DeviceBuffer of 2^n complex128, written piece by piece at a byte offset: no host array above 256 MiB."""
    import ctypes
    from symmer_amd import kernels, _lib
    buf = kernels.DeviceBuffer(16 << n)
    try:
        for first, piece in pieces(n, seed):
            _lib.check(_lib.lib().symgpu_dev_upload(ctypes.c_void_p(buf.ptr.value + 16 * first), _lib.addr(piece), piece.nbytes))
    except BaseException:
        buf.free()
        raise
    return buf


# ---- the windows ------------------------------------------------------------------------------------------------------------------------------
def windows(n):
    """[(first element, count)] ascending, disjoint: the first and last `big` elements, `big` elements straddling 2^(n-1) and each quarter
    point (at n = 28 also element 2^27, byte 2^31: that IS 2^(n-1)), and up to 64 seeded windows of `small` elements elsewhere.
    big = 4096 and small = 256 from 16 qubits on, scaled down below so that a small vector is not simply covered."""
    N = 1 << n
    big, small = min(4096, max(2, N >> 4)), min(256, max(1, N >> 6))
    fixed = [(0, big), (N - big, big)] + [(N // 4 * k - big // 2, big) for k in (1, 2, 3)]
    if n >= 28:
        fixed.append(((1 << 27) - big // 2, big))
    fixed = sorted(set(fixed))
    taken = np.zeros(N // small, dtype=bool)
    for first, count in fixed:
        taken[first // small:(first + count + small - 1) // small] = True
    free = np.flatnonzero(~taken)
    rng = np.random.default_rng(770000 + n)
    slots = rng.choice(free, size=min(64, free.shape[0] // 2), replace=False)
    return sorted(fixed + [(int(s) * small, small) for s in slots])


def window_indices(n):
    return np.concatenate([np.arange(first, first + count, dtype=np.int64) for first, count in windows(n)])


# ---- the exactness budget ------------------------------------------------------------------------------------------------------------------
def n_half(n, seed):
    return int(factors(n, seed)[1].sum())


def assert_exact_budget(n, m, coeff_bits, whole_vector=True):
    """n + 2m + coeff_bits <= 52 (without `whole_vector`: m + coeff_bits, an element alone): the condition under which every partial sum
    of the identities below is an exact double.  coeff_bits: the bits of the integer that bounds the coefficient sums in their own unit
    (`bits_of`)."""
    assert 0 <= m <= MAX_HALF, f'{m} half-magnitude qubits; at most {MAX_HALF} are allowed'
    used = (n + 2 * m if whole_vector else m) + coeff_bits
    assert used <= 52, f'{used} bits needed; a double holds 52 exactly'


def bits_of(coeff, unit=8):
    """Bits of sum(|Re c| + |Im c|) in units of 1 / unit, the coefficients asserted to be integers over `unit`."""
    c = np.atleast_1d(np.asarray(coeff, dtype=np.complex128)) * unit
    assert np.array_equal(c.real, np.rint(c.real)) and np.array_equal(c.imag, np.rint(c.imag)), f'a coefficient is not an integer over {unit}'
    return int(np.abs(c.real).sum() + np.abs(c.imag).sum()).bit_length()


def cheb_bits(coeff, centre, c):
    """Bits of an element of sum_k c_k T_k((H - centre) / half_width) psi beyond those of psi's own: with S = sum|coeff| + |centre|, T_K
    is at most (2 S / h)^K and a multiple of (8 h)^-K, so its integer is below (16 S)^K whatever the power of two h; c adds bits_of(c)."""
    K = np.atleast_1d(c).shape[0] - 1
    S = int(np.abs(np.asarray(coeff) * 8).sum() + abs(centre * 8))            # 8 S
    assert centre * 8 == int(centre * 8)
    return K * max(1, (2 * S).bit_length()) + bits_of(c)


# ---- operators as index functions ------------------------------------------------------------------------------------------------------------
def _xzy(symp):
    """(x, z as index masks, Y count) per row of bool[T, 2n]: qubit q at bit n-1-q."""
    symp = np.asarray(symp, dtype=bool)
    n = symp.shape[1] // 2
    w = np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64)
    return symp[:, :n].astype(np.int64) @ w, symp[:, n:].astype(np.int64) @ w, np.sum(symp[:, :n] & symp[:, n:], axis=1)


def _parity(v):
    v = np.asarray(v, dtype=np.int64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> s
    return v & 1


def _entry(z, y, b):
    """(-i)^Y (-1)^{|b & z|}: the one entry of row b of the string."""
    return UNITS[(3 * int(y)) & 3] * (1.0 - 2.0 * _parity(b & int(z)))


def apply_terms(symp, coeff, f):
    """The index function of H f for the index function f: (H f)[b] = sum_t c_t (-i)^{Y_t} (-1)^{|b & z_t|} f[b ^ x_t]."""
    x, z, y = _xzy(symp)
    coeff = np.asarray(coeff, dtype=np.complex128)

    def g(idx):
        idx = np.asarray(idx, dtype=np.int64)
        out = np.zeros(idx.shape, dtype=np.complex128)
        for t in range(len(x)):
            out = out + coeff[t] * _entry(z[t], y[t], idx) * f(idx ^ int(x[t]))
        return out
    return g


def _span(xs):
    out = {0}
    for x in {int(v) for v in xs}:
        out |= {s ^ x for s in out}
    return sorted(out)


def _apply_table(x, z, y, coeff, idx, table):
    """H on a table {shift s: f[idx ^ s]} over a set of shifts closed under every x_t: the same sum as apply_terms, each f looked up.
    (-1)^{|(idx ^ s) & z|} = (-1)^{|idx & z|} (-1)^{|s & z|}: the entry at idx once per term, a sign per shift."""
    entry = [coeff[t] * _entry(z[t], y[t], idx) for t in range(len(x))]
    out = {}
    for s in table:
        acc = np.zeros(idx.shape, dtype=np.complex128)
        for t in range(len(x)):
            sign = -1.0 if bin(s & int(z[t])).count('1') & 1 else 1.0
            acc = acc + sign * (entry[t] * table[s ^ int(x[t])])
        out[s] = acc
    return out


def cheb_window(symp, coeff, centre, half_width, c, n, seed, idx, every_order=False):
    """(sum_k c_k T_k((H - centre) / half_width) psi)[idx] by the three-term recurrence on index functions.  T_k at idx needs T_{k-1} at
    idx ^ x_t for every term: the T^K evaluations are shared through a table over the XOR span of the X-parts.  With `every_order`:
    the list of the partial sums up to K = 0, 1, ..., each the result of the call with c[:K + 1]."""
    assert np.log2(half_width) == int(np.log2(half_width))
    assert_exact_budget(n, n_half(n, seed), cheb_bits(coeff, centre, c), whole_vector=False)
    idx = np.asarray(idx, dtype=np.int64)
    x, z, y = _xzy(symp)
    coeff, c = np.asarray(coeff, dtype=np.complex128), np.atleast_1d(np.asarray(c, dtype=np.complex128))
    prev = {s: amplitudes(n, seed, idx ^ s) for s in _span(x)}
    out, before = c[0] * prev[0], None
    sums = [out]
    for k in range(1, c.shape[0]):
        h = _apply_table(x, z, y, coeff, idx, prev)
        scale = (1.0 if k == 1 else 2.0) / half_width
        cur = {s: scale * (h[s] - centre * prev[s]) - (0 if before is None else before[s]) for s in prev}
        out = out + c[k] * cur[0]
        sums.append(out)
        before, prev = prev, cur
    return sums if every_order else out


def rotate_window(symp, cos_t, sin_t, n, seed, idx):
    """(prod_k (c_k + i s_k P_k) psi)[idx], rotation 0 first: psi'[b] = c psi[b] + i s (P psi)[b], composed through the same table."""
    idx = np.asarray(idx, dtype=np.int64)
    x, z, y = _xzy(symp)
    assert all(abs(c) + abs(s) <= 1 and 2 * c == int(2 * c) and 2 * s == int(2 * s) for c, s in zip(cos_t, sin_t))
    assert_exact_budget(n, n_half(n, seed), len(x), whole_vector=False)          # a rotation halves the unit at most and does not grow the values
    table = {s: amplitudes(n, seed, idx ^ s) for s in _span(x)}
    for k in range(len(x)):
        table = {s: cos_t[k] * table[s] + 1j * sin_t[k] * (_entry(z[k], y[k], idx ^ s) * table[s ^ int(x[k])]) for s in table}
    return table[0]


# ---- whole-vector closed forms --------------------------------------------------------------------------------------------------------------
PAULI = {(0, 0): np.eye(2, dtype=np.complex128), (1, 0): np.array([[0, 1], [1, 0]], dtype=np.complex128),
         (0, 1): np.array([[1, 0], [0, -1]], dtype=np.complex128), (1, 1): np.array([[0, -1j], [1j, 0]], dtype=np.complex128)}


def product_expectation(rows, n, seed):
    """<psi| P_1 P_2 ... |psi> for the strings `rows` (bool[2n] each, multiplied in this order): the product over the qubits of
    phi_q^+ (sigma_1 sigma_2 ...) phi_q.  Every factor is a small dyadic number, the product exact."""
    phi = factor_values(n, seed)
    rows = [np.asarray(r, dtype=bool) for r in rows]
    out = 1.0 + 0j
    for q in range(n):
        m = np.eye(2, dtype=np.complex128)
        for r in rows:
            m = m @ PAULI[(int(r[q]), int(r[n + q]))]
        out = out * (phi[q].conj() @ m @ phi[q])
    return out


def pauli_expectation(row, n, seed):
    """<psi| P |psi> of one string, real."""
    v = product_expectation([row], n, seed)
    assert v.imag == 0
    return float(v.real)


def energy(symp, coeff, n, seed):
    """Re <psi| H |psi> = sum_t Re(c_t) <P_t>, exact under the budget."""
    assert_exact_budget(n, n_half(n, seed), bits_of(coeff))
    return float(sum((complex(c) * pauli_expectation(r, n, seed)).real for r, c in zip(np.asarray(symp, dtype=bool), coeff)))


def commutator_expectation(symp, coeff, row, n, seed):
    """<psi| i [H, P] |psi> for the string `row`: sum_t Re(i c_t (<Q_t P> - <P Q_t>)); only the anticommuting terms contribute."""
    assert_exact_budget(n, n_half(n, seed), bits_of(coeff) + 1)
    assert not np.any(np.asarray(coeff).imag), 'the gradient kernels form -2 Im <H psi, P psi>, which is <i [H, P]> for a Hermitian H only'
    total = 0j
    for q, c in zip(np.asarray(symp, dtype=bool), coeff):
        total += 1j * complex(c) * (product_expectation([q, row], n, seed) - product_expectation([row, q], n, seed))
    return float(total.real)


def norm2(n, seed):
    """|psi|^2 = prod_q (|a_q|^2 + |b_q|^2) = 2^(n-m) (5/4)^m."""
    out = 1.0
    for e in factors(n, seed)[1]:
        out *= 1.0 + 4.0 ** -int(e)
    return out


def rdm_exact(n, seed, kept):
    """The reduced density matrix over `kept`: the Kronecker product of |phi_q><phi_q| over the kept qubits in ascending order (the
    smallest the leftmost factor) times the norms of the traced ones."""
    assert_exact_budget(n, n_half(n, seed), 0)
    kept = sorted({int(q) for q in kept})
    phi = factor_values(n, seed)
    rho = np.ones((1, 1), dtype=np.complex128)
    for q in kept:
        rho = np.kron(rho, np.outer(phi[q], phi[q].conj()))
    for q in range(n):
        if q not in kept:
            rho = rho * (phi[q] @ phi[q].conj()).real
    return rho


# ---- the basis change ---------------------------------------------------------------------------------------------------------------------
def rotated_factors(n, seed, x_qubits, y_qubits):
    """clongdouble[n, 2]: the single-qubit factors after H (x_qubits) and H S^+ (y_qubits) as the header's butterfly defines them — on a
    Y-qubit first b <- (b.im, -b.re), then a' = (a + b) r, b' = (a - b) r, r the DOUBLE nearest 1 / sqrt 2 — in extended precision (64
    bits of mantissa), so that the closed form's own rounding, 2^-63 per operation, does not count."""
    assert np.finfo(np.longdouble).nmant >= 63, 'the basis-change reference needs an extended-precision long double'
    phi = factor_values(n, seed).astype(np.clongdouble)
    r = np.longdouble(SQRT_HALF)
    for q in sorted(set(x_qubits) | set(y_qubits)):
        a, b = phi[q]
        if q in set(y_qubits):
            b = b.imag - 1j * b.real
        phi[q] = ((a + b) * r, (a - b) * r)
    return phi


def basis_window(n, seed, x_qubits, y_qubits, idx):
    """(the product of the rotated factors at idx, the a-priori bound of the device's deviation from it per component).

    The bound: L x 2 ulp of the amplitude's magnitude for L butterfly layers, an ulp taken as 2^-52 |amplitude|.  A layer is two rounded
    operations per component on the device, a0 +- a1 and the product with r, each within u = 2^-53 of its result's component, so within
    sqrt 2 u of the amplitude as a complex number.  Along a qubit that is still to be rotated the two amplitudes of a pair are, on the
    device too, EXACT multiples of one another (by i^p 2^-e, which commutes with every rounding), so a later layer maps value and error
    alike by (1 +- ratio) r and the relative error is carried on unchanged, never amplified by cancellation: after L layers
    |error| <= 2 L sqrt 2 u |amplitude| < 2 L 2^-52 |amplitude|."""
    idx = np.asarray(idx, dtype=np.int64)
    phi = rotated_factors(n, seed, x_qubits, y_qubits)
    out = np.ones(idx.shape, dtype=np.clongdouble)
    for q in range(n):
        out = out * np.where((idx >> (n - 1 - q)) & 1, phi[q, 1], phi[q, 0])
    layers = len(set(x_qubits) | set(y_qubits))
    return out, (layers * 2 * 2.0 ** -52 * np.abs(out)).astype(np.float64)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------------
def _block_weights(n, seed, prefix, width):
    """The sum of |psi|^2 over the 2^(n - width) indices whose top `width` bits are `prefix`: 4^-k over the chosen halves times the
    norms of the qubits below.  A dyadic number, exact."""
    half = factors(n, seed)[1]
    prefix = np.asarray(prefix, dtype=np.int64)
    k = np.zeros(prefix.shape, dtype=np.int64)
    for q in range(width):
        k += ((prefix >> (width - 1 - q)) & 1) * half[q]
    low = 1.0
    for q in range(width, n):
        low *= 1.0 + 4.0 ** -int(half[q])
    return np.ldexp(low, -2 * k)


def tree_depth(n):
    return max(1, -(-n // RADIX_BITS))


def index_of_uniform(n, seed, u):
    """The sample of every uniform u by the descent of sp_walk (csrc/sample.hip) down the radix-16 sum tree: r = u total; at every
    level the FIRST child with r < acc, acc the running sum of the children; r less the sum before that child; if no child qualifies,
    the last one (every weight here is positive).  The children's sums come from `_block_weights`, not from a tree; they and every
    running sum are exact, r = u total and r - sub are the two rounded operations of sp_walk, done here in the same doubles."""
    assert_exact_budget(n, n_half(n, seed), 0)
    u = np.asarray(u, dtype=np.float64)
    r = u * norm2(n, seed)
    node = np.zeros(u.shape, dtype=np.int64)
    for j in range(tree_depth(n) - 1, -1, -1):
        width = n - RADIX_BITS * j                                    # index bits that name a child of this level
        fan = min(16, 1 << width)
        child = node[:, None] * 16 + np.arange(fan, dtype=np.int64)[None, :]
        acc = np.cumsum(_block_weights(n, seed, child, width), axis=1)
        below = r[:, None] < acc
        k = np.where(below.any(axis=1), np.argmax(below, axis=1), fan - 1)
        sub = acc[np.arange(u.shape[0]), np.maximum(k - 1, 0)]
        r = np.where(k > 0, r - sub, r)
        node = node * 16 + k
    return node


def cumulative_below(n, seed, index):
    """sum_{b < index} |psi[b]|^2 as an exact Fraction: for every set bit of `index`, the block that shares the bits above and has 0 there."""
    from fractions import Fraction
    half = factors(n, seed)[1]
    total = Fraction(0)
    for q in range(n):
        if (index >> (n - 1 - q)) & 1:
            w = Fraction(1)
            for p in range(q):
                if (index >> (n - 1 - p)) & 1:
                    w /= 4 ** int(half[p])
            for p in range(q + 1, n):
                w *= 1 + Fraction(1, 4 ** int(half[p]))
            total += w                                               # qubit q itself at 0: |a_q|^2 = 1
    return total


# ---- the operators of the large cases, every one a function of n ---------------------------------------------------------------------------
def rows_of(n, strings):
    """bool[T, 2n] of strings given as {qubit: 'X' | 'Y' | 'Z'} dictionaries."""
    symp = np.zeros((len(strings), 2 * n), dtype=bool)
    for t, s in enumerate(strings):
        for q, p in s.items():
            symp[t, q], symp[t, n + q] = p in 'XY', p in 'YZ'
    return symp


def matvec_operator(n):
    """(symp, coeff) of eight terms: X on qubit 0 alone and Y_0 Z_mid (two terms sharing an X-part, the top index bit), X on qubit
    n-1 alone, a Y string over every qubit, a Z-only term, the identity, and a pair that cancels.  Coefficients are integers over 8."""
    mid = n // 2
    strings = [{0: 'X'}, {0: 'Y', mid: 'Z'}, {n - 1: 'X'}, {q: 'Y' for q in range(n)}, {0: 'Z', mid: 'Z', n - 1: 'Z'}, {},
               {1: 'X', n - 2: 'X'}, {1: 'X', n - 2: 'X'}]
    coeff = np.array([1.0, 0.375j, -0.5, 0.25, 0.75, -0.125, 0.625, -0.625], dtype=np.complex128)
    return rows_of(n, strings), coeff


def number_operator(n):
    """sum_q (1 - Z_q) / 2: the identity with n / 2 and every Z_q with -1 / 2."""
    return rows_of(n, [{}] + [{q: 'Z'} for q in range(n)]), np.array([n / 2.0] + [-0.5] * n, dtype=np.complex128)


def ansatz_generators(n):
    """(symp, cos, sin): a run of tileable generators (X-parts on few qubits near the low end), one string with X or Y on 13 positions
    (more than a tile holds: a direct pass) and one that touches qubit 0, with exact (cos, sin) pairs."""
    wide = {q: ('X' if q % 2 else 'Y') for q in range(2, min(n - 1, 15))}             # qubits 2 .. 14: 13 positions from 16 qubits on
    strings = [{n - 1: 'Y'}, {n - 2: 'X', n - 1: 'Z'}, {n - 3: 'Y', n - 2: 'Z', 2: 'Z'}, wide, {0: 'Y', n - 1: 'Z'}, {n - 1: 'X', 1: 'Z'}]
    cos_t = np.array([0.5, 0.0, 0.5, 0.0, 0.5, -1.0])
    sin_t = np.array([0.5, 1.0, 0.5, -1.0, 0.5, 0.0])
    return rows_of(n, strings), cos_t, sin_t


def pool_strings(n):
    """Four pool strings: Z_0 (no X-part), Y_0 Z_{n-1} (partner across the top index bit), Z_0 X_{n-1} (across the lowest) — the three
    with a gradient that is not zero on hermitian_operator for both seeds at 27 qubits — and one on three qubits."""
    return rows_of(n, [{0: 'Z'}, {0: 'Y', n - 1: 'Z'}, {0: 'Z', n - 1: 'X'}, {1: 'Y', n - 2: 'X', n - 1: 'Y'}])


def aligned_operator(n, seed):
    """(symp, coeff) of three strings whose expectation in psi(n, seed) is NOT zero — on every qubit the one of X and Y with
    Re or Im of conj(a_q) b_q non-zero — over all qubits, qubit 0 alone, and qubits {0, n // 2, n-1}: an energy that a dropped term,
    a wrong partner index or a wrong Y phase changes."""
    phi = factor_values(n, seed)
    letter = ['X' if (phi[q, 0].conjugate() * phi[q, 1]).real != 0 else 'Y' for q in range(n)]
    strings = [{q: letter[q] for q in range(n)}, {0: letter[0]}, {q: letter[q] for q in (0, n // 2, n - 1)}]
    return rows_of(n, strings), np.array([0.5, -0.25, 0.375], dtype=np.complex128)


_BOUNDARY = {}


def boundary_uniforms(n, seed, top=10):
    """The u = k / 2^20 in (0, 1) for which u total IS the cumulative weight below an index with only its `top` highest bits set: draws
    that sit exactly on a boundary and belong to the upper interval.  The share of the total below such an index depends on the top
    qubits alone: sum over its set bits q of prod_{p < q} f_p / N_p times 1 / N_q, f_p = 1 or 4^-e_p by the bit, N_p = 1 + 4^-e_p."""
    from fractions import Fraction
    top = min(top, n)
    if (n, seed, top) not in _BOUNDARY:
        half = [int(e) for e in factors(n, seed)[1][:top]]
        out = []
        for p in range(1, 1 << top):
            share, prefix = Fraction(0), Fraction(1)
            for q in range(top):
                norm = 1 + Fraction(1, 4 ** half[q])
                if (p >> (top - 1 - q)) & 1:
                    share += prefix / norm
                    prefix *= Fraction(1, 4 ** half[q]) / norm
                else:
                    prefix /= norm
            if (1 << 20) % share.denominator == 0:
                out.append(float(share))
        _BOUNDARY[(n, seed, top)] = np.array(out, dtype=np.float64)
    return _BOUNDARY[(n, seed, top)]


def sampling_uniforms(n, seed, count):
    """count uniforms k / 2^20: 0, the largest below 1, every boundary value of `boundary_uniforms` (at most a quarter), the rest seeded."""
    edge = boundary_uniforms(n, seed)[:count // 4]
    rng = np.random.default_rng(880000 + 100 * n + seed)
    rest = rng.integers(0, 1 << 20, count - 2 - edge.shape[0]) / float(1 << 20)
    return np.concatenate([[0.0, 1.0 - 2.0 ** -20], edge, rest])


def hermitian_operator(n, seed):
    """(symp, coeff) of the gradient cases: the terms of matvec_operator and aligned_operator with real coefficients (the one imaginary
    coefficient taken as its magnitude), so that H is Hermitian, as the gradient kernels assume."""
    a, b = matvec_operator(n), aligned_operator(n, seed)
    coeff = np.concatenate([a[1], b[1]])
    return np.vstack([a[0], b[0]]), (coeff.real + coeff.imag).astype(np.complex128)
