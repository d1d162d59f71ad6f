"""NumPy / dict restatement of what csrc/expval.hip computes (include/symgpu.h, symgpu_expval_terms_dev), and an independent dense
evaluator for n <= 4.  For a term with symplectic row (x, z) and Y count y = |x & z|

    <phi|P|psi> = i^y  sum over b in supp psi with b ^ x in supp phi of  conj(phi[b ^ x]) psi[b] (-1)^|z & b|

The sums run in the order the header pins: the rows of psi in chunks of ``chunk_size(S)``, each chunk added to 0 in row order, the chunk
sums added to 0 in ascending order, then i^y as a component swap; the total is 0 + c_0 e_0 + c_1 e_1 + ... with plain complex products.
Every product and sum is written out per component, so that no library routine chooses an order.  States are (bits int[S, n], coeff
complex[S]) and must be CLEAN (``clean_state``): no basis string twice."""
import numpy as np

LDS, GLOBAL = 1, 2


def chunk_size(S):
    c = 64
    while c * 64 < S:
        c *= 2
    return c


def table_cap(S):
    cap = 64
    while cap < 2 * S:
        cap *= 2
    return cap


def expected_form(S_phi, n_qubits):
    """The header's rule: the staged form when S (16 + 8 Wq) + 4 cap <= 65536."""
    wq = (n_qubits + 63) // 64
    return LDS if S_phi * (16 + 8 * wq) + 4 * table_cap(S_phi) <= 65536 else GLOBAL


def clean_state(bits, coeff, zero_threshold=1e-15):
    """Repeated basis strings merged (their coefficients added in order of appearance), |c| <= threshold dropped: what
    PauliwordOp * QuantumState does to a state anyway.  Kept in order of first appearance."""
    bits = np.asarray(bits).astype(np.uint8)
    acc = {}
    for row, c in zip(bits, np.asarray(coeff, dtype=np.complex128)):
        key = row.tobytes()
        acc[key] = acc[key] + c if key in acc else complex(c)
    keep = [(k, c) for k, c in acc.items() if abs(c) > zero_threshold]
    out_bits = np.array([np.frombuffer(k, dtype=np.uint8) for k, _ in keep], dtype=np.uint8).reshape(len(keep), bits.shape[1])
    return out_bits, np.array([c for _, c in keep], dtype=np.complex128)


def _phase(re, im, e):
    return ((re, im), (-im, re), (-re, -im), (im, -re))[e & 3]


def term_elements(symp, phi_bits, phi_c, psi_bits, psi_c):
    """complex128[T]: <phi|P_k|psi> for every row of the symplectic matrix ``symp`` (bool[T, 2n]), phi and psi clean."""
    symp = np.asarray(symp).astype(np.uint8)
    T, n = symp.shape[0], symp.shape[1] // 2
    phi_bits, psi_bits = np.asarray(phi_bits).astype(np.uint8), np.asarray(psi_bits).astype(np.uint8)
    phi_c, psi_c = np.asarray(phi_c, dtype=np.complex128), np.asarray(psi_c, dtype=np.complex128)
    where = {row.tobytes(): j for j, row in enumerate(phi_bits)}
    assert len(where) == phi_bits.shape[0], 'phi is not clean'
    assert len({row.tobytes() for row in psi_bits}) == psi_bits.shape[0], 'psi is not clean'
    S, C = psi_bits.shape[0], chunk_size(psi_bits.shape[0])
    out = np.zeros(T, dtype=np.complex128)
    for k in range(T):
        x, z = symp[k, :n], symp[k, n:]
        moved = psi_bits ^ x
        odd = (psi_bits & z).sum(axis=1) & 1
        hits = [(b, j) for b in range(S) for j in [where.get(moved[b].tobytes())] if j is not None]
        re = im = cre = cim = 0.0
        chunk = 0
        for b, j in hits:
            if b // C != chunk:                                        # a chunk without hits adds 0: left out
                re, im, cre, cim, chunk = re + cre, im + cim, 0.0, 0.0, b // C
            f, c = phi_c[j], psi_c[b]
            pr = f.real * c.real + f.imag * c.imag                    # conj(f) * c
            pi = f.real * c.imag - f.imag * c.real
            cre += -pr if odd[b] else pr
            cim += -pi if odd[b] else pi
        re, im = re + cre, im + cim
        out[k] = complex(*_phase(re, im, int((x & z).sum())))
    return out


def total(coeff, elements):
    """0 + c_0 e_0 + c_1 e_1 + ... as the one wavefront adds it."""
    re = im = 0.0
    for c, e in zip(np.asarray(coeff, dtype=np.complex128), elements):
        re += c.real * e.real - c.imag * e.imag
        im += c.real * e.imag + c.imag * e.real
    return complex(re, im)


def expval(symp, coeff, psi_bits, psi_c):
    """(per-term expectation values float64[T], <psi|H|psi>) of a state given as the caller has it (cleaned here)."""
    bits, c = clean_state(psi_bits, psi_c)
    e = term_elements(symp, bits, c, bits, c)
    return e.real.copy(), total(coeff, e).real


# ---- independent check: Kronecker products, n <= 4 -----------------------------------------------------------------------------------------
_PAULI = {(0, 0): np.eye(2, dtype=np.complex128), (1, 0): np.array([[0, 1], [1, 0]], dtype=np.complex128),
          (0, 1): np.array([[1, 0], [0, -1]], dtype=np.complex128), (1, 1): np.array([[0, -1j], [1j, 0]], dtype=np.complex128)}


def dense_vector(bits, coeff, n):
    """The state as a dense vector: basis string s at index int(s, 2), qubit 0 the most significant bit; repeated strings add."""
    v = np.zeros(1 << n, dtype=np.complex128)
    for row, c in zip(np.asarray(bits).astype(int), np.asarray(coeff, dtype=np.complex128)):
        v[int(''.join(str(i) for i in row), 2) if n else 0] += c
    return v


def dense_term_elements(symp, phi_bits, phi_c, psi_bits, psi_c):
    symp = np.asarray(symp).astype(int)
    n = symp.shape[1] // 2
    assert n <= 4
    phi, psi = dense_vector(phi_bits, phi_c, n), dense_vector(psi_bits, psi_c, n)
    out = np.zeros(symp.shape[0], dtype=np.complex128)
    for k, row in enumerate(symp):
        m = np.eye(1, dtype=np.complex128)
        for q in range(n):
            m = np.kron(m, _PAULI[(row[q], row[n + q])])
        out[k] = phi.conj() @ (m @ psi)
    return out


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
def state_symp(bits):
    """The operator a QuantumState carries: X where the bit is 1, Z where it is 0."""
    bits = np.asarray(bits, dtype=bool)
    return np.hstack([bits, ~bits])


def amplitudes(rng, count, kind):
    """'dyadic': multiples of 1/8 in [-1, 1] per component (every product and sum of a few thousand of them is exact in any order);
    'gaussian': standard normal components."""
    if kind == 'dyadic':
        return (rng.integers(-8, 9, count) + 1j * rng.integers(-8, 9, count)) / 8.0
    return rng.standard_normal(count) + 1j * rng.standard_normal(count)


def random_case(rng, n, T, S, kind):
    """(symp bool[T, 2n], coeff, bits uint8[S, n], amp): S DIFFERENT basis strings that are zero outside m = ceil(log2 S) + 1 support qubits
    (at n >= 63: qubit 0, the word boundaries and the last qubit first); every other term has its x inside the support (it maps about half of
    the states back into it), the others anywhere; z anywhere.  Gaussian states are normalised."""
    m = min(n, max(1, int(np.ceil(np.log2(max(S, 1)))) + 1))
    assert S <= 1 << m, 'not that many distinct strings on so few qubits'
    first = [q for q in (0, 62, 63, 64, 65, 127, 128, n - 1) if q < n] if n >= 63 else []
    first = list(dict.fromkeys(first))[:m]
    rest = [q for q in rng.permutation(n) if q not in first]
    qubits = np.array(first + rest[:m - len(first)], dtype=np.int64)
    codes = rng.choice(1 << m, size=S, replace=False)
    bits = np.zeros((S, n), dtype=np.uint8)
    bits[:, qubits] = (codes[:, None] >> np.arange(m)) & 1
    symp = np.zeros((T, 2 * n), dtype=bool)
    symp[:, :n] = rng.random((T, n)) < min(0.3, 3.0 / n)
    symp[::2, :n] = False
    symp[np.ix_(np.arange(0, T, 2), qubits)] = rng.random(((T + 1) // 2, m)) < 0.3
    symp[:, n:] = rng.random((T, n)) < min(0.5, 8.0 / n)
    symp[:, n + qubits] = rng.random((T, m)) < 0.5
    amp = amplitudes(rng, S, kind)
    amp[amp == 0] = 0.125                                              # a cleanup would drop the string: S is meant
    if kind != 'dyadic':
        amp = amp / np.linalg.norm(amp)
    return symp, amplitudes(rng, T, kind), bits, amp
