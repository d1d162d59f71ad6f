"""NumPy restatement of the reduced density matrix (include/symgpu.h, section f9) that tests/test_gpu_rdm.py holds csrc/rdm.hip against,
itself held against the reference's stored answers (tests/golden/rdm.npz, tools/gen_golden_rdm.py) by tests/test_rdm_oracle.py.

Two forms, which must agree: ``rdm_tensordot`` — the reference's own formula, a ``tensordot`` of the ``[2] * n`` amplitudes with their
conjugate over the traced axes — and ``rdm_deposit`` — the header's: with qubit q at bit n-1-q of a basis index, the kept bits KM and the
traced bits TM, b(a, e) = dep(a, KM) | dep(e, TM), M[a][e] = psi[b(a, e)], rho = M M^+.

The two tolerances.  ``entry_tolerance``: with m = 2^(n-k) and r_a the 2-norm of row a of M,
    tol[a][a'] = 4 (m + 8) 2^-53 r_a r_a'
— the worst-case rounding of a length-m complex inner product in any summation order, with or without contraction (each of the two real
sums of 2m products errs by at most gamma_{2m} sum |p q| <= gamma_{2m} r_a r_a' by Cauchy-Schwarz), with a factor 2 over the textbook
bound.  ``entropy_tolerance``: eigenvalues of two Hermitian matrices that differ by E differ by at most ||E||_2 <= ||tol||_F = delta
(Weyl); |x ln x - y ln y| <= -delta ln delta for |x - y| <= delta <= 1/2; there are 2^k eigenvalues: 2^k (-delta ln delta)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rdm.npz')


def kept_of(n, qubits):
    """The kept qubits as the call takes them: de-duplicated, ascending."""
    kept = sorted({int(q) for q in qubits})
    assert all(0 <= q < n for q in kept)
    return kept


def deposit(values, mask):
    """The bits of every value, lowest first, to the set bit positions of ``mask``, lowest first."""
    values = np.asarray(values, dtype=np.uint64)
    out, at = np.zeros_like(values), 0
    for pos in range(64):
        if (mask >> pos) & 1:
            out |= ((values >> np.uint64(at)) & np.uint64(1)) << np.uint64(pos)
            at += 1
    return out


def index_table(n, qubits):
    """b(a, e) as an int64 [2^k, 2^(n-k)] table."""
    kept = kept_of(n, qubits)
    k = len(kept)
    KM = sum(1 << (n - 1 - q) for q in kept)
    TM = ((1 << n) - 1) & ~KM
    rows, cols = deposit(np.arange(1 << k), KM), deposit(np.arange(1 << (n - k)), TM)
    return (rows[:, None] | cols[None, :]).astype(np.int64)


def matrix_M(psi, n, qubits):
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    assert psi.shape[0] == 1 << n
    return psi[index_table(n, qubits)]


def rdm_deposit(psi, n, qubits):
    M = matrix_M(psi, n, qubits)
    return M @ M.conj().T


def rdm_tensordot(psi, n, qubits):
    kept = kept_of(n, qubits)
    traced = [q for q in range(n) if q not in kept]
    t = np.asarray(psi, dtype=np.complex128).reshape([2] * n)
    d = 1 << len(kept)
    return np.tensordot(t, t.conj(), axes=(traced, traced)).reshape(d, d)


def entry_tolerance(psi, n, qubits):
    M = matrix_M(psi, n, qubits)
    r = np.sqrt(np.sum(M.real ** 2 + M.imag ** 2, axis=1))
    return 4.0 * (M.shape[1] + 8) * 2.0 ** -53 * np.outer(r, r)


def entropy(rho):
    w = np.linalg.eigvalsh(rho)
    w = w[w > 0]
    return float(-np.sum(w * np.log(w)))


def entropy_tolerance(tol):
    delta = float(np.linalg.norm(tol))
    assert delta <= 0.5, delta
    return 0.0 if delta == 0.0 else tol.shape[0] * (-delta * np.log(delta))


def dense_amplitudes(n, bits, amp):
    """The 2^n amplitudes of a state given as basis strings and amplitudes, as ``QuantumState.to_dense_matrix`` lays them out: string s at
    index int(s, 2), repeated strings added."""
    index = np.asarray(bits, dtype=np.int64) @ (1 << np.arange(n - 1, -1, -1, dtype=np.int64))
    out = np.zeros(1 << n, dtype=np.complex128)
    np.add.at(out, index, np.asarray(amp, dtype=np.complex128))
    return out


def golden_cases():
    """[(tag, case)]: case = {n, kind, vec_type, bits, amp, lists: [{qubits, traced, rdm, ptrace, entropy}]}."""
    z = np.load(GOLDEN)
    cases = []
    for c in range(int(z['n_cases'])):
        tag = f'{c:02d}'
        case = {'n': int(z[f'{tag}/n']), 'kind': str(z[f'{tag}/kind']), 'vec_type': str(z[f'{tag}/vec_type']), 'bits': z[f'{tag}/bits'],
                'amp': z[f'{tag}/amp']}
        case['lists'] = [{'qubits': [int(q) for q in z[f'{tag}/{s}/qubits']], 'traced': [int(q) for q in z[f'{tag}/{s}/traced']],
                          'rdm': z[f'{tag}/{s}/rdm'], 'ptrace': z[f'{tag}/{s}/ptrace'], 'entropy': float(z[f'{tag}/{s}/entropy'])}
                         for s in range(int(z[f'{tag}/n_lists']))]
        cases.append((f'{tag}-n{case["n"]}-{case["kind"]}', case))
    return cases


def kept_patterns(n, k):
    """The three kept sets to look at: the k qubits whose bits are the LOWEST index bits, the HIGHEST, and interleaved from the lowest
    bit up (every other qubit while they last, then the next free ones)."""
    low, high = list(range(n - k, n)), list(range(k))
    inter = list(range(n - 1, -1, -2))[:k]
    inter += [q for q in range(n - 1, -1, -1) if q not in inter][:k - len(inter)]
    return {'low': low, 'high': high, 'interleaved': sorted(inter)}
