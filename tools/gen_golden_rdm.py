"""Writes tests/golden/rdm.npz: answers of the REFERENCE's ``QuantumState.get_rdm``, ``QuantumState.partial_trace_over_qubits``
(symmer/operators/base.py:2025-2054) and ``get_entanglement_entropy`` (symmer/utils.py:78-94).  Build container only: the reference is
imported through ``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has neither.  The file holds
data only: per case the state (basis strings, amplitudes, ket or bra) and, per qubit list, the list as given, the reference's ``get_rdm``
of it, the sorted complement, the reference's ``partial_trace_over_qubits`` of that complement, and the reference's entropy.

    python tools/gen_golden_rdm.py

The reference calls ``np.product``, which NumPy 2.2 no longer has: this script sets ``np.product = np.prod`` before the first call (the
two were the same function); with that alias the reference runs unchanged.

Cases: n in {1, 2, 3, 5, 8, 10}; GHZ, W and product states; dense Gaussian and dyadic amplitudes; a bra; a state given with repeated
basis strings; per state the kept sets at the top, at the bottom and interleaved, the empty set, all qubits (n <= 5), and one list given
unsorted and with a repeat.  No kept set has more than 6 qubits.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'rdm.npz')


def _load_shim():
    spec = importlib.util.spec_from_file_location('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)


def all_strings(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(int).reshape(1 << n, n)


def make_state(rng, n, kind):
    """(bits [S, n], amplitudes [S], vec_type)."""
    if kind == 'ghz':
        return np.array([[0] * n, [1] * n]), np.array([1, 1]) / np.sqrt(2), 'ket'
    if kind == 'w':
        return np.eye(n, dtype=int), np.ones(n) / np.sqrt(n), 'ket'
    if kind == 'product':
        amp = np.ones(1, dtype=complex)
        for _ in range(n):
            one = rng.standard_normal(2) + 1j * rng.standard_normal(2)
            amp = np.kron(amp, one / np.linalg.norm(one))
        return all_strings(n), amp, 'ket'
    if kind == 'dyadic':                                               # not normalised
        return all_strings(n), (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / 8.0, 'ket'
    if kind in ('gaussian', 'bra'):
        amp = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
        return all_strings(n), amp / np.linalg.norm(amp), 'bra' if kind == 'bra' else 'ket'
    assert kind == 'repeated'                                          # every third string once more, with another amplitude
    S = max(2, (1 << n) // 2)
    bits = all_strings(n)[rng.choice(1 << n, size=S, replace=False)]
    amp = rng.standard_normal(S) + 1j * rng.standard_normal(S)
    again = np.arange(0, S, 3)
    extra = rng.standard_normal(again.size) + 1j * rng.standard_normal(again.size)
    merged = amp.copy()
    merged[again] += extra
    return np.vstack([bits, bits[again]]), np.concatenate([amp, extra]) / np.linalg.norm(merged), 'ket'


def qubit_lists(n):
    k = min(6, max(1, n // 2))
    top, bottom, inter = list(range(k)), list(range(n - k, n)), list(range(0, n, 2))[:6]
    lists = [[], top, bottom, inter, inter[::-1] + inter[:1], [n - 1]]
    if n <= 5:
        lists.append(list(range(n)))
    if n >= 3:
        lists.append([n - 1, 0, n - 2, 0])
    seen, out = set(), []
    for q in lists:
        if tuple(q) not in seen:
            seen.add(tuple(q))
            out.append(q)
    return out


def main():
    _load_shim()
    np.product = np.prod                                               # see the docstring
    from symmer.operators import QuantumState as RefState
    from symmer.utils import get_entanglement_entropy as ref_entropy
    from symmer import process
    process.method = 'single_thread'
    rng = np.random.default_rng(20261020)
    shapes = [(n, kind) for n in (1, 2, 3, 5, 8, 10) for kind in ('ghz', 'w', 'product', 'gaussian', 'dyadic')]
    shapes += [(3, 'bra'), (8, 'bra'), (3, 'repeated'), (5, 'repeated'), (10, 'repeated')]
    out = {'n_cases': np.int64(len(shapes))}
    for c, (n, kind) in enumerate(shapes):
        bits, amp, vec_type = make_state(rng, n, kind)
        psi = RefState(bits, amp, vec_type=vec_type)
        tag = f'{c:02d}'
        lists = qubit_lists(n)
        out[f'{tag}/n'], out[f'{tag}/kind'], out[f'{tag}/vec_type'] = np.int64(n), np.array(kind), np.array(vec_type)
        out[f'{tag}/bits'], out[f'{tag}/amp'], out[f'{tag}/n_lists'] = bits.astype(np.uint8), amp.astype(np.complex128), np.int64(len(lists))
        for s, qubits in enumerate(lists):
            traced = sorted(set(range(n)) - set(qubits))
            rdm, ptrace = np.asarray(psi.get_rdm(qubits)), np.asarray(psi.partial_trace_over_qubits(traced))
            d = 1 << len(set(qubits))
            assert rdm.shape == (d, d) and ptrace.shape == (d, d)
            out[f'{tag}/{s}/qubits'], out[f'{tag}/{s}/traced'] = np.array(qubits, dtype=np.int64), np.array(traced, dtype=np.int64)
            out[f'{tag}/{s}/rdm'], out[f'{tag}/{s}/ptrace'] = rdm.astype(np.complex128), ptrace.astype(np.complex128)
            out[f'{tag}/{s}/entropy'] = np.float64(ref_entropy(psi, qubits))
        print(f'case {tag}: n = {n:2d} {kind:8s} {vec_type} S = {bits.shape[0]:4d}, {len(lists)} qubit lists, '
              f'entropies {[round(float(out[f"{tag}/{s}/entropy"]), 4) for s in range(len(lists))]}')
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
