"""Writes tests/golden/expval.npz: answers of the REFERENCE's ``PauliwordOp.expval`` and ``single_term_expval``
(symmer/operators/base.py:796-819, 2438-2471).  Build container only: the reference is imported through ``oracle/tools/ref_shim.py``
(by path), which needs the reference checkout; the GPU box has neither.  The file holds data only: per case the inputs (symplectic
matrix, term coefficients, the state's basis strings and amplitudes) and the reference's ``expval`` and per-term values.

    python tools/gen_golden_expval.py

Cases: n in {1, 2, 3, 5, 8, 63, 64, 65, 130}, normalised psi, dyadic and Gaussian coefficients, both branches of ``expval`` (the
bra x op x ket product when n_terms > psi.n_terms > 10, term by term otherwise), one state given with repeated basis strings.  At
n >= 63 the state's support is confined to five or six qubits (the word boundaries 62 .. 65 among them where they exist) and x is drawn on
those qubits only, so that most terms map the support onto itself; z is drawn everywhere.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'expval.npz')

# normalised dyadic amplitudes: S states of equal modulus 2^-k
DYADIC_AMPLITUDES = {1: [1, -1, 1j, -1j], 2: [(a + b * 1j) / 2 for a in (1, -1) for b in (1, -1)], 4: [.5, -.5, .5j, -.5j],
                     8: [(a + b * 1j) / 4 for a in (1, -1) for b in (1, -1)], 16: [.25, -.25, .25j, -.25j],
                     32: [(a + b * 1j) / 8 for a in (1, -1) for b in (1, -1)]}
SUPPORT_QUBITS = {63: [0, 7, 30, 41, 62], 64: [0, 7, 30, 62, 63], 65: [0, 7, 62, 63, 64], 130: [0, 62, 63, 64, 65, 129]}


def _load_shim():
    spec = importlib.util.spec_from_file_location('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)


def distinct_strings(rng, S, n, qubits):
    """S different basis strings of n qubits that are zero outside ``qubits``."""
    assert S <= 1 << len(qubits)
    codes = rng.choice(1 << len(qubits), size=S, replace=False)
    bits = np.zeros((S, n), dtype=int)
    for j, q in enumerate(qubits):
        bits[:, q] = (codes >> j) & 1
    return bits


def make_case(rng, n, T, S, kind, dup=False):
    qubits = list(range(n)) if n < 63 else SUPPORT_QUBITS[n]
    bits = distinct_strings(rng, S, n, qubits)
    symp = np.zeros((T, 2 * n), dtype=bool)
    symp[:, qubits] = rng.random((T, len(qubits))) < (0.5 if n < 63 else 0.3)
    symp[:, n:] = rng.random((T, n)) < (0.5 if n < 63 else 0.1)
    symp[:, [n + q for q in qubits]] = rng.random((T, len(qubits))) < 0.5
    if T == 4 ** n:                                                    # every Pauli term once
        symp = np.array([[(t >> j) & 1 for j in range(2 * n)] for t in range(T)], dtype=bool)
    if kind == 'dyadic':
        coeff = (rng.integers(-8, 9, T) + 1j * rng.integers(-8, 9, T)) / 8.0
        amp = rng.choice(np.array(DYADIC_AMPLITUDES[S], dtype=complex), size=S)
    else:
        coeff = rng.standard_normal(T) + 1j * rng.standard_normal(T)
        amp = rng.standard_normal(S) + 1j * rng.standard_normal(S)
        if dup:                                                        # every third string once more, with another amplitude
            again = np.arange(0, S, 3)
            bits = np.vstack([bits, bits[again]])
            extra = rng.standard_normal(again.size) + 1j * rng.standard_normal(again.size)
            merged = amp.copy()
            merged[again] += extra
            scale = np.linalg.norm(merged)
            amp = np.concatenate([amp, extra]) / scale
        else:
            amp = amp / np.linalg.norm(amp)
    return n, symp, coeff, bits, amp, kind


def main():
    _load_shim()
    from symmer.operators import PauliwordOp as RefOp, QuantumState as RefState
    from symmer.operators.base import single_term_expval as ref_single
    from symmer import process
    process.method = 'single_thread'
    rng = np.random.default_rng(20241019)
    shapes = [  # (n, T, S, kind, duplicates)
        (1, 4, 1, 'dyadic', False), (1, 3, 2, 'gaussian', False), (2, 16, 2, 'dyadic', False), (2, 7, 4, 'gaussian', False),
        (3, 12, 4, 'dyadic', False), (3, 9, 8, 'gaussian', False), (5, 10, 16, 'dyadic', False), (5, 30, 16, 'dyadic', False),
        (5, 25, 12, 'gaussian', False), (5, 8, 20, 'gaussian', True), (8, 20, 32, 'dyadic', False), (8, 40, 32, 'dyadic', False),
        (8, 60, 30, 'gaussian', False), (8, 25, 100, 'gaussian', True), (63, 25, 16, 'dyadic', False), (63, 24, 20, 'gaussian', False),
        (64, 25, 8, 'dyadic', False), (64, 30, 24, 'gaussian', False), (65, 25, 32, 'dyadic', False), (65, 40, 20, 'gaussian', False),
        (130, 25, 16, 'dyadic', False), (130, 40, 30, 'gaussian', True)]
    out = {'n_cases': np.int64(len(shapes))}
    for k, shape in enumerate(shapes):
        n, symp, coeff, bits, amp, kind = make_case(rng, *shape)
        H, psi = RefOp(symp, coeff), RefState(bits, amp)
        product_branch = H.n_terms > psi.n_terms and psi.n_terms > 10
        value = H.expval(psi)
        terms = np.array([ref_single(H[j], psi) for j in range(H.n_terms)], dtype=np.float64)
        assert abs(np.linalg.norm(psi.cleanup().state_op.coeff_vec) - 1) < 1e-12
        assert abs(np.sum(terms * coeff).real - value) < 1e-12, (np.sum(terms * coeff).real, value)
        tag = f'{k:02d}'
        out[f'{tag}/n'], out[f'{tag}/kind'], out[f'{tag}/product_branch'] = np.int64(n), np.array(kind), np.bool_(product_branch)
        out[f'{tag}/symp'], out[f'{tag}/coeff'] = symp, coeff.astype(np.complex128)
        out[f'{tag}/psi_bits'], out[f'{tag}/psi_coeff'] = bits.astype(np.uint8), amp.astype(np.complex128)
        out[f'{tag}/expval'], out[f'{tag}/term_expvals'] = np.float64(np.real(value)), terms
        print(f'case {tag}: n = {n:3d} T = {symp.shape[0]:3d} S = {bits.shape[0]:3d} {kind:8s} '
              f'{"product" if product_branch else "terms  "} branch, {np.count_nonzero(np.abs(terms) > 1e-14)} non-zero terms, expval {np.real(value):+.6f}')
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
