"""Writes tests/golden/measure_basis.json: answers of the REFERENCE's ``change_of_basis_XY_to_Z`` (symmer/operators/base.py:2474 ff.) and
``QuantumState.measure_state_in_computational_basis`` (base.py:2188-2212).  Build container only: the reference is imported through
``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has neither.  The file holds data only: per case the
state (basis strings, amplitudes), the operator (symplectic rows, coefficients) and the reference's results — the change-of-basis operator
U, the state ``psi_new`` and the operator ``Z_new`` — as rows and [re, im] pairs.

    python tools/gen_golden_measure_basis.py

Cases: 3 to 5 qubits; single terms with X, Y, Z and I mixed; operators whose terms are all measured by the first row's layer (so Z_new has
I and Z only) and operators with a term the layer does not diagonalise; sparse and dense states, Gaussian and dyadic amplitudes.
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'measure_basis.json')


def _load_shim():
    spec = importlib.util.spec_from_file_location('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)


def pairs(c):
    return [[float(np.real(v)), float(np.imag(v))] for v in np.asarray(c, dtype=np.complex128).reshape(-1)]


def all_strings(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(int).reshape(1 << n, n)


CASES = [
    # (n, state kind, Pauli strings, coefficients)
    (3, 'dense', ['XYZ'], [1.0]),
    (3, 'dyadic', ['YYI'], [1.0]),
    (3, 'sparse', ['ZIZ', 'IZI'], [0.5, -0.25]),
    (4, 'dense', ['XIYZ', 'XIII', 'IIYZ', 'IZIZ'], [0.75, -0.5, 0.25, 1.5]),
    (4, 'sparse', ['YXXY', 'YIIY', 'IXXI'], [1.0, 2.0, -3.0]),
    (4, 'dense', ['XXII', 'IIZZ', 'ZZII', 'IXXI'], [1.0, 0.5, -0.5, 0.125]),
    (5, 'dense', ['XYZIX', 'IYIIX', 'XIZII', 'IIIZI'], [0.3, -0.7, 1.1, 0.9]),
    (5, 'dyadic', ['YIYIY', 'XIIII'], [1.0, 1.0]),
    (5, 'sparse', ['IIIII', 'IXIYI'], [2.0, -1.0]),
]


def make_state(rng, n, kind):
    if kind == 'dense':
        amp = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
        return all_strings(n), amp / np.linalg.norm(amp)
    if kind == 'dyadic':
        amp = (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / 8.0
        amp[0] = 1.0
        return all_strings(n), amp / np.linalg.norm(amp)
    S = max(2, (1 << n) // 3)
    bits = all_strings(n)[np.sort(rng.choice(1 << n, size=S, replace=False))]
    amp = rng.standard_normal(S) + 1j * rng.standard_normal(S)
    return bits, amp / np.linalg.norm(amp)


def main():
    _load_shim()
    np.product = np.prod
    from symmer.operators import QuantumState as RefState, PauliwordOp as RefOp
    from symmer.operators.base import change_of_basis_XY_to_Z as ref_change
    from symmer import process
    process.method = 'single_thread'
    rng = np.random.default_rng(20261021)
    out = []
    for n, kind, strings, coeffs in CASES:
        bits, amp = make_state(rng, n, kind)
        psi, P = RefState(bits, amp), RefOp.from_list(strings, coeffs)
        U = ref_change(P)
        psi_new, Z_new = psi.measure_state_in_computational_basis(P)
        out.append({'n': n, 'kind': kind, 'bits': bits.astype(int).tolist(), 'amp': pairs(amp),
                    'P_symp': P.symp_matrix.astype(int).tolist(), 'P_coeff': pairs(P.coeff_vec),
                    'U_symp': U.symp_matrix.astype(int).tolist(), 'U_coeff': pairs(U.coeff_vec),
                    'psi_new_bits': np.asarray(psi_new.state_matrix).astype(int).tolist(), 'psi_new_amp': pairs(psi_new.state_op.coeff_vec),
                    'Z_new_symp': Z_new.symp_matrix.astype(int).tolist(), 'Z_new_coeff': pairs(Z_new.coeff_vec)})
        print(f'n = {n} {kind:6s} {strings}: U {U.n_terms} terms, psi_new {psi_new.n_terms} terms, Z_new {Z_new.n_terms} terms')
    with open(OUT, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
