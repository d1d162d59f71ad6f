"""GPU: symgpu_basis_change (csrc/basis.hip) — one layer of H and H S^+ on a dense statevector in its two forms — and what stands on it:
kernels.basis_change_dev and QuantumState.measure_state_in_computational_basis.  The tiled form, the direct form and the restatement of
tests/_sample_oracle.py (held against the Kronecker product and the reference's recorded answers by tests/test_sample_oracle.py) agree
byte for byte; <psi|P|psi> = <psi'|Z_new|psi'> within the 1e-12 of tests/test_gpu_expval.py."""
import ctypes
import os

import numpy as np
import pytest

import _sample_oracle as so
from symmer_amd import PauliwordOp, QuantumState, _lib, kernels
from symmer_amd.operators import term_expvals

pytestmark = pytest.mark.gpu
TOL = 1e-12                      # tests/test_gpu_expval.py
GOLDEN = so.golden_cases()


class forced:
    """``with forced('direct'):`` — SYMGPU_BASIS_FORM for the calls inside; None leaves the choice to the library."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.before = os.environ.pop('SYMGPU_BASIS_FORM', None)
        if self.form is not None:
            os.environ['SYMGPU_BASIS_FORM'] = self.form

    def __exit__(self, *exc):
        os.environ.pop('SYMGPU_BASIS_FORM', None)
        if self.before is not None:
            os.environ['SYMGPU_BASIS_FORM'] = self.before
        return False


def masks(n, rng):
    """(name, x qubits, y qubits): empty, all X, all Y, mixed, only the four lowest index bits (the last four qubits), only the highest
    index bit (qubit 0), and every second qubit as Y."""
    qubits = list(range(n))
    kind = rng.integers(0, 3, n)
    return [('empty', [], []), ('all X', qubits, []), ('all Y', [], qubits),
            ('mixed', [q for q in qubits if kind[q] == 1], [q for q in qubits if kind[q] == 2]),
            ('lowest four bits', qubits[-4:][::2], qubits[-4:][1::2]), ('highest bit', [0], []), ('highest bit Y', [], [0]),
            ('every second', [], qubits[::2])]


@pytest.mark.parametrize('n', (1, 4, 5, 12, 13, 16))
def test_tiled_equals_direct_equals_the_restatement(n):
    rng = np.random.default_rng(100 + n)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi[rng.integers(0, 1 << n, max(1, (1 << n) // 8))] = 0           # zeros: their signs are part of the bytes
    for name, xs, ys in masks(n, rng):
        want = so.basis_change(psi, n, xs, ys)
        got = {}
        for form, code in ((None, kernels.BASIS_TILED), ('direct', kernels.BASIS_DIRECT)):
            with kernels.DeviceBuffer.upload(psi) as buf, forced(form):
                ran = kernels.basis_change_dev(buf, n, xs, ys)
                got[form] = buf.download(np.complex128, 1 << n)
            assert ran == (code if xs or ys else 0), (name, form, ran)
        assert got[None].tobytes() == got['direct'].tobytes(), name
        assert got[None].tobytes() == want.tobytes(), (name, np.flatnonzero(got[None] != want)[:5])
        if not xs and not ys:
            assert got[None].tobytes() == psi.tobytes()


@pytest.mark.parametrize('n', (1, 4, 5, 12))
def test_expectation_values_move_with_the_basis(n):
    rng = np.random.default_rng(200 + n)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    state = QuantumState.from_array((psi / np.linalg.norm(psi)).reshape(-1, 1))
    # a first row with X, Y, Z and I mixed, terms it measures (sub-strings of it) and, last, one it does not
    kind = rng.integers(0, 4, n)
    kind[0] = 1
    if n >= 4:
        kind[n - 1] = 3                                              # Z on the last qubit: the layer leaves it alone
    x0, z0 = (kind == 1) | (kind == 2), (kind == 2) | (kind == 3)
    rows = [np.concatenate([x0, z0])]
    for _ in range(6):
        keep = rng.random(n) < 0.6
        rows.append(np.concatenate([x0 & keep, z0 & keep]))
    P = PauliwordOp(np.array(rows), rng.standard_normal(len(rows)))
    psi_new, Z_new = state.measure_state_in_computational_basis(P)
    assert not np.any(Z_new.X_block) and np.array_equal(Z_new.Z_block, P.X_block | P.Z_block) and np.array_equal(Z_new.coeff_vec, P.coeff_vec)
    assert np.max(np.abs(term_expvals(P, state) - term_expvals(Z_new, psi_new))) <= TOL
    assert abs(P.expval(state) - Z_new.expval(psi_new)) <= TOL
    if n in (4, 5):                                                  # a term with X outside the layer: the reference's U P U^+ on the product kernels
        other = np.zeros(2 * n, dtype=bool)
        other[n - 1] = True
        Q =PauliwordOp(np.array(rows + [other]), rng.standard_normal(len(rows) + 1))
        psi_q, Z_q = state.measure_state_in_computational_basis(Q)
        assert abs(Q.expval(state) - Z_q.expval(psi_q)) <= TOL
        assert np.max(np.abs(psi_q.to_dense_matrix - psi_new.to_dense_matrix)) == 0


@pytest.mark.parametrize('k', range(len(GOLDEN)))
def test_golden_cases_through_measure_state(k):
    case = GOLDEN[k]
    n = case['n']
    state, P = QuantumState(case['bits'], case['amp']), PauliwordOp(case['P_symp'].astype(bool), case['P_coeff'])
    psi_new, Z_new = state.measure_state_in_computational_basis(P)
    want_psi = so.dense_amplitudes(n, case['psi_new_bits'], case['psi_new_amp'])
    assert np.max(np.abs(np.asarray(psi_new.to_dense_matrix).reshape(-1) - want_psi)) <= 1e-14
    as_dict = lambda symp, coeff: {tuple(int(v) for v in row): complex(c) for row, c in zip(symp, coeff) if abs(c) > 1e-14}
    got, want = as_dict(Z_new.cleanup().symp_matrix, Z_new.cleanup().coeff_vec), as_dict(case['Z_new_symp'], case['Z_new_coeff'])
    assert set(got) == set(want) and all(abs(got[key] - want[key]) <= 1e-13 for key in want)
    with pytest.raises(AssertionError, match='bra'):
        state.dagger.measure_state_in_computational_basis(P)


def test_refusals():
    lib = _lib.lib()
    psi = np.arange(16, dtype=np.complex128)
    with kernels.DeviceBuffer.upload(psi) as buf:
        form = ctypes.c_int(9)
        before = kernels.counters(('DEV_BLOCKS_LIVE',))
        for args in ((None, 4, 1, 2), (buf.ptr, 0, 0, 0), (buf.ptr, 33, 1, 0), (buf.ptr, 4, 3, 6), (buf.ptr, 4, 16, 0), (buf.ptr, 4, 0, 1 << 40)):
            assert lib.symgpu_basis_change(*args, ctypes.addressof(form)) == _lib.E_INVALID and form.value == 0, args
        assert np.array_equal(kernels.counters(('DEV_BLOCKS_LIVE',)), before)
        assert buf.download(np.complex128, 16).tobytes() == psi.tobytes(), 'a refused call wrote the vector'
        assert lib.symgpu_basis_change(buf.ptr, 4, 8, 1, None) == _lib.OK                      # form may be NULL
        assert buf.download(np.complex128, 16).tobytes() == so.basis_change(psi, 4, [3], [0]).tobytes()
        with pytest.raises(ValueError):
            kernels.basis_change_dev(buf, 4, [1], [1])
        with pytest.raises(ValueError):
            kernels.basis_change_dev(buf, 4, [4], [])
        with pytest.raises(ValueError):
            kernels.basis_change_dev(buf, 5, [0], [])
