"""CPU: tests/_rdm_oracle.py — the restatement of the reduced density matrix that tests/test_gpu_rdm.py holds csrc/rdm.hip against —
reproduces every answer of the reference stored in tests/golden/rdm.npz (tools/gen_golden_rdm.py): ``get_rdm``,
``partial_trace_over_qubits`` and ``get_entanglement_entropy``, within the two tolerances of the oracle.  Also: its two forms agree
(bit for bit on dyadic amplitudes), and the entry point, its binding and the methods are where the rest of the package expects them."""
import ctypes
import os

import numpy as np
import pytest

import _rdm_oracle as ro
from _integration_doc import header_prototypes

CASES = ro.golden_cases()


def test_golden_file_covers_what_it_should():
    assert {1, 2, 3, 5, 8, 10} == {case['n'] for _, case in CASES}
    assert {'ghz', 'w', 'product', 'gaussian', 'dyadic', 'bra', 'repeated'} == {case['kind'] for _, case in CASES}
    assert any(case['vec_type'] == 'bra' for _, case in CASES)
    assert any(len({tuple(b) for b in case['bits']}) < len(case['bits']) for _, case in CASES), 'no state with repeated basis strings'
    for _, case in CASES:
        n, lists = case['n'], [entry['qubits'] for entry in case['lists']]
        assert [] in lists
        if n >= 3:
            assert any(q != sorted(q) for q in lists) and any(len(set(q)) < len(q) for q in lists), 'no unsorted / repeated list'
            assert any(q and q == list(range(len(q))) for q in lists) and any(q and q == list(range(n - len(q), n)) for q in lists)
            assert any(len(q) > 1 and sorted(set(q)) == list(range(0, n, 2))[:len(set(q))] for q in lists), 'no interleaved list'
        for entry in case['lists']:
            d = 1 << len(set(entry['qubits']))
            assert entry['rdm'].shape == (d, d) and entry['ptrace'].shape == (d, d)
            assert sorted(set(entry['qubits']) | set(entry['traced'])) == list(range(n)) and not set(entry['qubits']) & set(entry['traced'])


@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_restatement_reproduces_the_reference(tag, case):
    n = case['n']
    psi = ro.dense_amplitudes(n, case['bits'], case['amp'])
    for entry in case['lists']:
        tol = ro.entry_tolerance(psi, n, entry['qubits'])
        by_deposit, by_tensordot = ro.rdm_deposit(psi, n, entry['qubits']), ro.rdm_tensordot(psi, n, entry['qubits'])
        for got in (by_deposit, by_tensordot):
            assert np.all(np.abs(got - entry['rdm']) <= tol), (entry['qubits'], np.abs(got - entry['rdm']).max())
            assert np.all(np.abs(got - entry['ptrace']) <= tol), (entry['traced'], np.abs(got - entry['ptrace']).max())
        if case['kind'] == 'dyadic':
            assert np.array_equal(by_deposit, by_tensordot) and np.array_equal(by_deposit, entry['rdm'])
        e_tol = ro.entropy_tolerance(tol)
        print(f'{tag} {entry["qubits"]}: entropy {ro.entropy(by_deposit):.15g} reference {entry["entropy"]:.15g} tolerance {e_tol:.3g}')
        assert abs(ro.entropy(by_deposit) - entry['entropy']) <= e_tol, (entry['qubits'], ro.entropy(by_deposit), entry['entropy'], e_tol)


def test_conventions_known_answers():
    # 3 qubits, psi[b] = b: kept {0} (the top index bit) pairs b with b + 4; kept {2} (the lowest bit) pairs even with odd
    psi = np.arange(8, dtype=np.complex128)
    assert np.array_equal(ro.index_table(3, [0]), [[0, 1, 2, 3], [4, 5, 6, 7]])
    assert np.array_equal(ro.index_table(3, [2]), [[0, 2, 4, 6], [1, 3, 5, 7]])
    assert np.array_equal(ro.index_table(3, [2, 0, 2]), [[0, 2], [1, 3], [4, 6], [5, 7]])          # qubit 0 is the high bit of the row
    assert np.array_equal(ro.rdm_deposit(psi, 3, [0]), [[14, 38], [38, 126]])
    assert np.array_equal(ro.rdm_deposit(psi, 3, []), [[140]]) and np.array_equal(ro.rdm_deposit(psi, 3, [0, 1, 2]), np.outer(psi, psi.conj()))
    ghz = np.zeros(8, dtype=np.complex128)
    ghz[[0, 7]] = np.sqrt(0.5)
    assert np.allclose(ro.rdm_deposit(ghz, 3, [1]), np.eye(2) / 2, rtol=0, atol=1e-15) and abs(ro.entropy(ro.rdm_deposit(ghz, 3, [1])) - np.log(2)) < 1e-14
    for n, k in ((5, 2), (12, 3), (7, 7), (6, 0)):
        pats = ro.kept_patterns(n, k)
        assert pats['low'] == list(range(n - k, n)) and pats['high'] == list(range(k))
        assert all(len(set(p)) == k and p == sorted(p) for p in pats.values())
    assert ro.kept_patterns(12, 3)['interleaved'] == [7, 9, 11] and ro.kept_patterns(4, 3)['interleaved'] == [1, 2, 3]


def test_entry_point_binding_and_methods_are_in_place():
    import symmer_amd
    from symmer_amd import QuantumState, _lib, kernels, utils
    assert callable(QuantumState.get_rdm) and callable(QuantumState.partial_trace_over_qubits)
    assert callable(utils.get_entanglement_entropy) and symmer_amd.get_entanglement_entropy is utils.get_entanglement_entropy
    assert 'get_entanglement_entropy' in symmer_amd.__all__
    assert callable(kernels.rdm_dev) and (kernels.RDM_STREAM, kernels.RDM_TILED) == (1, 2)
    assert len(header_prototypes()['symgpu_rdm']) == 6 and len(_lib.SIGNATURES['symgpu_rdm']) == 6
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), '..', 'include', 'symgpu.h')).read()
    assert '#define SYMGPU_RDM_STREAM 1' in header and '#define SYMGPU_RDM_TILED 2' in header
    if os.path.exists(_lib.LIB_PATH):                               # dlopen only: no GPU call
        lib = ctypes.CDLL(_lib.LIB_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
        assert hasattr(lib, 'symgpu_rdm')


def test_python_layer_refuses_before_any_device_call():
    """The limits are checked on the host, before a vector of 2^n amplitudes is built or a device is looked for."""
    from symmer_amd import QuantumState, get_entanglement_entropy, kernels
    wide = QuantumState(np.zeros((1, 33), dtype=int), [1])
    with pytest.raises(ValueError, match='32'):
        wide.get_rdm([0])
    with pytest.raises(ValueError, match='32'):
        wide.partial_trace_over_qubits(list(range(1, 33)))
    with pytest.raises(ValueError, match='32'):
        get_entanglement_entropy(wide, [0])
    s20 = QuantumState(np.zeros((1, 20), dtype=int), [1])
    with pytest.raises(ValueError, match='12'):
        s20.get_rdm(range(13))
    with pytest.raises(ValueError, match='12'):
        s20.partial_trace_over_qubits(range(7))
    with pytest.raises(ValueError, match='repeated'):
        s20.partial_trace_over_qubits([3, 4, 3])
    with pytest.raises(ValueError, match='outside'):
        s20.get_rdm([20])
    with pytest.raises(ValueError, match='outside'):
        s20.partial_trace_over_qubits([-1])
    s26 = QuantumState(np.zeros((1, 26), dtype=int), [1])
    with pytest.raises(ValueError, match='12'):
        get_entanglement_entropy(s26, range(13))
    with pytest.raises(ValueError, match='outside'):
        get_entanglement_entropy(s20, [25])
    with pytest.raises(ValueError, match='amplitudes'):
        get_entanglement_entropy(np.ones(6), [0])
    for bad in (dict(n_qubits=33, kept=[0]), dict(n_qubits=0, kept=[]), dict(n_qubits=20, kept=range(13)), dict(n_qubits=4, kept=[4]), dict(n_qubits=4, kept=[-1])):
        with pytest.raises(ValueError):
            kernels.rdm_dev(np.ones(2, dtype=complex), **bad)
