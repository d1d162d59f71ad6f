"""CPU: tests/_noncon_oracle.py — the restatement of the noncontextual objective that tests/test_gpu_noncon.py holds csrc/noncon.hip
against — reproduces every answer of the reference stored in tests/golden/noncon_solve.npz (tools/gen_golden_noncon_solve.py): the energy
of every case from the recorded G_indices, C_indices and pauli_mult_signs, and nu where the minimiser is unique.  Also: the new class and
the two entry points are where the rest of the package expects them."""
import ctypes
import os

import numpy as np
import pytest

import _noncon_oracle as no
from _integration_doc import header_prototypes

CASES = no.golden_cases()


def test_golden_file_covers_what_it_should():
    assert len(CASES) >= 35
    assert {3, 8, 13} <= {int(case['n']) for _, case in CASES}
    for _, case in CASES:
        T = case['symp'].shape[0]
        assert case['symp'].shape == (T, 2 * int(case['n'])) and case['coeff'].shape == (T,)
        assert case['G_indices'].shape == (T, case['generators'].shape[0]) and case['C_indices'].shape == (T, case['cliques'].shape[0])
        assert np.all(np.count_nonzero(case['C_indices'], axis=1) <= 1), 'a recorded term has more than one clique bit'
        assert set(np.unique(case['pauli_mult_signs'])) <= {-1, 1}
    assert any(case['cliques'].shape[0] == 0 and case['symp'].shape[0] > 4 for _, case in CASES), 'no all-commuting case'
    assert any(case['cliques'].shape[0] > 0 and np.count_nonzero(~case['C_indices'].any(axis=1)) == 1 for _, case in CASES), 'no case without S0 terms'
    with_state = [case for _, case in CASES if 'ref_state' in case]
    assert len(with_state) == 5
    assert any(np.all(case['sector'] != 0) for case in with_state) and any(np.any(case['sector'] == 0) for case in with_state)
    assert max(case['generators'].shape[0] for _, case in CASES) >= 11 and max(case['symp'].shape[0] for _, case in CASES) >= 1500


@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_restated_objective_reproduces_reference_energy(tag, case):
    energy, nu, energies = no.solve(case['coeff'], case['G_indices'], case['C_indices'], case['pauli_mult_signs'], case.get('sector'))
    tol = no.tolerance(case['coeff'].real)
    assert abs(energy - float(case['energy'])) <= tol, (energy, float(case['energy']), tol)
    assert bool(case['unique']) == no.unique_minimum(energies, case['coeff'])
    if case['unique']:
        assert np.array_equal(nu, case['nu']), 'the tie rule / bit order of the restatement is not the reference\'s'
    if 'sector' in case:
        fixed = case['sector'] != 0
        assert np.array_equal(case['nu'][fixed], case['sector'][fixed])


@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_restated_phase_rule_reproduces_reference_signs(tag, case):
    gens = np.vstack([case['generators'], case['cliques']])
    selection = np.hstack([case['G_indices'], case['C_indices']]).astype(bool)
    assert np.array_equal(no.product_signs(case['symp'], gens, selection), case['pauli_mult_signs'])


def test_restated_phase_rule_known_answers():
    sym = lambda labels: np.array([[ch in 'XY' for ch in lab] + [ch in 'ZY' for ch in lab] for lab in labels])
    gens = sym(['XI', 'ZI', 'YY', 'XX'])
    terms = sym(['YI', 'YI', 'ZZ', 'II', 'XI'])
    selection = np.array([[1, 1, 0, 0],      # X Z = -iY
                          [0, 1, 1, 0],      # another row
                          [0, 0, 1, 1],      # (YY)(XX) = (-iZ)(-iZ) = -ZZ
                          [0, 0, 0, 0],      # the empty product
                          [1, 0, 0, 0]], dtype=bool)
    assert list(no.product_signs(terms, gens, selection)) == [0, 0, -1, 1, 1]


def test_enough_cases_have_a_unique_minimiser():
    n_unique = sum(bool(case['unique']) for _, case in CASES)
    assert 4 * n_unique >= 3 * len(CASES), f'{n_unique} of {len(CASES)}'


def test_tie_rule_known_answers():
    # one clique whose two terms share generator 0 (bit 1 of m for f = 2), nothing else uses it: E(m) = E(m ^ 2) exactly
    coeff, mask, clique = np.array([0.75, -1.5, 0.5]), np.array([2, 2, 1], dtype=np.uint64), np.array([0, 0, -1], dtype=np.int32)
    energies = no.landscape(coeff, mask, clique, 2, 1)
    assert np.array_equal(energies, [-0.25, -1.25, -0.25, -1.25])
    assert no.best_mask(energies) == 3 and list(no.nu_of_mask(3, 2)) == [-1, -1] and list(no.nu_of_mask(1, 2)) == [1, -1]
    # no terms: every energy is 0, the reference's first assignment (all -1) is the largest mask
    assert no.best_mask(no.landscape(np.zeros(0), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32), 3, 0)) == 7
    assert no.best_mask(no.landscape(np.zeros(0), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32), 0, 0)) == 0


def test_class_and_entry_points_are_in_place():
    import symmer_amd
    from symmer_amd import NoncontextualOp, NoncontextualSolver, PauliwordOp, _lib, kernels, operators
    assert issubclass(NoncontextualOp, PauliwordOp) and operators.NoncontextualOp is NoncontextualOp
    assert {'NoncontextualOp', 'NoncontextualSolver'} <= set(symmer_amd.__all__)
    for name in ('from_PauliwordOp', 'from_hamiltonian', 'noncontextual_generators', 'noncontextual_reconstruction',
                 'get_symmetry_contributions', 'get_energy', 'solve', 'noncon_state'):
        assert callable(getattr(NoncontextualOp, name))
    assert callable(NoncontextualSolver.energy_via_brute_force) and callable(NoncontextualSolver.energy_via_relaxation)
    assert callable(kernels.noncon_signs_dev) and callable(kernels.noncon_search)
    protos = header_prototypes()
    assert len(protos['symgpu_noncon_signs_dev']) == 5 and len(protos['symgpu_noncon_search']) == 10
    assert len(_lib.SIGNATURES['symgpu_noncon_signs_dev']) == 5 and len(_lib.SIGNATURES['symgpu_noncon_search']) == 10
    if os.path.exists(_lib.LIB_PATH):                               # dlopen only: no GPU call
        lib = ctypes.CDLL(_lib.LIB_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
        assert hasattr(lib, 'symgpu_noncon_signs_dev') and hasattr(lib, 'symgpu_noncon_search')
