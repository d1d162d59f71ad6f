"""CPU: tests/_expval_oracle.py — the restatement of csrc/expval.hip that tests/test_gpu_expval.py holds the kernel against — is itself
held against (1) answers of the REFERENCE (tests/golden/expval.npz, tools/gen_golden_expval.py) within 1e-12: both sides are the
reference's mathematics, the measured gap is 1.4e-15 at most; (2) an independent dense evaluator (Kronecker products) with ``==`` on dyadic
inputs at n <= 4, every one of the 16 Pauli terms at n = 2 included."""
import os

import numpy as np
import pytest

import _expval_oracle as ora

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expval.npz'))
N_CASES = int(GOLD['n_cases'])
TOL = 1e-12


def golden_case(k):
    tag = f'{k:02d}'
    return {name: GOLD[f'{tag}/{name}'] for name in ('n', 'kind', 'product_branch', 'symp', 'coeff', 'psi_bits', 'psi_coeff', 'expval', 'term_expvals')}


def test_goldens_cover_what_they_claim():
    cases = [golden_case(k) for k in range(N_CASES)]
    assert N_CASES >= 20
    assert {int(c['n']) for c in cases} == {1, 2, 3, 5, 8, 63, 64, 65, 130}
    assert {str(c['kind']) for c in cases} == {'dyadic', 'gaussian'}
    assert {bool(c['product_branch']) for c in cases} == {True, False}
    for c in cases:
        bits, amp = ora.clean_state(c['psi_bits'], c['psi_coeff'])
        assert abs(np.linalg.norm(amp) - 1) < 1e-12, 'psi is not normalised'
        assert bool(c['product_branch']) == (c['symp'].shape[0] > c['psi_bits'].shape[0] > 10)
        if int(c['n']) >= 63:
            assert 3 * np.count_nonzero(np.abs(c['term_expvals']) > 1e-14) >= c['symp'].shape[0], 'fewer than a third of the terms land in the support'
    assert any(ora.clean_state(c['psi_bits'], c['psi_coeff'])[0].shape[0] < c['psi_bits'].shape[0] for c in cases), 'no state with repeated strings'


@pytest.mark.parametrize('k', range(N_CASES))
def test_oracle_matches_the_reference(k):
    c = golden_case(k)
    terms, value = ora.expval(c['symp'], c['coeff'], c['psi_bits'], c['psi_coeff'])
    gap_t, gap_v = np.max(np.abs(terms - c['term_expvals'])), abs(value - float(c['expval']))
    print(f'case {k}: largest per-term gap {gap_t:.3e}, expval gap {gap_v:.3e}')
    assert gap_t <= TOL and gap_v <= TOL
    bits, amp = ora.clean_state(c['psi_bits'], c['psi_coeff'])
    assert np.max(np.abs(ora.term_elements(c['symp'], bits, amp, bits, amp).imag)) <= TOL, '<psi|P|psi> is real'


def all_paulis(n):
    return np.array([[(t >> j) & 1 for j in range(2 * n)] for t in range(4 ** n)], dtype=bool)


@pytest.mark.parametrize('n,S_phi,S_psi', [(1, 1, 2), (1, 2, 2), (2, 3, 4), (2, 4, 2), (3, 5, 7), (4, 16, 9), (4, 6, 16)])
def test_oracle_equals_the_dense_evaluator_on_dyadic_inputs(n, S_phi, S_psi):
    rng = np.random.default_rng(100 * n + 10 * S_phi + S_psi)
    symp = all_paulis(n) if n <= 2 else rng.random((40, 2 * n)) < 0.5
    strings = np.array([[(s >> (n - 1 - q)) & 1 for q in range(n)] for s in range(1 << n)], dtype=np.uint8)
    phi_bits, psi_bits = strings[rng.permutation(1 << n)[:S_phi]], strings[rng.permutation(1 << n)[:S_psi]]
    phi_c, psi_c, coeff = ora.amplitudes(rng, S_phi, 'dyadic'), ora.amplitudes(rng, S_psi, 'dyadic'), ora.amplitudes(rng, symp.shape[0], 'dyadic')
    for a_bits, a_c in ((phi_bits, phi_c), (psi_bits, psi_c)):                 # phi != psi, then phi == psi
        got = ora.term_elements(symp, a_bits, a_c, psi_bits, psi_c)
        want = ora.dense_term_elements(symp, a_bits, a_c, psi_bits, psi_c)
        assert np.all(got == want), (got, want)
        assert ora.total(coeff, got) == np.sum(coeff * want)
    assert np.count_nonzero(ora.term_elements(symp, psi_bits, psi_c, psi_bits, psi_c)) > 0


def test_clean_state_merges_and_drops():
    bits = np.array([[0, 1], [1, 1], [0, 1], [1, 0], [1, 1], [1, 0]])
    out_bits, out_c = ora.clean_state(bits, [0.5, 0.25, 0.5j, 1.0, 0.125, -1.0])
    assert out_bits.tolist() == [[0, 1], [1, 1]] and out_c.tolist() == [0.5 + 0.5j, 0.375]


def test_form_rule_and_chunks_as_the_header_states_them():
    assert [ora.expected_form(S, 30) for S in (1, 2047, 2048, 2049)] == [ora.LDS, ora.LDS, ora.LDS, ora.GLOBAL]      # Wq = 1: S <= 2048
    assert [ora.expected_form(S, 70) for S in (1536, 1537)] == [ora.LDS, ora.GLOBAL]
    assert [ora.expected_form(S, 130) for S in (1228, 1229)] == [ora.LDS, ora.GLOBAL]
    assert [ora.chunk_size(S) for S in (1, 64, 65, 4096, 4097, 100000)] == [64, 64, 64, 64, 128, 2048]
    assert [ora.table_cap(S) for S in (1, 32, 33, 512, 513)] == [64, 64, 128, 1024, 2048]


def test_random_case_gives_distinct_strings_and_hits():
    for n, T, S in ((1, 4, 2), (10, 65, 70), (64, 20, 24), (130, 20, 24)):
        symp, coeff, bits, amp = ora.random_case(np.random.default_rng(n), n, T, S, 'dyadic')
        assert ora.clean_state(bits, np.ones(S))[0].shape[0] == S
        e = ora.term_elements(symp, bits, amp, bits, amp)
        assert 3 * np.count_nonzero(e) >= T, 'fewer than a third of the terms are non-zero'
