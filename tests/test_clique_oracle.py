"""CPU: tests/_clique_oracle.py — the restatement that tests/test_gpu_clique.py holds csrc/clique.hip against — reproduces every answer of
the reference stored in tests/golden/clique_cover.npz (tools/gen_golden_clique_cover.py): the QWC table, and for the three relations and
both strategies the clique of every term and the order of the terms inside each clique."""
import numpy as np
import pytest

import _clique_oracle as co

CASES = co.golden_cases()


def test_golden_file_covers_what_it_should():
    assert len(CASES) >= 12
    ns = {case['n'] for _, case in CASES}
    assert {2, 3, 10, 130} <= ns
    for _, case in CASES:
        T = case['symp'].shape[0]
        assert 5 <= T <= 200 and case['symp'].shape[1] == 2 * case['n']
        assert len(np.unique(case['symp'], axis=0)) == T and len(np.unique(np.abs(case['coeff']))) == T
        assert all((rel, strat) in case for rel in co.RELATIONS for strat in co.STRATEGIES)
    assert any(not case['symp'][t].any() for _, case in CASES for t in range(case['symp'].shape[0])), 'no case holds the identity row'


@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_qwc_table_matches_reference(tag, case):
    got = co.relation_table(case['symp'], case['symp'], 'QWC')
    assert np.array_equal(got, case['qwc'])
    assert got.diagonal().all()                                        # a term qubit-wise commutes with itself
    # C and AC are complementary, and C is the symplectic form
    n = case['n']
    x, z = case['symp'][:, :n].astype(int), case['symp'][:, n:].astype(int)
    commute = (x @ z.T + z @ x.T) % 2 == 0
    assert np.array_equal(co.relation_table(case['symp'], case['symp'], 'C'), commute)
    assert np.array_equal(co.relation_table(case['symp'], case['symp'], 'AC'), ~commute)


@pytest.mark.parametrize('strategy', co.STRATEGIES)
@pytest.mark.parametrize('relation', co.RELATIONS)
@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_first_fit_matches_reference(tag, case, relation, strategy):
    ref_colour, ref_members = case[(relation, strategy)]
    order = co.term_order(case['symp'], case['coeff'], relation, strategy)
    colours, n_colours = co.colouring(case['symp'], order, relation)
    assert n_colours == ref_colour.max() + 1
    assert np.array_equal(colours, ref_colour)
    assert sum(co.cliques_in_order(colours, order), []) == list(ref_members)


def test_first_fit_known_answers():
    # a path 0 - 1 - 2 - 3 of CONFLICTS (related = everything else), walked in index order: colours alternate
    related = np.ones((4, 4), dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 3)):
        related[a, b] = related[b, a] = False
    assert list(co.first_fit(related, np.arange(4))[0]) == [0, 1, 0, 1]
    # walked from the middle: 1, 2 take colours 0, 1; 0 conflicts with 1 only -> colour 1; 3 conflicts with 2 only -> colour 0
    assert list(co.first_fit(related, np.array([1, 2, 0, 3]))[0]) == [1, 0, 1, 0]
    # nothing related: one colour each, in walking order
    assert list(co.first_fit(np.zeros((3, 3), dtype=bool), np.array([2, 0, 1]))[0]) == [1, 2, 0]
