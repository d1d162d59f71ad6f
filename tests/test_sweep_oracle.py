"""CPU: the oracles of the noncontextual sweep (tests/_sweep_oracle.py) against the reference's recorded answers
(tests/golden/noncon_sweep.npz, tools/gen_golden_noncon_sweep.py) and against each other.  ``ref_sweep`` is the reference loop (padded
adjacency matrix, unique rows); ``rule_sweep`` is the rule csrc/noncon_sweep.hip implements (labels SYM / clique, word-wide tests).
tests/test_gpu_noncon_sweep.py holds the kernel against both."""
import re
import os

import numpy as np
import pytest

from symmer_amd import _lib
import _sweep_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = so.golden()
CASES = so.golden_cases(GOLD)


def test_golden_file_holds_the_cases_the_generator_promises():
    kinds = [kind for _, kind, _, _ in CASES]
    assert kinds.count('dfs') >= 10 and kinds.count('sweep') >= 8
    sizes = [len(coeff) for _, _, _, coeff in CASES]
    assert max(sizes) == 631 and 156 in sizes and 300 in sizes
    for tag, kind, symp, coeff in CASES:
        mags = np.sort(np.abs(coeff))
        assert np.all(np.diff(mags) > 0), f'case {tag}: the magnitude order has a tie'
        assert len(np.unique(symp, axis=0)) == len(symp)
        for name in ('single_magnitude', 'single_random', 'diag_first') + (('dfs_magnitude', 'dfs_largest') if kind == 'dfs' else ()):
            assert f'{tag}/{name}/symp' in GOLD.files and f'{tag}/{name}/coeff' in GOLD.files
    assert os.path.getsize(os.path.join(so.GOLDEN, 'noncon_sweep.npz')) < 256 * 1024


@pytest.mark.parametrize('tag, kind, symp, coeff', CASES, ids=[c[0] for c in CASES])
def test_ref_sweep_and_rule_sweep_reproduce_the_reference(tag, kind, symp, coeff):
    adj = so.adjacency(symp)
    want = GOLD[f'{tag}/kept']
    assert np.array_equal(so.ref_sweep(adj), want)
    kept, labels = so.rule_sweep(adj)
    assert np.array_equal(kept, want)
    assert np.array_equal(np.flatnonzero(labels != so.REJECTED), want)


def _rows_of(symp, coeff):
    """{row bytes: coefficient} of an operator with distinct rows"""
    return {row.tobytes(): c for row, c in zip(np.asarray(symp, dtype=bool), coeff)}


@pytest.mark.parametrize('tag, kind, symp, coeff', CASES, ids=[c[0] for c in CASES])
def test_rule_sweep_reproduces_the_constructors_of_the_reference(tag, kind, symp, coeff):
    """The orders the constructors sweep in, restated: magnitude; np.random.shuffle under the recorded seed; diagonal first; every roll
    with the reference's scores and its first-best rule."""
    adj, T = so.adjacency(symp), len(coeff)
    by_magnitude = np.argsort(-abs(coeff))

    def same(kept, name):
        return _rows_of(symp[kept], coeff[kept]) == _rows_of(GOLD[f'{tag}/{name}/symp'], GOLD[f'{tag}/{name}/coeff'])

    assert same(so.rule_sweep(adj, by_magnitude)[0], 'single_magnitude')
    np.random.seed(int(GOLD[f'{tag}/random_seed']))
    shuffled = np.arange(T)
    np.random.shuffle(shuffled)
    assert same(so.rule_sweep(adj, shuffled)[0], 'single_random')
    diagonal = ~np.any(symp[:, : symp.shape[1] // 2], axis=1)
    off = np.flatnonzero(~diagonal)
    assert same(so.rule_sweep(adj, np.concatenate([np.flatnonzero(diagonal), off[np.argsort(-abs(coeff[off]))]]))[0], 'diag_first')
    if kind == 'dfs':
        rolls = [so.rule_sweep(adj, np.roll(by_magnitude, -n))[0] for n in range(T)]
        assert same(sorted(rolls, key=lambda kept: -np.sum(abs(coeff[kept])))[0], 'dfs_magnitude')
        assert same(sorted(rolls, key=lambda kept: -len(kept))[0], 'dfs_largest')


def test_rule_equals_reference_loop_on_random_small_operators():
    count = 0
    for symp in so.small_random_cases(20261021, 2000):
        adj = so.adjacency(symp)
        assert np.array_equal(so.rule_sweep(adj)[0], so.ref_sweep(adj)), symp.astype(int)
        count += 1
    assert count == 2000


def test_rule_equals_reference_loop_on_all_rolls_of_fifty_operators():
    rng = np.random.default_rng(77)
    for k in range(50):
        n, T = int(rng.integers(3, 6)), 24
        adj = so.adjacency(so.random_symp(rng, n, T, half_diagonal=k % 2 == 0))
        order = rng.permutation(T)
        for s in range(T):
            visit = np.roll(order, -s)
            assert np.array_equal(so.rule_sweep(adj, visit)[0], so.ref_sweep(adj, visit)), (k, s)


@pytest.mark.parametrize('name, strings, labels', so.BY_HAND, ids=[c[0] for c in so.BY_HAND])
def test_by_hand_cases(name, strings, labels):
    adj = so.adjacency(so.symp_of(strings))
    kept, got = so.rule_sweep(adj)
    assert list(got) == list(labels)
    assert np.array_equal(kept, np.flatnonzero(np.array(labels) != so.REJECTED))
    assert np.array_equal(so.ref_sweep(adj), kept)


def test_labels_describe_the_kept_operator():
    """Kept terms with a clique label commute iff the labels are equal; SYM terms commute with every kept term; m is never 1."""
    for symp in so.small_random_cases(5, 300):
        adj = so.adjacency(symp)
        kept, labels = so.rule_sweep(adj)
        lab = labels[kept]
        sub = adj[np.ix_(kept, kept)]
        assert np.all(sub[lab == so.SYM])
        cl = lab >= 0
        assert np.array_equal(sub[np.ix_(cl, cl)], lab[cl][:, None] == lab[cl][None, :])
        assert len(set(lab[cl])) != 1 and set(lab[cl]) == set(range(len(set(lab[cl]))))


def test_twelve_terms_and_one_more():
    """The reference's 12-term noncontextual operator — three cliques of four — with IIX visited sixth: it commutes with IZI and ZII
    but not with IIY and ZZY, part of the first clique, and is the one term rejected (the smoke run's case)."""
    adj = so.adjacency(so.symp_of(so.TWELVE_AND_ONE))
    kept, labels = so.rule_sweep(adj)
    assert np.array_equal(kept, so.ref_sweep(adj))
    assert list(kept) == so.TWELVE_AND_ONE_KEPT and list(labels) == so.TWELVE_AND_ONE_LABELS
    assert list(so.rule_sweep(so.adjacency(so.symp_of(so.TWELVE)))[0]) == list(range(12))


def test_header_prototype_and_signature_table_agree():
    hdr = open(os.path.join(ROOT, 'include', 'symgpu.h')).read()
    m = re.search(r'int symgpu_noncon_sweep_dev\((.*?)\);', hdr, re.S)
    assert m and len(re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')) == 7 == len(_lib.SIGNATURES['symgpu_noncon_sweep_dev'])
    assert '#define SYMGPU_NONCON_SWEEP_MAX_T 131072' in hdr
    from symmer_amd import kernels
    assert kernels.NONCON_SWEEP_MAX_T == 131072
