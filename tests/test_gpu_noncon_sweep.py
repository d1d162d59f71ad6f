"""GPU: csrc/noncon_sweep.hip — symgpu_noncon_sweep_dev — and what sits on it (kernels.noncon_sweep, utils.perform_noncontextual_sweep,
NoncontextualOp._single_sweep_noncontextual_operator / _dfs_noncontextual_op / _diag_first_noncontextual_op / from_sweep) against the
reference's own answers (tests/golden/noncon_sweep.npz) and against tests/_sweep_oracle.py (held against the reference in
tests/test_sweep_oracle.py).  Everything is integers: every comparison is exact.

The kernel gives a thread of its workgroup the words i, i + blockDim, ... of a commutation row; the sizes below sit on both sides of one
word, of one wavefront of words and of one workgroup of words (the workgroup size times 64 terms)."""
import ctypes

import numpy as np
import pytest

from symmer_amd import NoncontextualOp, PauliwordOp, kernels, packing, _lib
from symmer_amd.kernels import DeviceOp
from symmer_amd.operators.utils import perform_noncontextual_sweep
import _sweep_oracle as so

pytestmark = pytest.mark.gpu
GOLD = so.golden()
CASES = so.golden_cases(GOLD)
WORKGROUP = 256                                                      # NSW_THREADS of csrc/noncon_sweep.hip


def upload(symp):
    return DeviceOp.upload(packing.pack_rows(np.asarray(symp, dtype=bool)))


def device_sweeps(symp, order=None, starts=None, want_info=False):
    with upload(symp) as op:
        return kernels.noncon_sweep(op, order=order, starts=starts, want_labels=True, want_info=want_info)


def oracle_sweeps(adj, order=None, starts=None):
    """(kept bool[n_starts, T], labels int32[n_starts, T]) by position of ``order``, from the rule in NumPy"""
    T = adj.shape[0]
    order = np.arange(T) if order is None else np.asarray(order)
    starts = [0] if starts is None else starts
    kept, labels = np.zeros((len(starts), T), dtype=bool), np.zeros((len(starts), T), dtype=np.int32)
    for k, s in enumerate(starts):
        _, by_index = so.rule_sweep(adj, np.roll(order, -int(s)))
        labels[k] = by_index[order]
        kept[k] = labels[k] != so.REJECTED
    return kept, labels


def check_against_rule(symp, order=None, starts=None, adj=None):
    adj = so.adjacency(symp) if adj is None else adj
    kept, labels, info = device_sweeps(symp, order, starts, want_info=True)
    want_kept, want_labels = oracle_sweeps(adj, order, starts)
    assert np.array_equal(kept, want_kept)
    assert np.array_equal(labels, want_labels)
    return kept, labels, info


def gold_op(tag, name):
    return PauliwordOp(GOLD[f'{tag}/{name}/symp'].astype(bool), GOLD[f'{tag}/{name}/coeff'])


# ---------------------------------------------------------------- golden parity ----------------------------------------------------------
@pytest.mark.parametrize('tag, kind, symp, coeff', CASES, ids=[c[0] for c in CASES])
def test_perform_noncontextual_sweep_keeps_what_the_reference_keeps(tag, kind, symp, coeff):
    H = PauliwordOp(symp, coeff)
    swept = perform_noncontextual_sweep(H)
    kept = GOLD[f'{tag}/kept']
    assert np.array_equal(swept.symp_matrix, symp[kept]) and np.array_equal(swept.coeff_vec, coeff[kept])
    assert swept == PauliwordOp(symp[kept], coeff[kept])
    mask = device_sweeps(symp)[0][0]
    assert np.array_equal(np.flatnonzero(mask), kept)


@pytest.mark.parametrize('tag, kind, symp, coeff', CASES, ids=[c[0] for c in CASES])
def test_constructors_give_the_operators_of_the_reference(tag, kind, symp, coeff):
    H = PauliwordOp(symp, coeff)
    single = NoncontextualOp._single_sweep_noncontextual_operator(H, strategy='magnitude')
    want = gold_op(tag, 'single_magnitude')
    assert isinstance(single, NoncontextualOp) and single == want
    assert np.array_equal(single.symp_matrix, want.symp_matrix) and np.array_equal(single.coeff_vec, want.coeff_vec)     # and in its order
    np.random.seed(int(GOLD[f'{tag}/random_seed']))
    shuffled = NoncontextualOp._single_sweep_noncontextual_operator(H, strategy='random')
    want = gold_op(tag, 'single_random')
    assert shuffled == want and np.array_equal(shuffled.symp_matrix, want.symp_matrix)
    assert NoncontextualOp._diag_first_noncontextual_op(H) == gold_op(tag, 'diag_first')
    assert NoncontextualOp._single_sweep_noncontextual_operator(H, strategy='CurrentOrder') == PauliwordOp(symp[GOLD[f'{tag}/kept']], coeff[GOLD[f'{tag}/kept']])
    if kind == 'dfs':
        for strategy in ('magnitude', 'largest'):
            got, want = NoncontextualOp._dfs_noncontextual_op(H, strategy=strategy), gold_op(tag, f'dfs_{strategy}')
            assert got == want
            assert np.array_equal(got.symp_matrix, want.symp_matrix) and np.array_equal(got.coeff_vec, want.coeff_vec)


def test_from_sweep_parses_the_strategies():
    tag, kind, symp, coeff = next(c for c in CASES if c[1] == 'dfs' and len(c[3]) <= 60)
    H = PauliwordOp(symp, coeff)
    assert NoncontextualOp.from_sweep(H) == gold_op(tag, 'single_magnitude')
    assert NoncontextualOp.from_sweep(H, strategy='SingleSweep_magnitude') == gold_op(tag, 'single_magnitude')
    np.random.seed(int(GOLD[f'{tag}/random_seed']))
    assert NoncontextualOp.from_sweep(H, strategy='SingleSweep_random') == gold_op(tag, 'single_random')
    assert NoncontextualOp.from_sweep(H, strategy='SingleSweep_CurrentOrder') == PauliwordOp(symp[GOLD[f'{tag}/kept']], coeff[GOLD[f'{tag}/kept']])
    assert NoncontextualOp.from_sweep(H, strategy='DFS_magnitude') == gold_op(tag, 'dfs_magnitude')
    assert NoncontextualOp.from_sweep(H, strategy='DFS_largest') == gold_op(tag, 'dfs_largest')
    assert NoncontextualOp.from_sweep(H, strategy='diag_first') == gold_op(tag, 'diag_first')
    with pytest.raises(ValueError, match='Unrecognised strategy, must be one of magnitude, random or CurrentOrder'):
        NoncontextualOp.from_sweep(H, strategy='SingleSweep_weight')
    with pytest.raises(ValueError, match='Unrecognised noncontextual operator strategy'):
        NoncontextualOp.from_sweep(H, strategy='DFS_smallest')
    with pytest.raises(ValueError, match='Unrecognised noncontextual operator strategy'):
        NoncontextualOp.from_sweep(H, strategy='diag')
    with pytest.raises(NotImplementedError):                         # the old door stays shut
        NoncontextualOp.from_hamiltonian(H, strategy='SingleSweep_magnitude')


# ---------------------------------------------------------------- every branch, forced ---------------------------------------------------
@pytest.mark.parametrize('name, strings, labels', so.BY_HAND, ids=[c[0] for c in so.BY_HAND])
def test_by_hand_cases(name, strings, labels):
    symp = so.symp_of(strings)
    kept, got, info = check_against_rule(symp)
    assert list(got[0]) == list(labels)
    assert np.array_equal(kept[0], np.array(labels) != so.REJECTED)
    cliques = max(labels) + 1
    assert info[3] == cliques and info[1] == 1 and info[2] == 1 and info[0] == len(strings) * ((len(strings) + 63) // 64) * 8


def test_demotion_rewrites_masks_across_word_boundaries():
    # the first anticommuting term after 70 and after 130 commuting ones: clique 0 has members in two and in three words
    for count in (70, 130):
        strings, labels = so.demotion_case(count)
        got = device_sweeps(so.symp_of(strings))[1][0]
        zero = np.flatnonzero(got == 0)
        assert list(got) == labels and zero.min() < 64 <= zero.max() and (count < 130 or zero.max() >= 128)


# ---------------------------------------------------------------- edges ------------------------------------------------------------------
@pytest.mark.parametrize('T', [2, 63, 64, 65, 129])
def test_sizes_around_a_word(T):
    rng = np.random.default_rng(900 + T)
    for half_diagonal in (False, True):
        symp = so.random_symp(rng, 5, T, half_diagonal=half_diagonal, density=0.3)
        order = rng.permutation(T)
        check_against_rule(symp)
        check_against_rule(symp, order=order, starts=[0, T - 1, T // 2])


def test_no_terms_and_one_term_launch_nothing():
    with DeviceOp.upload(np.zeros((0, 2), dtype='<u8')) as op:
        kept, labels, info = kernels.noncon_sweep(op, want_labels=True, want_info=True)
        assert kept.shape == (1, 0) and labels.shape == (1, 0) and list(info) == [0, 0, 0, 0]
        kept = kernels.noncon_sweep(op, starts=[0, 5])               # nothing to start at: any start goes
        assert kept.shape == (2, 0)
    kept, labels, info = device_sweeps(so.symp_of(['XY']), starts=[0, 0, 0], want_info=True)
    assert kept.tolist() == [[True]] * 3 and labels.tolist() == [[so.SYM]] * 3 and list(info) == [0, 0, 0, 0]
    empty = PauliwordOp(np.zeros((0, 6), dtype=bool), [])
    assert perform_noncontextual_sweep(empty) is empty
    one = PauliwordOp.from_list(['XYZ'], [0.5])
    assert perform_noncontextual_sweep(one) == one


def test_more_terms_than_a_workgroup_has_words():
    """T = 256 * 64 + 1: thread 0 owns two words of every row.  8 qubits, distinct terms; the oracle at this size is the rule."""
    T, n = WORKGROUP * 64 + 1, 8
    rng = np.random.default_rng(16385)
    codes = rng.choice(1 << (2 * n), size=T, replace=False)
    symp = ((codes[:, None] >> np.arange(2 * n)) & 1).astype(bool)
    symp[::3, :n] = False                                            # a third diagonal (rows now repeat): kept terms in every word
    symp[T - 1] = False                                              # the identity last: kept, the one bit of the last word
    kept, labels, info = device_sweeps(symp, want_info=True)
    want_kept, want_labels = so.rule_sweep(so.LazyAdjacency(symp))
    assert np.array_equal(np.flatnonzero(kept[0]), np.sort(want_kept)) and np.array_equal(labels[0], want_labels)
    assert info[0] == T * (WORKGROUP + 1) * 8 and info[1] == 1 and info[2] == 1 and info[3] >= 2
    assert kept[0, T - 1] and labels[0, T - 1] == so.SYM and len(np.unique(np.flatnonzero(kept[0]) // 64)) > WORKGROUP // 2


def test_duplicate_rows_and_identity_terms_in_an_uncleaned_operator():
    rng = np.random.default_rng(31)
    for T in (40, 100):
        symp = so.random_symp(rng, 2, T)                             # 16 distinct strings: every one repeats, the identity among them
        assert len(np.unique(symp, axis=0)) < T and not symp.any(axis=1).all()
        kept, labels, _ = check_against_rule(symp, starts=range(0, T, 7))
        first = {row.tobytes(): i for i, row in reversed(list(enumerate(symp)))}
        for s in range(kept.shape[0]):                                  # a repeated row gets the label of its kind, or none of them is kept
            for i, row in enumerate(symp):
                assert labels[s, i] == labels[s, first[row.tobytes()]]


def test_130_qubits_three_words_a_half():
    rng = np.random.default_rng(130)
    symp = so.random_symp(rng, 130, 90, half_diagonal=True, density=0.02)
    assert packing.pack_rows(symp).shape[1] == 6
    kept, labels, info = check_against_rule(symp, order=rng.permutation(90), starts=[0, 17, 89])
    assert 2 < kept[0].sum() < 90 and info[3] >= 2


# ---------------------------------------------------------------- rolls ------------------------------------------------------------------
def test_all_rolls_in_one_call_equal_single_calls_and_the_oracle():
    T = 200
    rng = np.random.default_rng(200)
    symp = so.random_symp(rng, 6, T, half_diagonal=True, density=0.3)
    order = rng.permutation(T)
    with upload(symp) as op:
        kept, labels, info = kernels.noncon_sweep(op, order=order, starts=np.arange(T), want_labels=True, want_info=True)
        assert info[1] == T and info[2] == 1
        for s in range(T):
            one_kept, one_labels = kernels.noncon_sweep(op, order=order, starts=[s], want_labels=True)
            assert one_kept.tobytes() == kept[s:s + 1].tobytes() and one_labels.tobytes() == labels[s:s + 1].tobytes()
        without_labels = kernels.noncon_sweep(op, order=order, starts=np.arange(T))
        assert without_labels.tobytes() == kept.tobytes()
    want_kept, want_labels = oracle_sweeps(so.adjacency(symp), order, range(T))
    assert np.array_equal(kept, want_kept) and np.array_equal(labels, want_labels)
    assert len({k.tobytes() for k in kept}) > 1


def test_a_batch_larger_than_the_resident_grid():
    T, n_starts = 65, 6000
    rng = np.random.default_rng(65)
    symp = so.random_symp(rng, 5, T, half_diagonal=True, density=0.3)
    starts = np.arange(n_starts) % T
    kept, labels, info = device_sweeps(symp, starts=starts, want_info=True)
    assert info[1] < n_starts and info[2] > 1 and info[2] == -(-n_starts // info[1])
    want_kept, want_labels = oracle_sweeps(so.adjacency(symp), None, range(T))
    assert np.array_equal(kept, want_kept[starts]) and np.array_equal(labels, want_labels[starts])


def test_max_rolls():
    tag, kind, symp, coeff = next(c for c in CASES if c[1] == 'dfs' and 40 <= len(c[3]) <= 60)
    H, adj, T = PauliwordOp(symp, coeff), so.adjacency(symp), len(coeff)
    by_magnitude = np.argsort(-abs(coeff))
    rolls = [so.rule_sweep(adj, np.roll(by_magnitude, -n))[0] for n in range(T)]
    for max_rolls in (1, 2, 7, T, T + 5):
        for strategy, score in (('magnitude', lambda kept: -np.sum(abs(coeff[kept]))), ('largest', lambda kept: -len(kept))):
            best = sorted(rolls[:max_rolls], key=score)[0]
            got = NoncontextualOp._dfs_noncontextual_op(H, strategy=strategy, max_rolls=max_rolls)
            assert np.array_equal(got.symp_matrix, symp[best]) and np.array_equal(got.coeff_vec, coeff[best])
    assert NoncontextualOp.from_sweep(H, 'DFS_magnitude', max_rolls=1) == gold_op(tag, 'single_magnitude')
    with pytest.raises(ValueError):
        NoncontextualOp._dfs_noncontextual_op(H, max_rolls=0)


def test_first_best_roll_wins_a_tie():
    """'largest' scores by the number of kept terms: an operator is searched (on the host, with the rule) on which the best count is
    reached by two rolls that keep different terms, the later of them with the larger magnitude — the first one must win."""
    rng = np.random.default_rng(12)
    found = None
    for _ in range(400):
        symp = np.unique(so.random_symp(rng, 3, 14, half_diagonal=True), axis=0)
        symp = symp[rng.permutation(len(symp))]
        coeff = rng.permutation(len(symp)) + 1.0
        adj, order = so.adjacency(symp), np.argsort(-coeff)
        rolls = [so.rule_sweep(adj, np.roll(order, -n))[0] for n in range(len(coeff))]
        counts = np.array([len(r) for r in rolls])
        tied = np.flatnonzero(counts == counts.max())
        if len(tied) >= 2 and coeff[rolls[tied[-1]]].sum() > coeff[rolls[tied[0]]].sum() and set(rolls[tied[0]]) != set(rolls[tied[-1]]):
            found = (symp, coeff, rolls[tied[0]])
            break
    assert found is not None
    symp, coeff, first = found
    got = NoncontextualOp._dfs_noncontextual_op(PauliwordOp(symp, coeff), strategy='largest')
    assert np.array_equal(got.symp_matrix, symp[first]) and np.array_equal(got.coeff_vec, coeff[first])


# ---------------------------------------------------------------- refusals ---------------------------------------------------------------
def raw_sweep(handle, order, starts, T):
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    bits = np.zeros((len(starts), (T + 63) // 64), dtype='<u8')
    rc = _lib.lib().symgpu_noncon_sweep_dev(handle, _lib.addr(order), len(starts), _lib.addr(starts), _lib.addr(bits), None, None)
    return rc, bits


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(7)
    symp = so.random_symp(rng, 4, 30)
    want = oracle_sweeps(so.adjacency(symp))[0]
    device_sweeps(symp)                                              # (what the context allocates on first use is there before the gauge is read)
    live = kernels.counter('DEV_BLOCKS_LIVE')
    with upload(symp) as op:
        def still_works():
            assert np.array_equal(kernels.noncon_sweep(op), want)

        still_works()
        repeated, out_of_range = np.arange(30), np.arange(30)
        repeated[3] = 4
        out_of_range[29] = 30
        for order in (repeated, out_of_range, -np.arange(30)):
            rc, _ = raw_sweep(op.handle, order, [0], 30)
            assert rc == _lib.E_INVALID and 'not a permutation' in _lib.last_error()
            still_works()
            with pytest.raises(ValueError, match='permutation'):
                kernels.noncon_sweep(op, order=order)
        with pytest.raises(ValueError, match='permutation'):
            kernels.noncon_sweep(op, order=np.arange(29))
        for starts in ([30], [-1], [0, 5, 31]):
            rc, _ = raw_sweep(op.handle, None, starts, 30)
            assert rc == _lib.E_INVALID and 'start outside' in _lib.last_error()
            still_works()
            with pytest.raises(ValueError, match='start'):
                kernels.noncon_sweep(op, starts=starts)
        rc, _ = raw_sweep(None, None, [0], 30)
        assert rc == _lib.E_INVALID and 'null handle' in _lib.last_error()
        still_works()
        with DeviceOp.random(kernels.NONCON_SWEEP_MAX_T + 1, 8, 0.3, 5) as big:
            rc, _ = raw_sweep(big.handle, None, [0], kernels.NONCON_SWEEP_MAX_T + 1)
            assert rc == _lib.E_INVALID and '131,072' in _lib.last_error()
            still_works()
            with pytest.raises(ValueError, match='at most 131072'):
                kernels.noncon_sweep(big)
        still_works()
    assert kernels.counter('DEV_BLOCKS_LIVE') == live, 'a refusal or a sweep left device memory behind'


# ---------------------------------------------------------------- reproducibility and what the result is for ----------------------------
def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(3)
    symp = so.random_symp(rng, 7, 300, half_diagonal=True, density=0.3)
    order = rng.permutation(300)
    a = device_sweeps(symp, order, np.arange(0, 300, 3))
    b = device_sweeps(symp, order, np.arange(0, 300, 3))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_swept_hamiltonians_are_noncontextual_and_solve():
    for tag, kind, symp, coeff in CASES[:2]:                         # B+ and BH
        H = PauliwordOp(symp, coeff)
        assert not H.is_noncontextual
        for strategy in ('SingleSweep_magnitude', 'diag_first'):
            NC = NoncontextualOp.from_sweep(H, strategy=strategy)    # __init__ asserts noncontextuality, builds generators and reconstruction
            assert PauliwordOp(NC.symp_matrix, NC.coeff_vec).is_noncontextual and NC.n_terms >= 4
        diagonal = NoncontextualOp.from_hamiltonian(H, strategy='diag')
        assert NC.n_terms > diagonal.n_terms                         # diag_first keeps every diagonal term, and here some more
        NC.solve()
        # the minimum over all assignments is not above the all-ones assignment (the two are summed in different orders: 1e-9 sum|c| covers it)
        ones = NC.get_energy(np.ones(NC.symmetry_generators.n_terms, dtype=int))
        assert np.isfinite(NC.energy) and NC.energy <= ones + 1e-9 * np.sum(abs(coeff))
