"""The oracle halves of tests/_thread_tasks.py alone (no GPU, no library): what the workers of tests/test_gpu_threads_statevector.py are
given.  Every worker's shapes are distinct; every shape rule — restated in _thread_tasks.py from include/symgpu.h f7 - f10 and DESIGN.md
3.14 - 3.17 — has workers on both sides, for four workers as for eight; the dyadic cases meet the conditions of
tests/_statevector_families.py under which every partial sum is exact, so equality with the oracle is a fair bar; the sizes stay within
13 qubits, a few hundred terms and 20,000 shots."""
import numpy as np
import pytest

import _ansatz_oracle as ao
import _sample_oracle as so
import _statevector_families as sf
import _thread_tasks as tt

WORKERS = (4, 8)
_cases = {}


def cases(n_workers):
    """{task: [case of worker 0, 1, ...]}, built once per run size."""
    if n_workers not in _cases:
        _cases[n_workers] = {name: [case(tt.worker_rng(n_workers, w, name), w) for w in range(n_workers)] for name, case in tt.CASES.items()}
    return _cases[n_workers]


def test_the_rules_as_the_header_states_them():
    assert tt.sort_passes(1) == 1 and tt.sort_passes(256) == 1 and tt.sort_passes(257) == 2 and tt.sort_passes(8192) == 2 and tt.sort_passes(65537) == 3
    assert tt.sample_form(64, 5000) == 'HIST' and tt.sample_form(8192, 100) == 'SORT'
    m, S = 4096, 1000                                                # the boundary itself: 28 m + 8 S <= 48 S  <=>  S >= 28 m / 40
    assert tt.sample_form(m, 28 * m // 40 + 1) == 'HIST' and tt.sample_form(m, 28 * m // 40 - 1) == 'SORT' and tt.sample_form(m, S) == 'SORT'
    assert [tt.rdm_form(k) for k in (0, 3, 4, 12)] == ['STREAM', 'STREAM', 'TILED', 'TILED']
    assert tt.basis_tile_groups(13, range(13)) == 2 and tt.basis_tile_groups(12, range(12)) == 1 and tt.basis_tile_groups(13, []) == 0
    assert tt.basis_tile_groups(13, range(1, 13)) == 1              # bits 0 .. 11: eight above bit 3
    assert tt.basis_tile_groups(32, range(32)) == 4 and tt.basis_tile_groups(3, range(3)) == 1
    assert tt.expval_form(2048, 11) == 'LDS' and tt.expval_form(2049, 12) == 'GLOBAL' and tt.expval_form(1536, 65) == 'LDS' and tt.expval_form(1537, 65) == 'GLOBAL'
    assert tt.noncon_blocks(6, 10) == 1 and tt.noncon_blocks(12, 10) == 4
    assert tt.GS_TOL == 1e-10


@pytest.mark.parametrize('n_workers', WORKERS)
def test_every_workers_shapes_are_distinct(n_workers):
    for name, per_worker in cases(n_workers).items():
        shapes = [c.shape for c in per_worker]
        assert len(set(shapes)) == n_workers, f'{name}: two workers share a shape: {shapes}'


@pytest.mark.parametrize('n_workers', WORKERS)
def test_every_rule_has_workers_on_both_sides(n_workers):
    all_cases = cases(n_workers)
    seen = set().union(*(c.forms for per_worker in all_cases.values() for c in per_worker))
    assert seen == tt.REQUIRED_FORMS, (sorted(seen - tt.REQUIRED_FORMS), sorted(tt.REQUIRED_FORMS - seen))
    for name, sides in (('expval', {'expval:LDS', 'expval:GLOBAL'}), ('rdm', {'rdm:STREAM', 'rdm:TILED'}), ('sample', {'sample:HIST', 'sample:SORT'}),
                        ('ansatz', {'ansatz:DIRECT', 'ansatz:TILED'})):
        assert set().union(*(c.forms for c in all_cases[name])) == sides, name
    # every worker's sample task runs both counting forms itself, one plan each
    assert all(c.forms == {'sample:HIST', 'sample:SORT'} and c.pairs[1].first > 1 << 40 and c.u_first > 1 << 40 for c in all_cases['sample'])
    assert {c.groups for c in all_cases['basis']} == {1, 2}
    assert {c.count_form for c in all_cases['sampled_expval']} == {'HIST', 'SORT'}
    assert {(c.T + 255) // 256 for c in all_cases['clique']} == {1, 2}
    assert {c.sector is None for c in all_cases['exact_gs']} == {True, False}
    assert {c.other for c in all_cases['clique']} == {'C', 'AC'}
    # RDM by the kept count itself, on both sides of 3
    ks = {len(c.kept) for c in all_cases['rdm']}
    assert min(ks) <= 3 < max(ks)
    # expval by S against the last S that fits: 2048 rows of 24 bytes and 4096 slots are exactly 64 KiB
    sizes = [c.shape[2] for c in all_cases['expval']]
    assert min(sizes) <= 2048 < max(sizes)


@pytest.mark.parametrize('n_workers', WORKERS)
def test_the_wide_generator_takes_a_direct_pass_between_two_tiled_runs(n_workers):
    for c in cases(n_workers)['ansatz']:
        segs = ao.plan_runs(c.symp)
        kinds = [s[3] for s in segs]
        if c.n == 13:
            at = kinds.index(False)
            assert kinds.count(False) == 1 and 0 < at < len(kinds) - 1 and segs[at][1] - segs[at][0] == 1, segs
            assert bin(int(ao.gens_of(c.symp)[0][segs[at][0]])).count('1') == 13
        else:
            assert all(kinds), segs
        assert segs[0][0] == 0 and segs[-1][1] == c.symp.shape[0] and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))


@pytest.mark.parametrize('n_workers', WORKERS)
def test_dyadic_cases_are_exact(n_workers):
    all_cases = cases(n_workers)
    for name in ('expval', 'matvec', 'plan_churn'):
        for c in all_cases[name]:
            coeff, n, v = c.dyadic
            sf.assert_dyadic_is_exact(coeff, n)
            sf.assert_dyadic_vector(v)
    for c in all_cases['expval']:
        assert len(np.unique(c.bits, axis=0)) == len(c.amp) and np.all(c.amp != 0)          # a clean state: S is its row count
    eighths = lambda a: np.array_equal(a.real * 8, np.rint(a.real * 8)) and np.array_equal(a.imag * 8, np.rint(a.imag * 8)) and np.abs(a * 8).max() <= 8 * 2 ** 0.5
    for c in all_cases['rdm']:
        assert eighths(c.psi) and (1 << c.n) * 2 * 64 < 2 ** 52 and np.all(c.tol >= 0)
    for c in all_cases['from_matrix']:
        assert eighths(c.matrix) and np.array_equal(c.matrix[np.repeat(np.arange(1 << c.n), np.diff(c.indptr)), c.indices], c.data)
        assert np.count_nonzero(c.matrix) == len(c.data) and np.all(np.diff(c.want[0] * (1 << c.n) + c.want[1]) > 0)
    for c in all_cases['sample'] + all_cases['plan_churn']:
        for amp in ([p.amp for p in c.pairs] if hasattr(c, 'pairs') else [c.amp]):
            w64 = so.weights(amp) * 64
            total = int(w64.sum())
            # (entries 0 and m - 1 absorb the deficit: they alone may exceed 1 in a component)
            assert eighths(amp[1:-1]) and np.array_equal(amp * 8, np.rint(amp.real * 8) + 1j * np.rint(amp.imag * 8))
            assert np.array_equal(w64, np.rint(w64)) and total & (total - 1) == 0 and total < 2 ** 52, 'the total is not a power of two'


@pytest.mark.parametrize('n_workers', WORKERS)
def test_sizes_stay_small(n_workers):
    all_cases = cases(n_workers)
    qubits = [c.n for per_worker in all_cases.values() for c in per_worker if hasattr(c, 'n')]
    assert max(qubits) == tt.MAX_QUBITS, 'the two-group basis layer and the direct ansatz pass need 13 qubits, and nothing needs more'
    assert max(p.m for c in all_cases['sample'] for p in c.pairs) <= 1 << tt.MAX_QUBITS
    terms = [c.symp.shape[0] for per_worker in all_cases.values() for c in per_worker if hasattr(c, 'symp')]
    assert max(terms) <= tt.MAX_TERMS
    shots = [p.S for c in all_cases['sample'] for p in c.pairs] + [c.shots for c in all_cases['sampled_expval']] + \
            [c.draws for c in all_cases['sampled_expval']] + [c.S for c in all_cases['plan_churn']]
    assert max(shots) <= tt.MAX_SHOTS


def test_the_oracle_halves_agree_with_one_another():
    """One worker's cases, held to a second route through the oracles: what the device is compared with is not a typo of this module."""
    c = cases(4)
    ex = c['expval'][0]
    dense = np.zeros(1 << ex.n, dtype=np.complex128)
    dense[ex.bits.astype(np.int64) @ (1 << np.arange(ex.n - 1, -1, -1))] = ex.amp
    assert ex.total.real == ao.energy(ex.symp, ex.coeff, dense) and ex.total.imag == 0                 # dyadic: exact by either route
    mv = c['matvec'][1]
    assert np.array_equal(mv.want, sf.csr_times(mv.symp, mv.coeff, mv.v))
    an = c['ansatz'][1]
    assert np.abs(an.back - an.ref).max() <= 16 * an.symp.shape[0] * 2.0 ** -53                      # the inverse undoes the rotations
    rd = c['rdm'][3]
    assert np.trace(rd.rho).real == np.sum(rd.psi.real ** 2 + rd.psi.imag ** 2) and np.array_equal(rd.rho, rd.rho.conj().T)
    sa = c['sampled_expval'][0]
    assert np.all(np.abs(sa.sums) <= sa.shots) and sa.state_counts.sum() == sa.draws == sa.dense_counts[1].sum()
    fm = c['from_matrix'][2]
    assert np.array_equal(np.unique(fm.want[0]), np.unique(np.flatnonzero(fm.matrix)[:, None] // (1 << fm.n) ^ np.flatnonzero(fm.matrix)[:, None] % (1 << fm.n)))
