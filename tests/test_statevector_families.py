"""No device: the cross-feature identities of tests/_statevector_families.py hold on the NumPy oracles alone — exactly for dyadic cases,
within the summed a-priori bounds for Gaussian ones — and the seed lists that tests/test_gpu_fuzz3.py runs cover what they are there for:
for the tiled ansatz form, cut runs, direct segments, runs opened by a diagonal generator, merged direct generators and every range
kind at every size from 14 qubits on (by ao.plan_runs, the restated cut rule); for the density matrix, every count of kept qubits among
the four lowest index bits and at least 40 values of the position mask (by rdm_position_mask, the restated rdm_shape)."""
import numpy as np
import pytest

import _ansatz_oracle as ao
import _matvec_oracle as mo
import _rdm_oracle as ro
import _sparse_oracle as so
import _statevector_families as sf

SMALL = 9                                       # the identities need dense matrices and per-state Python loops: n <= 9 here


def small_operator(seed, **kw):
    return sf.operator(seed, n_max=SMALL, **kw)


# ---- (a) matvec = sparse matrix times v ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(16))
def test_matvec_is_the_sparse_matrix_times_v(seed):
    op = small_operator(seed)
    v = sf.vector(seed, op.n, op.kind)
    lhs, rhs = mo.matvec(op.symp, op.coeff, v), sf.csr_times(op.symp, op.coeff, v)
    if op.kind == 'dyadic':
        sf.assert_dyadic_is_exact(op.coeff, op.n)
        sf.assert_dyadic_vector(v)
        assert np.array_equal(lhs, rhs) and np.array_equal(rhs, so.to_dense(op.symp, op.coeff) @ v)
    else:
        assert np.abs(lhs - rhs).max() <= mo.error_bound(op.symp, op.coeff, v)


# ---- (b) Re <v|H|v> four ways --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(16))
def test_energy_by_every_route(seed):
    op = small_operator(seed, hermitian=True, t_max=40)
    v = sf.vector(seed, op.n, op.kind)
    routes = sf.energy_routes(op.symp, op.coeff, v)
    exact = op.kind == 'dyadic'
    if exact:
        sf.assert_dyadic_is_exact(op.coeff, op.n)
    R = 0.0 if exact else sf.energy_bound(op.n, op.symp.shape[0], op.coeff)
    for a in routes:
        for b in routes:
            assert abs(routes[a] - routes[b]) <= 2 * R, (a, b, routes)
    # the fourth route: a single term supported on a kept set, through the reduced density matrix
    case = sf.kept_case(seed)
    n, kept = min(case.n, SMALL), [q for q in case.kept if q < SMALL]
    w = sf.vector(seed, n, op.kind)
    sub, padded = sf.strings_on(seed, n, kept)
    for s, p in zip(sub, padded):
        through_rho, bound = sf.rdm_route(w, n, kept, s)
        direct = sf.energy_routes(p.reshape(1, -1), [1.0], w)
        for name, value in direct.items():
            assert abs(through_rho - value) <= (0.0 if exact else bound + sf.energy_bound(n, 1, [1.0])), (name, kept, through_rho, value)


# ---- (c) the last gradient component is the pool gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(8))
def test_last_gradient_component_is_the_pool_gradient(seed):
    n = 3 + seed % 5
    op = sf.operator(seed, hermitian=True, n=n, t_max=12)
    rng = np.random.default_rng(sf.BASE['ansatz'] + 1000 + seed)
    K = int(rng.integers(1, 7))
    gens = rng.random((K, 2 * n)) < 0.4
    theta = rng.uniform(-np.pi, np.pi, K)
    ref = sf.vector(seed, n, 'gaussian')
    shift, pool = sf.gradient_pair(op.symp, op.coeff, gens, theta, ref)
    R = ao.bound(n, K, op.symp.shape[0], op.coeff)
    # each of the two lies within 2 R of the exact derivative (the bar tests/test_gpu_ansatz.py holds the device's gradients to)
    assert abs(shift - pool) <= 4 * R, (shift, pool, R)
    assert np.sign(shift) == np.sign(pool) or abs(shift) <= 4 * R


# ---- (d) decompose(to_dense(H)) = cleaned H -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(16))
def test_decomposition_of_the_matrix_gives_the_cleaned_operator_back(seed):
    op = sf.operator(seed, n_max=7)
    got, want, dense = sf.roundtrip(op.symp, op.coeff)
    if op.kind == 'dyadic':
        sf.assert_dyadic_is_exact(op.coeff, op.n)
        assert sf.compare_terms(got, want, 0) == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])          # and in the same (x, z) order
        assert np.array_equal(dense, so.kron_dense(op.symp, op.coeff))                      # the matrix itself is the definition's
    else:
        sf.compare_terms(got, want, sf.decomp_bound(op.symp, op.coeff, dense))


# ---- what the families hold ----------------------------------------------------------------------------------------------------------------
def test_operator_family_mixes_what_it_names():
    ops = [sf.operator(seed) for seed in range(64)]
    planted = {p for op in ops for p in op.planted}
    assert planted == {'repeated', 'identity', 'diagonal', 'all_y', 'shared_x', 'cancelling'}
    assert {op.shape for op in ops} == {'mixed', 'one_x', 'distinct_x'} and {op.kind for op in ops} == {'dyadic', 'gaussian'}
    assert min(op.n for op in ops) <= 4 and max(op.n for op in ops) == 16 and sum(op.n >= 11 for op in ops) > 32
    assert min(op.symp.shape[0] for op in ops) <= 3 and max(op.symp.shape[0] for op in ops) >= 200
    for op in ops:
        x = so.bits_to_int(op.symp[:, :op.n])
        assert op.symp.shape == (len(op.coeff), 2 * op.n) and 1 <= len(op.coeff) <= 300
        if op.shape == 'one_x':
            assert len(set(x.tolist())) == 1
        if op.shape == 'distinct_x':
            assert len(set(x.tolist())) == len(x)
        if op.kind == 'dyadic':
            sf.assert_dyadic_is_exact(op.coeff, op.n)
    herm = sf.operator(5, hermitian=True)
    assert herm.coeff.dtype == np.float64 and np.array_equal(herm.symp, sf.operator(5).symp)


def test_sweep_operators_are_exact_where_they_claim_to_be():
    for seed in sf.MATVEC_SEEDS:
        op = sf.operator(seed)
        if op.kind == 'dyadic':
            sf.assert_dyadic_is_exact(op.coeff, op.n)
            sf.assert_dyadic_vector(sf.vector(seed, op.n, 'dyadic'))
    assert {sf.operator(seed).kind for seed in sf.MATVEC_SEEDS} == {'dyadic', 'gaussian'}
    assert {sf.operator(seed, hermitian=True, n_max=12).kind for seed in sf.EXPVAL_SEEDS} == {'dyadic', 'gaussian'}
    assert {sf.operator(seed, hermitian=True, n_max=8).kind for seed in sf.ROUNDTRIP_SEEDS} == {'dyadic', 'gaussian'}
    assert max(sf.operator(seed).n for seed in sf.MATVEC_SEEDS) == 16


# ---- ansatz coverage -----------------------------------------------------------------------------------------------------------------------
def test_ansatz_seeds_cover_the_tiled_form():
    cases = [sf.ansatz_case(seed) for seed in sf.ANSATZ_SEEDS]
    assert {c.n for c in cases} == {11, 12, 13, 14, 15, 16}
    with_direct = opened_by_diagonal = merged_direct = 0
    kinds_at = {n: set() for n in (14, 15, 16)}
    for c in cases:
        segs = ao.plan_runs(c.symp)
        K = c.symp.shape[0]
        assert 36 <= K <= 44 and segs[0][0] == 0 and segs[-1][1] == K and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        x = ao.gens_of(c.symp)[0]
        runs = [s for s in segs if s[3]]
        direct = [s for s in segs if not s[3]]
        if c.n >= 14:
            assert len(runs) >= 2, (c.seed, segs)
            kinds_at[c.n] |= {r[0] for r in c.ranges}
        else:
            assert len(runs) == 1 or c.n == 13
        with_direct += bool(direct)
        opened_by_diagonal += any(x[s[0]] == 0 for s in runs)
        merged_direct += any(s[1] - s[0] >= 2 for s in direct)
        for kind, kb, ke, inverse in c.ranges:
            inside = [s for s in runs if s[0] < kb < s[1]]
            if kind == 'inside':
                assert inside and kb < ke < inside[0][1]
            if kind == 'spanning':
                assert inside and any(s[0] < ke < s[1] and s[0] >= inside[0][1] for s in runs)
            if kind == 'direct':
                assert (kb, ke, 0, False) in segs
            if kind == 'empty':
                assert kb == ke
        assert {(r[0], r[3]) for r in c.ranges if r[0] in ('inside', 'spanning')} in (set(), {('inside', False), ('inside', True)},
                                                                                      {('spanning', False), ('spanning', True)},
                                                                                      {('inside', False), ('inside', True), ('spanning', False), ('spanning', True)})
    print(f'{len(cases)} sequences: {with_direct} with a direct segment, {opened_by_diagonal} with a run opened by a diagonal generator, '
          f'{merged_direct} with merged direct generators')
    assert 2 * with_direct >= len(cases)
    assert opened_by_diagonal >= 3 and merged_direct >= 1
    for n, kinds in kinds_at.items():
        assert kinds == {'whole', 'empty', 'inside', 'spanning', 'direct'}, (n, kinds)
    # a run opened by a diagonal generator right after a direct pass
    assert any(a[3] is False and b[3] and ao.gens_of(c.symp)[0][b[0]] == 0 for c in cases for a, b in zip(ao.plan_runs(c.symp), ao.plan_runs(c.symp)[1:]))


# ---- kept-set coverage ---------------------------------------------------------------------------------------------------------------------
def test_rdm_position_mask_restates_the_three_patterns():
    """Known values: the lowest kept bits sit lowest in the tile, the highest above the traced ones, interleaved ones alternate."""
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 2)['low'], 'stream') == 0b11
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 2)['high'], 'stream') == 0b11 << 8
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 2)['interleaved'], 'stream') == 0b101
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 7)['low'], 'tiled') == 0b111111
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 7)['high'], 'tiled') == 0b111111 << 4
    assert sf.rdm_position_mask(12, ro.kept_patterns(12, 4)['interleaved'], 'tiled') == 0b1010101
    assert sf.rdm_position_mask(3, [0, 1, 2], 'tiled') == 0b111 and sf.rdm_position_mask(5, [], 'stream') == 0


def test_rdm_seeds_cover_the_position_masks():
    cases = [sf.kept_case(seed) for seed in sf.RDM_SEEDS]
    low_counts, masks, ks = set(), set(), set()
    for c in cases:
        k = len(c.kept)
        assert 1 <= c.n <= 16 and 0 <= k <= min(8, c.n) and c.kept == sorted(set(c.kept)) and all(0 <= q < c.n for q in c.kept)
        low_counts.add(sum(1 for q in c.kept if c.n - 1 - q < 4))
        ks.add(k)
        for form in sf.rdm_forms(k):
            masks.add(sf.rdm_position_mask(c.n, c.kept, 'stream' if form is None else 'tiled'))
    print(f'{len(cases)} kept sets: {len(masks)} position masks, k in {sorted(ks)}')
    assert low_counts == {0, 1, 2, 3, 4}
    assert ks >= {0, 1, 2, 3} and max(ks) == 8                       # both forms run at every k <= 3
    assert len(masks) >= 40
    assert any(c.n - len(c.kept) < 4 for c in cases) and any(4 <= c.n - len(c.kept) < 8 for c in cases) and any(c.n - len(c.kept) >= 8 for c in cases)
    assert {c.kind for c in cases} == {'dyadic', 'gaussian'} and max(c.n for c in cases) == 16
    three = {tuple(ro.kept_patterns(c.n, len(c.kept))[p]) for c in cases for p in ('low', 'high', 'interleaved')}
    assert sum(tuple(c.kept) not in three for c in cases) >= len(cases) // 2     # most are none of the three hand-made patterns


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_case():
    for seed in (0, 7, 23):
        a, b = sf.operator(seed), sf.operator(seed)
        assert np.array_equal(a.symp, b.symp) and np.array_equal(a.coeff, b.coeff) and (a.n, a.kind, a.shape, a.planted) == (b.n, b.kind, b.shape, b.planted)
        assert np.array_equal(sf.vector(seed, 9, 'gaussian'), sf.vector(seed, 9, 'gaussian')) and np.array_equal(sf.vector(seed, 9, 'dyadic'), sf.vector(seed, 9, 'dyadic'))
        a, b = sf.ansatz_case(seed), sf.ansatz_case(seed)
        assert np.array_equal(a.symp, b.symp) and np.array_equal(a.theta, b.theta) and a.ranges == b.ranges and a.n == b.n
        a, b = sf.kept_case(seed), sf.kept_case(seed)
        assert (a.n, a.kept, a.kind) == (b.n, b.kept, b.kind)
        assert all(np.array_equal(p, q) for p, q in zip(sf.strings_on(seed, 9, [1, 4, 6]), sf.strings_on(seed, 9, [1, 4, 6])))
    assert not np.array_equal(sf.operator(1).coeff, sf.operator(2).coeff)
