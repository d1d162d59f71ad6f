"""CPU: every answer tests/_f3_f4_families.py claims by construction, proved with oracle.oracle_np alone — check_adjmat_noncontextual of
commutes_termwise(s, s), cleanup_op, and a plain Python loop for the inner product.  tests/test_gpu_f3_f4.py judges the kernels
of csrc/project.hip by that same oracle on these same inputs; the construction and the oracle have to agree before a GPU is asked, so an edit to a
family that loses its property fails here, without one."""
import numpy as np
import pytest

from oracle import oracle_np as onp
import _f3_f4_families as fam


def oracle_answer(symp):
    return onp.check_adjmat_noncontextual(onp.commutes_termwise(symp, symp))


# ---------------------------------------------------------------------------------------------------------------- noncontextuality ----
def test_oracle_unique_rows_by_key_equals_unique_along_axis():
    """check_adjmat_noncontextual takes its unique rows through one opaque key per row; utils.py:587 is np.unique(axis=0).  Same answer, on
    symmetric 0/1 matrices with few distinct rows (both answers occur) and on the adjacency matrices of random operators."""
    rng = np.random.default_rng(12)
    seen = set()
    for trial in range(300):
        m = int(rng.integers(1, 12))
        if trial % 2:
            lab = rng.integers(0, 3, m)
            adj = (lab[:, None] == lab[None, :]) | (lab[:, None] == 0) | (lab[None, :] == 0)
            if trial % 4 == 1 and m > 2:
                i, j = rng.integers(0, m, 2)
                adj[i, j] = adj[j, i] = not adj[i, j]
        else:
            s = rng.random((m, 6)) < 0.4
            adj = onp.commutes_termwise(s, s)
        nu = np.where(~np.all(adj, axis=1))[0]
        literal = bool(np.all(np.count_nonzero(np.unique(adj[nu, :][:, nu], axis=0), axis=0) == 1))
        assert onp.check_adjmat_noncontextual(adj) is literal
        seen.add(literal)
    assert seen == {True, False}


def test_heads_anticommute_pairwise_and_tails_commute():
    n = 9
    H = fam.heads(n)
    assert np.array_equal(onp.commutes_termwise(H, H), np.eye(7, dtype=bool))
    tails = np.array([fam._tail(n, np.random.default_rng(s)) for s in range(20)])
    assert onp.commutes_termwise(tails, np.vstack([H, tails])).all()
    bridge = H[0] ^ H[1] ^ H[6]
    assert onp.commutes_termwise(bridge[None], H).ravel().tolist() == [True] * 2 + [False] * 4 + [True]


@pytest.mark.parametrize('T', sorted(fam.NONCONTEXTUAL))
def test_noncontextual_family_answers(T):
    cases = fam.noncontextual_family(T)
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids) and ids[0] == 'true' and ids[-3:] == ['duplicate', 'universal_last', 'commuting']
    assert sum(not c[2] for c in cases) == (3 if fam.NONCONTEXTUAL[T][0] >= 3 else 2) * len(fam.positions(T))
    for name, symp, answer in cases:
        assert symp.shape[0] == T and symp.dtype == bool, name
        assert oracle_answer(symp) is answer, (T, name)
    # the near-miss term sits where the id says: the rows around it are the True operator's (the two largest T: one position)
    added = [c for c in cases if c[0].startswith(('partial', 'bridge'))]
    for name, symp, _ in (added if T < 4000 else added[-1:]):
        p = int(name.split('@')[1])
        assert oracle_answer(np.delete(symp, p, axis=0)) is True, (T, name)


@pytest.mark.parametrize('T', sorted(fam.ONE_CLIQUE))
def test_one_clique_commutes_throughout(T):
    for name, symp, answer in fam.noncontextual_family(T, fam.ONE_CLIQUE):
        assert answer is True and symp.shape[0] == T
        assert onp.commutes_termwise(symp, symp).all() and oracle_answer(symp) is True, (T, name)


def test_wide_family_answers():
    cases = fam.noncontextual_family(fam.T_WIDE)
    assert [c[0] for c in cases] == ['true', f'bridge@{fam.T_WIDE - 1}', 'partial@0']
    assert 2 * (((fam.T_WIDE + 63) // 64 + 1) // 2) > 128
    for name, symp, answer in cases:
        assert symp.shape[0] == fam.T_WIDE and oracle_answer(symp) is answer, name


def test_clique_structure_of_the_true_operator():
    """What makes the answer True, on one operator: universal terms commute with everything, cliques commute inside and anticommute
    across; clique counts, universal counts and the clique of one member are what the table says."""
    rng = np.random.default_rng(4)
    symp, clique, member = fam._cliques(129, 1, fam.split_sizes(129, 7, 1, True), 30, rng)
    adj = onp.commutes_termwise(symp, symp)
    assert np.array_equal(adj, (clique[:, None] == clique[None, :]) | (clique[:, None] < 0) | (clique[None, :] < 0))
    assert np.bincount(clique + 1).tolist() == [1, 22, 21, 21, 21, 21, 21, 1]
    n = symp.shape[1] // 2
    for c in range(6):
        z = symp[:, n + fam.Q]
        assert z[(clique == c) & (member == 0)].all() and not z[(clique == c) & (member == 1)].any()
    assert {fam.NONCONTEXTUAL[T][0] for T in fam.NONCONTEXTUAL} == {2, 3, 7} and {fam.NONCONTEXTUAL[T][1] for T in fam.NONCONTEXTUAL} == {0, 1, 'half'}
    assert {3 + v[2] for v in fam.NONCONTEXTUAL.values()} <= set(range(8, 71)) | {130}


# --------------------------------------------------------------------------------------------------------------------- bra * ket ----
def loop_with_match(a_c, b_c, match):
    """The same sum with the partner rows the construction names (no look-up of rows at all)."""
    re, im = np.float64(0.0), np.float64(0.0)
    with np.errstate(all='ignore'):
        for i, j in enumerate(match):
            if j >= 0:
                ar, ai, br, bi = np.float64(a_c[i].real), np.float64(a_c[i].imag), np.float64(b_c[j].real), np.float64(b_c[j].imag)
                re, im = re + (ar * br - ai * bi), im + (ar * bi + ai * br)
            else:
                re, im = re + np.float64(0.0), im + np.float64(0.0)
    return re, im


@pytest.mark.parametrize('Na,Nb,nq', fam.INNER_SHAPES)
def test_states_are_clean_and_share_what_they_claim(Na, Nb, nq):
    for overlap in fam.OVERLAPS:
        if overlap == 'third' and min(Na, Nb) < 3:
            continue
        kinds = fam.AMPLITUDES if max(Na, Nb) <= 2000 else ('nonfinite',)
        for kind in kinds:
            rng = np.random.default_rng([Na, Nb, nq])
            a, ac, b, bc, match = fam.states(rng, Na, Nb, nq, overlap, kind)
            assert a.shape == (Na, nq) and b.shape == (Nb, nq) and ac.shape == (Na,) and bc.shape == (Nb,)
            assert np.unique(a, axis=0).shape[0] == Na and np.unique(b, axis=0).shape[0] == Nb, 'rows repeat inside a state'
            shared = {'none': 0, 'all': min(Na, Nb), 'third': max(1, min(Na, Nb) // 3)}[overlap]
            hit = match >= 0
            assert hit.sum() == shared and np.unique(match[hit]).size == shared
            assert np.array_equal(a[hit], b[match[hit]])
            keys_b = {r.tobytes() for r in b}
            assert not any(r.tobytes() in keys_b for r in a[~hit]), 'an unmatched row of a is in b'
            # the oracle's cleanup leaves a clean state as it is (non-finite amplitudes: without threshold, so that the NaN rows stay)
            thr = None if kind == 'nonfinite' else 1e-15
            for bits, c in ((a, ac), (b, bc)):
                if bits.shape[0] <= 2000:
                    rows, cc = onp.cleanup_op(fam.state_symp(bits), c, thr)
                    assert np.array_equal(rows, fam.state_symp(bits)) and np.array_equal(cc, c, equal_nan=True)      # (0 + -0.0 is +0.0: equal as values)
            re, im = fam.inner_sequential(a, ac, b, bc)
            re2, im2 = loop_with_match(ac, bc, match)
            assert fam.same_bits(re, re2) and fam.same_bits(im, im2), (overlap, kind)
            if kind == 'dyadic':
                # exact integer arithmetic on the sixteenths: the answer in any order
                A = np.rint(np.stack([ac.real, ac.imag]) * 16).astype(np.int64)[:, hit]
                B = np.rint(np.stack([bc.real, bc.imag]) * 16).astype(np.int64)[:, match[hit]]
                assert int(np.sum(A[0] * B[0] - A[1] * B[1])) == re * 256 and int(np.sum(A[0] * B[1] + A[1] * B[0])) == im * 256
            if kind == 'nonfinite':
                assert not np.isfinite(ac).all() and not np.isfinite(bc).all()
                if shared >= len(fam.SPECIALS) + 3:
                    assert np.isnan(re) or np.isnan(im), 'the planted infinities and NaNs did not meet'
                    assert not np.isfinite(ac[hit]).all() and not np.isfinite(bc[match[hit]]).all()
                elif shared == 0:
                    assert re == 0 and im == 0, 'a row the other state lacks adds 0 whatever its amplitude'


def test_wide_amplitudes_depend_on_the_order_of_additions():
    """What the 'wide' kind is for: the sequential sum in a's order differs in its low bits from the same products added in another
    order and from the fused multiply-add form of the imaginary part — a kernel that reorders or contracts cannot match it bit for bit."""
    a, ac, b, bc, match = fam.states(np.random.default_rng(9), 300, 1024, 64, 'all', 'wide')
    re, im = fam.inner_sequential(a, ac, b, bc)
    rev = fam.inner_sequential(a[::-1], ac[::-1], b, bc)
    assert not (fam.same_bits(re, rev[0]) and fam.same_bits(im, rev[1]))
    lo, hi = np.abs(np.hstack([ac.real, ac.imag])).min(), np.abs(np.hstack([ac.real, ac.imag])).max()
    assert lo < 1e-7 and hi > 1e7


def test_inner_cases_cover_the_capacity_steps():
    cases = fam.inner_cases()
    assert {(c[0], c[1]) for c in cases} == {(1, 1), (64, 64), (65, 512), (65, 513), (300, 1024), (300, 1025), (1000, 200000), (100000, 100000)}
    assert {c[2] for c in cases} == {1, 64, 65, 1000, 130}
    for Na, Nb, nq, overlap, kind in cases:
        assert not (max(Na, Nb) >= 100000 and nq > 130)
    for kind in fam.AMPLITUDES:
        assert (100000, 100000, 130, 'third', kind) in cases and (300, 1025, 64, 'all', kind) in cases


# -------------------------------------------------------------------------------------------------------------------- projection ----
@pytest.mark.parametrize('name', sorted(fam.PROJECTION))
def test_projection_family_answers(name):
    case = fam.projection_family(name)
    n, qubits, T, survivors, collapse, coeff = fam.PROJECTION[name]
    symp, stab, eig, keep = case['symp'], case['stab'], case['eig'], case['keep']
    assert symp.shape == (T, 2 * n) and stab.shape == (len(qubits), 2 * n) and (stab.sum(axis=1) == 1).all()
    assert keep.size == n - len(qubits) and case['n_survived'] == {'all': T, 'none': 0, 'half': (T + 1) // 2}[survivors]
    rows, c, n_survived = fam.projection_expected(symp, case['coeff'], stab, eig, keep)
    assert n_survived == case['n_survived']
    if len(qubits) >= 3:
        assert {-1, 0, 1} <= set(eig.tolist()) and 0 < stab[:, :n].any(axis=1).sum() < len(qubits), 'one kind or one eigenvalue only'
    if n_survived == 0:
        assert rows.shape == (1, 2 * keep.size) and not rows.any() and c[0] == 0
    if collapse:
        assert rows.shape[0] <= 4 ** collapse and n_survived >= 30000, 'tens of thousands of terms onto a few rows'
        assert rows[:, :keep.size].any(axis=0).sum() == collapse
        if keep.size > 64:
            assert rows[:, 0].any() and rows[:, keep.size - 1].any(), 'Paulis in the first and the last output word'
    elif n_survived and keep.size >= 63:
        assert rows.shape[0] > n_survived // 2
    # signs: at least one surviving term is negated when a stabiliser has eigenvalue -1
    if n_survived >= 100 and (eig == -1).any():
        cols = np.nonzero(stab)[1][eig == -1]
        assert symp[:, cols].any()


def test_projection_cases_cover_the_widths():
    keeps = {v[0] - len(v[1]) for v in fam.PROJECTION.values()}
    assert {1, 63, 64, 65, 128, 129} <= keeps
    assert {v[0] for v in fam.PROJECTION.values()} == {65, 128, 130, 200, 1000}
    assert {v[2] for v in fam.PROJECTION.values()} == {1, 255, 256, 257, 70000}
    assert {v[3] for v in fam.PROJECTION.values()} == {'none', 'all', 'half'}
    for n, qubits, *_ in fam.PROJECTION.values():
        assert len(set(qubits)) == len(qubits) and max(qubits) < n
    stabilised = set().union(*[{(n, q) for q in qubits} for n, qubits, *_ in fam.PROJECTION.values()])
    assert {(65, 63), (65, 64), (130, 129), (130, 63), (130, 64), (200, 0), (200, 199), (1000, 999), (1000, 0)} <= stabilised


def test_threshold_case_has_sums_at_the_threshold():
    case = fam.threshold_case()
    rows_all, c_all, _ = fam.projection_expected(case['symp'], case['coeff'], case['stab'], case['eig'], case['keep'], None)
    rows, c, _ = fam.projection_expected(case['symp'], case['coeff'], case['stab'], case['eig'], case['keep'], case['thr'])
    mags = np.abs(c_all)
    assert (mags == case['thr']).any() and (mags < case['thr']).any() and (mags > case['thr']).any()
    assert rows.shape[0] == (mags > case['thr']).sum() and (np.abs(c) > case['thr']).all()
    assert np.array_equal(rows, rows_all[mags > case['thr']])
