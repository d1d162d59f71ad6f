"""GPU: every flow of the fused product + cleanup (csrc/cleanup_driver.hip plan_cleanup, cleanup_keys.hip order_flagged, pair_dups.hip) on
operands whose answers are known BY CONSTRUCTION (tests/_pair_families.py; tests/test_pair_families.py proves them against the C oracle on
the CPU): rows, order and coefficient bits equal the builder's answer, and the flow each call took — read from the debug counters
FLOW_* and GIVEUP_* (kernels.counters; SYMGPU_COUNTER_LIST of include/symgpu.h says what each counts) — is the one the restated plan gives
for the shape and the switches:

  FLOW_COMPLETE_SORT        packed keys ordered by the complete sort               GIVEUP_LIST_OVERFLOW    ... list overflow
  FLOW_FLAGS_HASH_TABLES    flag pass from the operand hash tables                 GIVEUP_OPERAND_BUCKET   ... operand bucket over 255 terms
  FLOW_FLAGS_PARTIAL_SORT   flag pass behind the partial sort (k_find_suspects)    FLOW_SORTED_WHOLE       whole array sorted after the flag pass
  FLOW_FLAGS_GAVE_UP        a flag pass gave up                                    FLOW_SORTED_FLAGGED     flagged keys sorted alone
  GIVEUP_PRODUCT_BUCKET     hash-table pass: product bucket over 16,384 pairs      FLOW_MARKED_FROM_BYTES  single terms marked from bytes (k_mark_bytes)
  GIVEUP_COUNTER_SATURATED  ... counter saturated                                  FLOW_FULL_SORT_REPEAT   attempt repeated with the full 64-bit sort

The families put pairs that share a row where the flag passes branch — the corners of the pair index, both groups of the 8,192-bucket
form, product bucket 0 of P * P, rows shared between the operands (the zero-word rule), 4-bit counters at and past saturation — and heavy
terms whose pairs survive ALONE, so that the marking of single terms is seen to keep and not only to drop.  A lost merge is a missing or a
spurious row here, or a wrong Gaussian integer.  Sums are exact in any order: the order of summation stays with the oracle tests.

What does not depend on the hash seed is asserted as a path: up to 8 pairs on one key never saturate a 4-bit counter (the pass completes,
the flagged keys are sorted alone, marking from bytes), 16 and more always do; every row twice always overflows the list; the blocks
always burst a product or an operand bucket.  15 pairs on one key: the result only — one chance hit on the same counter tips it.  After a
reseed in this process (HASH_RESEEDS) only the result is asserted."""
import numpy as np
import pytest

from symmer_amd import kernels
import _pair_families as fam

pytestmark = pytest.mark.gpu

SWITCHES = ('SYMGPU_CLEANUP_DIRECT', 'SYMGPU_CLEANUP_KEYBYTES', 'SYMGPU_CLEANUP_SUSPECTS', 'SYMGPU_CLEANUP_NOSQUARE', 'SYMGPU_CLEANUP_UNPACKED',
            'SYMGPU_CLEANUP_LAZY', 'SYMGPU_CLEANUP_NOFLOOR', 'SYMGPU_WIDE')
# environment -> the same switches as arguments of the restated plan
ENVS = {
    'default': ({}, {}),
    'DIRECT=0': ({'SYMGPU_CLEANUP_DIRECT': '0'}, {'direct': False}),
    'KEYBYTES=0': ({'SYMGPU_CLEANUP_KEYBYTES': '0'}, {'key_bytes': False}),
    'SUSPECTS=0': ({'SYMGPU_CLEANUP_SUSPECTS': '0'}, {'suspects': 0}),
    'SUSPECTS=2': ({'SYMGPU_CLEANUP_SUSPECTS': '2'}, {'suspects': 2}),
    'NOSQUARE=1': ({'SYMGPU_CLEANUP_NOSQUARE': '1'}, {'nosquare': True}),
    'UNPACKED=1': ({'SYMGPU_CLEANUP_UNPACKED': '1'}, {'unpacked': True}),
}


def set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                      # read per call (cleanup_driver.hip read_cleanup_switches, pair_dups_fits)


def describe(delta):
    return '[' + '; '.join(f'{fam.FLOW_COUNTERS[k]}' + (f' x {d}' if d != 1 else '') for k, d in enumerate(delta) if d) + ']'


def counted(call, what):
    """-> (result of the call, what it counted — None after a reseed of the row hash, in this call or earlier in the process)."""
    reseeds, before = kernels.counter('HASH_RESEEDS'), kernels.counters(fam.FLOW_COUNTERS)
    out = call()
    delta = (kernels.counters(fam.FLOW_COUNTERS) - before).tolist()
    print(f'{what}: {describe(delta)}')
    return out, (delta if reseeds == 0 and kernels.counter('HASH_RESEEDS') == 0 else None)


def assert_flow(delta, want, what):
    """One attempt with the counters `want`.  (FLOW_FULL_SORT_REPEAT is left open: a run of more than 48 equal sorted key prefixes that holds a second key
    — the identity segment of P * P beside one chance neighbour — sends the call through a second attempt with the full 64-bit sort, which counts
    nothing else.  It depends on the hash seed and is not a flow of the plan.)"""
    if delta is not None:
        R = fam.C_REPEAT
        assert delta[:R] == want[:R] and delta[R] <= 1, f'{what}: expected {describe(want)}, the call took {describe(delta)}'


def assert_answer(got, want, what, first=None):
    rows, coeff = got[0], got[1]
    erows, ecoeff, fi, fo = want
    assert rows.shape == erows.shape, f'{what}: {rows.shape[0]} rows, expected {erows.shape[0]}'
    if not np.array_equal(rows, erows):
        k = int(np.flatnonzero((rows != erows).any(axis=1))[0])
        raise AssertionError(f'{what}: rows differ from output position {k} on (expected there: pair i = {int(fi[k])}, o = {int(fo[k])})')
    bad = np.flatnonzero((np.ascontiguousarray(coeff).view(np.uint64).reshape(-1, 2) != np.ascontiguousarray(ecoeff).view(np.uint64).reshape(-1, 2)).any(axis=1))
    assert bad.size == 0, f'{what}: {bad.size} coefficients differ, first at position {int(bad[0])} (pair i = {int(fi[bad[0]])}, o = {int(fo[bad[0]])}): {coeff[bad[0]]} for {ecoeff[bad[0]]}'
    if first is not None:
        assert np.array_equal(first[0], fi) and np.array_equal(first[1], fo), f'{what}: first-occurrence indices'


def plan_of(P, **sw):
    return fam.plan_cleanup(P.Ni, P.No, P.squared, P.thr, **sw)


def run(P, want_flow, what):
    """P through kernels.mul_cleanup (P * P: one device operand for both factors) and, for general products, through mul_cleanup_indexed
    with inner_is_left both ways; every call's result against the builder's answer and its counters through want_flow(delta, what)."""
    got, delta = counted(lambda: kernels.mul_cleanup(P.inner, P.ci, P.outer, P.co, True, P.thr), what)
    assert_answer(got, P.answer(True), what)
    want_flow(delta, what)
    if P.squared:
        return
    for left in (True, False):
        w = f'{what}, indexed, inner_is_left={left}'
        got, delta = counted(lambda: kernels.mul_cleanup_indexed(P.inner, P.ci, P.outer, P.co, left, P.thr), w)
        assert_answer(got, P.answer(left), w, first=(got[2], got[3]))
        want_flow(delta, w)


def exactly(pl, outcome='alone', reasons=()):
    want = fam.expected_counters(pl, outcome, reasons)
    return lambda delta, what: assert_flow(delta, want, f'{what} ({fam.flow_name(pl)})')


# shape -> the form the restated plan must give (tests/test_pair_families.py pins the same table without a GPU)
SHAPES = [((1025, 512), 'sorted flag pass'), ((1448, None), 'sorted flag pass'),
          ((1255, 1254), 'hash-table flag pass B = 8, bytes'), ((2049, 1024), 'hash-table flag pass B = 8, bytes'),
          ((1800, 1750), 'hash-table flag pass B = 9, bytes'), ((3600, 3500), 'hash-table flag pass B = 11, bytes'),
          ((1774, None), 'hash-table flag pass B = 8, bytes'), ((2508, None), 'hash-table flag pass B = 9, bytes'),
          ((10033, None), 'hash-table flag pass B = 12, bytes'), ((10034, None), 'hash-table flag pass B = 13, 16-bit counters, bytes'),
          ((12288, None), 'hash-table flag pass B = 13, 16-bit counters, bytes'), ((12289, None), 'sorted flag pass'),
          ((5438, 5438), 'sorted flag pass'), ((60000, 30), 'sorted flag pass'), ((70000, 25), 'sorted flag pass')]
SHAPE_IDS = [f'{a}x{b}' if b else f'squared-{a}' for (a, b), _ in SHAPES]
NARROW = {(60000, 30), (70000, 25)}                                    # too few outer terms for the multiplicities 15, 16 and 40


@pytest.mark.parametrize('shape,form', SHAPES, ids=SHAPE_IDS)
def test_planted_up_to_8_pairs_on_a_key(shape, form, monkeypatch):
    """Multiplicities 2, 3 and 8 (corner pairs included), further rows of two pairs in every product bucket, four heavy terms: the flag
    pass — whichever the shape takes — completes, the flagged keys are sorted alone, and where the hash tables serve, marking is from bytes."""
    set_switches(monkeypatch, {})
    P = fam.make('planted-small', *shape)
    pl = plan_of(P)
    assert fam.flow_name(pl) == form
    run(P, exactly(pl, 'alone'), f'planted-small {shape}')


@pytest.mark.parametrize('shape,form', [s for s in SHAPES if s[0] not in NARROW], ids=[i for i, s in zip(SHAPE_IDS, SHAPES) if s[0] not in NARROW])
def test_planted_up_to_40_pairs_on_a_key(shape, form, monkeypatch):
    """Multiplicities 2, 3, 8, 15, 16 and 40: behind the partial sort nothing changes (runs of equal keys are short); the hash-table pass
    meets a saturated 4-bit counter, gives up for that reason and no other, and the whole array is sorted."""
    set_switches(monkeypatch, {})
    P = fam.make('planted', *shape)
    pl = plan_of(P)
    assert fam.flow_name(pl) == form
    run(P, exactly(pl, 'whole', (fam.C_R_SAT,)) if pl['direct'] else exactly(pl, 'alone'), f'planted {shape}')


@pytest.mark.parametrize('n', [40, 1000])
@pytest.mark.parametrize('shape', [(1774, None), (1255, 1254)], ids=['squared-1774', '1255x1254'])
def test_planted_other_row_lengths(shape, n, monkeypatch):
    """one 16-byte chunk a row (80 random bits) and sixteen"""
    set_switches(monkeypatch, {})
    P = fam.make('planted-small', *shape, n=n)
    run(P, exactly(plan_of(P), 'alone'), f'planted-small {shape}, {n} qubits')


SWITCH_SHAPES = [(1774, None), (1255, 1254), (10034, None)]


@pytest.mark.parametrize('env', list(ENVS))
@pytest.mark.parametrize('shape', SWITCH_SHAPES, ids=['squared-1774-B8', '1255x1254-B8', 'squared-10034-B13'])
def test_switches_change_the_flow_and_not_the_answer(shape, env, monkeypatch):
    """SYMGPU_CLEANUP_DIRECT=0: the flag pass behind the partial sort; KEYBYTES=0: the hash-table pass on 8-byte keys, no marking from bytes;
    SUSPECTS=0: the complete sort; SUSPECTS=2: the whole array sorted behind a flag pass that did not give up; NOSQUARE=1: P * P on the keys
    of all N^2 pairs — every key has its twin, so the complete sort; UNPACKED=1: 64-bit keys and an index sort, none of these counters."""
    environ, sw = ENVS[env]
    set_switches(monkeypatch, environ)
    P = fam.make('planted-small', *shape)
    pl = plan_of(P, **sw)
    run(P, exactly(pl, 'whole' if env == 'SUSPECTS=2' else 'alone'), f'planted-small {shape}, {env}')


@pytest.mark.parametrize('shape', [(1255, 1254), (1774, None), (10034, None)], ids=['1255x1254', 'squared-1774', 'squared-10034'])
@pytest.mark.parametrize('m', [3, 15, 16])
def test_shared_rows(m, shape, monkeypatch):
    """General: the operands share m rows — the identity m times, through the zero-word rule of the flag pass.  P * P: m rows repeated twice
    or three times — identity pairs off the diagonal, inside one operand bucket (the `inside` loop of product bucket 0).  m = 3: the pass
    completes; m = 16 (and m = 15 in P * P, where the repeats make 31 identity pairs): a counter saturates; m = 15, general: result only."""
    set_switches(monkeypatch, {})
    P = fam.make(f'shared-{m}', *shape)
    pl = plan_of(P)
    assert pl['direct']
    top = P.max_multiplicity()
    if top <= 9:
        want = exactly(pl, 'alone')
    elif top >= 16:
        want = exactly(pl, 'whole', (fam.C_R_SAT,))
    else:
        want = lambda delta, what: None
    run(P, want, f'shared-{m} {shape}, {top} pairs on one key')


@pytest.mark.parametrize('shape', [(1255, 1254), (1800, 1750)], ids=['1255x1254', '1800x1750'])
def test_every_row_twice_overflows_the_list(shape, monkeypatch):
    """every pair has its partner: each product bucket lists all of its ~12,000 pairs — the list (1,792) overflows, nothing else gives up"""
    set_switches(monkeypatch, {})
    P = fam.make('twice', *shape)
    pl = plan_of(P)
    run(P, exactly(pl, 'whole', (fam.C_R_LIST,)), f'every row twice {shape}')
    set_switches(monkeypatch, {'SYMGPU_CLEANUP_DIRECT': '0'})            # behind the partial sort: all keys flagged, no give-up
    run(P, exactly(plan_of(P, direct=False), 'whole'), f'every row twice {shape}, DIRECT=0')


def test_blocks_burst_the_buckets(monkeypatch):
    """block(200, 100): 20,000 equal pairs in one product bucket (over 16,384; the 200 copies of a row against any term may saturate a
    counter as well); block(300, 5): 300 terms in one operand bucket (over 255: the pass stops before it looks at a pair); block(300, 300)
    behind the partial sort: a run of 90,000 equal keys, past the 64 steps of 1,024 keys that k_find_suspects reads on — it gives up and
    the whole array is sorted.  (A run of more than 48 equal 32-bit prefixes that holds a second key repeats the attempt with the full sort:
    FLOW_FULL_SORT_REPEAT may or may not move here.)"""
    G, B, S, L, O, W, A = fam.C_GIVEUP, fam.C_R_BUCKET, fam.C_R_SAT, fam.C_R_LIST, fam.C_R_OPERAND, fam.C_WHOLE, fam.C_ALONE
    shape = (1255, 1254)

    def some(need, never):
        def check(delta, what):
            if delta is not None:
                assert all(delta[k] >= 1 for k in need) and all(delta[k] == 0 for k in never), f'{what}: the call took {describe(delta)}'
        return check

    set_switches(monkeypatch, {})
    run(fam.make('block-200x100', *shape), some((fam.C_DIRECT, G, B, W), (L, O, A, fam.C_SORTED, fam.C_FULL)), 'block 200 x 100')
    run(fam.make('block-300x5', *shape), some((fam.C_DIRECT, G, O, W), (B, S, L, A, fam.C_SORTED, fam.C_FULL)), 'block 300 x 5')
    set_switches(monkeypatch, {'SYMGPU_CLEANUP_DIRECT': '0'})
    run(fam.make('block-300x300', *shape), some((fam.C_SORTED, G, W), (B, S, L, O, A, fam.C_DIRECT, fam.C_FULL)), 'block 300 x 300, DIRECT=0')
