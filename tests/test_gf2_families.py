"""CPU: the matrix families of tests/_gf2_families.py are what their docstrings say, and the two oracles agree on them.

Two checks per family, at reduced size: (1) oracle_c.rref — the expected value of every GPU test of the GF(2) elimination — equals the
NumPy restatement of the reference loop, oracle_np.rref_noswap, in reduced matrix, reference-order XOR count and pivots (the NumPy oracle
returns no pivots: they are the leading columns of the non-zero reduced rows); (2) the structural property the family is built for,
computed with NumPy on the INPUT (or, for the rank, by the oracle).  An edit to a family that loses the property fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from oracle import oracle_c as oc
import _gf2_families as fam

VARIANTS = fam.variants()
IDS = [v[0] for v in VARIANTS]
# reduced sizes: three blocks of rows and a few words more than a four-word window / than 300 columns of twins
SIZES = [(150, 700), (65, 333)]


def build(fn, kw, R, C, seed=11):
    return fn(np.random.default_rng(seed), R, C, **kw)


@pytest.mark.parametrize('R,C', SIZES)
@pytest.mark.parametrize('name,fn,kw', VARIANTS, ids=IDS)
def test_oracles_agree_on_family(name, fn, kw, R, C):
    m = build(fn, kw, R, C)
    assert m.shape == (R, C) and m.dtype == bool
    red_c, xors_c, piv_c = oc.rref(fam.pack(m), want_pivots=True)
    red_np, xors_np = onp.rref_noswap(m, count_xors=True)
    assert np.array_equal(red_c, fam.pack(red_np)), 'reduced matrices differ (padding bits included)'
    assert xors_c == xors_np
    assert np.array_equal(piv_c, fam.pivots_of(red_np))
    good = piv_c[piv_c >= 0]
    assert len(set(good.tolist())) == good.size, 'pivot columns must be distinct'


def test_families_are_seeded():
    for name, fn, kw in VARIANTS:
        assert np.array_equal(build(fn, kw, 70, 400, seed=3), build(fn, kw, 70, 400, seed=3)), name


def word_span(cols):
    cols = np.asarray(cols)
    cols = cols[cols >= 0]
    return int(cols.max() // 64 - cols.min() // 64 + 1)


def test_dense_leads_within_two_words():
    for d in (0.5, 0.2):
        m = build(fam.dense, dict(density=d), 150, 700)
        lead = fam.leads(m)
        assert (lead >= 0).all() and word_span(lead[:64]) <= 2


@pytest.mark.parametrize('C', [700, 16384, 16448])
def test_staircase_leads(C):
    R, step = 150, 67
    m = build(fam.staircase, dict(step=step), R, C)
    lead = fam.leads(m)
    assert np.array_equal(lead, (np.arange(R) * step) % C)
    assert word_span(lead[:64]) > 4, 'the first block fits a four-word window'
    if C >= 32 * step:
        # what sends rows of at most 256 words to the full-row panel: a row among the first 32 leads outside the window at row 0's word
        assert (lead[:32] // 64 >= fam.WINDOW_WORDS).any()


def test_reverse_staircase_leads_move_left():
    R, C, step = 150, 16448, 67
    m = build(fam.reverse_staircase, dict(step=step), R, C)
    lead = fam.leads(m)
    assert np.array_equal(lead, (R - 1 - np.arange(R)) * step)
    assert (np.diff(lead) < 0).all()
    # inside a block the smallest leading word is more than a window left of the first row's: window_start must clamp
    assert lead[0] // 64 - lead[63] // 64 >= fam.WINDOW_WORDS


@pytest.mark.parametrize('w', [64, 128, 192, 256, 300])
def test_window_twins_agree_then_differ(w):
    R, C = 151, 700
    m = build(fam.window_twins, dict(w=w), R, C)
    for k in range(R // 2):
        assert np.array_equal(m[2 * k, :w], m[2 * k + 1, :w])
        assert m[2 * k, w] != m[2 * k + 1, w]
        assert m[2 * k, :w].any(), 'a twin pair that is zero on the shared columns cancels nothing'
    # after the reference loop's first step the twin of row 0 is zero on the w shared columns and non-zero beyond
    x = m[1] ^ m[0]
    assert not x[:w].any() and x[w:].any()


@pytest.mark.parametrize('k', [1, 20, 63, 64, 65])
def test_low_rank_rank(k):
    R, C = 150, 700
    m = build(fam.low_rank, dict(k=k), R, C)
    _, _, piv = oc.rref(fam.pack(m), want_pivots=True)
    rank = int((piv >= 0).sum())
    assert 1 <= rank <= k
    if k >= 20:
        assert rank >= k - 3, 'the random basis lost more rank than chance explains'
    # rows that are non-zero on entry and have no pivot became zero on the way: all non-zero rows but `rank` of them (k = 1: half of
    # the rows are zero from the start)
    nonzero = int(m.any(axis=1).sum())
    assert nonzero >= R // 2 - 25
    assert int(((piv < 0) & m.any(axis=1)).sum()) == nonzero - rank >= 40


def test_zero_and_duplicate_layout():
    R, C = 300, 700
    m = build(fam.zero_and_duplicate, dict(), R, C)
    zero = ~m.any(axis=1)
    assert zero[0] and zero[R - 1] and zero[64:128].all() and not zero[1] and not zero[63] and not zero[128]
    copies = [r for r in range(2, R) if np.array_equal(m[r], m[1])]
    assert len(copies) >= 5 and max(copies) >= 256 and {r // 64 for r in copies} >= {2, 3, 4}
    small = build(fam.zero_and_duplicate, dict(), 65, 333)
    z = ~small.any(axis=1)
    assert z[0] and z[64] and z[16:32].all()


@pytest.mark.parametrize('right', [False, True])
def test_identity_plus_noise_pivots(right):
    R, C = 150, 700
    m = build(fam.identity_plus_noise, dict(right=right), R, C)
    off = C - R if right else 0
    lead = fam.leads(m)
    assert np.array_equal(lead, off + np.arange(R)), 'row r leads on the diagonal'
    assert {0, 63} <= set((lead % 64).tolist()), 'pivots in the lowest and the highest bit of a word'
    if right:
        assert not m[:, :off].any() and lead.max() // 64 == (C - 1) // 64
        assert m[:, off:].sum() > R, 'no noise beside the identity'
    else:
        assert m[:, R:].any()


@pytest.mark.parametrize('slope,words', [(1.5, 2), (2.5, 3), (3.5, 4), (4.5, 5)])
def test_banded_blocks_straddle_words(slope, words):
    R, C = 150, 700
    m = build(fam.banded, dict(slope=slope), R, C)
    lead = fam.leads(m)
    assert np.array_equal(lead, np.minimum(C - 1, (np.arange(R) * slope).astype(int)))
    assert word_span(lead[:64]) == words
    assert (m.sum(axis=1) <= 40).all()


def test_single_column_and_single_bit_rows():
    R, C = 150, 700
    m = build(fam.single_column, dict(), R, C)
    assert (m.sum(axis=1) == 1).all() and (fam.leads(m) == C // 2).all()
    _, xors, piv = oc.rref(fam.pack(m), want_pivots=True)
    assert xors == R - 1 and piv[0] == C // 2 and (piv[1:] == -1).all()      # mask_0 holds every other row
    b = build(fam.single_bit_rows, dict(), R, C)
    lead = fam.leads(b)
    assert (b.sum(axis=1) == 1).all() and np.array_equal(lead, (64 * np.arange(R) + 63) % C)
    assert (lead[:10] % 64 == 63).all() and np.array_equal(lead[:10] // 64, np.arange(10))


def test_pack_roundtrip_and_padding():
    rng = np.random.default_rng(5)
    for C in (1, 63, 64, 65, 130):
        m = rng.random((7, C)) < 0.5
        p = fam.pack(m)
        assert p.shape == (7, max(1, (C + 63) // 64)) and np.array_equal(fam.unpack(p, C), m)
        assert np.array_equal(p, onp.pack_rows(np.hstack([m, m]))[:, :p.shape[1]])      # the oracle's own bit rule
        if C % 64:
            assert not (p[:, -1] >> np.uint64(C % 64)).any()
