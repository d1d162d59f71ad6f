"""CPU: the operand families of tests/_pair_families.py have the answers they claim, and the restated plan of the product + cleanup gives
the flows computed from the source (cleanup_driver.hip plan_cleanup, pair_dups.hip pair_dups_fits / pd_lds_bytes).

Every builder's answer — rows, order, coefficient bits — equals oracle_c.mul_allpairs + oracle_c.cleanup at reduced sizes (the same code
path of the builder) and at the smallest shapes of each family that tests/test_gpu_pair_flows.py runs, up to 2.1e6 pairs; at the larger
shapes only what is cheap: rows distinct where claimed, the planted relations, first indices against brute force.  An edit to a family
that loses its property fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from symmer_amd import packing
import _pair_families as fam


def oracle_answer(P, inner_is_left=True):
    rows, coeff = oc.mul_allpairs(P.inner, P.ci, P.outer, P.co, inner_is_left)
    return oc.cleanup(rows, coeff, P.thr)


def assert_answer(P, inner_is_left=True):
    rows, coeff, fi, fo = P.answer(inner_is_left)
    er, ec = oracle_answer(P, inner_is_left)
    assert rows.shape == er.shape and np.array_equal(rows, er), (P.note, rows.shape, er.shape)
    assert np.array_equal(np.ascontiguousarray(coeff).view(np.uint64), np.ascontiguousarray(ec).view(np.uint64)), P.note
    assert np.array_equal(P.inner[fi] ^ P.outer[fo], rows)
    return rows, coeff, fi, fo


def check_structure(P, n_first=12):
    """what is cheap at any size: distinct rows where claimed, the planted relations, first indices against brute force"""
    for rows, distinct in ((P.inner, P.distinct[0]), (P.outer, P.distinct[1])):
        if distinct:
            assert np.unique(rows, axis=0).shape[0] == rows.shape[0], P.note
    for ii, oo, p in P.relations:
        assert np.array_equal(P.outer[oo], P.inner[ii] ^ p), P.note
    rows, coeff, fi, fo = P.answer()
    first = fo * P.Ni + fi
    assert (np.diff(first) > 0).all()
    if len(first) == 0:
        return
    pick = np.unique(np.concatenate([[0, len(first) - 1], np.random.default_rng(1).integers(0, len(first), n_first)]))
    for k in pick:
        assert P.brute_first(rows[k]) == first[k], (P.note, int(k))
    parts = np.ascontiguousarray(coeff).view(np.float64)
    assert (np.abs(coeff) > P.thr).all() and not (np.signbit(parts) & (parts == 0)).any(), 'a negative zero in an answer'


def test_rows_and_phase_follow_the_library_conventions():
    rng = np.random.default_rng(3)
    for n in (40, 64, 100, 1000):
        r = fam.random_rows(rng, 50, n)
        symp = packing.unpack_rows(r, n)
        assert np.array_equal(packing.pack_rows(symp), r), 'padding bits must be zero'
        assert 0.4 < symp.mean() < 0.6
        a, b = r[:25], r[25:]
        ca, cb = fam.units(rng, 25), fam.units(rng, 25)
        for left in (True, False):
            P = fam.Product(n, a, ca, b, cb, [0], [0])
            i, o = np.tile(np.arange(25), 25), np.repeat(np.arange(25), 25)
            er, ec = oc.mul_allpairs(a, ca, b, cb, left)
            assert np.array_equal(a[i] ^ b[o], er)
            assert np.array_equal(P.pair_coeff(i, o, left), ec), (n, left)


# reduced sizes: the same code path of every builder
SMALL = [('planted', 330, 300), ('planted', 420, None), ('planted-small', 90, 80), ('planted-small', 131, None),
         ('shared-3', 40, 37), ('shared-3', 45, None), ('shared-15', 64, 65), ('shared-15', 100, None), ('shared-16', 129, 64), ('shared-16', 128, None),
         ('twice', 129, 128), ('twice', 64, 200), ('block-200x100', 255, 250), ('block-300x5', 400, 33), ('block-300x300', 301, 300)]


@pytest.mark.parametrize('family,Ni,No', SMALL, ids=[f'{f}-{a}x{b}' for f, a, b in SMALL])
def test_answer_equals_the_oracle_at_reduced_sizes(family, Ni, No):
    for n in (100, 40) if family == 'planted-small' else (100,):
        P = fam.make(family, Ni, No, n)
        assert (P.Ni, P.No, P.squared) == (Ni, No or Ni, No is None)
        assert_answer(P, True)
        if not P.squared:
            assert_answer(P, False)
        check_structure(P, 4)


# the smallest general and squared shapes of each family on the GPU, up to 2.1e6 pairs
GPU_SMALLEST = [('planted', 1025, 512), ('planted', 1255, 1254), ('planted', 1448, None), ('planted-small', 1255, 1254),
                ('shared-3', 1255, 1254), ('shared-16', 1448, None), ('twice', 1255, 1254), ('block-200x100', 1255, 1254),
                ('block-300x5', 1255, 1254), ('block-300x300', 1255, 1254)]


@pytest.mark.parametrize('family,Ni,No', GPU_SMALLEST, ids=[f'{f}-{a}x{b}' for f, a, b in GPU_SMALLEST])
def test_answer_equals_the_oracle_at_the_smallest_gpu_shapes(family, Ni, No):
    P = fam.make(family, Ni, No)
    rows, coeff, fi, fo = assert_answer(P, True)
    assert rows.shape[0] > 0


LARGER = [('planted', 3600, 3500), ('planted', 5438, 5438), ('planted-small', 60000, 30), ('planted-small', 70000, 25), ('planted', 1774, None),
          ('planted', 12288, None), ('planted', 12289, None), ('shared-16', 1774, None), ('shared-3', 10034, None), ('twice', 1800, 1750)]


@pytest.mark.parametrize('family,Ni,No', LARGER, ids=[f'{f}-{a}x{b}' for f, a, b in LARGER])
def test_structure_at_the_larger_shapes(family, Ni, No):
    check_structure(fam.make(family, Ni, No))


def test_families_say_what_they_plant():
    P = fam.make('planted', 1255, 1254)
    assert P.max_multiplicity() == 40 and len(P.relations) > 300
    assert fam.make('planted-small', 1255, 1254).max_multiplicity() == 8
    assert fam.make('planted-small', 1774, None).max_multiplicity() == 8
    assert fam.make('shared-3', 1774, None).max_multiplicity() == 9            # a term of one triple against a term of the other: 3 x 3 pairs (identity off the diagonal: 3 + 1 + 3)
    assert fam.make('shared-16', 1255, 1254).max_multiplicity() == 16
    P = fam.make('twice', 1255, 1254)
    Ka, Kb, g = P.partner
    assert np.array_equal(P.inner[Ka:2 * Ka], P.inner[:Ka] ^ g) and np.array_equal(P.outer[Kb:2 * Kb], P.outer[:Kb] ^ g)
    assert np.count_nonzero(P.ci) == 64 == np.count_nonzero(P.co)
    P = fam.make('block-200x100', 1255, 1254)
    ra, sb = P.copies
    assert len(ra) == 200 and len(sb) == 100 and (P.inner[ra] == P.inner[ra[0]]).all() and (P.outer[sb] == P.outer[sb[0]]).all()
    assert np.unique(P.inner, axis=0).shape[0] == 1255 - 199 and P.max_multiplicity() == 20000
    # the corners are listed pairs that share their row
    P = fam.make('planted', 1800, 1750)
    rows, coeff, fi, fo = P.answer()
    listed = set(zip(P.cand_i.tolist(), P.cand_o.tolist()))
    assert {(0, 0), (1799, 1749), (1799, 0), (0, 1749)} <= listed
    P = fam.make('planted', 1774, None)
    assert {(1, 0), (1773, 0), (1773, 1772)} <= set(zip(P.cand_i.tolist(), P.cand_o.tolist()))


# ---------------------------------------------------------------- the restated plan ---------------------------------------------------------
def flow(Ni, No=None, **sw):
    return fam.flow_name(fam.plan_cleanup(Ni, No or Ni, No is None, **sw))


def test_restated_plan_known_values():
    """values computed from the current source (plan_cleanup, sorted_bits, pair_dups_fits, pd_lds_bytes)"""
    assert flow(1447) == 'complete sort, not lazy'
    assert flow(1448) == 'sorted flag pass'
    assert flow(1773) == 'sorted flag pass'
    assert flow(1774) == 'hash-table flag pass B = 8, bytes'
    assert flow(2508) == 'hash-table flag pass B = 9, bytes'
    assert flow(10033) == 'hash-table flag pass B = 12, bytes'
    assert flow(10034) == 'hash-table flag pass B = 13, 16-bit counters, bytes'
    assert flow(12288) == 'hash-table flag pass B = 13, 16-bit counters, bytes'
    assert flow(12289) == 'sorted flag pass'
    pl = fam.plan_cleanup(1024, 512, False)
    assert pl['nbits'] == 24 and pl['lazy'] and fam.flow_name(pl) == 'complete sort, lazy'
    assert flow(1025, 512) == 'sorted flag pass'
    assert flow(1255, 1254) == 'hash-table flag pass B = 8, bytes'
    assert flow(2049, 1024) == 'hash-table flag pass B = 8, bytes'
    assert flow(1800, 1750) == 'hash-table flag pass B = 9, bytes'
    assert flow(3600, 3500) == 'hash-table flag pass B = 11, bytes'
    assert flow(5000, 5000) == 'hash-table flag pass B = 11, bytes'
    assert flow(5438, 5438) == 'sorted flag pass'                     # LDS too small
    assert flow(60000, 30) == 'sorted flag pass'                      # LDS too small
    assert flow(70000, 25) == 'sorted flag pass'                      # more than 65,535 terms
    # why
    assert fam.pair_dups_fits(5438, 5438, False, 5438 * 5438) is None and 5438 * 5438 >> 12 <= fam.PD_TARGET
    assert fam.pd_lds_bytes(2 * 5438, 1 << 12, False, 17) > fam.PD_LDS_MAX >= fam.pd_lds_bytes(2 * 5000, 1 << 11, False, 17)
    assert fam.pd_lds_bytes(60030, 1 << 8, False, 17) > fam.PD_LDS_MAX and 60030 <= 65535 < 70025
    assert fam.pair_dups_fits(1773, 1773, True, 1773 * 1774 // 2) is None and (1773 * 1774 // 2) >> 7 <= fam.PD_TARGET
    assert fam.pair_dups_fits(12289, 12289, True, 12289 * 12290 // 2) is None and (12289 * 12290 // 2) >> 13 > fam.PD_TARGET_16
    assert 1447 * 1448 // 2 < 1 << 20 <= 1448 * 1449 // 2
    # the switches
    assert flow(1774, direct=False) == 'sorted flag pass'
    assert flow(1774, key_bytes=False) == 'hash-table flag pass B = 8, keys'
    assert flow(1774, suspects=0) == 'complete sort, lazy'
    assert flow(1774, unpacked=True) == '64-bit keys + index sort'
    pl = fam.plan_cleanup(1774, 1774, True, nosquare=True)
    assert not pl['squared'] and pl['Tk'] == 1774 * 1774 and fam.flow_name(pl) == 'complete sort, lazy'      # every key has its twin: no flag pass
    assert fam.plan_cleanup(1774, 1774, True, suspects=2)['key_bytes']


def test_expected_counters():
    c = fam.expected_counters
    assert c(fam.plan_cleanup(1447, 1447, True)) == [1] + [0] * 11
    assert c(fam.plan_cleanup(1448, 1448, True)) == [0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert c(fam.plan_cleanup(1774, 1774, True)) == [0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    assert c(fam.plan_cleanup(1774, 1774, True), 'whole', (fam.C_R_SAT,)) == [0, 1, 0, 1, 0, 1, 0, 0, 1, 0, 1, 0]
    assert c(fam.plan_cleanup(1774, 1774, True, suspects=2), 'whole') == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0]
    assert c(fam.plan_cleanup(1774, 1774, True, direct=False), 'gave up') == [0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert c(fam.plan_cleanup(1774, 1774, True, unpacked=True)) == [0] * 12
    assert len(fam.FLOW_COUNTERS) == 12 and len(fam.PRODUCT_PATHS) == 5
