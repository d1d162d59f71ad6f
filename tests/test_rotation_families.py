"""CPU: the rotation families of tests/_rotation_families.py have the answers they claim.

Every expected answer (formed qubit by qubit from the Pauli multiplication table) is compared bit for bit — rows, row order, coefficients —
with oracle_np.perform_rotations / rotate_by_single_pword, the NumPy restatement of the reference; the packed step that the GPU tests use
at large sizes is compared with the table step; every operator is checked to be clean; and plan_chain of rotate_driver.hip, restated in
Python with the constants read from the header text, must send the shapes of tests/test_gpu_rotation_families.py to the form each one is
there for.  An edit that loses one of these properties — or a changed limit in rotate_common.h — fails here, without a GPU."""
import os

import numpy as np
import pytest

from oracle import oracle_np as onp
from symmer_amd import packing
import _rotation_families as fam

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'symmer_amd', 'csrc')


def constants():
    text = open(os.path.join(CSRC, 'rotate_common.h')).read() + open(os.path.join(CSRC, 'rotate_chain.hip')).read()
    return fam.header_constants(text)


def oracle_run(case):
    symp = fam.packed_to_symp(case.rows, case.n)
    qs = fam.packed_to_symp(case.qs, case.n)
    return onp.perform_rotations(symp, case.coeff, [(qs[r], float(case.ks[r]) * np.pi / 2) for r in range(len(case.ks))])


def check_case(case):
    """clean operand; expectation = oracle (whole run and step by step); packed step = table step."""
    assert fam.is_clean(case.rows, case.coeff), case.name
    assert case.exp_rows.shape == case.rows.shape and fam.is_clean(case.exp_rows, case.exp_coeff), case.name
    er, ec = oracle_run(case)
    assert np.array_equal(packing.pack_rows(er), case.exp_rows), f'{case.name}: rows / row order differ from oracle_np.perform_rotations'
    assert np.array_equal(ec, case.exp_coeff), f'{case.name}: coefficients differ from oracle_np.perform_rotations'
    rows_t, c_t, rows_p, c_p = case.rows, case.coeff, case.rows, case.coeff
    symp, c_o = fam.packed_to_symp(case.rows, case.n), case.coeff
    qsymp = fam.packed_to_symp(case.qs, case.n)
    for r, k in enumerate(case.ks):
        rows_t, c_t, a_t = fam.table_step(rows_t, c_t, case.qs[r], int(k), case.n)
        rows_p, c_p, a_p = fam.packed_step(rows_p, c_p, case.qs[r], int(k))
        symp, c_o = onp.rotate_by_single_pword(symp, c_o, qsymp[r], float(k) * np.pi / 2)
        assert a_t == a_p and np.array_equal(rows_t, rows_p) and np.array_equal(c_t, c_p), f'{case.name}: packed step != table step at rotation {r}'
        assert np.array_equal(packing.pack_rows(symp), rows_t) and np.array_equal(c_o, c_t), f'{case.name}: table step != oracle at rotation {r}'
    assert np.array_equal(rows_t, case.exp_rows) and np.array_equal(c_t, case.exp_coeff)


# ---------------------------------------------------------------- the tables and the layouts ----------------------------------------------
def test_multiplication_table_is_that_of_the_pauli_matrices():
    m = {fam.I_: np.eye(2, dtype=complex), fam.X_: np.array([[0, 1], [1, 0]], dtype=complex), fam.Z_: np.array([[1, 0], [0, -1]], dtype=complex),
         fam.Y_: np.array([[0, -1j], [1j, 0]], dtype=complex)}
    for p in range(4):
        for q in range(4):
            assert np.array_equal(m[p] @ m[q], (1j) ** int(fam.EXP[p, q]) * m[int(fam.PROD[p, q])]), (p, q)
            assert bool(fam.ANTI[p, q]) == (not np.array_equal(m[p] @ m[q], m[q] @ m[p]))
            assert fam.PROD[p, q] == p ^ q                                            # code = x + 2 z: the product's bits are the XOR


def test_layouts_are_those_of_the_library():
    rng = np.random.default_rng(0)
    for n in (1, 40, 64, 65, 128, 130, 449):
        codes = rng.integers(0, 4, (9, n)).astype(np.uint8)
        symp = np.hstack([(codes & 1) != 0, (codes & 2) != 0])
        p = fam.codes_to_packed(codes)
        assert np.array_equal(p, packing.pack_rows(symp)) and np.array_equal(p, onp.pack_rows(symp))
        assert np.array_equal(fam.packed_to_codes(p, n), codes) and np.array_equal(fam.packed_to_symp(p, n), symp)
    c = fam.dyadic(rng, 1000)
    for e in range(8):
        assert np.array_equal(fam.mul_i(c, np.full(1000, e)), c * (1j) ** (e % 4))
    assert (np.abs(c) >= 1 / 16).all()


def test_distinct_rows():
    rng = np.random.default_rng(1)
    for n, T, reserve in ((40, 5000, 1), (64, 3000, 1), (65, 300, 1), (2, 2, 1), (512, 129, 0)):
        rows = fam.distinct_rows(n, T, rng, reserve=reserve)
        codes = fam.packed_to_codes(rows, n)
        assert fam.is_clean(rows, np.ones(T)) and np.array_equal(fam.codes_to_packed(codes), rows)        # no bit outside the n qubits
        assert not codes[:, n - reserve:].any()
        if T >= 300:
            assert 0.6 < (codes[:, 33:n - reserve] != 0).mean() < 0.9 if n - reserve > 40 else True
    assert not fam.is_clean(np.zeros((2, 2), dtype='<u8'), np.ones(2)) and not fam.is_clean(np.eye(2, dtype='<u8'), np.array([1, 1e-12]))


# ---------------------------------------------------------------- last-qubit --------------------------------------------------------------
@pytest.mark.parametrize('n,T', [(64, 129), (40, 300), (65, 300), (128, 1100), (449, 129), (512, 300), (130, 1100)])
def test_last_qubit(n, T):
    rng = np.random.default_rng(100 + n + T)
    for a_set in fam.A_SETS:
        for q_pauli in (fam.X_, fam.Z_, fam.Y_):
            ks = [1, 2, 3, 0, 1]
            case, A = fam.last_qubit(n, T, a_set, q_pauli, ks, rng)
            check_case(case)
            codes = fam.packed_to_codes(case.rows, n)
            if A.shape[0] < T and A.shape[0] > 1:
                assert set(codes[A, n - 1].tolist()) == set(fam.ANTICOMMUTING[q_pauli]) and set(np.delete(codes[:, n - 1], A).tolist()) == {fam.I_, q_pauli}
            # exactly the rows of A anticommute, at every step; the first step moves them to the front in their order
            _, _, counts = fam.run(case.rows, case.coeff, case.qs, case.ks, n)
            assert counts == [A.shape[0]] * len(ks), (case.name, counts)
            r1, c1, _ = fam.table_step(case.rows, case.coeff, case.qs[0], 2, n)
            if A.shape[0]:
                order = np.concatenate([A, np.setdiff1d(np.arange(T), A)])
                want_c = case.coeff[order].copy()
                want_c[:A.shape[0]] *= -1
                assert np.array_equal(r1, case.rows[order]) and np.array_equal(c1, want_c)
    case, A = fam.last_qubit(n, T, 'every_other', fam.X_, [1, 1, 3, 2, 0, 3], rng, cycle_q=True)
    check_case(case)
    assert len({q.tobytes() for q in case.qs}) == 3


def test_index_sets():
    assert [fam.ladder_blocks(n) for n in (64, 65, 130, 183, 184, 193, 449, 512, 1024, 4096, 4100)] == [1, 1, 1, 1, 2, 2, 4, 4, 8, 32, 32]
    assert fam.index_set('1023mod1024', 2500).tolist() == [1023, 2047] and fam.index_set('0mod1024', 2500).tolist() == [0, 1024, 2048]
    assert fam.index_set('1023mod1024', 300).shape[0] == 0 and fam.index_set('last', 300).tolist() == [299] and fam.index_set('every_other', 5).tolist() == [0, 2, 4]


# ---------------------------------------------------------------- Y-ladder ----------------------------------------------------------------
@pytest.mark.parametrize('top', [False, True])
@pytest.mark.parametrize('n,T', [(64, 129), (65, 40), (130, 70), (449, 129), (512, 300), (1024, 64), (961, 40), (4100, 20)])
def test_y_ladder(n, T, top):
    case = fam.y_ladder(n, T, np.random.default_rng(200 + n), top=top)
    check_case(case)
    codes = fam.packed_to_codes(case.rows, n)
    qc = fam.packed_to_codes(case.qs, n)
    assert np.array_equal((codes == fam.Y_).sum(axis=1), np.arange(T) % 8) and np.array_equal((qc == fam.Y_).sum(axis=1), np.arange(len(case.ks)) % 8)
    assert not ((codes == fam.Y_).any(axis=0) & (qc == fam.Y_).any(axis=0)).any()
    # one Y per 128-qubit block (as far as there are blocks), or all of them in the last block
    ycols = np.flatnonzero((codes == fam.Y_).any(axis=0)) // 128
    nb = fam.ladder_blocks(n)
    assert ycols.tolist() == ([nb - 1] * 7 if top else sorted(j % nb for j in range(7)))
    # the first step (k = 1): the rows with X on qubit 0 come first, coefficients negated; nothing else changes but Q's Paulis
    r1, c1, a1 = fam.table_step(case.rows, case.coeff, case.qs[0], 1, n)
    A = np.flatnonzero(np.arange(T) % 3 != 0)
    assert a1 == A.shape[0] and np.array_equal(c1[:a1], -case.coeff[A]) and np.array_equal(r1[:a1], case.rows[A] ^ case.qs[0][None, :])


# ---------------------------------------------------------------- identity and all-commute steps ------------------------------------------
@pytest.mark.parametrize('with_action', [False, True])
@pytest.mark.parametrize('n,T', [(64, 129), (130, 300), (449, 200)])
def test_commuting_steps(n, T, with_action):
    case = fam.commuting_steps(n, T, np.random.default_rng(300 + n), with_action=with_action)
    check_case(case)
    _, _, counts = fam.run(case.rows, case.coeff, case.qs, case.ks, n)
    n_z = int((np.arange(T) % 3 == 1).sum())
    if with_action:
        assert counts == [0, 0, n_z, 0, 0, n_z, 0, 0, n_z]
    else:
        assert counts == [0] * 5 and np.array_equal(case.exp_rows, case.rows) and np.array_equal(case.exp_coeff, case.coeff)
    assert not case.qs[1].any()


# ---------------------------------------------------------------- long runs ---------------------------------------------------------------
@pytest.mark.parametrize('K', fam.LONG_K)
def test_long_run(K):
    n, T = (100, 150) if K % 2 else (64, 140)
    case = fam.long_run(n, T, K, np.random.default_rng(400 + K))
    assert case.ks.tolist() == [r % 4 for r in range(K)]
    check_case(case)
    if K in (9, 41):
        case = fam.long_run(449, 40, K, np.random.default_rng(450 + K), q_words=3)
        check_case(case)
        used = (case.qs[:, :8] | case.qs[:, 8:]) != 0
        assert (used.sum(axis=1) <= 3).all() and used[:, 7].any() and used[:, :7].any(axis=0).sum() >= 4


@pytest.mark.parametrize('K', [8, 11, 40, 41])
def test_long_run_fourfold_is_the_identity_up_to_order(K):
    n, T = 70, 130
    case = fam.long_run(n, T, K, np.random.default_rng(500 + K), fourfold=True)
    check_case(case)
    K4 = K - K % 4
    rows, coeff, counts = fam.run(case.rows, case.coeff, case.qs[:K4], case.ks[:K4], n)
    assert all(0 < a < T for a in counts)

    def as_set(r, c):
        return sorted(zip((x.tobytes() for x in r), c.tolist()))
    assert as_set(rows, coeff) == as_set(case.rows, case.coeff) and not np.array_equal(rows, case.rows)
    # ... and partitioned by the last rotation: its anticommuting rows first
    anti = ~onp.commutes_termwise(fam.packed_to_symp(rows, n), fam.packed_to_symp(case.qs[K4 - 1:K4], n)).ravel()
    assert anti[:counts[-1]].all() and not anti[counts[-1]:].any()


# ---------------------------------------------------------------- the plan ----------------------------------------------------------------
REG0 = dict(chain_reg=False)
TWO = dict(chain_reg=False, local_t=0)
# (qubits, rows, switches, form): the shapes of tests/test_gpu_rotation_families.py
PLAN_SHAPES = (
    [(n, T, {}, 'Registers') for n in (40, 64, 65, 128, 193, 256, 449, 512, 961, 1024, 1985, 2048) for T in (129, 300)]
    + [(64, (1 << 20) + 3, {}, 'Registers'), (512, 131072 + 5, {}, 'Registers'), (2048, 32768 + 7, {}, 'Registers'), (1985, 32768, {}, 'Registers'),
       (40, 1 << 22, {}, 'Registers')]
    + [(n, T, TWO, 'TwoLaunch') for n in (40, 64, 65, 128, 193, 256, 449, 512, 961, 1024, 1985, 2048, 4033, 4096) for T in (129, 1023, 1024, 1025, 4096, 4097)]
    + [(64, 262144, TWO, 'TwoLaunch'), (64, 262145, TWO, 'FourLaunch'), (130, 300, {}, 'FourLaunch'), (4100, 300, {}, 'FourLaunch'),
       (130, 300, TWO, 'FourLaunch'), (4100, 300, TWO, 'FourLaunch'),
       (449, 128, REG0, 'Lds'), (4096, 64, REG0, 'Lds'), (4096, 65, REG0, 'SingleWorkgroup'), (4100, 100, REG0, 'SingleWorkgroup'), (130, 128, REG0, 'Lds'),
       (100, 8192, dict(chain_reg=False, local_t=8192), 'SingleWorkgroup'), (100, 8193, dict(chain_reg=False, local_t=8192), 'TwoLaunch'),
       (100, 300, dict(local_t=0), 'Registers'), (100, 100, dict(local_t=128), 'Lds')])


def test_header_constants_and_plan():
    c = constants()
    assert set(c) == {'CHAIN_TMAX', 'CHAIN_LOCAL_T', 'CHAIN_TWO_T', 'CHAIN_LDS_T', 'CHAIN_IDX_BITS', 'CHAIN_SEG'}, c
    for n, T, sw, form in PLAN_SHAPES:
        assert fam.plan_chain(T, fam.wq_of(n), c, **sw) == form, (n, T, sw, form)
    # what the shapes are there for
    assert T_LIMIT(c) == 1 << 22 and fam.plan_chain(T_LIMIT(c) + 1, 1, c) != 'Registers'
    assert c['CHAIN_TWO_T'] == 262144 and c['CHAIN_SEG'] == 40
    assert [fam.register_chunks(T, fam.wq_of(n)) for n, T in ((64, (1 << 20) + 3), (512, 131077), (2048, 32775), (1985, 32768), (1000, 100000), (2048, 900), (40, 1 << 22))] \
        == [2, 2, 4, 4, 2, 1, 2]
    assert 2 * 64 * 128 * 8 == 128 * 1024                                           # (4096, 64): exactly the LDS form's 128 KiB
    assert (1 << 20) + 3 > 1 << 19                                                  # beyond the one-launch sort


def T_LIMIT(c):
    return 1 << c['CHAIN_IDX_BITS']


# ---------------------------------------------------------------- the one-launch rotation's plan -------------------------------------------
def resident_constants():
    return fam.resident_constants(fam.resident_header_text())


def last_rows_that_fit(wq, nreg, hbm, c):
    """The largest block R whose layout fits RES_LDS_MAX — both sides of the boundary checked against the restated layout sum."""
    R = 1
    while fam.res_layout_total(R + 1, wq, nreg, hbm, c) <= c['RES_LDS_MAX']:
        R += 1
    assert fam.res_layout_total(R, wq, nreg, hbm, c) <= c['RES_LDS_MAX'] < fam.res_layout_total(R + 1, wq, nreg, hbm, c)
    return R


def test_resident_plan_at_its_edges():
    """plan_resident (rotate_resident.hip), restated on the constants of rotate_resident.h, for a device of 256 compute units: geometry and
    residency form at every edge the C++ has.  The sizes follow from the layout: a row of wq chunks takes 16 wq + 26 bytes of LDS, a
    workgroup 3,200 bytes more, and the Registers form holds 2 x 1,024 chunks (32,768 bytes) outside it."""
    c = resident_constants()
    assert set(c) == set(fam.RES_NAMES), c
    assert (c['RES_LDS_MAX'], c['RES_MIN_ROWS'], c['RES_MAX_WG'], c['RES_MAX_W'], c['JOIN_MAX_T']) == (160 * 1024, 64, 256, 128, (1 << 22) - 1)
    plan = lambda T, wq, **kw: fam.plan_resident(T, wq, c, **kw)
    # one workgroup up to RES_MIN_ROWS rows, then two; beyond 256 x 64 rows the blocks grow
    assert [plan(T, 16) for T in (1, 63, 64, 65)] == [('Lds', 1, 1), ('Lds', 1, 63), ('Lds', 1, 64), ('Lds', 2, 33)]
    assert plan(256 * 64, 16) == ('Lds', 256, 64) and plan(256 * 64 + 1, 16) == ('Lds', 253, 65)
    # LDS -> registers -> rows in memory for rows of a power-of-two number of chunks <= 32
    for wq, r_lds, r_reg in ((16, 569, 685), (32, 298, 359)):
        assert last_rows_that_fit(wq, 0, 0, c) == r_lds and last_rows_that_fit(wq, c['RES_REG_ROUNDS'], 0, c) == r_reg
        assert plan(256 * r_lds, wq) == ('Lds', 256, r_lds) and plan(256 * r_lds + 1, wq) == ('Registers', 256, r_lds + 1)
        assert plan(256 * r_reg, wq) == ('Registers', 256, r_reg) and plan(256 * r_reg + 1, wq) == ('RowsInMemory', 256, r_reg + 1)
        # SYMGPU_ROT_HBM=0 refuses what the default takes; =2 forces the form at any size
        assert plan(256 * r_reg + 1, wq, hbm=0) is None and plan(256 * r_reg, wq, hbm=0) == ('Registers', 256, r_reg)
        assert plan(1, wq, hbm=2) == ('RowsInMemory', 1, 1) and plan(256 * r_lds, wq, hbm=2) == ('RowsInMemory', 256, r_lds)
    # 3 chunks a row: not a power of two, from LDS straight to rows in memory
    r3 = last_rows_that_fit(3, 0, 0, c)
    assert r3 == 2170 and plan(256 * r3, 3) == ('Lds', 256, r3) and plan(256 * r3 + 1, 3) == ('RowsInMemory', 256, r3 + 1)
    # 64 chunks (128 words) a row is the longest; no register form above 32 chunks
    r64 = last_rows_that_fit(64, 0, 0, c)
    assert r64 == 152
    assert plan(1, 64) == ('Lds', 1, 1) and plan(1, 65) is None
    assert plan(256 * r64, 64) == ('Lds', 256, r64) and plan(256 * r64 + 1, 64) == ('RowsInMemory', 255, r64 + 1)   # (G re-derived: 255 blocks of 153 rows)
    # The per-row state alone bounds the block: 26 bytes a row.  RES_MAX_R (16,384 rows: 16 ranking passes, 16-bit counts) and JOIN_MAX_T lie
    # beyond that bound at every width, so a block of RES_MAX_R rows is refused by the layout already (425,984 bytes), as is the next
    r_mem = last_rows_that_fit(1, 0, 1, c)
    assert r_mem == 6178 and all(last_rows_that_fit(wq, 0, 1, c) == r_mem for wq in (3, 16, 64))
    assert plan(256 * r_mem, 16) == ('RowsInMemory', 256, r_mem) and plan(256 * r_mem + 1, 16) is None
    assert c['RES_MAX_R'] == 16384 and fam.res_layout_total(c['RES_MAX_R'], 1, 0, 1, c) > c['RES_LDS_MAX']
    assert plan(c['RES_MAX_R'], 1, num_cu=1) is None and plan(c['RES_MAX_R'] + 1, 1, num_cu=1) is None
    assert plan(256 * c['RES_MAX_R'] - 3, 1) is None                                # (R = 16,384 with T < JOIN_MAX_T)
    assert plan(c['JOIN_MAX_T'], 1) is None and plan(c['JOIN_MAX_T'] - 1, 1) is None
    # fewer compute units: fewer, larger blocks
    assert plan(20000, 16, num_cu=64) == ('Lds', 64, 313) and plan(20000, 16, num_cu=304) == ('Lds', 254, 79)
    # rows may merge in a non-Clifford rotation and for odd k: only for an operator known to be free of duplicates
    for k, ok in ((-1, False), (1, False), (3, False), (0, True), (2, True)):
        assert (plan(1000, 16, dup_free=False, k=k) is not None) == ok, k
        assert plan(1000, 16, dup_free=True, k=k) == ('Lds', 16, 63), k
