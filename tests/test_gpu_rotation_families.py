"""GPU: every form of a run of Clifford rotations (symgpu_rotate_clifford_chain_dev: csrc/rotate_chain.hip, rotate_chain_forms.hip, planned in
rotate_driver.hip plan_chain) and every stage that completes a single rotation, on operands whose answers are known without the kernels'
popcount formula (tests/_rotation_families.py; tests/test_rotation_families.py proves them against the NumPy oracle on the CPU).  Every
case is compared bit for bit — rows, row order, coefficients — with the table-based expectation or, above 400,000 Pauli codes, with the
packed step (proven against the table on the CPU); no case goes without, whatever its size.  The form that served each call is asserted
through the debug counters (kernels.counters; SYMGPU_COUNTER_LIST of include/symgpu.h says what each counts):

  CHAIN_REGISTERS   CHAIN_LDS   CHAIN_SINGLE_WORKGROUP   CHAIN_TWO_LAUNCHES (per rotation)   CHAIN_FOUR_LAUNCHES (per rotation)
  CHAIN_SORT_ONE_LAUNCH / CHAIN_SORT_LAUNCHES  segments of the register chain sorted by the one-launch / the multi-launch sort
  ROTATE_HASH_JOIN / ROTATE_CLIFFORD_FAST / ROTATE_GENERAL  single rotations by the stage that completed them;
  ROTATE_GENERAL_BY_DUP_CHECK: of ROTATE_GENERAL, after the duplicate check

Only the switches of the library as shipped are used (SYMGPU_CHAIN_REG, SYMGPU_CHAIN_LOCAL_T); everything else is chosen by shape.
(One qubit cannot hold 129 distinct rows, so the Wq = 1 row length that is no multiple of 64 is n = 40 and not 64 Wq - 63 = 1.)"""
import numpy as np
import pytest

from symmer_amd import kernels, packing, _lib, PauliwordOp
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
import _rotation_families as fam

pytestmark = pytest.mark.gpu

COUNTERS = fam.FORM_COUNTERS + ('CHAIN_SORT_ONE_LAUNCH', 'CHAIN_SORT_LAUNCHES', 'ROTATE_HASH_JOIN', 'ROTATE_CLIFFORD_FAST', 'ROTATE_GENERAL',
                                'ROTATE_GENERAL_BY_DUP_CHECK')
REGISTERS, LDS, SINGLE, TWO_LAUNCH, FOUR_LAUNCH, SORT_ONE, SORT_MULTI, JOIN, FAST, GENERAL, DUP_GENERAL = range(11)   # index COUNTERS
NAMES = fam.FORMS + ('one-launch sort', 'multi-launch sort', 'hash join', 'Clifford fast path', 'general path', 'duplicate check -> general path')
ENV_NAMES = ('SYMGPU_CHAIN_REG', 'SYMGPU_CHAIN_LOCAL_T', 'SYMGPU_ROT_RESIDENT', 'SYMGPU_ROTATE_GENERAL', 'SYMGPU_ROT_HBM')
DEFAULT = {}
REG0 = {'SYMGPU_CHAIN_REG': '0'}
TWO = {'SYMGPU_CHAIN_REG': '0', 'SYMGPU_CHAIN_LOCAL_T': '0'}
TABLE_CODES = 400000                                                    # up to here the expectation comes from the table itself
TALLY = np.zeros(11, dtype=np.int64)                                    # what the calls of this file were served by
SEEN = set()


@pytest.fixture(autouse=True)
def _seen(request):
    SEEN.add(request.function.__name__)


def counters():
    return kernels.counters(COUNTERS)


def set_switches(monkeypatch, env):
    for k in ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                       # read on every call (rotate_driver.hip read_rotate_switches)


def step_for(n, T):
    return fam.table_step if n * T <= TABLE_CODES else fam.packed_step


def clean_handle(rows, coeff):
    """The operand as the chain entry point wants it: through a device cleanup, which must keep every row where it is."""
    up = DeviceOp.upload(rows, coeff)
    try:
        dev = kernels.cleanup_dev(up)
    finally:
        up.free()
    assert dev.n_terms == rows.shape[0], 'the family is not clean: the device cleanup merged or dropped rows'
    return dev


def assert_same(what, rows, coeff, exp_rows, exp_coeff):
    assert rows.shape == exp_rows.shape, f'{what}: {rows.shape[0]} rows of {rows.shape[1]} words, expected {exp_rows.shape}'
    bad = np.flatnonzero((rows != exp_rows).any(axis=1))
    if bad.shape[0]:
        t = int(bad[0])
        w = int(np.flatnonzero(rows[t] != exp_rows[t])[0])
        same_set = sorted(r.tobytes() for r in rows) == sorted(r.tobytes() for r in exp_rows) if rows.shape[0] <= 10000 else None
        raise AssertionError(f'{what}: {bad.shape[0]} of {rows.shape[0]} rows differ, first row {t} word {w}: {int(rows[t, w]):#018x}, expected '
                             f'{int(exp_rows[t, w]):#018x}; the same rows in another order: {same_set}')
    badc = np.flatnonzero(coeff != exp_coeff)
    assert badc.shape[0] == 0, (f'{what}: {badc.shape[0]} coefficients differ (rows and order are right), first row {int(badc[0])}: '
                                f'{coeff[badc[0]]}, expected {exp_coeff[badc[0]]}')


def check_served(what, delta, form, T=0, K=0):
    """Exactly one call, by `form`; the register chain sorted ceil(K / 40) segments — by the multi-launch sort above 2^19 rows, else by the
    one-launch sort unless the library has switched that off in this process; no single-rotation stage ran."""
    global TALLY
    TALLY += delta
    took = [NAMES[i] for i in range(11) for _ in range(int(delta[i]))]
    want = np.zeros(5, dtype=np.int64)
    want[form] = 1
    assert np.array_equal(delta[:5], want), f'{what}: expected one call by {NAMES[form]}, the counters say {took}'
    assert not delta[JOIN:].any(), f'{what}: a run of Clifford rotations went through single-rotation stages: {took}'
    if form != REGISTERS:
        assert delta[SORT_ONE] == 0 and delta[SORT_MULTI] == 0, f'{what}: {took}'
        return
    segments = (K + 39) // 40
    assert delta[SORT_ONE] + delta[SORT_MULTI] == segments, f'{what}: {segments} segments, {took}'
    if T > (1 << 19):
        assert delta[SORT_MULTI] == segments, f'{what}: {T} keys cannot have gone to the one-launch sort: {took}'
    elif not any('radix sort' in d for d in _lib.degraded()):
        assert delta[SORT_ONE] == segments, f'{what}: {took}'


def chain(case, form, monkeypatch, env=DEFAULT):
    """One call of the chain entry point on the family's operand: the form that served it, and the whole result."""
    set_switches(monkeypatch, env)
    dev = clean_handle(case.rows, case.coeff)
    try:
        before = counters()
        out = kernels.rotate_clifford_chain_dev(dev, case.qs, case.ks)
        delta = counters() - before
        try:
            rows, coeff = out.download()
        finally:
            out.free()
    finally:
        dev.free()
    what = f'{case.name} K={len(case.ks)} [{NAMES[form]}]'
    check_served(what, delta, form, case.rows.shape[0], len(case.ks))
    assert_same(what, rows, coeff, case.exp_rows, case.exp_coeff)


def row_lengths(wq):
    """n = 64 Wq (a multiple of 128 too from Wq = 2 on) and a length whose last qubit is the first bit of the last word."""
    return (64 * wq, 64 * wq - 63 if wq > 1 else 40)


PAULIS = (fam.X_, fam.Z_, fam.Y_)


def last_qubit_cases(n, T, ks, seed, sets=fam.A_SETS):
    rng = np.random.default_rng(seed)
    for i, a_set in enumerate(sets):
        if i and fam.index_set(a_set, T).shape[0] == 0:
            continue                                                       # (no row of that residue at this T: the same operand as 'none')
        yield fam.last_qubit(n, T, a_set, PAULIS[i % 3], ks, rng, step=step_for(n, T), cycle_q=(i % 2 == 1))[0]


# ---------------------------------------------------------------- 1. the register chain -----------------------------------------------------
REG_WQ = (1, 2, 4, 8, 16, 32)


@pytest.mark.parametrize('T', [129, 300])
@pytest.mark.parametrize('wq', REG_WQ)
def test_registers_last_qubit(wq, T, monkeypatch):
    """k_cchain_reg<WQ, 1> for every row width (Wq = 8: n = 512 and 449): the deciding Pauli on the last qubit — the top bit of the last
    word at n = 64 Wq, its bottom bit at n = 64 Wq - 63 — with no, every, one (first / last) or every other row anticommuting."""
    for n in row_lengths(wq):
        for case in last_qubit_cases(n, T, [1, 2, 3, 0, 1, 1], 1000 + n + T):
            chain(case, REGISTERS, monkeypatch)


@pytest.mark.parametrize('T', [129, 300])
@pytest.mark.parametrize('wq', REG_WQ)
def test_registers_y_ladder_and_commuting_steps(wq, T, monkeypatch):
    """Y counts 0 .. 7 spread one per 16-byte chunk (right mod 4 only if ch_row_sum adds all the lanes) or packed into the top chunk;
    Q = I and Z strings on Z-type rows inside a run."""
    n = max(64, 64 * wq - 63)
    rng = np.random.default_rng(2000 + n + T)
    for top in (False, True):
        chain(fam.y_ladder(n, T, rng, top=top), REGISTERS, monkeypatch)
        chain(fam.y_ladder(64 * wq, T, rng, top=top, ks=(3, 1, 1, 1, 2, 1, 3, 1, 1, 0, 1)), REGISTERS, monkeypatch)
    for with_action in (False, True):
        chain(fam.commuting_steps(n, T, rng, with_action=with_action), REGISTERS, monkeypatch)


@pytest.mark.parametrize('K', fam.LONG_K)
def test_registers_long_runs(K, monkeypatch):
    """The partition bit of rotation r is bit 22 + r of the key: K = 10 / 11 around the key's word boundary, 32 / 33 around the lo / hi words of
    the packed ks, 39 / 40 / 41 and 80 / 81 around the 40-rotation segments (whose sorted keys are the `perm` gather of the next)."""
    rng = np.random.default_rng(3000 + K)
    chain(fam.long_run(449, 300, K, rng), REGISTERS, monkeypatch)                             # Wq = 8, k = 0, 1, 2, 3, 0, ...
    chain(fam.long_run(100, 129, K, rng, fourfold=True), REGISTERS, monkeypatch)             # Wq = 2, every Q four times


# (qubits, rows, rotations, chunks per lane)
CHUNK_CASES = [(64, (1 << 20) + 3, 12, 2), (64, (1 << 20) + 3, 41, 2), (512, 131072 + 5, 9, 2), (2048, 32768 + 7, 9, 4), (1985, 32768, 41, 4)]


@pytest.mark.parametrize('n,T,K,nch', CHUNK_CASES, ids=[f'{n}-{T}-{K}' for n, T, K, _ in CHUNK_CASES])
def test_registers_chunks_per_lane(n, T, K, nch, monkeypatch):
    """k_cchain_reg<WQ, 2> (Wq = 1, 8) and <32, 4>: T Wq / 128 >= 8192.  2^20 + 3 rows are beyond the one-launch sort (2^19 keys): the
    multi-launch sort feeds the `perm` gather, across two segments at K = 41; the last, partial block of the grid holds 3 / 5 / 7 rows."""
    assert fam.register_chunks(T, fam.wq_of(n)) == nch
    case = fam.long_run(n, T, K, np.random.default_rng(4000 + n + K), q_words=2, step=fam.packed_step)
    chain(case, REGISTERS, monkeypatch)


def test_registers_row_limit_and_refusal(monkeypatch):
    """2^22 rows: the 22-bit index field of the key is full and partition bit 0 sits directly above it.  The operand is made clean on the
    device, and what the device holds is what the packed oracle starts from.  One row more is refused, and no form is counted."""
    n, T, K = 40, 1 << 22, 3
    rng = np.random.default_rng(5000)
    set_switches(monkeypatch, DEFAULT)
    rows = fam.distinct_rows(n, T + 1, rng, reserve=0)
    coeff = fam.dyadic(rng, T + 1)
    qs = fam.distinct_rows(n, K, rng, reserve=0)
    ks = np.array([1, 3, 2], dtype=np.int32)
    up = DeviceOp.upload(rows, coeff)
    big = kernels.cleanup_dev(up)
    up.free()
    part = dev = out = None
    try:
        assert big.n_terms == T + 1
        before = counters()
        with pytest.raises(_lib.SymgpuError, match='2\\^22'):
            kernels.rotate_clifford_chain_dev(big, qs, ks)
        assert not (counters() - before).any()
        part = kernels.slice_dev(big, 0, T)
        dev = kernels.cleanup_dev(part)
        r0, c0 = dev.download()
        assert np.array_equal(r0, rows[:T]) and np.array_equal(c0, coeff[:T]), 'the device cleanup changed a duplicate-free operand'
        before = counters()
        out = kernels.rotate_clifford_chain_dev(dev, qs, ks)
        delta = counters() - before
        got_r, got_c = out.download()
    finally:
        for h in (big, part, dev, out):
            if h is not None:
                h.free()
    check_served('2^22 rows', delta, REGISTERS, T, K)
    er, ec, counts = fam.run(r0, c0, qs, ks, n, step=fam.packed_step)
    assert all(0 < a < T for a in counts)
    assert_same('2^22 rows of 40 qubits', got_r, got_c, er, ec)


# ---------------------------------------------------------------- 2. two launches per rotation ----------------------------------------------
TWO_WQ = (1, 2, 4, 8, 16, 32, 64)
TWO_T = (129, 1023, 1024, 1025, 4096, 4097)


@pytest.mark.parametrize('T', TWO_T)
@pytest.mark.parametrize('wq', TWO_WQ)
def test_two_launch(wq, T, monkeypatch):
    """k_cchain_flags / k_cchain_move<WQ, ROWS> for every row width (Wq = 64: n = 4096 and 4033) around the 1024-row group (1023 / 1024 /
    1025: the only anticommuting row just before and just after the group edge) and around T = 4096, above which a block takes 64 rows
    (Wq = 32: 8 passes, Wq = 64: 16 passes and rows exchanged by __shfl_xor(.., 32))."""
    for n in row_lengths(wq):
        for case in last_qubit_cases(n, T, [1, 2, 3], 6000 + n + T):
            chain(case, TWO_LAUNCH, monkeypatch, TWO)
    n = max(64, 64 * wq - 63)
    rng = np.random.default_rng(6500 + n + T)
    chain(fam.y_ladder(n, T, rng, ks=(1, 3, 1, 2, 3), step=step_for(n, T)), TWO_LAUNCH, monkeypatch, TWO)
    chain(fam.y_ladder(64 * wq, T, rng, top=True, ks=(3, 1, 1, 1, 2, 1, 3, 1), step=step_for(n, T)), TWO_LAUNCH, monkeypatch, TWO)
    chain(fam.commuting_steps(n, T, rng, step=step_for(n, T)), TWO_LAUNCH, monkeypatch, TWO)
    chain(fam.long_run(n, T, 5, rng, q_words=3, step=step_for(n, T)), TWO_LAUNCH, monkeypatch, TWO)


@pytest.mark.parametrize('T,form', [(262144, TWO_LAUNCH), (262145, FOUR_LAUNCH)])
def test_two_launch_row_limit(T, form, monkeypatch):
    """T = 262,144 = CHAIN_TWO_T: all 256 group counts; one row more goes to the four-launch form."""
    n = 64
    rng = np.random.default_rng(7000 + T)
    chain(fam.long_run(n, T, 3, rng, step=fam.packed_step), form, monkeypatch, TWO)
    for a_set in ('last', '1023mod1024'):
        chain(fam.last_qubit(n, T, a_set, fam.Y_, [1, 2, 3], rng, step=fam.packed_step)[0], form, monkeypatch, TWO)


# ---------------------------------------------------------------- 3. four launches per rotation ---------------------------------------------
@pytest.mark.parametrize('n,T,K', [(130, 300, 9), (4100, 300, 5)])
def test_four_launch(n, T, K, monkeypatch):
    """Rows of 3 and of 65 chunks: no power of two, and beyond the 64 lanes of a row (the kernels loop over words).  No switch set."""
    ks = [1, 2, 3, 0, 1, 3, 1, 2, 1][:K]
    for case in last_qubit_cases(n, T, ks, 8000 + n):
        chain(case, FOUR_LAUNCH, monkeypatch)
    rng = np.random.default_rng(8500 + n)
    chain(fam.y_ladder(n, T, rng, step=step_for(n, T)), FOUR_LAUNCH, monkeypatch)
    chain(fam.y_ladder(n, T, rng, top=True, step=step_for(n, T)), FOUR_LAUNCH, monkeypatch)
    chain(fam.commuting_steps(n, T, rng, step=step_for(n, T)), FOUR_LAUNCH, monkeypatch)
    chain(fam.long_run(n, T, K, rng, q_words=4, step=step_for(n, T)), FOUR_LAUNCH, monkeypatch)
    chain(fam.long_run(n, T, K, rng, step=step_for(n, T)), FOUR_LAUNCH, monkeypatch, TWO)       # no power of two: the switches change nothing


# ---------------------------------------------------------------- 4. one launch for the whole run -------------------------------------------
LOCAL_8192 = {'SYMGPU_CHAIN_REG': '0', 'SYMGPU_CHAIN_LOCAL_T': '8192'}
SMALL_CASES = [(449, 128, 12, REG0, LDS), (4096, 64, 12, REG0, LDS), (4096, 65, 12, REG0, SINGLE), (4100, 100, 5, REG0, SINGLE), (130, 128, 9, REG0, LDS),
               (100, 8192, 5, LOCAL_8192, SINGLE)]


@pytest.mark.parametrize('n,T,K,env,form', SMALL_CASES, ids=[f'{n}-{T}-{NAMES[form]}' for n, T, _, _, form in SMALL_CASES])
def test_lds_and_single_workgroup(n, T, K, env, form, monkeypatch):
    """k_clifford_chain_lds up to its 128 rows and its 128 KiB (64 rows of 4,096 qubits; 65 rows go to k_clifford_chain), rows of more
    than 128 words, rows of 3 chunks, and the single workgroup's 8,192 rows (8 per thread of its slot scan)."""
    ks = ([1, 2, 3, 0, 1, 3, 1, 2, 1, 1, 3, 2])[:K]
    for case in last_qubit_cases(n, T, ks, 9000 + n + T):
        chain(case, form, monkeypatch, env)
    rng = np.random.default_rng(9500 + n + T)
    st = step_for(n, T)
    chain(fam.y_ladder(n, T, rng, step=st), form, monkeypatch, env)
    chain(fam.y_ladder(n, T, rng, top=True, step=st), form, monkeypatch, env)
    for with_action in (False, True):
        chain(fam.commuting_steps(n, T, rng, with_action=with_action, step=st), form, monkeypatch, env)
    chain(fam.long_run(n, T, K, rng, q_words=4, step=st), form, monkeypatch, env)


# ---------------------------------------------------------------- 5. through the driver -----------------------------------------------------
@pytest.mark.parametrize('resident', ['0', None])
def test_perform_rotations_counts_two_runs_around_a_single_rotation(resident, monkeypatch):
    """PauliwordOp.perform_rotations on a last-qubit operand: the first rotation is a single one (the operator is not known to be clean),
    rotations 1 .. 2 are one run, the non-Clifford rotation 3 is a single one again and rotations 4 .. 6 the second run.  With the
    one-launch rotation off the two single rotations are completed by the Clifford fast path (after the duplicate check) and by the hash
    join; with it on, by whichever stage takes them — two in all.  No output row of the non-Clifford step has a partner (the rows differ
    outside the last qubit), so every coefficient is ONE product of a dyadic number with cos or sin, the same product the oracle forms."""
    n, T = 449, 300
    rng = np.random.default_rng(10000)
    case, A = fam.last_qubit(n, T, 'every_other', fam.X_, [1, 3, 2, 1, 1, 3, 1], rng, cycle_q=True)
    angles = [float(k) * np.pi / 2 for k in case.ks]
    angles[3] = 0.3
    symp, qsymp = fam.packed_to_symp(case.rows, n), fam.packed_to_symp(case.qs, n)
    er, ec = onp.perform_rotations(symp, case.coeff, [(qsymp[r], angles[r]) for r in range(7)])
    # the Clifford rotations in front of the non-Clifford one, from the table
    tr, tc, _ = fam.run(case.rows, case.coeff, case.qs[:3], case.ks[:3], n)
    o3 = onp.perform_rotations(symp, case.coeff, [(qsymp[r], angles[r]) for r in range(3)])
    assert np.array_equal(packing.pack_rows(o3[0]), tr) and np.array_equal(o3[1], tc)
    set_switches(monkeypatch, {} if resident is None else {'SYMGPU_ROT_RESIDENT': resident})
    P = PauliwordOp(symp, case.coeff)
    rotations = [(PauliwordOp(qsymp[r].reshape(1, -1), [1]), angles[r]) for r in range(7)]
    before, resident_before = counters(), kernels.counter('RESIDENT_DONE')
    R = P.perform_rotations(rotations)
    delta, by_resident = counters() - before, kernels.counter('RESIDENT_DONE') - resident_before
    global TALLY
    TALLY += delta
    took = [NAMES[i] for i in range(11) for _ in range(int(delta[i]))] + ['one-launch rotation'] * by_resident
    assert delta[:5].tolist() == [2, 0, 0, 0, 0] and delta[SORT_ONE] + delta[SORT_MULTI] == 2, took
    assert by_resident + delta[JOIN] + delta[FAST] + delta[GENERAL] == 2 and delta[DUP_GENERAL] == 0, took
    if resident == '0':
        assert by_resident == 0 and delta[FAST] == 1 and delta[JOIN] == 1, took
    got_c = R.coeff_vec
    print('largest coefficient difference to the oracle:', np.abs(got_c - ec).max() if got_c.shape == ec.shape else 'shapes differ')
    assert_same(f'perform_rotations, one-launch rotation {"on" if resident is None else "off"}', R.packed, got_c, packing.pack_rows(er), ec)


# ---------------------------------------------------------------- 6. the stages of a single rotation ----------------------------------------
def single(dev, q, angle):
    before, resident_before = counters(), kernels.counter('RESIDENT_DONE')
    res, allc = kernels.rotate_single_dev(dev, q, angle)
    delta = counters() - before
    global TALLY
    TALLY += delta
    assert kernels.counter('RESIDENT_DONE') == resident_before and not delta[:7].any(), 'not a multi-launch single rotation'
    assert not allc
    try:
        return res.download(), delta[JOIN:].tolist()
    finally:
        res.free()


def test_single_rotation_stages(monkeypatch):
    """One small rotation each that must be completed by the hash join, by the Clifford fast path (of a handle known to be duplicate-free,
    and of an uploaded one after the duplicate check), by the general path on request, and by the general path because the duplicate
    check of an odd-k Clifford rotation found the one duplicate row.  Results against the oracle (non-Clifford: the suite's 1e-12)."""
    n, T = 100, 300
    rng = np.random.default_rng(11000)
    case, A = fam.last_qubit(n, T, 'every_other', fam.Y_, [1], rng)
    symp, q = fam.packed_to_symp(case.rows, n), fam.packed_to_symp(case.qs[:1], n)[0]
    half = np.pi / 2
    dev = clean_handle(case.rows, case.coeff)
    up = DeviceOp.upload(case.rows, case.coeff)
    # rows 8 and 250 equal (both in A: they anticommute with Q) with equal coefficients: the odd-k rotation merges their products into 2 c
    dsymp, dcoeff = symp.copy(), case.coeff.copy()
    assert 8 in A and 250 in A
    dsymp[250], dcoeff[250] = dsymp[8], dcoeff[8]
    dup = DeviceOp.upload(packing.pack_rows(dsymp), dcoeff)
    try:
        set_switches(monkeypatch, {'SYMGPU_ROT_RESIDENT': '0'})
        (r, c), stages = single(dev, case.qs[0], 0.3)
        assert stages == [1, 0, 0, 0], stages
        er, ec = onp.rotate_by_single_pword(symp, case.coeff, q, 0.3)
        assert np.array_equal(r, packing.pack_rows(er)) and np.allclose(c, ec, rtol=0, atol=1e-12)
        for k in (1, 2, 3):
            (r, c), stages = single(dev, case.qs[0], k * half)
            assert stages == [0, 1, 0, 0], (k, stages)
            tr, tc, _ = fam.table_step(case.rows, case.coeff, case.qs[0], k, n)
            assert_same(f'Clifford fast path, k = {k}', r, c, tr, tc)
        (r, c), stages = single(up, case.qs[0], half)                       # duplicate status unknown: checked, none found
        assert stages == [0, 1, 0, 0], stages
        assert_same('Clifford fast path after the duplicate check', r, c, *fam.table_step(case.rows, case.coeff, case.qs[0], 1, n)[:2])
        (r, c), stages = single(dup, case.qs[0], half)
        assert stages == [0, 0, 1, 1], stages
        er, ec = onp.rotate_by_single_pword(dsymp, dcoeff, q, half)
        assert er.shape[0] == T - 1
        assert_same('duplicate check -> general path', r, c, packing.pack_rows(er), ec)
        (r, c), stages = single(dup, case.qs[0], 2 * half)                  # even k multiplies nothing: no check, the fast path, both rows kept
        assert stages == [0, 1, 0, 0], stages
        er, ec = onp.rotate_by_single_pword(dsymp, dcoeff, q, 2 * half)
        assert_same('even k with a duplicate row', r, c, packing.pack_rows(er), ec)
        set_switches(monkeypatch, {'SYMGPU_ROTATE_GENERAL': '1'})
        for k in (1, 2):
            (r, c), stages = single(dev, case.qs[0], k * half)
            assert stages == [0, 0, 1, 0], (k, stages)
            tr, tc, _ = fam.table_step(case.rows, case.coeff, case.qs[0], k, n)
            assert_same(f'general path on request, k = {k}', r, c, tr, tc)
    finally:
        for h in (dev, up, dup):
            h.free()


# ---------------------------------------------------------------- 7. what served this file --------------------------------------------------
def test_zz_every_form_and_sort_variant_served_calls():
    """The tally of the counters over this file (printed; read it with -rP).  When the whole file has run, no form, no sort variant and
    no single-rotation stage may have gone unused."""
    print('served by: ' + ', '.join(f'{NAMES[i]} {int(TALLY[i])}' for i in range(11)))
    tests = {name for name, f in globals().items() if name.startswith('test_') and callable(f)} - {'test_zz_every_form_and_sort_variant_served_calls'}
    if tests <= SEEN:
        assert (TALLY > 0).all(), [NAMES[i] for i in range(11) if TALLY[i] == 0]
