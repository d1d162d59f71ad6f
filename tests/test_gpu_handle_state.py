"""GPU: what a handle (symgpu_op_s, csrc/common.h) keeps between calls — the cached layouts, the row hashes, the first-occurrence index
and the duplicate-free flag — across SEQUENCES of calls on one handle.  Every other file makes one call on fresh operands; here a cache
is warmed, the rows under it are changed, and the next call must answer for the rows the handle holds now.

The deterministic matrix (test_every_cache_follows_the_rows).  For each cache one consumer that provably reads it; the path counter
shows that the consumer ran, the build counter (OP_*_BUILDS) whether the cache was rebuilt (1) or hit (0):

  cache            consumer                                                     path counter                   build counter
  wm  word-major   symgpu_mul_allpairs_dev, handle = inner; n = 130 (3 chunks   PRODUCT_WORD_MAJOR_THEN_ROWS   OP_WORD_MAJOR_BUILDS
                   a half row: no phase-byte stream), n = 70 under              (or _BESIDE_ROWS)
                   SYMGPU_PRODUCT_FUSED=0
  yc  Y counts     symgpu_mul_allpairs_dev, handle = inner, n = 70 (default)    PRODUCT_PHASE_STREAM           OP_YCOUNT_BUILDS
  bt  bit-major    symgpu_commutes_dev, handle = right operand, under           COMMUTE_M4R_TILE               OP_BIT_MAJOR_BUILDS
                   SYMGPU_COMMUTE_M4R=1
  hash             symgpu_rotate_single_dev, non-Clifford, handle = operand,    ROTATE_HASH_JOIN               OP_ROW_HASH_BUILDS
                   under SYMGPU_ROT_RESIDENT=0 (the hash join); the one-launch
                   kernel (RESIDENT_DONE) and the Clifford fast path
                   (ROTATE_CLIFFORD_FAST) in the tests of handed-on hashes below

Steps: warm (build + 1), repeat (+ 0: the hit), then every mutator followed by the consumer: + 1 after a writer of rows (symgpu_op_write
over all rows, of two rows in the middle, growing T; symgpu_op_copy_rows into the middle; symgpu_op_set_rows down and back up; the handle
as `out` of symgpu_mul_allpairs_dev, twice), + 0 after symgpu_op_set_coeff, symgpu_op_scale and symgpu_op_set_first_index.  Every answer is
the host model's (tests/_handle_model.py, checked against oracle_np on the CPU) bit for bit, and the answers before and after every row
mutator differ, so a stale copy cannot pass.  The rotation's generator is the XOR of two rows the handle holds NOW: a join on stale hashes
misses that partner.

Then: hashes handed on to results and overwritten there; the duplicate-free flag earned as a side effect of a rotation and dropped by
every writer; the flag as the gate of three entry points; the first-occurrence index; and the seeded sequences of the host model replayed
step by step with every observer after every step (test_model_sequences).

What fails if a writer forgets op_invalidate (read off the code for symgpu_op_write; the same cells name the other writers):
  wm        test_every_cache_follows_the_rows[wm-70] / [wm-130] at "op_write over all rows": wm_T == T still holds, the product's
            coefficients are those of the old rows and the build counter stays at 0
  yc        [yc-70] at the same step, and test_ycount_entry_point_reads_the_cached_counts
  bt        [bt-70] / [bt-130] at the same step
  hash      [hash-70] / [hash-130] at the same step (the join misses the planted partner), test_overwritten_rows_are_hashed_again
  first     test_first_occurrence_index_goes_with_the_rows: the index of the old rows is still handed out
  dup_free  test_a_flag_earned_by_a_rotation_does_not_outlive_the_rows[op_write-*] (both twins come back),
            test_the_flag_gates_three_entry_points ("op_write of one row")
Hashes of another seed: tests/_weak_hash_worker5.py.  Handed-on hashes travel with the seed they were taken under, so a Clifford fast
path that handed them on whatever the context's seed would still be caught by the seed comparison of the next rotation; one that also
labelled them with the current seed fails worker 5 (mode `multi`) at the rotation after the Clifford one: no build where one is due."""
import ctypes

import numpy as np
import pytest

import _handle_model as hm
import _expval_oracle as eo
import _f3_f4_families as fam
from symmer_amd import _lib, kernels
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
from _golden import assert_op_equal

pytestmark = pytest.mark.gpu
addr, byref = _lib.addr, ctypes.byref
BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')
ROTATION_STAGES = ('RESIDENT_DONE', 'ROTATE_HASH_JOIN', 'ROTATE_CLIFFORD_FAST', 'ROTATE_GENERAL')


@pytest.fixture(scope='module', autouse=True)
def every_handle_is_freed():
    """DEV_BLOCKS_LIVE is the same before and after the module's tests, after one warm-up of what the context keeps: the hash tables (a
    cleanup) and the table of the rotation's hash join (a non-Clifford rotation of an operand not known to be duplicate free)."""
    rng = np.random.default_rng(0)
    with DeviceOp.upload(hm._random_rows(rng, 40, 70), hm._dyadic(rng, 40)) as raw, kernels.cleanup_dev(raw) as clean:
        for op in (raw, clean):
            res, _ = rotate(op, hm._random_rows(rng, 1, 70)[0], -1, 0.5, 0.75)
            if res is not None:
                res.free()
    before = kernels.counters(BALANCE)
    yield
    assert np.array_equal(kernels.counters(BALANCE), before)


class Counted:
    """with Counted(names) as c: ...; c.delta[name] = how far the counter moved."""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        self.before = kernels.counters(self.names)
        return self

    def __exit__(self, *exc):
        self.delta = dict(zip(self.names, (kernels.counters(self.names) - self.before).tolist()))
        return False


def rotate(op, q, k, cos_t=0.0, sin_t=0.0):
    """symgpu_rotate_single_dev with cos, sin and clifford_k as given -> (DeviceOp or None, all_commute)."""
    q = np.ascontiguousarray(q, dtype='<u8')
    out, allc = ctypes.c_void_p(), ctypes.c_int(0)
    _lib.check(_lib.lib().symgpu_rotate_single_dev(op.handle, addr(q), float(cos_t), float(sin_t), int(k), 1e-15, byref(out), ctypes.addressof(allc)))
    assert bool(allc.value) == (not out.value)
    return (None if allc.value else DeviceOp(out)), bool(allc.value)


def claims_distinct(op):
    """The cheapest probe of the duplicate-free flag: symgpu_rotate_clifford_chain_dev with no rotation accepts exactly when it is set."""
    out = ctypes.c_void_p()
    rc = _lib.lib().symgpu_rotate_clifford_chain_dev(op.handle, None, None, 0, byref(out))
    if rc == _lib.OK:
        DeviceOp(out).free()
        return True
    assert rc == _lib.E_INVALID and not out.value, (rc, _lib.last_error())
    return False


def mul_into(out, inner, outer, o0, o1, left=True):
    _lib.check(_lib.lib().symgpu_mul_allpairs_dev(inner.handle, outer.handle, int(o0), int(o1), 1 if left else 0, out.handle))


def same(op, rows, coeff):
    got_r, got_c = op.download()
    assert got_r.shape == rows.shape and np.array_equal(got_r, rows) and np.array_equal(got_c, coeff)


class Rig:
    """The device side of a hm.Model: one handle per slot, `apply` performs a step of the model's vocabulary through the library."""

    def __init__(self, n, n_slots):
        self.n, self.wq, self.h = n, hm.words(n), [None] * n_slots

    def put(self, s, new):
        if self.h[s] is not None:
            self.h[s].free()
        self.h[s] = new

    def free(self):
        for s in range(len(self.h)):
            self.put(s, None)

    def apply(self, step, all_commute=False):
        kind, h = step[0], self.h
        if kind == 'fresh':
            _, s, rows, coeff = step
            op = DeviceOp.alloc(hm.CAP, self.wq, True)
            op.write(0, np.ascontiguousarray(rows), np.ascontiguousarray(coeff), rows.shape[0])
            self.put(s, op)
        elif kind == 'write':
            _, s, at, rows, coeff = step
            h[s].write(at, np.ascontiguousarray(rows), np.ascontiguousarray(coeff), rows.shape[0])
        elif kind == 'copy_rows':
            _, s, at, src, begin, k = step
            h[s].copy_rows_from(h[src], begin, k, at)
        elif kind == 'set_rows':
            h[step[1]].set_rows(step[2])
        elif kind == 'set_coeff':
            h[step[1]].set_coeff(step[2])
        elif kind == 'scale':
            h[step[1]].scale(step[2], step[3])
        elif kind == 'mul_into':
            _, s, inner, outer, o0, o1, left = step
            mul_into(h[s], h[inner], h[outer], o0, o1, left)
        elif kind == 'clone':
            self.put(step[1], h[step[2]].clone())
        elif kind == 'gather':
            self.put(step[1], kernels.op_gather(h[step[2]], step[3]))
        elif kind == 'concat':
            self.put(step[1], kernels.concat_dev([h[step[2]], h[step[3]]]))
        elif kind == 'slice':
            self.put(step[1], kernels.slice_dev(h[step[2]], step[3], step[4]))
        elif kind == 'cleanup':
            self.put(step[1], kernels.cleanup_dev(h[step[2]]))
        elif kind == 'mul_cleanup':
            self.put(step[1], kernels.mul_cleanup_handles(h[step[2]], h[step[3]], step[4]))
        elif kind == 'rotate':
            _, dst, src, q, k, cos_t, sin_t = step
            res, allc = rotate(h[src], q, k, cos_t, sin_t)
            assert allc == all_commute, 'the library and the model disagree on whether every row commutes with the generator'
            if res is not None:
                self.put(dst, res)
        elif kind == 'chain':
            self.put(step[1], kernels.rotate_clifford_chain_dev(h[step[1]], step[2], step[3]))
        else:
            raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------- B: the deterministic matrix ----
# cache -> (build counter, path counters of which exactly one moves by 1 per call, {n: environment})
CONSUMERS = {
    'wm': ('OP_WORD_MAJOR_BUILDS', ('PRODUCT_WORD_MAJOR_THEN_ROWS', 'PRODUCT_WORD_MAJOR_BESIDE_ROWS'), {70: {'SYMGPU_PRODUCT_FUSED': '0'}, 130: {}}),
    'yc': ('OP_YCOUNT_BUILDS', ('PRODUCT_PHASE_STREAM',), {70: {}}),
    'bt': ('OP_BIT_MAJOR_BUILDS', ('COMMUTE_M4R_TILE',), {70: {'SYMGPU_COMMUTE_M4R': '1'}, 130: {'SYMGPU_COMMUTE_M4R': '1'}}),
    'hash': ('OP_ROW_HASH_BUILDS', ('ROTATE_HASH_JOIN',), {70: {'SYMGPU_ROT_RESIDENT': '0'}, 130: {'SYMGPU_ROT_RESIDENT': '0'}}),
}
ALL_BUILDS = tuple(v[0] for v in CONSUMERS.values())
H, SRC, OUTER = 0, 1, 2            # the slots of the matrix: the handle under test, the source of row copies / inner operand, an outer operand


def partner_of(rows):
    """Q = rows[a] ^ rows[b] of the first anticommuting pair: a rotation by it must merge rows[a] Q into rows[b]."""
    for a in range(rows.shape[0]):
        for b in range(a + 1, rows.shape[0]):
            if not hm.commutes(rows[a:a + 1], rows[b:b + 1])[0, 0]:
                return rows[a] ^ rows[b]
    raise AssertionError('no two rows anticommute')


@pytest.mark.parametrize('cache,n', [(c, n) for c, v in CONSUMERS.items() for n in v[2]])
def test_every_cache_follows_the_rows(cache, n, monkeypatch):
    build, paths, env = CONSUMERS[cache]
    for key, value in env[n].items():
        monkeypatch.setenv(key, value)
    rng = np.random.default_rng([7, n, len(cache)])
    T = 100
    model, rig = hm.Model(3), Rig(n, 3)
    left_rows = hm._random_rows(rng, 70, n)                                  # the left operand of the commutation consumer
    probe_rows, probe_coeff = hm._random_rows(rng, 3, n), hm._dyadic(rng, 3)  # the outer operand of the product consumer
    left, probe, scratch = DeviceOp.upload(left_rows), DeviceOp.upload(probe_rows, probe_coeff), DeviceOp.alloc(3 * hm.CAP, hm.words(n), True)
    probe.ycount()                                                           # its own Y counts are built here, not under the counters below

    def expected():
        rows, coeff = model.slots[H].live()
        if cache in ('wm', 'yc'):
            return hm.product(rows, coeff, probe_rows, probe_coeff, True)
        if cache == 'bt':
            return (hm.commutes(left_rows, rows),)
        return hm.rotate(rows, coeff, partner_of(rows), -1, 0.5, 0.75)[:2]

    def consume():
        if cache in ('wm', 'yc'):
            mul_into(scratch, rig.h[H], probe, 0, 3)
            return scratch.download()
        if cache == 'bt':
            return (kernels.commutes_handles(left, rig.h[H]),)
        res, all_commute = rotate(rig.h[H], partner_of(model.slots[H].live()[0]), -1, 0.5, 0.75)
        assert not all_commute
        with res:
            return res.download()

    previous = [None]

    def check(label, want_builds, answer_changes):
        want = expected()
        with Counted(*ALL_BUILDS, *paths) as c:
            got = consume()
        print(f'{cache} n={n} {label}: builds {c.delta[build]} (want {want_builds}), paths {[c.delta[p] for p in paths]}')
        assert len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), label
        assert sum(c.delta[p] for p in paths) == 1, (label, c.delta)
        assert c.delta[build] == want_builds, (label, c.delta)
        if cache != 'yc':                                                    # (the product also reads the Y counts where it streams phase bytes)
            assert all(c.delta[b] == 0 for b in ALL_BUILDS if b not in (build, 'OP_YCOUNT_BUILDS')), (label, c.delta)
        if answer_changes:
            assert not all(p.shape == w.shape and np.array_equal(p, w) for p, w in zip(previous[0], want)), f'{label}: the mutator did not change the answer'
        previous[0] = want

    def step(label, s, want_builds, answer_changes=True):
        model.apply(s)
        rig.apply(s)
        assert rig.h[H].n_terms == model.slots[H].T
        check(label, want_builds, answer_changes)

    try:
        for s in (('fresh', H, hm._random_rows(rng, T, n), hm._dyadic(rng, T)), ('fresh', SRC, hm._random_rows(rng, T, n), hm._dyadic(rng, T)),
                  ('fresh', OUTER, hm._random_rows(rng, 60, n), hm._dyadic(rng, 60))):
            model.apply(s)
            rig.apply(s)
        check('warm', 1, False)
        check('repeat', 0, False)
        step('op_write over all rows', ('write', H, 0, hm._random_rows(rng, T, n), hm._dyadic(rng, T)), 1)
        step('op_write of two rows in the middle', ('write', H, T // 2, hm._random_rows(rng, 2, n), hm._dyadic(rng, 2)), 1)
        step('op_write that grows T', ('write', H, T - 1, hm._random_rows(rng, 4, n), hm._dyadic(rng, 4)), 1)
        step('op_copy_rows into the middle', ('copy_rows', H, 40, SRC, 10, 30), 1)
        step('set_rows down', ('set_rows', H, T - 30), 1)
        step('set_rows back up', ('set_rows', H, T + 3), 1)                   # rows [T - 30, T + 3) are read again
        step('out of mul_allpairs_dev, first slab', ('mul_into', H, SRC, OUTER, 0, 1, True), 1)
        step('out of mul_allpairs_dev, second slab', ('mul_into', H, SRC, OUTER, 1, 2, True), 1)
        check('repeat after the slabs', 0, False)
        step('set_coeff', ('set_coeff', H, hm._dyadic(rng, model.slots[H].T)), 0, answer_changes=cache != 'bt')
        step('scale', ('scale', H, 0.5j, True), 0, answer_changes=cache != 'bt')
        kernels.op_set_first_index(rig.h[H], np.arange(model.slots[H].T, dtype='<u8'))
        check('op_set_first_index', 0, False)
        assert np.array_equal(kernels.op_first_index(rig.h[H]), np.arange(model.slots[H].T, dtype='<u8'))
    finally:
        rig.free()
        for op in (left, probe, scratch):
            op.free()


def test_ycount_entry_point_reads_the_cached_counts():
    """symgpu_op_ycount is the other reader of `yc`: built once, hit, rebuilt after an overwrite with T unchanged."""
    rng = np.random.default_rng(17)
    rows, other = hm._random_rows(rng, 90, 70), hm._random_rows(rng, 90, 70)
    assert not np.array_equal(hm.y_count(rows), hm.y_count(other))
    with DeviceOp.upload(rows) as op:
        for label, want_rows, builds in (('warm', rows, 1), ('repeat', rows, 0), ('overwritten', other, 1), ('repeat', other, 0)):
            if label == 'overwritten':
                op.write(0, other, None, 90)
            with Counted('OP_YCOUNT_BUILDS') as c:
                got = op.ycount()
            assert np.array_equal(got, hm.y_count(want_rows)) and c.delta['OP_YCOUNT_BUILDS'] == builds, (label, c.delta)


# ------------------------------------------------------------------------------------------------ hashes: no guard against T ----
def rotate_and_compare(op, rows, coeff, q, k, cos_t=0.0, sin_t=0.0):
    """One rotation of the handle against the model on its mirror -> (result handle, result rows, result coefficients, counter deltas)."""
    er, ec, all_commute = hm.rotate(rows, coeff, q, k, cos_t, sin_t)
    assert not all_commute
    with Counted('OP_ROW_HASH_BUILDS', *ROTATION_STAGES) as c:
        res, allc = rotate(op, q, k, cos_t, sin_t)
    assert not allc and sum(c.delta[s] for s in ROTATION_STAGES) == 1, c.delta
    same(res, er, ec)
    return res, er, ec, c.delta


@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('resident', ['0', None])
def test_overwritten_rows_are_hashed_again(n, resident, monkeypatch):
    """A handle's hashes carry their seed and nothing else: no row count, no version.  Hashes cached on an operand by a non-Clifford
    rotation, hashes handed on to a rotation's result, to the result of a second rotation, and through a Clifford rotation: each handle
    is overwritten with other rows over [0, T) — T unchanged — and rotated by the XOR of two of its NEW rows.  A join on the old hashes
    would miss that partner.  Before each overwrite a plain repeat shows that the hashes really were there (no build)."""
    if resident is not None:
        monkeypatch.setenv('SYMGPU_ROT_RESIDENT', resident)
    join = 'ROTATE_HASH_JOIN' if resident == '0' else None
    rng = np.random.default_rng([23, n])
    T = 40
    rows, coeff = hm._random_rows(rng, T, n), hm._dyadic(rng, T)
    live = []

    def overwrite(op, t):
        new_rows, new_coeff = hm._random_rows(rng, t, n), hm._dyadic(rng, t)
        op.write(0, new_rows, new_coeff, t)
        assert op.n_terms == t
        return new_rows, new_coeff

    try:
        P = DeviceOp.upload(rows, coeff)
        live.append(P)
        # the operand: hashed by its first rotation, hit by the second, hashed again after the overwrite
        R1, r1, c1, d = rotate_and_compare(P, rows, coeff, partner_of(rows), -1, 0.5, 0.75)
        live.append(R1)
        assert d['OP_ROW_HASH_BUILDS'] == 1 and (join is None or d[join] == 1), d
        res, _, _, d = rotate_and_compare(P, rows, coeff, partner_of(rows[5:]), -1, 0.75, 0.5)
        res.free()
        assert d['OP_ROW_HASH_BUILDS'] == 0, d
        rows, coeff = overwrite(P, T)
        res, _, _, d = rotate_and_compare(P, rows, coeff, partner_of(rows), -1, 0.5, 0.75)
        res.free()
        assert d['OP_ROW_HASH_BUILDS'] == 1, d
        # the result of a rotation (hashes handed on): hit, overwritten, hashed again; then the same for the result of its rotation
        for depth in (1, 2):
            res, _, _, d = rotate_and_compare(R1, r1, c1, partner_of(r1[3:]), -1, 0.75, 0.5)
            res.free()
            assert d['OP_ROW_HASH_BUILDS'] == 0, (depth, d)                   # handed on: nothing to hash
            r1, c1 = overwrite(R1, r1.shape[0])
            R2, r2, c2, d = rotate_and_compare(R1, r1, c1, partner_of(r1), -1, 0.5, 0.75)
            assert d['OP_ROW_HASH_BUILDS'] == 1 and (join is None or d[join] == 1), (depth, d)
            live.append(R2)
            R1, r1, c1 = R2, r2, c2
        # through a Clifford rotation (the fast path hands the operand's hashes on, XORed with h(Q)), then a non-Clifford one of the result
        for k in (1, 2):
            C, rc_, cc_, d = rotate_and_compare(R1, r1, c1, partner_of(r1), k)
            live.append(C)
            assert d['OP_ROW_HASH_BUILDS'] == 0 and (resident != '0' or d['ROTATE_CLIFFORD_FAST'] == 1), (k, d)
            res, _, _, d = rotate_and_compare(C, rc_, cc_, partner_of(rc_[2:]), -1, 0.75, 0.5)
            res.free()
            assert d['OP_ROW_HASH_BUILDS'] == 0, (k, d)                       # the Clifford result came with hashes
            rc_, cc_ = overwrite(C, rc_.shape[0])
            res, _, _, d = rotate_and_compare(C, rc_, cc_, partner_of(rc_), -1, 0.5, 0.75)
            res.free()
            assert d['OP_ROW_HASH_BUILDS'] == 1, (k, d)
    finally:
        for op in live:
            op.free()


# ------------------------------------------------------------------------------- the duplicate-free flag earned as a side effect ----
@pytest.mark.parametrize('plant', ['op_write', 'op_copy_rows', 'mul_allpairs_dev', 'set_coeff'])
@pytest.mark.parametrize('n', [70, 130])
def test_a_flag_earned_by_a_rotation_does_not_outlive_the_rows(plant, n, monkeypatch):
    """Distinct rows are uploaded (flag clear), one non-Clifford rotation marks the INPUT duplicate free, then a writer plants a
    duplicate.  The odd Clifford rotation that follows must look for duplicates again, find one and merge (ROTATE_GENERAL_BY_DUP_CHECK), and
    be the reference's rotation; had the flag survived, the per-row fast path would return both copies.  set_coeff is the contrast: the
    rows stay, the flag stays, no check, the fast path."""
    monkeypatch.setenv('SYMGPU_ROT_RESIDENT', '0')
    rng = np.random.default_rng([29, n])
    T = 80
    rows, coeff = hm._random_rows(rng, T, n), hm._dyadic(rng, T)
    twice_rows, twice_coeff = np.vstack([rows[5], rows[5]]), hm._dyadic(rng, 2)
    U = lambda r: hm.unpack(r, n)
    with DeviceOp.alloc(2 * T, hm.words(n), True) as op, DeviceOp.upload(rows, coeff) as src, DeviceOp.upload(twice_rows, twice_coeff) as twice:
        op.write(0, rows, coeff, T)
        assert not claims_distinct(op)
        res, _ = rotate(op, partner_of(rows), -1, 0.5, 0.75)
        res.free()
        assert claims_distinct(op), 'the hash join did not mark its duplicate-free input'
        if plant == 'op_write':                                              # a copy of row 0 over row 1
            op.write(1, rows[0:1].copy(), coeff[0:1].copy(), 1)
            rows[1], coeff[1] = rows[0], coeff[0]
        elif plant == 'op_copy_rows':                                        # the same from a handle that holds the same rows
            op.copy_rows_from(src, 0, 1, 1)
            rows[1], coeff[1] = rows[0], coeff[0]
        elif plant == 'mul_allpairs_dev':                                    # both outer rows are one row: every product row comes twice
            mul_into(op, src, twice, 0, 2)
            rows, coeff = hm.product(rows, coeff, twice_rows, twice_coeff, True)
        else:
            coeff = hm._dyadic(rng, T)
            op.set_coeff(coeff)
        planted = plant != 'set_coeff'
        assert claims_distinct(op) == (not planted) and hm.distinct(rows) == (not planted)
        q = next(r for r in hm._random_rows(rng, 50, n) if not hm.commutes(rows[0:1], r[None, :])[0, 0])     # row 0 (which has a twin) is rotated
        er, ec = onp.rotate_by_single_pword(U(rows), coeff, U(q[None, :])[0], np.pi / 2)
        assert not planted or er.shape[0] < rows.shape[0]                    # the reference merged the twins
        with Counted('ROTATE_GENERAL_BY_DUP_CHECK', 'ROTATE_CLIFFORD_FAST', 'ROTATE_GENERAL') as c:
            res, all_commute = rotate(op, q, 1)
        with res:
            assert not all_commute
            got_r, got_c = res.download()
            assert_op_equal(U(got_r), got_c, er, ec)
            assert c.delta == ({'ROTATE_GENERAL_BY_DUP_CHECK': 1, 'ROTATE_CLIFFORD_FAST': 0, 'ROTATE_GENERAL': 1} if planted else
                               {'ROTATE_GENERAL_BY_DUP_CHECK': 0, 'ROTATE_CLIFFORD_FAST': 1, 'ROTATE_GENERAL': 0}), c.delta
            assert claims_distinct(res) == (not planted)


# ------------------------------------------------------------------------------------------------------------ the flag as a gate ----
def state(rng, n, t):
    """A clean state of t distinct basis strings on n qubits as packed rows, with dyadic amplitudes."""
    bits = np.zeros((t, n), dtype=bool)
    bits[:, :16] = (np.arange(1, t + 1)[:, None] >> np.arange(16)) & 1       # distinct by construction
    bits[:, 16:] = rng.random((t, n - 16)) < 0.5
    return bits, hm.pack(fam.state_symp(bits)), fam.amplitudes(rng, t, 'dyadic')


def gates(op, term_op):
    """How the three entry points that require a duplicate-free operand answer for `op` -> (chain probe, state_inner_dev, expval_terms_dev),
    each True (accepted) or False (SYMGPU_E_INVALID); nothing may leak either way."""
    lib = _lib.lib()
    before = kernels.counters(BALANCE)
    out2, total = np.zeros(2), np.zeros(2)
    answers = [claims_distinct(op)]
    for rc in (lib.symgpu_state_inner_dev(op.handle, op.handle, addr(out2)),
               lib.symgpu_expval_terms_dev(term_op.handle, op.handle, op.handle, None, addr(total), None)):
        assert rc in (_lib.OK, _lib.E_INVALID), (rc, _lib.last_error())
        answers.append(rc == _lib.OK)
    assert np.array_equal(kernels.counters(BALANCE), before), 'a gated call leaked or double-freed a block'
    return tuple(answers), complex(*out2), complex(*total)


@pytest.mark.parametrize('n', [70, 130])
def test_the_flag_gates_three_entry_points(n):
    rng = np.random.default_rng([31, n])
    T = 90
    bits, rows, amp = state(rng, n, T)
    term_symp = rng.random((12, 2 * n)) < 0.1
    term_symp[:, :n] = False                                                 # diagonal terms: every one has a non-zero expectation value
    term_coeff = eo.amplitudes(rng, 12, 'dyadic')
    inner_want = fam.inner_sequential(rows, amp, rows, amp)
    expval_want = eo.total(term_coeff, eo.term_elements(term_symp, bits, amp, bits, amp))
    yes, no = (True, True, True), (False, False, False)
    with DeviceOp.upload(rows, amp) as raw, DeviceOp.upload(hm.pack(term_symp), term_coeff) as terms, DeviceOp.upload(hm._random_rows(rng, 5, n), hm._dyadic(rng, 5)) as src:
        kernels.cleanup_dev(raw).free()                                      # (what the context keeps after its first cleanup)
        gates(raw, terms)
        assert gates(raw, terms)[0] == no, 'a fresh upload claims to be duplicate free'
        mutators = {
            'op_write of one row': lambda h: h.write(3, rows[3:4].copy(), amp[3:4].copy(), 1),            # the very same row: a write is a write
            'op_copy_rows': lambda h: h.copy_rows_from(src, 0, 2, 4),
            'set_rows': lambda h: h.set_rows(T - 1),
            'out of mul_allpairs_dev': lambda h: mul_into(h, src, src, 0, 2),
        }
        for label, mutate in mutators.items():
            with kernels.cleanup_dev(raw) as clean:
                same(clean, rows, amp)
                answers, inner, total = gates(clean, terms)
                assert answers == yes, label
                assert fam.same_bits(inner.real, inner_want[0]) and fam.same_bits(inner.imag, inner_want[1]) and total == expval_want
                clean.set_coeff(amp)
                clean.scale(1.0, False)
                assert gates(clean, terms)[0] == yes, 'set_coeff / scale dropped the flag'
                mutate(clean)
                assert gates(clean, terms)[0] == no, label
        # who may claim the flag without a cleanup of their own, and who may not
        with kernels.cleanup_dev(raw) as clean:
            with clean.clone() as twin:
                assert gates(twin, terms)[0] == yes, 'a clone of a duplicate-free handle holds the same rows'
            with kernels.op_gather(clean, np.array([4, 9, 4], dtype=np.int64)) as g, kernels.concat_dev([clean, clean]) as cc, \
                    kernels.slice_dev(clean, 2, 40) as sl, DeviceOp.upload(rows, amp) as fresh, raw.clone() as raw_twin:
                for label, h in (('op_gather with a repeated index', g), ('concat_dev with itself', cc), ('slice_dev', sl), ('upload', fresh),
                                 ('clone of an unflagged handle', raw_twin)):
                    assert gates(h, terms)[0] == no, label


# ------------------------------------------------------------------------------------------------ the first-occurrence index ----
@pytest.mark.parametrize('n', [70, 130])
def test_first_occurrence_index_goes_with_the_rows(n):
    rng = np.random.default_rng([37, n])
    T = 90
    rows, coeff = hm._random_rows(rng, T, n), hm._dyadic(rng, T)
    rows[60:80] = rows[10:30]                                                # twenty repeated rows
    er, ec = hm.cleanup(rows, coeff)
    index = {r.tobytes(): t for t, r in reversed(list(enumerate(rows)))}     # the first occurrence of every row
    first = np.array([index[r.tobytes()] for r in er], dtype='<u8')
    lib = _lib.lib()

    def indexed(fn, *operands):
        out = ctypes.c_void_p()
        _lib.check(fn(*[o.handle for o in operands], *((1,) if len(operands) == 2 else ()), 1e-15, 1, byref(out)))
        return DeviceOp(out)

    def refuses(op):
        buf = np.zeros(max(1, op.n_terms), dtype='<u8')
        assert lib.symgpu_op_first_index(op.handle, addr(buf), buf.shape[0]) == _lib.E_INVALID
        assert 'does not come from an *_indexed cleanup' in _lib.last_error()
        one = np.zeros(1, dtype=np.int64)
        assert lib.symgpu_part_global_index(op.handle, addr(one), 1, addr(one), 1, 1) == _lib.E_INVALID
        assert 'does not come from' in _lib.last_error()

    a_rows, a_coeff, b_rows, b_coeff = rows[:6], coeff[:6], rows[6:11].copy(), coeff[6:11]
    b_rows[4] = b_rows[0] ^ a_rows[0] ^ a_rows[1]                            # a planted merge: a0 b4 = a1 b0
    pr, pc = hm.product(a_rows, a_coeff, b_rows, b_coeff, True)
    per, pec = hm.cleanup(pr, pc)
    p_index = {r.tobytes(): t for t, r in reversed(list(enumerate(pr)))}
    p_first = np.array([((p_index[r.tobytes()] // 6) << 32) | (p_index[r.tobytes()] % 6) for r in per], dtype='<u8')
    assert per.shape[0] < 30
    mutators = {
        'op_write': lambda h: h.write(0, rows[80:81].copy(), coeff[80:81].copy(), 1),
        'op_copy_rows': lambda h, src=None: h.copy_rows_from(src, 0, 1, 1),
        'set_rows': lambda h: h.set_rows(h.n_terms - 1),
    }
    with DeviceOp.upload(rows, coeff) as raw, DeviceOp.upload(a_rows, a_coeff) as A, DeviceOp.upload(b_rows, b_coeff) as B:
        refuses(raw)
        for label in list(mutators) + ['out of mul_allpairs_dev']:
            with indexed(lib.symgpu_cleanup_indexed_dev, raw) as res, indexed(lib.symgpu_mul_cleanup_indexed_dev, A, B) as prod:
                same(res, er, ec)
                same(prod, per, pec)
                assert np.array_equal(kernels.op_first_index(res), first) and np.array_equal(kernels.op_first_index(prod), p_first)
                res.set_coeff(ec)
                res.scale(2.0, False)
                assert np.array_equal(kernels.op_first_index(res), first), 'set_coeff / scale dropped the index'
                for h in (res, prod):
                    if label == 'op_copy_rows':
                        mutators[label](h, raw)
                    elif label == 'out of mul_allpairs_dev':
                        mul_into(h, A, B, 0, 1)
                    else:
                        mutators[label](h)
                    refuses(h)
        # an index attached by hand stays through a change of coefficients and goes with the rows
        with DeviceOp.upload(er, ec) as op:
            keys = np.arange(100, 100 + er.shape[0], dtype='<u8')
            kernels.op_set_first_index(op, keys)
            op.set_coeff(ec * 0.5)
            assert np.array_equal(kernels.op_first_index(op), keys)
            op.write(2, er[0:1].copy(), ec[0:1].copy(), 1)
            refuses(op)


# -------------------------------------------------------------------------------------------------- D: the model's sequences ----
def observe(rig, model, seq, s, probe, scratch, monkeypatch, where):
    """Every observer on slot s against the model's mirror."""
    slot, h = model.slots[s], rig.h[s]
    rows, coeff = slot.live()
    t, _, cap = h.info()
    assert t == slot.T and cap >= slot.cap, (where, t, slot.T, cap, slot.cap)
    got_r, got_c = h.download()
    assert np.array_equal(got_r, rows) and np.array_equal(got_c, coeff), (where, 'download')
    assert np.array_equal(h.ycount(), hm.y_count(rows)), (where, 'ycount')
    o = (s + 1) % seq.n_slots
    table = hm.commutes(model.slots[o].live()[0], rows)
    for m4r in ('0', '1'):
        monkeypatch.setenv('SYMGPU_COMMUTE_M4R', m4r)
        assert np.array_equal(kernels.commutes_handles(rig.h[o], h), table), (where, 'commutes', m4r)
    monkeypatch.delenv('SYMGPU_COMMUTE_M4R')
    pr, pc = hm.product(rows, coeff, seq.probe_rows, seq.probe_coeff, True)
    for fused in ('1', '0'):
        monkeypatch.setenv('SYMGPU_PRODUCT_FUSED', fused)
        mul_into(scratch, h, probe, 0, seq.probe_rows.shape[0])
        got_r, got_c = scratch.download()
        assert np.array_equal(got_r, pr) and np.array_equal(got_c, pc), (where, 'product', fused)
    monkeypatch.delenv('SYMGPU_PRODUCT_FUSED')
    claimed = claims_distinct(h)
    assert not claimed or slot.distinct(), (where, 'the handle claims to be duplicate free and holds two equal rows')
    assert claimed or not slot.distinct_known, (where, 'the handle does not know that its rows are distinct')


@pytest.mark.parametrize('n', hm.GPU_SIZES)
@pytest.mark.parametrize('seed', hm.GPU_SEEDS)
def test_model_sequences(seed, n, monkeypatch):
    """The sequence of (seed, n) step by step on real handles (tests/test_handle_model.py asserts on the CPU that it holds every hazard);
    after every step every observer on every slot the step touched.  No step is left out: one the library refuses fails the test."""
    seq = hm.generate(seed, n)
    model, rig = hm.Model(seq.n_slots), Rig(n, seq.n_slots)
    probe = DeviceOp.upload(seq.probe_rows, seq.probe_coeff)
    scratch = DeviceOp.alloc(seq.probe_rows.shape[0] * (hm.MAX_T + 20), hm.words(n), True)
    try:
        for i, step in enumerate(seq.steps):
            all_commute = step[0] == 'rotate' and model.all_commute(step)
            touched = model.apply(step)
            rig.apply(step, all_commute)
            if i + 1 < seq.n_slots:
                continue                                                     # the observers need every slot to exist
            for s in (range(seq.n_slots) if i + 1 == seq.n_slots else touched):
                observe(rig, model, seq, s, probe, scratch, monkeypatch, (seed, n, i, step[0], s))
    finally:
        rig.free()
        probe.free()
        scratch.free()
