# as _weak_hash_worker.py .. _weak_hash_worker4.py, for row hashes that OUTLIVE their seed: a fresh process with SYMGPU_HASH_WEAK_ODD=1, whose first
# seed keeps four hash bits.  A rotation caches hashes on its operand and hands them on to its result under that seed; then a cleanup meets the
# collisions and reseeds the context's hash; then the operand and the results are rotated again.  Every handle's hash_seed no longer matches the
# context's, so each of them must be hashed afresh (OP_ROW_HASH_BUILDS rises: the proof that the mismatch branch ran) and a Clifford rotation must
# not hand the old hashes on.  Modes: `resident` (the library's default: the one-launch kernel where the operand qualifies, rotate_resident.hip)
# and `multi` (SYMGPU_ROT_RESIDENT=0: hash join and Clifford fast path, rotate_analyze.hip / rotate_fast.hip).
# The operand is clean without a cleanup having run (a cleanup of these rows would reseed at once and no hash of seed 1 would ever be cached): cleaned
# on the host, uploaded, indexed 0..T-1 and passed through symgpu_merge_indexed_dev without cleanup, which sorts by index and marks its result
# duplicate free (as _weak_hash_worker3.py does).
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
mode = sys.argv[1]
assert mode in ('resident', 'multi')
if mode == 'multi':
    os.environ['SYMGPU_ROT_RESIDENT'] = '0'
from symmer_amd import kernels, packing
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
from _golden import assert_op_equal

n, T = 70, 200
rng = np.random.default_rng(35)
dy = lambda t: (rng.integers(1, 9, t) * rng.choice([-1, 1], t) + 1j * rng.integers(-8, 9, t)) / 16.0
reseeds = lambda: kernels.counter('HASH_RESEEDS')
builds = lambda: kernels.counter('OP_ROW_HASH_BUILDS')


def partner(symp, start=0):
    """Q = the XOR of two anticommuting rows: the rotation must merge one into the other."""
    for a in range(start, symp.shape[0]):
        for b in range(a + 1, symp.shape[0]):
            if not onp.commutes_termwise(symp[a:a + 1], symp[b:b + 1])[0, 0]:
                return symp[a] ^ symp[b]
    raise AssertionError('no two rows anticommute')


def flagged(symp, coeff):
    raw = DeviceOp.upload(packing.pack_rows(symp), coeff)
    kernels.op_set_first_index(raw, np.arange(symp.shape[0], dtype='<u8'))
    op = kernels.merge_indexed_dev([raw], key_bits=0, do_cleanup=False)
    raw.free()
    return op


def rotated(op, symp, coeff, q, angle, want_builds, what):
    """One rotation of the handle against the oracle on what the handle holds (exact at a Clifford angle, within 1e-12 otherwise) ->
    (result handle, its rows and coefficients as downloaded: the next rotation's input)."""
    before = builds()
    res, all_commute = kernels.rotate_single_dev(op, packing.pack_rows(q.reshape(1, -1))[0], angle)
    assert not all_commute, what
    er, ec = onp.rotate_by_single_pword(symp, coeff, q, angle)
    rows, c = res.download()
    rows = packing.unpack_rows(rows, n)
    assert_op_equal(rows, c, er, ec, exact=angle != 0.3, tol=1e-12)
    print(what, 'row-hash builds', builds() - before, flush=True)
    assert builds() - before == want_builds, (what, builds() - before, want_builds)
    return res, rows, c


symp, c = onp.cleanup_op(rng.random((T, 2 * n)) < 0.3, dy(T))
assert symp.shape[0] == T
P = flagged(symp, c)
# 1. hashes of seed 1 on P (cached by the rotation) and on two results (handed on)
R1, r1, c1 = rotated(P, symp, c, partner(symp), 0.3, 1, 'P, first rotation')
Rb, rb, cb = rotated(P, symp, c, partner(symp, 7), 0.3, 0, 'P, second rotation (cached hashes)')
assert r1.shape[0] < 2 * T and reseeds() == 0, 'the hashes above were not taken under the first seed'
# 2. a cleanup of more distinct rows than the weak hash has classes: reseed
big = DeviceOp.upload(packing.pack_rows(rng.random((300, 2 * n)) < 0.3), dy(300))
cleaned = kernels.cleanup_dev(big)
assert cleaned.n_terms == 300 and reseeds() >= 1, 'the weak first seed must have forced a reseed'
# 3. P again: its hashes are of the old seed
res, _, _ = rotated(P, symp, c, partner(symp, 3), 0.3, 1, 'P after the reseed')
res.free()
res, _, _ = rotated(P, symp, c, partner(symp, 5), np.pi / 2, 0, 'P after the reseed, odd Clifford')
res.free()
# 4. R1 (handed-on hashes of the old seed): non-Clifford, then Clifford, then non-Clifford, each on the result of the one before
R2, r2, c2 = rotated(R1, r1, c1, partner(r1), 0.3, 1, 'R1 after the reseed')
R3, r3, c3 = rotated(R2, r2, c2, partner(r2, 2), np.pi / 2, 0, 'its result, odd Clifford')
R4, _, _ = rotated(R3, r3, c3, partner(r3, 4), 0.3, 0, 'and a non-Clifford rotation of that (hashes of the new seed, handed on twice)')
# the other result: the Clifford rotation comes first and must not hand the old hashes on, so the rotation after it hashes
Rc, rc_, cc_ = rotated(Rb, rb, cb, partner(rb), np.pi / 2, 0, 'Rb after the reseed, odd Clifford')
Rd, _, _ = rotated(Rc, rc_, cc_, partner(rc_, 1), 0.3, 1, 'and a non-Clifford rotation of that')
for h in (P, R1, Rb, big, cleaned, R2, R3, R4, Rc, Rd):
    h.free()
print('WEAK_HASH_OK', mode, reseeds(), flush=True)
