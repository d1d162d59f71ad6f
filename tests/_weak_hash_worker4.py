# as _weak_hash_worker.py .. _weak_hash_worker3.py, for symgpu_expval_terms_dev (csrc/expval.hip): a fresh process with SYMGPU_HASH_WEAK_ODD=1, whose
# first seed keeps four hash bits.  The call is the FIRST hashing call of the process, on handles that no cleanup has touched (a cleanup that meets a
# collision reseeds to the full hash and the table would never see the weak one): rows uploaded, indexed 0..S-1 and passed through
# symgpu_merge_indexed_dev without cleanup, which orders by index (no hash) and marks its result duplicate free.  S = 300 basis strings and T = 64
# terms in 16 hash classes: every probe walks rows that are different with equal hashes; dyadic amplitudes, so the answer is exact.  Both forms.
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from symmer_amd import kernels, packing
from symmer_amd.kernels import DeviceOp
import _expval_oracle as ora


def reseeds():
    return kernels.counter('HASH_RESEEDS')


def unhashed_state(bits, amp):
    raw = DeviceOp.upload(packing.pack_rows(ora.state_symp(bits)), amp)
    kernels.op_set_first_index(raw, np.arange(bits.shape[0], dtype='<u8'))
    h = kernels.merge_indexed_dev([raw], key_bits=0, do_cleanup=False)
    raw.free()
    rows, c = h.download()
    assert np.array_equal(rows, packing.pack_rows(ora.state_symp(bits))) and np.array_equal(c, amp), 'the indexed merge reordered the state'
    return h


rng = np.random.default_rng(64)
n, T, S = 12, 64, 300
symp, coeff, bits, amp = ora.random_case(rng, n, T, S, 'dyadic')
phi_bits, phi_amp = bits[:200], ora.amplitudes(rng, 200, 'dyadic') + 0.125j
op = DeviceOp.upload(packing.pack_rows(symp), coeff)
psi, phi = unhashed_state(bits, amp), unhashed_state(phi_bits, phi_amp)
want = ora.term_elements(symp, bits, amp, bits, amp)
want_x = ora.term_elements(symp, phi_bits, phi_amp, bits, amp)
assert np.count_nonzero(want) * 3 >= T and np.count_nonzero(want_x) * 3 >= T
for forced in (None, 'global'):
    os.environ.pop('SYMGPU_EXPVAL_FORM', None)
    if forced:
        os.environ['SYMGPU_EXPVAL_FORM'] = forced
    got, total, form = kernels.expval_terms_dev(op, psi, psi)
    assert reseeds() == 0, 'something reseeded the hash before the look-ups ran'
    assert form == (ora.GLOBAL if forced else ora.LDS)
    assert np.all(got == want) and total == ora.total(coeff, want), np.flatnonzero(got != want)[:8]
    got, total, form = kernels.expval_terms_dev(op, phi, psi)
    assert np.all(got == want_x) and total == ora.total(coeff, want_x), np.flatnonzero(got != want_x)[:8]
os.environ.pop('SYMGPU_EXPVAL_FORM', None)
# the seed the calls hashed with is still the current one (nothing has reseeded): a cleanup of the same 300 distinct rows under it must now meet rows
# with equal hashes and reseed, or the hash was never the four-bit one and the look-ups above compared no unequal rows
assert reseeds() == 0
raw = DeviceOp.upload(packing.pack_rows(ora.state_symp(bits)), amp)
cleaned = kernels.cleanup_dev(raw)
assert cleaned.n_terms == S
detail = reseeds()
assert detail >= 1, 'the hash of the first seed was not weak: the look-ups saw no colliding rows'
for h in (op, psi, phi, raw, cleaned):
    h.free()
print('WEAK_HASH4_OK', detail, flush=True)
