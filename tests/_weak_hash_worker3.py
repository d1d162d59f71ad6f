# as _weak_hash_worker.py / _weak_hash_worker2.py, for the entry points of csrc/project.hip: a fresh process with SYMGPU_HASH_WEAK_ODD=1, whose
# first seed keeps four hash bits.  Modes:
#   inner          symgpu_state_inner_dev FIRST in the process, on handles that no cleanup has touched (a cleanup that meets a collision reseeds to
#                  the full hash and the join would never see the weak one): rows uploaded, indexed 0..T-1 and passed through
#                  symgpu_merge_indexed_dev without cleanup, which orders by index (a radix sort of the indices, no hash) and marks its
#                  result duplicate free.  500 x 3000 rows in 16 hash classes: every probe walks rows that are different with equal hashes.
#   noncontextual  T = 1000: the True operator first (wrongly merged characters would lose set bits and answer False), then a bridge as last term
#   project        70,000 terms collapsing onto at most 64 rows: the cleanup behind the projection on colliding hashes
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from symmer_amd import PauliwordOp, kernels, packing
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
import _f3_f4_families as fam

mode = sys.argv[1]


def reseeds():
    return kernels.counter('HASH_RESEEDS')


if mode == 'inner':
    rng = np.random.default_rng(61)
    a_bits, a_c, b_bits, b_c, match = fam.states(rng, 500, 3000, 70, 'third', 'gauss')
    handles = []
    for bits, c in ((a_bits, a_c), (b_bits, b_c)):
        raw = DeviceOp.upload(packing.pack_rows(fam.state_symp(bits)), c)
        kernels.op_set_first_index(raw, np.arange(bits.shape[0], dtype='<u8'))
        handles.append(kernels.merge_indexed_dev([raw], key_bits=0, do_cleanup=False))
        raw.free()
    for h, bits, c in zip(handles, (a_bits, b_bits), (a_c, b_c)):
        rows, cc = h.download()
        assert np.array_equal(rows, packing.pack_rows(fam.state_symp(bits))) and np.array_equal(cc, c), 'the indexed merge reordered the state'
    got = kernels.state_inner_dev(handles[0], handles[1])
    assert reseeds() == 0, 'something reseeded the hash before the join ran'
    want = fam.inner_sequential(a_bits, a_c, b_bits, b_c)
    assert (match >= 0).sum() == 166
    print('inner', repr(got), repr(want), flush=True)
    assert fam.same_bits(got.real, want[0]) and fam.same_bits(got.imag, want[1]), (got.real.hex(), got.imag.hex(), float(want[0]).hex(), float(want[1]).hex())
    got_t = kernels.state_inner_dev(handles[1], handles[0])
    want_t = fam.inner_sequential(b_bits, b_c, a_bits, a_c)
    assert fam.same_bits(got_t.real, want_t[0]) and fam.same_bits(got_t.imag, want_t[1])
    # the seed that both joins hashed with is still the current one (nothing has reseeded): a cleanup of the same 3000 distinct rows under it
    # must now meet rows with equal hashes and reseed, or the hash was never the four-bit one and the joins above compared no unequal rows
    assert reseeds() == 0
    raw = DeviceOp.upload(packing.pack_rows(fam.state_symp(b_bits)), b_c)
    cleaned = kernels.cleanup_dev(raw)
    assert cleaned.n_terms == b_bits.shape[0]
    detail = reseeds()
    assert detail >= 1, 'the hash of the first seed was not weak: the join saw no colliding rows'
    for h in handles + [raw, cleaned]:
        h.free()
elif mode == 'noncontextual':
    T = 1000
    cases = [c for c in fam.noncontextual_family(T) if c[0] in ('true', f'bridge@{T - 1}')]
    assert [c[0] for c in cases] == ['true', f'bridge@{T - 1}']
    for name, symp, claimed in cases:
        answer = onp.check_adjmat_noncontextual(onp.commutes_termwise(symp, symp))
        assert answer is claimed
        op = PauliwordOp._from_packed(packing.pack_rows(symp), symp.shape[1] // 2, np.ones(T))
        assert op.is_noncontextual is answer, name
    detail = reseeds()                                                     # (three or four distinct characters in 16 classes need not collide)
elif mode == 'project':
    case = fam.projection_family('collapse3-dyadic')
    n = case['symp'].shape[1] // 2
    er, ec, n_survived = fam.projection_expected(case['symp'], case['coeff'], case['stab'], case['eig'], case['keep'])
    op = DeviceOp.upload(packing.pack_rows(case['symp']), case['coeff'])
    res, n_s = kernels.project_dev(op, packing.pack_rows(case['stab']), case['eig'], case['keep'], n)
    rows, c = res.download()
    assert n_s == n_survived and np.array_equal(packing.unpack_rows(rows, case['keep'].size), er) and np.array_equal(c, ec)
    detail = reseeds()
    assert er.shape[0] > 16 and detail >= 1, 'more distinct rows than hash classes: the weak first seed must have forced a reseed'
else:
    raise SystemExit(f'unknown mode {mode}')
print('WEAK_HASH3_OK', mode, detail, flush=True)
