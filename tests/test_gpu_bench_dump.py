"""GPU: `bench.py --dump-outputs DIR` writes what the timed product path computed in its last step — a seeded sample of the last output
slab's product rows with their coefficients — identical from run to run and equal to the C oracle's product of the same operands."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NI, M, N_QUBITS, STEPS = 400, 700, 1000, 2        # slabs of 256 outer rows: the last one holds outer rows 512..699, 188 * 400 = 75,200 rows (sampled)


def _bench_dump(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', '0', '--left-terms', str(NI),
                        '--right-terms', str(M), '--qubits', str(N_QUBITS), '--no-extras', '--no-cpu', '--dump-outputs', str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    doc = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][-1])
    assert doc['steps'] == STEPS and doc['ms_per_step'] > 0
    names = sorted(os.listdir(out_dir))
    assert names == ['product_coeff.npy', 'product_pair_index.npy', 'product_rows_u32.npy'], names
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in names) <= 64 * 10**6
    out = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in names}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


@pytest.mark.timeout(900)
def test_bench_dump_outputs_are_reproducible_and_match_the_oracle(tmp_path):
    from symmer_amd import _lib
    from symmer_amd.kernels import DeviceOp
    from oracle import oracle_c as oc
    a = _bench_dump(tmp_path / 'a')
    b = _bench_dump(tmp_path / 'b')
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the same operands as bench.py's single-rank product: left (inner) seed 1234, right (outer) seed 99991
    _lib.init(0)
    left, right = DeviceOp.random(NI, N_QUBITS, 0.3, seed=1234), DeviceOp.random(M, N_QUBITS, 0.3, seed=99991)
    (lr, lc), (rr, rc) = left.download(), right.download()
    left.free(); right.free()
    o_begin = ((M + 255) // 256 - 1) * 256
    er, ec = oc.mul_allpairs(lr, lc, rr[o_begin:], rc[o_begin:], True)
    pair = a['product_pair_index'].astype(np.int64)
    assert np.array_equal(pair, a['product_pair_index']) and len(np.unique(pair)) == pair.shape[0] == 65536
    r = pair - o_begin * NI
    assert r.min() >= 0 and r.max() < er.shape[0]
    words = a['product_rows_u32'].astype(np.uint64)
    rows = words[:, 0::2] | (words[:, 1::2] << np.uint64(32))
    assert np.array_equal(rows, er[r])
    assert np.array_equal(a['product_coeff'][:, 0], ec[r].real) and np.array_equal(a['product_coeff'][:, 1], ec[r].imag)
