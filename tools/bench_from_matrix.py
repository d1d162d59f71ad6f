"""PauliwordOp.from_matrix on the device (csrc/pauli_decomp.hip), timed on the GPU box: dense Gaussian matrices of n = 10, 11, 12 qubits
(all 4^n coefficients) and the CSR matrix of the BH STO-3G Hamiltonian (tests/golden/BH_STO-3G_SINGLET_JW.json).

Per shape: the whole C-ABI call (upload of the matrix, diagonals, gather, transform, select) between `symgpu_timer_start` /
`symgpu_timer_stop` and on the wall clock, best of `--reps` after one warm-up call.  Kernel times do not come from this process: with
`--profile` (the default) every shape is run once more in a child process under `rocprofv3 --kernel-trace --stats`, a run of its own,
and every kernel of the call is read from its database; per stage the tool prints the achieved bytes/s of the algorithmic
traffic 2 * 16 * D * 2^n (one read and one write of the [D][2^n] complex128 scratch) against the 8 TB/s HBM peak.

    python tools/bench_from_matrix.py [--reps 3] [--shapes dense:10,dense:11,dense:12,csr:BH] [--no-profile] [--out profiles/from_matrix_bench.txt]
"""
import argparse
import ctypes
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK = 8.0e12
STAGES = {'gather': ('k_pd_gather_dense', 'k_pd_scatter', 'k_pd_csr_keys', 'k_pd_csr_check_indptr', 'k_pd_heads', 'k_pd_compact_xs'),
          'transform': ('k_pd_wht_tile', 'k_pd_wht_strided'),
          'select': ('k_pd_count', 'k_pd_emit', 'k_pd_pick'),
          'other': ()}       # every kernel of another file: the radix sort of the CSR keys and the scans (sort.hip)


def make_input(shape, cache=None):
    """(n, dense matrix or None, CSR matrix or None).  `cache`: an .npz with the CSR arrays of a 'csr:' shape, so that a profiled child
    run launches no kernel besides from_matrix's (building the Hamiltonian's matrix takes the device too)."""
    kind, what = shape.split(':')
    if cache and kind == 'csr':
        import scipy.sparse
        z = np.load(cache)
        n = int(z['n'])
        return n, None, scipy.sparse.csr_matrix((z['data'], z['indices'], z['indptr']), shape=(1 << n, 1 << n))
    if kind == 'dense':
        n = int(what)
        rng = np.random.default_rng(n)
        m = rng.standard_normal((1 << n, 1 << n)) + 1j * rng.standard_normal((1 << n, 1 << n))
        return n, m, None
    from symmer_amd import PauliwordOp
    with open(os.path.join(ROOT, 'tests', 'golden', f'{what}_STO-3G_SINGLET_JW.json')) as f:
        d = json.load(f)
    H = PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()})
    return H.n_qubits, None, H.to_sparse_matrix


def run_shape(shape, reps, cache=None):
    from symmer_amd import _lib, kernels
    lib = _lib.lib()
    n, dense, sp = make_input(shape, cache)
    best_ev, best_wall, terms, form = None, None, 0, 0
    for rep in range(reps + 1):                                   # the first call warms the allocator and the kernels
        ms = ctypes.c_float(0)
        t0 = time.perf_counter()
        _lib.check(lib.symgpu_timer_start())
        if dense is not None:
            dev, terms, form = kernels.pauli_decompose_dense(dense, n)
        else:
            dev, terms, form = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n)
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        wall = time.perf_counter() - t0
        dev.free()
        if rep and (best_ev is None or ms.value < best_ev):
            best_ev, best_wall = ms.value, wall * 1e3
    if dense is not None:
        D, in_bytes = 1 << n, dense.nbytes
    else:
        D = len(np.unique(np.repeat(np.arange(1 << n), np.diff(sp.indptr)) ^ sp.indices))
        in_bytes = sp.data.nbytes + sp.indices.nbytes + sp.indptr.nbytes
    return dict(shape=shape, n=n, D=int(D), slots=int(D) << n, input_bytes=int(in_bytes), terms=int(terms),
                form={1: 'one pass', 2: 'two pass'}[form], call_ms_events=best_ev, call_ms_wall=best_wall,
                algorithmic_bytes_per_stage=2 * 16 * (int(D) << n))


def profile_shape(shape, reps):
    """Kernel times of one shape from a rocprofv3 run of its own: {kernel: (calls per from_matrix call, min us, avg us)}."""
    if not shutil.which('rocprofv3'):
        return None
    out = tempfile.mkdtemp(prefix='from_matrix_prof_')
    try:
        cache = os.path.join(out, 'input.npz')
        if shape.startswith('csr:'):
            n, _, sp = make_input(shape)
            np.savez(cache, n=n, data=sp.data, indices=sp.indices, indptr=sp.indptr)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out, '-o', 't', '--', sys.executable, os.path.abspath(__file__), '--shapes', shape,
               '--reps', str(reps), '--no-profile', '--out', os.devnull, '--cache', cache]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        db = [os.path.join(r, f) for r, _, fs in os.walk(out) for f in fs if f.endswith('_results.db')][0]
        rows = sqlite3.connect(db).execute("select name, count(*), min(duration), avg(duration) from kernels group by name").fetchall()
        return {name: (cnt / (reps + 1), mn / 1e3, av / 1e3) for name, cnt, mn, av in rows}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def stage_lines(res, kern):
    lines = []
    for stage, names in STAGES.items():
        us = sum(per_call * mn for k, (per_call, mn, _) in kern.items() if (any(nm in k for nm in names) if names else 'k_pd_' not in k))
        if us <= 0:
            continue
        if not names:                                             # launches of other files: a time, no traffic model
            lines.append(f'    {stage:9s} {us:10.1f} us per call')
            continue
        rate = res['algorithmic_bytes_per_stage'] / (us * 1e-6)
        lines.append(f'    {stage:9s} {us:10.1f} us per call   {rate / 1e9:9.1f} GB/s of 2*16*D*2^n   {rate / HBM_PEAK:6.3f} of the 8 TB/s peak')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='dense:10,dense:11,dense:12,csr:BH')
    ap.add_argument('--no-profile', action='store_true', help='no child runs under rocprofv3 (call times only)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'from_matrix_bench.txt'))
    ap.add_argument('--cache', default=None, help='(the profiled child runs) .npz holding the CSR arrays of a csr: shape')
    a = ap.parse_args()
    from symmer_amd import _lib
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    text = [f'# tools/bench_from_matrix.py --reps {a.reps} --shapes {a.shapes} on {name.value.decode()}',
            '# call times: symgpu_timer_* (HIP events) around the whole C-ABI call, matrix upload included; best of the repetitions',
            '# kernel times: a `rocprofv3 --kernel-trace --stats` run of their own per shape; minimum per kernel, summed per stage']
    results = [run_shape(s, a.reps, a.cache) for s in a.shapes.split(',')]
    for res in results:
        text.append(json.dumps(res))
    if not a.no_profile:
        for res in results:
            kern = profile_shape(res['shape'], a.reps)
            text.append(f'## {res["shape"]}: n = {res["n"]}, D = {res["D"]}, {res["form"]}, {res["terms"]} terms, call {res["call_ms_events"]:.3f} ms')
            if kern is None:
                text.append('    rocprofv3 not found: no kernel times')
                continue
            for k, (per_call, mn, av) in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                text.append(f'    {per_call:5.1f} x {mn:10.1f} us (avg {av:10.1f})  {k[:110]}')
            text += stage_lines(res, kern)
    print('\n'.join(text))
    if a.out != os.devnull:
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
