"""Times the noncontextual sweep (``symgpu_noncon_sweep_dev``, csrc/noncon_sweep.hip) on one MI355X and writes
profiles/noncon_sweep_bench.txt.  Not part of bench.py; reads nothing of the reference.

    python tools/bench_noncon_sweep.py

Operators: ``symgpu_op_random`` at bit density 0.02 (a term touches a few qubits, so that a sweep keeps a good share of the terms and
meets several cliques; the kept count and the clique count stand in every line).  Each device figure is the whole call — the
permutation of the rows, the T x T commutation table, the sweep launch, the masks read back — between ``symgpu_timer_start`` /
``symgpu_timer_stop`` (HIP events): one warm-up call, the median of three.

1. one sweep at T = 1,000 and 10,000 (100 qubits) and 100,000 (1,000 qubits); beside it ``symgpu_noncontextual_dev`` on the same operator,
   which computes the same table and little else: the difference is the sweep itself.
2. all T rolls in one call at T = 1,000 and 10,000, against T times the single sweep of 1.
3. the loop a user had before: ``is_noncontextual`` on the kept terms plus the candidate, once per candidate, T = 1,000 (wall clock).
4. the NumPy restatement of the reference's loop (tests/_sweep_oracle.py ``ref_sweep``: padded matrix, ``np.unique``) at T = 1,000, the
   adjacency matrix given (wall clock)."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'noncon_sweep_bench.txt')
DENSITY = 0.02


def timed(lib, check, call, warm=1, reps=3):
    ms, times, result = ctypes.c_float(0.0), [], None
    for it in range(warm + reps):
        check(lib.symgpu_timer_start())
        result = call()
        check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if it >= warm:
            times.append(ms.value * 1e-3)
    return float(np.median(times)), result


def main():
    from symmer_amd import PauliwordOp, kernels, _lib
    import _sweep_oracle as so
    _lib.init(0)
    lib, check = _lib.lib(), _lib.check
    say = lambda line: (lines.append(line), print(line, flush=True))
    lines = []
    say('noncontextual sweeps on one MI355X (tools/bench_noncon_sweep.py); device times are whole calls between HIP events, median of 3')
    say('')
    say('1. one sweep (symgpu_noncon_sweep_dev, one start), and the noncontextuality test of the whole operator (the same table)')
    single = {}
    for T, n in ((1000, 100), (10000, 100), (100000, 1000)):
        with kernels.DeviceOp.random(T, n, DENSITY, 7 + T) as op:
            t_sweep, (kept, labels, info) = timed(lib, check, lambda: kernels.noncon_sweep(op, want_labels=True, want_info=True))
            t_test, _ = timed(lib, check, lambda: kernels.noncontextual_dev(op))
        single[T] = t_sweep
        say(f'T = {T:6d} n = {n:4d}  sweep {t_sweep * 1e3:10.3f} ms  ({t_sweep / T * 1e6:6.2f} us a term)   is_noncontextual {t_test * 1e3:10.3f} ms   '
            f'table {info[0] / 2**20:8.1f} MiB  kept {int(kept.sum()):6d}  cliques {int(info[3]):4d}  SYM {int((labels == kernels.SWEEP_SYM).sum()):6d}')
    say('')
    say('2. all T rolls in one call, against T single sweeps')
    for T, n in ((1000, 100), (10000, 100)):
        with kernels.DeviceOp.random(T, n, DENSITY, 7 + T) as op:
            t_all, (kept, info) = timed(lib, check, lambda: kernels.noncon_sweep(op, starts=np.arange(T), want_info=True))
        say(f'T = {T:6d} n = {n:4d}  all rolls {t_all * 1e3:10.3f} ms  ({t_all / T * 1e6:8.2f} us a roll)   T x single {single[T] * T:9.3f} s   ratio '
            f'{single[T] * T / t_all:8.1f}   {int(info[1])} workgroups, {int(info[2])} sweeps a workgroup, kept {int(kept.sum(axis=1).min())} .. {int(kept.sum(axis=1).max())}')
    say('')
    say('3. is_noncontextual once per candidate on the device, 4. the reference loop in NumPy; T = 1,000, n = 100 (wall clock)')
    T, n = 1000, 100
    with kernels.DeviceOp.random(T, n, DENSITY, 7 + T) as op:
        symp = op.download_bool(n)
        device_kept = np.flatnonzero(kernels.noncon_sweep(op)[0])
    t0 = time.perf_counter()
    kept = [0]
    for t in range(1, T):
        if PauliwordOp(symp[kept + [t]], np.ones(len(kept) + 1)).is_noncontextual:
            kept.append(t)
    t_loop = time.perf_counter() - t0
    assert np.array_equal(kept, device_kept)
    adj = so.adjacency(symp)
    t0 = time.perf_counter()
    host_kept = so.ref_sweep(adj)
    t_host = time.perf_counter() - t0
    assert np.array_equal(host_kept, device_kept)
    say(f'per-candidate loop {t_loop:8.3f} s   NumPy reference loop {t_host:8.3f} s   one sweep call {single[T] * 1e3:8.3f} ms   '
        f'ratios {t_loop / single[T]:8.1f} and {t_host / single[T]:8.1f}')
    with open(OUT, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print(f'wrote {OUT}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
