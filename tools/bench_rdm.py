"""The reduced density matrix (csrc/rdm.hip) timed on the GPU box, with the two floors it can be held against measured on the same box.

rdm         one `symgpu_rdm` on a resident vector between `symgpu_timer_start` / `symgpu_timer_stop` (HIP events), `--warmup` calls not
            counted, median of `--reps` calls.  Shapes: n in `--sizes` x k in `--kept` x the three kept patterns — the kept qubits on the
            LOWEST index bits, on the HIGHEST, and interleaved from the lowest bit up.  The amplitudes are Gaussian (a block of 2^20
            repeated: the time does not depend on the values).
read floor  16 2^n bytes at the copy rate `symgpu_membw_probe` reports over 256 MiB (bytes read + written per second): one read of psi.
fma floor   4 4^k 2^(n-k) FP64 flops — the Hermitian half of the 8 4^k 2^(n-k) of M M^+ — at the rate `tools/ubench_fp64` reaches
            (independent v_fma_f64 chains, nothing else; built beside this script by
            `hipcc --offload-arch=gfx950 -O3 tools/ubench_fp64.hip -o tools/ubench_fp64` when the binary is missing or stale; no record
            is written without it).
host        NumPy's `tensordot` of the reference's formula (tests/_rdm_oracle.py rdm_tensordot) on the host, wall clock, once, for the
            interleaved pattern where 8 4^k 2^(n-k) <= `--host-flops`.
No threshold is set here: the table is the record.  Progress goes to stderr.

    python tools/bench_rdm.py [--reps 5] [--warmup 1] [--sizes 20,24,28] [--kept 1,2,3,4,6,8,10,12] [--out profiles/rdm_bench.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def fp64_rate():
    """TFLOP/s of tools/ubench_fp64, built here first when the binary is missing or older than its source.  The fma floor is a column
    the record must have: a failed build or run raises instead of leaving it out."""
    binary, source = os.path.join(ROOT, 'tools', 'ubench_fp64'), os.path.join(ROOT, 'tools', 'ubench_fp64.hip')
    if not os.path.exists(binary) or os.path.getmtime(binary) < os.path.getmtime(source):
        hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
        note(f'building {binary}')
        subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', source, '-o', binary], check=True, timeout=600)
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    if out.returncode != 0:
        raise RuntimeError(f'tools/ubench_fp64 failed ({out.returncode}): {out.stderr.strip()}')
    return float(out.stdout.split()[1])


def timed_rdm(psi, n, kept, rho, warmup, reps):
    from symmer_amd import _lib
    lib = _lib.lib()
    kept_arr = np.ascontiguousarray(kept, dtype=np.int32)
    info = np.zeros(6, dtype=np.int64)
    times = []
    for rep in range(warmup + reps):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        _lib.check(lib.symgpu_rdm(psi.ptr, n, kept_arr.ctypes.data, len(kept), rho.ptr, info.ctypes.data))
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= warmup:
            times.append(ms.value)
    return statistics.median(times), min(times), max(times), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sizes', default='20,24,28')
    ap.add_argument('--kept', default='1,2,3,4,6,8,10,12')
    ap.add_argument('--host-flops', type=float, default=5e10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rdm_bench.txt'))
    a = ap.parse_args()
    import _rdm_oracle as ro
    from symmer_amd import _lib, kernels
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    fill, copy = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.lib().symgpu_membw_probe(1 << 28, ctypes.addressof(fill), ctypes.addressof(copy)))
    tflops = fp64_rate()
    text = [f'# tools/bench_rdm.py --reps {a.reps} --warmup {a.warmup} --sizes {a.sizes} --kept {a.kept} on {name.value.decode()}',
            f'# symgpu_membw_probe over 256 MiB: fill {fill.value:.0f} GB/s, copy {copy.value:.0f} GB/s (read + written); read floor = 16 2^n bytes / copy rate',
            f'# tools/ubench_fp64: {tflops:.1f} TFLOP/s of v_fma_f64; fma floor = 4 4^k 2^(n-k) flops / that rate',
            f'# ms: HIP events around symgpu_rdm, {a.warmup} warm-up, median of {a.reps} (min .. max); GB/s = 16 2^n / ms; TF = 4 4^k 2^(n-k) / ms',
            '# host: numpy tensordot (the reference\'s formula), wall clock, once, interleaved pattern only; MFMA was not tried: VALU only',
            f'# {"n":>2} {"k":>2} {"pattern":<11} {"form":<6} {"chunks":>6} {"ms":>10} {"min":>10} {"max":>10} {"GB/s":>7} {"TF":>6} {"read floor":>10} {"fma floor":>10} {"host ms":>10}']
    rng = np.random.default_rng(1)
    block = rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)
    with kernels.DeviceBuffer(16 << 24) as rho:
        for n in (int(s) for s in a.sizes.split(',') if s):
            host_psi = np.tile(block, max(1, (1 << n) >> 20))[:1 << n]
            with kernels.DeviceBuffer.upload(host_psi) as psi:
                for k in (int(s) for s in a.kept.split(',') if s):
                    if k > n:
                        continue
                    for pattern, kept in ro.kept_patterns(n, k).items():
                        ms, lo, hi, info = timed_rdm(psi, n, kept, rho, a.warmup, a.reps)
                        flops = 4.0 * 4.0 ** k * 2.0 ** (n - k)
                        read_ms = (16 << n) / (copy.value * 1e9) * 1e3
                        fma_ms = flops / (tflops * 1e12) * 1e3
                        host_ms = None
                        if pattern == 'interleaved' and 2 * flops <= a.host_flops:
                            t0 = time.perf_counter()
                            ro.rdm_tensordot(host_psi, n, kept)
                            host_ms = (time.perf_counter() - t0) * 1e3
                        line = (f'  {n:>2} {k:>2} {pattern:<11} {"stream" if info[0] == kernels.RDM_STREAM else "tiled":<6} {info[2]:>6} {ms:>10.3f} {lo:>10.3f} {hi:>10.3f} '
                                f'{(16 << n) / (ms * 1e-3) / 1e9:>7.0f} {flops / (ms * 1e-3) / 1e12:>6.2f} {read_ms:>10.3f} '
                                f'{fma_ms:>10.3f} {"-" if host_ms is None else f"{host_ms:.1f}":>10}')
                        text.append(line)
                        note(line)
            del host_psi
    print('\n'.join(text), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
