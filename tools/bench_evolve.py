"""The Chebyshev propagator (csrc/evolve.hip, symmer_amd/evolution/time_evolution.py) timed on the GPU box.

1. One Chebyshev ORDER against one `symgpu_matvec_apply` on the same plan and vectors.  The matvec is the floor: an order forms the same
   row sum and then reads T_{k-1}[b], T_{k-2}[b] and out[b] and writes T_k[b] and out[b].  A call of `symgpu_cheb_apply` also allocates two
   vectors and synchronises once, so the time of an order is the SLOPE between two calls, (t(K = 20) - t(K = 4)) / 16, each the median of
   `--reps` calls between `symgpu_timer_start` / `symgpu_timer_stop` (HIP events) after two warm-up calls; the matvec is timed the same
   way.  Shapes: a transverse-field Ising chain (2 n - 1 terms, n + 1 X-parts) and a 1,000-term operator over 100 X-parts (the synthetic
   shape of tools/bench_matvec.py) at n = 20, 24, 28, and BH (12 qubits: the launch chain); 'norm1' interval, so the vectors stay bounded.
2. `evolve_state` end to end (wall clock, median of 3 after a warm-up run): plan, interval, upload, the steps, download — on BH (the fixture
   of tests/golden, t = 1) with both interval methods, on a 16-qubit Ising chain and a 16-qubit 1,000-term operator (t with
   sum|c| t = 20), beside SciPy's `expm_multiply` on the host CSR matrix of the same operator (its build listed apart).
Progress goes to stderr, one line per phase.

    python tools/bench_evolve.py [--reps 5] [--sizes 20,24,28] [--no-e2e] [--out profiles/evolve_bench.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np

from bench_matvec import bh, ising, note, synthetic, timed_apply

K_LOW, K_HIGH = 4, 20


def timed_cheb(plan, interval, K, x, y, reps):
    from symmer_amd import _lib
    lib = _lib.lib()
    coeffs = np.full(K + 1, 0.5 / (K + 1), dtype=np.complex128)
    times = []
    for rep in range(reps + 2):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        plan.chebyshev(interval[0], interval[1], coeffs, x, y)
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= 2:
            times.append(ms.value)
    return statistics.median(times)


def run_order(name, H, reps):
    from symmer_amd import kernels
    from symmer_amd.evolution import spectral_interval
    n, side = H.n_qubits, 1 << H.n_qubits
    rng = np.random.default_rng(1)
    v = np.empty(side, dtype=np.complex128)
    v.real, v.imag = rng.random(side), 0.5
    v /= np.sqrt(side)
    interval = spectral_interval(H, None, 'norm1')
    with kernels.MatvecPlan(H._device(), n) as plan, kernels.DeviceBuffer.upload(v) as x, kernels.DeviceBuffer(side * 16) as y:
        del v
        G = plan.info()[2]
        matvec_ms = timed_apply(plan, x, y, reps)
        low_ms, high_ms = timed_cheb(plan, interval, K_LOW, x, y, reps), timed_cheb(plan, interval, K_HIGH, x, y, reps)
    order_ms = (high_ms - low_ms) / (K_HIGH - K_LOW)
    res = dict(shape=name, n=n, T=H.n_terms, G=G, matvec_ms=matvec_ms, cheb_K4_ms=low_ms, cheb_K20_ms=high_ms, order_ms=order_ms,
               ratio_order_over_matvec=order_ms / matvec_ms, call_overhead_ms=low_ms - K_LOW * order_ms,
               order_GBps=(G + 4) * side * 16 / (order_ms * 1e-3) / 1e9, matvec_GBps=(G + 1) * side * 16 / (matvec_ms * 1e-3) / 1e9)
    note(f'  [{name}] G = {G}: matvec {matvec_ms:.3f} ms, order {order_ms:.3f} ms')
    return res


def median_ms(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        value = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), value


def run_e2e(name, H, t, methods):
    from scipy.sparse import csr_matrix
    from scipy.sparse.linalg import expm_multiply
    from symmer_amd import kernels
    from symmer_amd.evolution import evolve_state
    n, side = H.n_qubits, 1 << H.n_qubits
    rng = np.random.default_rng(2)
    psi = rng.standard_normal(side) + 1j * rng.standard_normal(side)
    psi /= np.linalg.norm(psi)
    res = dict(e2e=name, n=n, T=H.n_terms, t=t)
    states = {}
    for method in methods:
        ms, out = median_ms(lambda: evolve_state(H, psi, [t], tol=1e-10, spectral_bounds=method))
        states[method] = np.asarray(out.states[0].to_dense_matrix).reshape(-1)
        res[f'{method}_ms'], res[f'{method}_K'], res[f'{method}_half_width'] = ms, out.orders[0], out.interval[1]
        note(f'  [{name}] evolve_state {method}: K = {out.orders[0]}, {ms:.1f} ms')
    build_ms, A = median_ms(lambda: csr_matrix(kernels.to_csr(H._device(), n), shape=(side, side)))
    host_ms, want = median_ms(lambda: expm_multiply(-1j * t * A, psi), reps=1)
    res.update(csr_build_ms=build_ms, expm_multiply_ms=host_ms)
    for method in methods:
        res[f'{method}_diff_vs_expm_multiply'] = float(np.linalg.norm(states[method] - want))
    note(f'  [{name}] matrix {build_ms:.1f} ms, expm_multiply {host_ms:.1f} ms')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='20,24,28')
    ap.add_argument('--no-e2e', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evolve_bench.txt'))
    a = ap.parse_args()
    from symmer_amd import _lib
    from symmer_amd.evolution import evolve_state
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    fill, copy = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.lib().symgpu_membw_probe(1 << 28, ctypes.addressof(fill), ctypes.addressof(copy)))
    text = [f'# tools/bench_evolve.py --reps {a.reps} --sizes {a.sizes} on {name.value.decode()}',
            f'# symgpu_membw_probe over 256 MiB: fill {fill.value:.0f} GB/s, copy {copy.value:.0f} GB/s (read + written)',
            f'# order_ms: (symgpu_cheb_apply at K = {K_HIGH} - at K = {K_LOW}) / {K_HIGH - K_LOW}, each the median of HIP-event timings; matvec_ms: symgpu_matvec_apply on the',
            '#   same plan and vectors, the same way; order_GBps = (G + 4) 2^n 16 bytes / order_ms, matvec_GBps = (G + 1) 2^n 16 bytes / matvec_ms',
            '# end to end: wall clock, median of 3 after a warm-up run, tol = 1e-10; expm_multiply: SciPy on the host CSR matrix, one run after a warm-up']
    warm = ising(4)                                           # first calls load code objects: not part of any number below
    evolve_state(warm, np.ones(16) / 4, [0.5], spectral_bounds='lanczos')
    shapes = [('BH', bh())]                                   # molecular size: the launch chain, not the memory system
    for n in (int(s) for s in a.sizes.split(',') if s):
        shapes += [(f'ising{n}', ising(n)), (f'n{n}_T1000', synthetic(n, 1000, seed=n + 1000))]
    for shape, H in shapes:
        res = run_order(shape, H, a.reps)
        text.append(json.dumps(res))
        line = (f'## {shape}: n = {res["n"]}, T = {res["T"]}, G = {res["G"]}: matvec {res["matvec_ms"]:.3f} ms ({res["matvec_GBps"]:.0f} GB/s), one order '
                f'{res["order_ms"]:.3f} ms ({res["order_GBps"]:.0f} GB/s) = {res["ratio_order_over_matvec"]:.2f} x the matvec; a call costs '
                f'{res["call_overhead_ms"]:.3f} ms beyond its orders')
        text.append(line)
        print(line, flush=True)
    if not a.no_e2e:
        H16 = synthetic(16, 1000, seed=1016)
        cases = [('BH', bh(), 1.0, ('norm1', 'lanczos')), ('ising16', ising(16), 20.0 / (15 + 0.7 * 16), ('norm1', 'lanczos')),
                 ('n16_T1000', H16, 20.0 / float(np.abs(H16.coeff_vec).sum()), ('norm1', 'lanczos'))]
        for shape, H, t, methods in cases:
            res = run_e2e(shape, H, t, methods)
            text.append(json.dumps(res))
            line = f'## end to end {shape} (n = {res["n"]}, T = {res["T"]}, t = {t:.4g}): ' + '; '.join(
                f"evolve_state '{m}' K = {res[m + '_K']}, {res[m + '_ms']:.1f} ms (|diff| to expm_multiply {res[m + '_diff_vs_expm_multiply']:.1e})" for m in methods)
            line += f'; matrix {res["csr_build_ms"]:.1f} ms + expm_multiply {res["expm_multiply_ms"]:.1f} ms'
            text.append(line)
            print(line, flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
