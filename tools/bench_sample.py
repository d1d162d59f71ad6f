"""Measuring a statevector (csrc/sample.hip, csrc/basis.hip) timed on the GPU box.  Nothing here is a pass / fail gate: the table is the
record, and the rule that chooses the counting form (sp_count_form, csrc/sample.hip) is set from its `count` lines.

plan    one `symgpu_sample_plan` + `symgpu_sample_free` over 2^n resident Gaussian amplitudes between `symgpu_timer_start` / `_stop` (HIP
        events), beside one read of the vector at the copy rate `symgpu_membw_probe` reports over 256 MiB (as tools/bench_rdm.py does).
draw    one `symgpu_sample_draw` of S shots on the plan of `--draw-n` qubits (draws + counting in the form the rule picks), beside
        `np.random.multinomial` over the same probabilities and `np.searchsorted` of S uniforms in their cumulative sum on the host (wall
        clock, once; the host lines stop at `--host-shots`).
count   the two counting forms forced (SYMGPU_SAMPLE_COUNT) on the same draws across (m, S); `rule` is what the shipped rule picks.
basis   `symgpu_basis_change` tiled against direct on `--basis-n` qubits with 8 measured qubits (the 8 lowest index bits / the 8 highest
        / 8 spread) and with all of them.
bh      `sampled_expval` of the BH Hamiltonian (tests/golden/BH_STO-3G_SINGLET_JW.json) on its ground state from `exact_gs_energy`,
        wall clock, with the exact energy beside it.

    python tools/bench_sample.py [--reps 5] [--warmup 1] [--sizes 20,24,28] [--draw-n 24] [--basis-n 26] [--out profiles/sample_bench.txt]
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
import numpy as np


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def timed(call, warmup, reps):
    """Median, min, max of `call` in ms between the library's HIP events."""
    from symmer_amd import _lib
    lib, times = _lib.lib(), []
    for rep in range(warmup + reps):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        call()
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= warmup:
            times.append(ms.value)
    return statistics.median(times), min(times), max(times)


class env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.before = os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        if self.before is not None:
            os.environ[self.name] = self.before
        return False


def gaussian(n, block):
    return np.tile(block, max(1, (1 << n) >> 20))[:1 << n]


def tiled_passes(n, qubits):
    """The passes of the tiled form: the measured index bits, ascending, join a tile that starts with the 4 lowest bits while it holds at
    most min(n, 12) bits (the rule of csrc/basis.hip, restated)."""
    bits, passes, at = sorted(n - 1 - q for q in qubits), 0, 0
    while at < len(bits):
        tile = set(range(min(n, 4)))
        while at < len(bits) and len(tile | {bits[at]}) <= min(n, 12):
            tile.add(bits[at])
            at += 1
        passes += 1
    return passes


def symp_of(strings):
    n = len(strings[0])
    out = np.zeros((len(strings), 2 * n), dtype=bool)
    for r, s in enumerate(strings):
        for q, ch in enumerate(s):
            out[r, q], out[r, n + q] = ch in 'XY', ch in 'ZY'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sizes', default='20,24,28')
    ap.add_argument('--draw-n', type=int, default=24)
    ap.add_argument('--shots', default='10000,100000,1000000,10000000,100000000')
    ap.add_argument('--host-shots', type=int, default=10_000_000)
    ap.add_argument('--count-m', default='12,16,20,24')
    ap.add_argument('--count-shots', default='10000,100000,1000000,10000000')
    ap.add_argument('--basis-n', type=int, default=26)
    ap.add_argument('--bh-shots', type=int, default=100_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_bench.txt'))
    a = ap.parse_args()
    from symmer_amd import PauliwordOp, _lib, kernels, utils
    _lib.init(0)
    lib = _lib.lib()
    name = ctypes.create_string_buffer(256)
    _lib.check(lib.symgpu_device_name(ctypes.addressof(name), 256))
    fill, copy = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(lib.symgpu_membw_probe(1 << 28, ctypes.addressof(fill), ctypes.addressof(copy)))
    text = [f'# tools/bench_sample.py --reps {a.reps} --warmup {a.warmup} --sizes {a.sizes} --draw-n {a.draw_n} --basis-n {a.basis_n} on {name.value.decode()}',
            f'# symgpu_membw_probe over 256 MiB: fill {fill.value:.0f} GB/s, copy {copy.value:.0f} GB/s (read + written); read floor = 16 2^n bytes / copy rate',
            f'# ms: HIP events around the call, {a.warmup} warm-up, median of {a.reps} (min .. max); host lines: wall clock, once']

    def add(line):
        text.append(line)
        note(line)

    rng = np.random.default_rng(1)
    block = rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20)
    ints = lambda s: [int(v) for v in s.split(',') if v]

    # ---- plan ---------------------------------------------------------------------------------------------------------------------------
    add(f'# plan  {"n":>2} {"ms":>10} {"min":>10} {"max":>10} {"GB/s":>7} {"read floor":>10} {"depth":>5} {"plan bytes":>12}')
    for n in ints(a.sizes):
        with kernels.DeviceBuffer.upload(gaussian(n, block)) as psi:
            def build():
                handle = ctypes.c_void_p()
                _lib.check(lib.symgpu_sample_plan(psi.ptr, 1 << n, ctypes.byref(handle)))
                _lib.check(lib.symgpu_sample_free(handle))
            ms, lo, hi = timed(build, a.warmup, a.reps)
            with kernels.SamplePlan(psi, 1 << n) as plan:
                info = plan.info()
            add(f'  plan  {n:>2} {ms:>10.3f} {lo:>10.3f} {hi:>10.3f} {(16 << n) / (ms * 1e-3) / 1e9:>7.0f} {(16 << n) / (copy.value * 1e9) * 1e3:>10.3f} '
                f'{info[1]:>5} {info[2]:>12}')

    # ---- draws ----------------------------------------------------------------------------------------------------------------------------
    add(f'# draw  {"n":>2} {"shots":>10} {"form":<5} {"ms":>10} {"min":>10} {"max":>10} {"Mshots/s":>9} {"distinct":>9} {"multinomial ms":>14} {"searchsorted ms":>15}')
    n = a.draw_n
    host = gaussian(n, block)
    host = host / np.linalg.norm(host)
    with kernels.SamplePlan(host) as plan:
        prob = host.real ** 2 + host.imag ** 2
        prob /= prob.sum()
        cdf = np.cumsum(prob)
        for shots in ints(a.shots):
            cap = min(1 << n, shots)
            with kernels.DeviceBuffer(8 * cap) as idx, kernels.DeviceBuffer(8 * cap) as cnt:
                nd = ctypes.c_int64(0)
                ms, lo, hi = timed(lambda: _lib.check(lib.symgpu_sample_draw(plan.handle, shots, 1, 0, None, None, idx.ptr, cnt.ptr, ctypes.addressof(nd))),
                                   a.warmup, a.reps)
            form = {kernels.SAMPLE_HIST: 'hist', kernels.SAMPLE_SORT: 'sort'}[int(plan.info()[4])]
            multi = search = None
            if shots <= a.host_shots:
                t0 = time.perf_counter()
                np.random.default_rng(0).multinomial(shots, prob)
                multi = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                np.unique(np.searchsorted(cdf, np.random.default_rng(0).random(shots), side='right'), return_counts=True)
                search = (time.perf_counter() - t0) * 1e3
            add(f'  draw  {n:>2} {shots:>10} {form:<5} {ms:>10.3f} {lo:>10.3f} {hi:>10.3f} {shots / (ms * 1e-3) / 1e6:>9.1f} {nd.value:>9} '
                f'{"-" if multi is None else f"{multi:.1f}":>14} {"-" if search is None else f"{search:.1f}":>15}')
    del host, prob, cdf

    # ---- counting forms ---------------------------------------------------------------------------------------------------------------------
    add(f'# count {"log2 m":>6} {"shots":>10} {"hist ms":>10} {"sort ms":>10} {"rule":<5} {"faster":<6}')
    for log_m in ints(a.count_m):
        with kernels.SamplePlan(gaussian(log_m, block)) as plan:
            for shots in ints(a.count_shots):
                cap, ms = min(1 << log_m, shots), {}
                with kernels.DeviceBuffer(8 * cap) as idx, kernels.DeviceBuffer(8 * cap) as cnt:
                    nd = ctypes.c_int64(0)
                    draw = lambda: _lib.check(lib.symgpu_sample_draw(plan.handle, shots, 1, 0, None, None, idx.ptr, cnt.ptr, ctypes.addressof(nd)))
                    for form in ('hist', 'sort'):
                        with env('SYMGPU_SAMPLE_COUNT', form):
                            ms[form] = timed(draw, a.warmup, a.reps)[0]
                    with env('SYMGPU_SAMPLE_COUNT', None):
                        draw()
                    rule = {kernels.SAMPLE_HIST: 'hist', kernels.SAMPLE_SORT: 'sort'}[int(plan.info()[4])]
                add(f'  count {log_m:>6} {shots:>10} {ms["hist"]:>10.3f} {ms["sort"]:>10.3f} {rule:<5} {"hist" if ms["hist"] <= ms["sort"] else "sort":<6}')

    # ---- basis change -------------------------------------------------------------------------------------------------------------------------
    add(f'# basis {"n":>2} {"measured":<14} {"tiled ms":>10} {"direct ms":>10} {"tiled GB/s":>10} {"passes":>6}')
    n = a.basis_n
    with kernels.DeviceBuffer.upload(gaussian(n, block)) as psi:
        patterns = [('8 lowest bits', list(range(n - 8, n))), ('8 highest bits', list(range(8))), ('8 spread', list(range(0, n, max(1, n // 8)))[:8]),
                    (f'all {n}', list(range(n)))]
        for label, qubits in patterns:
            xs, ys, ms = qubits[::2], qubits[1::2], {}
            for form in (None, 'direct'):
                with env('SYMGPU_BASIS_FORM', form):
                    ms[form] = timed(lambda: kernels.basis_change_dev(psi, n, xs, ys), a.warmup, a.reps)[0]
            passes = tiled_passes(n, qubits)
            add(f'  basis {n:>2} {label:<14} {ms[None]:>10.3f} {ms["direct"]:>10.3f} {2 * passes * (16 << n) / (ms[None] * 1e-3) / 1e9:>10.0f} {passes:>6}')

    # ---- BH -----------------------------------------------------------------------------------------------------------------------------------
    with open(os.path.join(ROOT, 'tests', 'golden', 'BH_STO-3G_SINGLET_JW.json')) as f:
        ham = json.load(f)['hamiltonian']
    H = PauliwordOp(symp_of(list(ham)), np.array([v[0] for v in ham.values()]))
    exact, psi = utils.exact_gs_energy(H, return_array=True)
    utils.sampled_expval(H, psi, 1000, seed=1)                        # warm-up
    t0 = time.perf_counter()
    value, _, clique = utils.sampled_expval(H, psi, a.bh_shots, seed=1, return_terms=True)
    wall = (time.perf_counter() - t0) * 1e3
    add(f'## sampled_expval BH: n = {H.n_qubits}, T = {H.n_terms}, {int(clique.max()) + 1} QWC cliques, {a.bh_shots} shots a clique: {wall:.1f} ms wall clock; '
        f'sampled {value:.6f}, exact {exact:.6f}')
    print('\n'.join(text), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
