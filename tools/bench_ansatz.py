"""The statevector ansatz kernels (csrc/ansatz.hip) timed on the GPU box: the rotations exp(i theta P) in their two forms, the adjoint-sweep
gradient against parameter shift, and the pool gradient against pairs of energies.

apply       `symgpu_ansatz_apply` of a whole sequence on a resident vector between `symgpu_timer_start` / `symgpu_timer_stop` (HIP events),
            `--warmup` calls not counted, median of `--reps` calls; the default form (tiled runs) and SYMGPU_ANSATZ_FORM=direct on the same
            plan and vector.  Per-rotation time = that / K; GB/s = K 2^n 32 bytes (every amplitude read and written once per rotation, what
            the direct form moves) over the time, for both forms, so the tiled figure is an EFFECTIVE rate.
            Sequences: synthetic UCCSD-like ones at n = 20, 24, 26 (`--groups` groups of 8 generators that share 4 X/Y positions, Z on the
            qubits between each pair of positions), and BH's own UCCSD list (12 qubits, tests/golden).
energy_grad one `symgpu_ansatz_energy_grad` of BH (energy + all K derivatives), wall clock, against 2 K energy-only calls on the same plans
            (parameter shift on the device) and against one energy of the NumPy restatement (tests/_ansatz_oracle.py) on the host times 2 K.
pool        one `symgpu_pool_gradient` of BH's UCCSD pool on a state prepared by its first 8 generators, wall clock, against what it
            replaces: per pool element a plan of the 9 generators and two energies.
Wall-clock figures: `--warmup` calls not counted, median of 3.  Progress goes to stderr.

    python tools/bench_ansatz.py [--reps 10] [--warmup 2] [--sizes 20,24,26] [--groups 8] [--out profiles/ansatz_bench.txt]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def symp_of(strings):
    n = len(strings[0])
    out = np.zeros((len(strings), 2 * n), dtype=bool)
    for r, s in enumerate(strings):
        for q, ch in enumerate(s):
            out[r, q], out[r, n + q] = ch in 'XY', ch in 'ZY'
    return out


def bh():
    with open(os.path.join(ROOT, 'tests', 'golden', 'BH_STO-3G_SINGLET_JW.json')) as f:
        d = json.load(f)
    ham = d['hamiltonian']
    hf = np.zeros(1 << d['data']['n_qubits'], dtype=np.complex128)
    hf[int(''.join(map(str, d['data']['hf_array'])), 2)] = 1.0
    return symp_of(list(ham)), np.array([v[0] for v in ham.values()]), symp_of(list(d['data']['auxiliary_operators']['UCCSD_operator'])), hf


def uccsd_like(n, groups, seed):
    """`groups` double excitations on random positions p < q < r < s: the 8 strings with an odd number of Y's, Z between p, q and r, s."""
    rng = np.random.default_rng(seed)
    strings = []
    for _ in range(groups):
        p, q, r, s = sorted(rng.choice(n, 4, replace=False))
        for letters in ('XXXY', 'XXYX', 'XYXX', 'YXXX', 'XYYY', 'YXYY', 'YYXY', 'YYYX'):
            row = ['I'] * n
            for at in list(range(p + 1, q)) + list(range(r + 1, s)):
                row[at] = 'Z'
            for at, ch in zip((p, q, r, s), letters):
                row[at] = ch
            strings.append(''.join(row))
    return symp_of(strings)


def median_wall_ms(fn, warmup, reps=3):
    times = []
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def timed_apply(plan, theta, psi, warmup, reps):
    from symmer_amd import _lib
    lib = _lib.lib()
    times, form = [], 0
    for rep in range(warmup + reps):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        form = plan.apply(theta, psi)
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= warmup:
            times.append(ms.value)
    return statistics.median(times), form


def run_apply(name, gens, a):
    from symmer_amd import kernels, packing
    n, K = gens.shape[1] // 2, gens.shape[0]
    rng = np.random.default_rng(3)
    theta = rng.uniform(-np.pi, np.pi, K)
    res = dict(apply=name, n=n, K=K, warmup=a.warmup, reps=a.reps)
    with kernels.DeviceOp.upload(packing.pack_rows(gens)) as op, kernels.AnsatzPlan(op, n) as plan, kernels.DeviceBuffer(16 << n) as psi:
        res['runs'] = plan.info()[2]
        start = np.zeros(1 << n, dtype=np.complex128)
        start[0] = 1.0                                          # the rotations are unitary: repeated calls stay normalised
        psi.write(start)
        for label, env in (('tiled', None), ('direct', 'direct')):
            if env:
                os.environ['SYMGPU_ANSATZ_FORM'] = env
            try:
                ms, form = timed_apply(plan, theta, psi, a.warmup, a.reps)
            finally:
                os.environ.pop('SYMGPU_ANSATZ_FORM', None)
            res[f'{label}_ms'], res[f'{label}_form'] = ms, form
            res[f'{label}_us_per_rotation'] = ms * 1e3 / K
            res[f'{label}_GBps'] = K * (32 << n) / (ms * 1e-3) / 1e9
            note(f'  [{name}] {label}: {ms:.3f} ms, form {form}')
    res['direct_over_tiled'] = res['direct_ms'] / res['tiled_ms']
    return res


def run_bh(a):
    import _ansatz_oracle as ao
    from symmer_amd import PauliwordOp, kernels, packing
    h_symp, h_coeff, gens, hf = bh()
    n, K = gens.shape[1] // 2, gens.shape[0]
    rng = np.random.default_rng(4)
    theta = rng.uniform(-0.1, 0.1, K)
    res = dict(bh='energy_grad', n=n, K=K, T=h_symp.shape[0], warmup=a.warmup, reps=3)
    H = PauliwordOp(h_symp, h_coeff)
    with kernels.DeviceOp.upload(packing.pack_rows(gens)) as op, kernels.AnsatzPlan(op, n) as plan, H._matvec_plan() as plan_h, \
            kernels.DeviceBuffer.upload(hf) as ref, kernels.DeviceBuffer(16 << n) as psi:
        res['energy_grad_ms'] = median_wall_ms(lambda: plan.energy_grad(plan_h, theta, ref), a.warmup)

        def shift():
            for k in range(K):
                for sign in (1, -1):
                    x = theta.copy()
                    x[k] += sign * np.pi / 4
                    plan.energy_grad(plan_h, x, ref, want_grad=False)
        res['device_parameter_shift_ms'] = median_wall_ms(shift, 0, 3)
        e, g = plan.energy_grad(plan_h, theta, ref)
        t0 = time.perf_counter()
        e_o = ao.energy_at(h_symp, h_coeff, gens, theta, hf)
        res['host_oracle_one_energy_ms'] = (time.perf_counter() - t0) * 1e3
        res['host_oracle_parameter_shift_ms'] = 2 * K * res['host_oracle_one_energy_ms']
        res['energy_abs_diff'] = abs(e - e_o)
        note(f'  [BH] energy_grad {res["energy_grad_ms"]:.2f} ms, 2K energies {res["device_parameter_shift_ms"]:.1f} ms')
        # the pool gradient on the state of the first 8 generators against plans of 9 generators and two energies each
        th8 = np.concatenate([theta[:8], np.zeros(K - 8)])
        psi.write(hf)
        plan.apply(th8, psi, 0, 8)
        pres = dict(bh='pool_gradient', n=n, M=K, warmup=a.warmup, reps=3)
        pres['pool_gradient_ms'] = median_wall_ms(lambda: kernels.pool_gradient(plan_h, op, psi), a.warmup)
        got = kernels.pool_gradient(plan_h, op, psi)
        pairs = np.zeros(K)

        def by_pairs():
            for j in range(K):
                grown = np.vstack([gens[:8], gens[j:j + 1]])
                with kernels.DeviceOp.upload(packing.pack_rows(grown)) as op9, kernels.AnsatzPlan(op9, n) as plan9:
                    up = plan9.energy_grad(plan_h, np.append(theta[:8], np.pi / 4), ref, want_grad=False)[0]
                    dn = plan9.energy_grad(plan_h, np.append(theta[:8], -np.pi / 4), ref, want_grad=False)[0]
                    pairs[j] = up - dn
        pres['pairs_of_energies_ms'] = median_wall_ms(by_pairs, 0, 3)
        pres['max_abs_diff'] = float(np.abs(got - pairs).max())
        note(f'  [BH] pool_gradient {pres["pool_gradient_ms"]:.2f} ms, pairs {pres["pairs_of_energies_ms"]:.1f} ms')
    return res, pres, gens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', default='20,24,26')
    ap.add_argument('--groups', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ansatz_bench.txt'))
    a = ap.parse_args()
    from symmer_amd import _lib
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    fill, copy = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.lib().symgpu_membw_probe(1 << 28, ctypes.addressof(fill), ctypes.addressof(copy)))
    text = [f'# tools/bench_ansatz.py --reps {a.reps} --warmup {a.warmup} --sizes {a.sizes} --groups {a.groups} on {name.value.decode()}',
            f'# symgpu_membw_probe over 256 MiB: fill {fill.value:.0f} GB/s, copy {copy.value:.0f} GB/s (read + written)',
            f'# apply: HIP events around symgpu_ansatz_apply of the whole sequence, {a.warmup} warm-up calls, median of {a.reps}; GB/s = K 2^n 32 bytes / time',
            f'# BH lines: wall clock, {a.warmup} warm-up calls (none for the long baselines), median of 3']
    bh_res, pool_res, bh_gens = run_bh(a)
    shapes = [('BH_UCCSD', bh_gens)] + [(f'n{n}_uccsd_like', uccsd_like(n, a.groups, seed=n)) for n in (int(s) for s in a.sizes.split(',') if s)]
    for shape, gens in shapes:
        res = run_apply(shape, gens, a)
        text.append(json.dumps(res))
        line = (f'## apply {shape}: n = {res["n"]}, K = {res["K"]}, {res["runs"]} tiled runs: tiled {res["tiled_ms"]:.3f} ms = '
                f'{res["tiled_us_per_rotation"]:.2f} us a rotation ({res["tiled_GBps"]:.0f} GB/s effective), direct {res["direct_ms"]:.3f} ms = '
                f'{res["direct_us_per_rotation"]:.2f} us a rotation ({res["direct_GBps"]:.0f} GB/s): direct / tiled = {res["direct_over_tiled"]:.2f}')
        text.append(line)
        print(line, flush=True)
    text.append(json.dumps(bh_res))
    line = (f'## energy_grad BH: n = {bh_res["n"]}, K = {bh_res["K"]}, T = {bh_res["T"]}: one call {bh_res["energy_grad_ms"]:.2f} ms; 2 K energies on the device '
            f'{bh_res["device_parameter_shift_ms"]:.1f} ms = {bh_res["device_parameter_shift_ms"] / bh_res["energy_grad_ms"]:.0f} x; NumPy on the host '
            f'{bh_res["host_oracle_one_energy_ms"]:.1f} ms an energy, x 2 K = {bh_res["host_oracle_parameter_shift_ms"] / 1e3:.1f} s')
    text.append(line)
    print(line, flush=True)
    text.append(json.dumps(pool_res))
    line = (f'## pool_gradient BH: M = {pool_res["M"]}: one call {pool_res["pool_gradient_ms"]:.2f} ms; M plans and pairs of energies '
            f'{pool_res["pairs_of_energies_ms"]:.1f} ms = {pool_res["pairs_of_energies_ms"] / pool_res["pool_gradient_ms"]:.0f} x (max difference {pool_res["max_abs_diff"]:.1e})')
    text.append(line)
    print(line, flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
