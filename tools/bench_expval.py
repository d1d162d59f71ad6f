"""Batched expectation values (csrc/expval.hip) timed on the GPU box, against the per-term loop they replace.

Shapes (n qubits, T terms, S basis states): the molecular regime (8, 185, 70), (14, 1086, 1000), (20, 2000, 4000), (30, 10^4, 10^5) and the
large one (1000, 10^4, 10^5).  Per shape:
  call      `symgpu_expval_terms_dev` on resident handles (operator, cleaned state) between `symgpu_timer_start` / `symgpu_timer_stop` (HIP
            events), median of `--reps` calls after two warm-up calls, in the form the library picks and with SYMGPU_EXPVAL_FORM=global where
            the pick is the staged form; probes per second = T * S / that time
  new       the Python path behind `PauliwordOp.expval`'s term branch (device cleanup of psi + the call + the frees), wall clock, median
  expval    `P.expval(psi)` itself, wall clock, median, and the branch it took (n_terms > psi.n_terms > 10 is the reference's bra x op x ket
            product, which this library leaves as it was)
  loop      the baseline: sum(single_term_expval(P_k, psi) * c_k), the code `expval` ran before, timed ONCE; at T > 2000 over the first
            `--loop-terms` (200) terms only and scaled by T / that (said in the line).  At n = 1000 and S = 10^5 one term of the loop takes
            seconds of host time (each of its two products builds a QuantumState from a 2 * 10^5 x 1000 integer matrix): give it a few terms.
Progress goes to stderr, one line per phase.

    python tools/bench_expval.py [--reps 10] [--shapes 8:185:70,...] [--no-loop] [--loop-terms 200] [--out profiles/expval_bench.txt]
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

DEFAULT_SHAPES = '8:185:70,14:1086:1000,20:2000:4000,30:10000:100000,1000:10000:100000'
FORM_NAME = {0: 'none', 1: 'lds', 2: 'global'}


def make_input(n, T, S, seed):
    """A normalised Gaussian state of S different basis strings and T terms; half of the terms have x = the XOR of two strings of the state
    (at least two look-ups hit), the others a sparse random x."""
    rng = np.random.default_rng(seed)
    bits = np.zeros((0, n), dtype=np.uint8)
    while bits.shape[0] < S:
        more = (rng.random((2 * (S - bits.shape[0]) + 8, n)) < 0.5).astype(np.uint8)
        bits = np.unique(np.vstack([bits, more]), axis=0) if n <= 30 else np.vstack([bits, more])     # 1000 random bits do not repeat
    bits = bits[rng.permutation(bits.shape[0])[:S]]
    amp = rng.standard_normal(S) + 1j * rng.standard_normal(S)
    amp /= np.linalg.norm(amp)
    symp = np.zeros((T, 2 * n), dtype=bool)
    pairs = rng.integers(0, S, (T, 2))
    symp[:, :n] = rng.random((T, n)) < min(0.3, 4.0 / n)
    symp[::2, :n] = (bits[pairs[::2, 0]] ^ bits[pairs[::2, 1]]).astype(bool)
    symp[:, n:] = rng.random((T, n)) < min(0.5, 8.0 / n)
    coeff = rng.standard_normal(T) + 0j
    return symp, coeff, bits, amp


def timed_calls(op, state, reps):
    from symmer_amd import _lib, kernels
    lib = _lib.lib()
    times, form = [], 0
    for rep in range(reps + 2):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        _, total, form = kernels.expval_terms_dev(op, state, state)
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= 2:
            times.append(ms.value)
    return statistics.median(times), form, total


def wall_median(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        value = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), value


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def run_shape(n, T, S, reps, with_loop, loop_terms=200):
    from symmer_amd import PauliwordOp, QuantumState, kernels
    from symmer_amd.operators.quantum_state import single_term_expval, _expval_call
    symp, coeff, bits, amp = make_input(n, T, S, seed=n + T)
    note(f'[{n}:{T}:{S}] input made')
    P, psi = PauliwordOp(symp, coeff), QuantumState(bits, amp)
    note('  operator and state built')
    op = P._device()
    state = kernels.cleanup_dev(psi.state_op._device())
    res = dict(n=n, T=T, S=S, S_clean=state.n_terms, probes=T * S)
    os.environ.pop('SYMGPU_EXPVAL_FORM', None)
    ms, form, total = timed_calls(op, state, reps)
    res.update(form=FORM_NAME[form], call_ms=ms, probes_per_s=T * S / (ms * 1e-3))
    note(f'  call {ms:.3f} ms')
    if form == 1:
        os.environ['SYMGPU_EXPVAL_FORM'] = 'global'
        ms_g, form_g, total_g = timed_calls(op, state, reps)
        os.environ.pop('SYMGPU_EXPVAL_FORM', None)
        assert form_g == 2 and total_g == total, 'the forms disagree'
        res.update(call_ms_global_forced=ms_g, probes_per_s_global_forced=T * S / (ms_g * 1e-3))
    state.free()
    res['new_path_ms'], value_new = wall_median(lambda: _expval_call(P, psi, False)[1].real, max(3, reps // 2))
    note(f'  new path {res["new_path_ms"]:.3f} ms')
    res['expval_ms'], value = wall_median(lambda: P.expval(psi), max(3, reps // 2))
    res['expval_branch'] = 'product' if T > psi.n_terms > 10 else 'terms'
    res['expval'] = float(value)
    assert abs(value - value_new) < 1e-9 and abs(total.real - value_new) < 1e-9
    if with_loop:
        K = T if T <= 2000 else min(T, loop_terms)
        note(f'  P.expval {res["expval_ms"]:.3f} ms; the loop over {K} terms ...')
        t0 = time.perf_counter()
        loop = 0
        for k in range(K):
            loop += single_term_expval(P[k], psi) * coeff[k]
            if k % 50 == 49 or n >= 1000:
                note(f'    {k + 1} terms, {time.perf_counter() - t0:.1f} s')
        dt = (time.perf_counter() - t0) * 1e3
        res.update(loop_terms_timed=K, loop_ms=dt * T / K, loop_scaled=K != T)
        if K == T:
            assert abs(loop.real - value_new) < 1e-9, (loop, value_new)
        res['speedup_call'] = res['loop_ms'] / res['call_ms']
        res['speedup_new_path'] = res['loop_ms'] / res['new_path_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--shapes', default=DEFAULT_SHAPES)
    ap.add_argument('--no-loop', action='store_true', help='do not time the per-term baseline')
    ap.add_argument('--loop-terms', type=int, default=200, help='terms of the baseline loop timed where T > 2000')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'expval_bench.txt'))
    a = ap.parse_args()
    from symmer_amd import _lib
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    text = [f'# tools/bench_expval.py --reps {a.reps} --shapes {a.shapes} on {name.value.decode()}',
            '# call_ms: HIP events around symgpu_expval_terms_dev on resident handles, median; new_path_ms / expval_ms: wall clock, median',
            '# loop_ms: sum(single_term_expval(P_k, psi) * c_k), once; loop_scaled: timed on the first loop_terms_timed terms and multiplied by T / that']
    for shape in a.shapes.split(','):
        n, T, S = (int(v) for v in shape.split(':'))
        res = run_shape(n, T, S, a.reps, not a.no_loop, a.loop_terms)
        text.append(json.dumps(res))
        print(text[-1], flush=True)
        line = (f'## n = {n}, T = {T}, S = {S}: {res["form"]} form, call {res["call_ms"]:.3f} ms = {res["probes_per_s"]:.3e} probes/s'
                + (f' (global forced: {res["call_ms_global_forced"]:.3f} ms)' if 'call_ms_global_forced' in res else '')
                + f'; new path {res["new_path_ms"]:.3f} ms; P.expval {res["expval_ms"]:.3f} ms ({res["expval_branch"]} branch)')
        if 'loop_ms' in res:
            line += (f'; loop {res["loop_ms"]:.1f} ms' + (f' (scaled from {res["loop_terms_timed"]} terms)' if res['loop_scaled'] else '')
                     + f' = {res["speedup_new_path"]:.1f} x the new path')
        text.append(line)
        print(line, flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
