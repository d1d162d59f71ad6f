"""Times the brute-force noncontextual search (``symgpu_noncon_search``, csrc/noncon.hip) and ``NoncontextualOp.solve`` on one MI355X and
writes profiles/noncon_solve_bench.txt.  Not part of bench.py; reads nothing of the reference.

    python tools/bench_noncon_solve.py                       sections 1-3 with the built library
    python tools/bench_noncon_solve.py --sweep-lib PATH      section 4 appended: PATH is a library built with `make TUNING=1`, whose search
                                                             reads SYMGPU_NONCON_L (10, 11, 12) and SYMGPU_NONCON_SWIZZLE (0, 1) per call

1. the search at f = 16, 20, 24, 28 free generators with T = 1,000 and 10,000 terms and Q = 3 cliques, random masks, plus T = Q + 1 = 4, one term
   in S0 and in each clique (the same Q + 1 transforms per block and next to no fold: what a larger call adds to it is the fold of its terms) and T = 10,000 with every mask in the high bits (the whole fold on
   slot 0 of each group).  Each figure: the whole call — host ordering of the entries, upload, two launches, 16 bytes back — between
   ``symgpu_timer_start`` / ``symgpu_timer_stop`` (HIP events), two warm-up calls, the median of five.  Rates: assignments/s, and butterflies
   (one add and one subtract) per second against the FP64 vector peak of 78.6 TFLOP/s counted as FMAs, i.e. 39.3e12 adds/s.
2. the same objective through a vectorised NumPy restatement of the reference's evaluation (all terms x a block of assignments), f = 16 and
   20; at T = 10,000 and f = 20 a sixteenth of the assignments is timed and the time scaled.  The reference's own process-pool loop over
   assignments is slower still.
3. ``NoncontextualOp(...)`` and ``.solve()`` on the largest recorded operator of tests/golden/noncon_solve.npz, wall clock.
4. L and the bank swizzle of the work vector, at f = 24, T = 1,000 and 10,000."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'noncon_solve_bench.txt')
ADDS_PEAK = 39.3e12


def synthetic(rng, T, f, Q, high_only_from=None):
    """T terms with random masks; every group (S0 and each of the Q cliques) holds a term, so every call runs Q + 1 transforms per block"""
    assert T >= Q + 1
    coeff = rng.standard_normal(T)
    mask = rng.integers(0, 1 << f, T, dtype=np.uint64)
    if high_only_from is not None:
        mask &= np.uint64(((1 << f) - 1) & ~((1 << high_only_from) - 1))
    clique = rng.integers(-1, Q, T).astype(np.int32)
    clique[:Q + 1] = np.arange(-1, Q)
    return coeff, mask, clique


def timed_search(kernels, lib, check, coeff, mask, clique, f, Q, warm=2, reps=5):
    ms, times = ctypes.c_float(0.0), []
    for it in range(warm + reps):
        check(lib.symgpu_timer_start())
        energy, best, info = kernels.noncon_search(coeff, mask, clique, f, Q, want_info=True)
        check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if it >= warm:
            times.append(ms.value * 1e-3)
    return float(np.median(times)), energy, best, info


def numpy_landscape_min(coeff, mask, clique, f, Q, first=None, block=1 << 12):
    """the reference's arithmetic, vectorised over a block of assignments: (minimum, seconds)"""
    import _noncon_oracle as no
    size = (1 << f) if first is None else first
    groups = [np.flatnonzero(clique == q) for q in range(-1, Q)]
    t0, best = time.perf_counter(), np.inf
    for m0 in range(0, size, block):
        m = np.arange(m0, m0 + block, dtype=np.uint64)
        signed = coeff[None, :] * (1 - 2 * no._parity(mask[None, :] & m[:, None]))
        acc = np.zeros(block)
        for idx in groups[1:]:
            si = signed[:, idx].sum(axis=1)
            acc += si * si
        best = min(best, float((signed[:, groups[0]].sum(axis=1) - np.sqrt(acc)).min()))
    return best, time.perf_counter() - t0


def line_of(label, f, T, Q, t, info):
    L = int(info[0])
    l = min(f, L)
    butterflies = (1 << f) * (Q + 1) * l / 2
    return (f'{label:22s} f = {f:2d} T = {T:6d} Q = {Q}  {t * 1e3:10.3f} ms  {(1 << f) / t:9.3e} assignments/s  {butterflies / t:9.3e} butterflies/s '
            f'({100 * butterflies / t / ADDS_PEAK:5.2f} % of the FP64 add peak)  L = {L}, {int(info[1])} blocks, {int(info[3])} workgroups')


def main():
    sweep_lib = sys.argv[sys.argv.index('--sweep-lib') + 1] if '--sweep-lib' in sys.argv else None
    from symmer_amd import _lib
    if sweep_lib:
        _lib.LIB_PATH = os.path.abspath(sweep_lib)
    from symmer_amd import NoncontextualOp, kernels
    _lib.init(0)
    lib, check = _lib.lib(), _lib.check
    rng = np.random.default_rng(11)
    Q = 3
    lines = []
    if sweep_lib:
        lines += ['', '4. L and the bank swizzle of the work vector (library built with TUNING=1), f = 24, Q = 3: the six variants take turns, one call each,',
                  '   for 2 warm-up and 15 timed rounds; median [min .. max] of a variant\'s 15 calls']
        variants = [(L, swizzle) for L in (10, 11, 12) for swizzle in (0, 1)]
        ms = ctypes.c_float(0.0)
        for T in (1000, 10000):
            coeff, mask, clique = synthetic(rng, T, 24, Q)
            times, answers = {v: [] for v in variants}, set()
            for it in range(17):
                for L, swizzle in variants:
                    os.environ['SYMGPU_NONCON_L'], os.environ['SYMGPU_NONCON_SWIZZLE'] = str(L), str(swizzle)
                    check(lib.symgpu_timer_start())
                    energy, best, info = kernels.noncon_search(coeff, mask, clique, 24, Q, want_info=True)
                    check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
                    assert info[0] == L
                    answers.add((energy, best))
                    if it >= 2:
                        times[(L, swizzle)].append(ms.value)
            # another L adds in another order: the same assignment, the energy to rounding
            assert len({m for _, m in answers}) == 1 and np.ptp([e for e, _ in answers]) <= 1e-9 * np.abs(coeff).sum(), 'the variants disagree'
            for L, swizzle in variants:
                t = np.array(times[(L, swizzle)])
                lines.append(f'T = {T:6d}  L = {L} swizzle = {swizzle}   {np.median(t):7.3f} ms [{t.min():7.3f} .. {t.max():7.3f}]')
                print(lines[-1], flush=True)
        with open(OUT, 'a') as out:
            out.write('\n'.join(lines) + '\n')
        return 0

    lines += ['brute-force noncontextual search on one MI355X (tools/bench_noncon_solve.py); times are whole calls between HIP events, median of 5',
              '', '1. symgpu_noncon_search, Q = 3']
    device = {}
    for f in (16, 20, 24, 28):
        for label, T, high in (('transforms alone', Q + 1, None), ('random masks', 1000, None), ('random masks', 10000, None),
                               ('masks in the high bits', 10000, 11)):
            if high is not None and f <= high:
                continue
            coeff, mask, clique = synthetic(rng, T, f, Q, high)
            t, energy, best, info = timed_search(kernels, lib, check, coeff, mask, clique, f, Q)
            device[(f, T, label)] = (coeff, mask, clique, t, energy)
            lines.append(line_of(label, f, T, Q, t, info))
            print(lines[-1], flush=True)
    lines += ['', 'share of a call that is the fold of the terms, the host ordering and upload of the entries included (1 - the time of the transforms alone / the time of the call):']
    for f in (16, 20, 24, 28):
        alone = device[(f, Q + 1, 'transforms alone')][3]
        shares = [f'T = {T} {label}: {100 * (1 - alone / device[(f, T, label)][3]):4.0f} %' for (ff, T, label) in device if ff == f and T > Q + 1]
        lines.append(f'f = {f:2d}  ' + '   '.join(shares))
    lines += ['', '2. the same objective, vectorised NumPy on the host (blocks of 4096 assignments x all terms)']
    for f, T, part in ((16, 1000, None), (20, 1000, None), (16, 10000, None), (20, 10000, 1 << 16)):
        coeff, mask, clique, t_dev, e_dev = device[(f, T, 'random masks')]
        e_host, t_host = numpy_landscape_min(coeff, mask, clique, f, Q, first=part)
        scale = 1 if part is None else (1 << f) // part
        note = '' if part is None else f' ({part} assignments timed, x {scale})'
        if part is None:
            assert abs(e_host - e_dev) <= 1e-9 * np.abs(coeff).sum(), (e_host, e_dev)
        lines.append(f'f = {f:2d} T = {T:6d}  host {t_host * scale:9.3f} s{note}   device {t_dev * 1e3:9.3f} ms   ratio {t_host * scale / t_dev:9.1f}')
        print(lines[-1], flush=True)
    lines += ['', '3. NoncontextualOp end to end, the largest recorded operator (wall clock, second of two runs)']
    import _noncon_oracle as no
    tag, case = max(no.golden_cases(), key=lambda tc: tc[1]['symp'].shape[0] * tc[1]['generators'].shape[0])
    for _ in range(2):
        t0 = time.perf_counter()
        H = NoncontextualOp(case['symp'], case['coeff'])
        t1 = time.perf_counter()
        H.solve()
        t2 = time.perf_counter()
    assert abs(H.energy - float(case['energy'])) <= no.tolerance(case['coeff'].real)
    lines.append(f'case {tag}: n = {int(case["n"])} T = {H.n_terms} generators = {H.symmetry_generators.n_terms} cliques = {H.n_cliques}   '
                 f'construction {t1 - t0:.4f} s   solve {(t2 - t1) * 1e3:.3f} ms   energy {H.energy:.12f}')
    print(lines[-1], flush=True)
    with open(OUT, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    print(f'wrote {OUT}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
