"""The matrix-free product y = H v (csrc/matvec.hip) and exact_gs_energy (symmer_amd/utils.py) timed on the GPU box, against the route that
existed before them: `to_sparse_matrix` and SciPy on the host.

Shapes: BH (12 qubits, 631 terms, the fixture of tests/golden) and synthetic operators of n = 16, 20, 24 qubits with 10^3 and 10^4 terms
over T / 10 distinct X-parts (Gaussian real coefficients, Z-parts of density 0.3).  Per shape:
  plan      `symgpu_matvec_plan` on the resident operator, wall clock around the call (it ends in a stream synchronisation), median
  apply     `symgpu_matvec_apply` on resident vectors between `symgpu_timer_start` / `symgpu_timer_stop` (HIP events), median of `--reps`
            calls after two warm-up calls; (G + 1) 2^n 16 bytes over that time beside the copy rate of `symgpu_membw_probe` on the
            same box
  baseline  where the CSR matrix (G 2^n entries of 20 bytes) stays below `--csr-limit-gib`: `kernels.to_csr` on the resident operator (what `to_sparse_matrix` runs; median of 3
            after a warm-up build) and SciPy's `A @ v` on the host (median of 3)
End to end: `exact_gs_energy(H)` (it stops at a residual of 1e-10 sum|c|) against `eigsh(A, k=1, which='SA')` of the matrix (build listed
apart) on BH and on a 20-qubit transverse-field Ising chain (39 terms, 21 X-parts), wall clock, median of 3 each.  `eigsh` is timed twice:
with its default tol = 0 (machine precision: what the reference's exact_gs_energy calls) and with tol = 1e-10, the comparable criterion.
Progress goes to stderr, one line per phase.

    python tools/bench_matvec.py [--reps 10] [--sizes 16,20,24] [--terms 1000,10000] [--no-e2e] [--out profiles/matvec_bench.txt]
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


def bh():
    from symmer_amd import PauliwordOp
    with open(os.path.join(ROOT, 'tests', 'golden', 'BH_STO-3G_SINGLET_JW.json')) as f:
        d = json.load(f)
    return PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()})


def synthetic(n, T, seed):
    """T terms over T / 10 distinct X-parts (the first one the diagonal), real Gaussian coefficients."""
    from symmer_amd import PauliwordOp
    rng = np.random.default_rng(seed)
    G = max(1, T // 10)
    xs = np.unique(rng.integers(1, 1 << n, 2 * G))[:G - 1]
    xs = np.concatenate([[0], rng.permutation(xs)])
    x = xs[rng.integers(0, len(xs), T)]
    x[:len(xs)] = xs                                          # every X-part occurs
    symp = np.zeros((T, 2 * n), dtype=bool)
    symp[:, :n] = (x[:, None] >> np.arange(n - 1, -1, -1)) & 1
    symp[:, n:] = rng.random((T, n)) < 0.3
    return PauliwordOp(symp, rng.standard_normal(T) + 0j)


def ising(n, h=0.7):
    from symmer_amd import PauliwordOp
    zz = ['I' * q + 'ZZ' + 'I' * (n - q - 2) for q in range(n - 1)]
    xx = ['I' * q + 'X' + 'I' * (n - q - 1) for q in range(n)]
    return PauliwordOp.from_list(zz + xx, [-1.0] * (n - 1) + [-h] * n)


def timed_apply(plan, x, y, reps):
    from symmer_amd import _lib
    lib = _lib.lib()
    times = []
    for rep in range(reps + 2):
        ms = ctypes.c_float(0)
        _lib.check(lib.symgpu_timer_start())
        plan.apply(x, y)
        _lib.check(lib.symgpu_timer_stop(ctypes.addressof(ms)))
        if rep >= 2:
            times.append(ms.value)
    return statistics.median(times)


def run_shape(name, H, reps, csr_limit):
    from symmer_amd import kernels
    n, side = H.n_qubits, 1 << H.n_qubits
    rng = np.random.default_rng(1)
    v = rng.standard_normal(side) + 1j * rng.standard_normal(side)
    op = H._device()
    plan_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        plan = kernels.MatvecPlan(op, n)
        plan_ms.append((time.perf_counter() - t0) * 1e3)
        plan.free()
    res = dict(shape=name, n=n, T=H.n_terms, plan_ms=statistics.median(plan_ms))
    with kernels.MatvecPlan(op, n) as plan, kernels.DeviceBuffer.upload(v) as x, kernels.DeviceBuffer(side * 16) as y:
        G = plan.info()[2]
        res.update(G=G, plan_bytes=plan.info()[3])
        res['apply_ms'] = timed_apply(plan, x, y, reps)
        got = y.download(np.complex128, side)
    res['gather_GBps'] = (G + 1) * side * 16 / (res['apply_ms'] * 1e-3) / 1e9
    res['term_rows_per_s'] = H.n_terms * side / (res['apply_ms'] * 1e-3)
    note(f'  [{name}] G = {G}, plan {res["plan_ms"]:.3f} ms, apply {res["apply_ms"]:.3f} ms')
    csr_bytes = G * side * 20
    if csr_bytes <= csr_limit:
        from scipy.sparse import csr_matrix
        build = []
        for rep in range(4):                                  # the first build of a shape carries one-time costs: not counted
            t0 = time.perf_counter()
            A = csr_matrix(kernels.to_csr(op, n), shape=(side, side))
            build.append((time.perf_counter() - t0) * 1e3)
        res['csr_build_ms'] = statistics.median(build[1:])
        res['csr_nnz'] = int(A.nnz)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = A @ v
            times.append((time.perf_counter() - t0) * 1e3)
        res['csr_host_matvec_ms'] = statistics.median(times)
        res['max_abs_diff'] = float(np.abs(got - want).max())
        res['speedup_apply_vs_host_matvec'] = res['csr_host_matvec_ms'] / res['apply_ms']
        note(f'  [{name}] CSR build {res["csr_build_ms"]:.1f} ms, host A @ v {res["csr_host_matvec_ms"]:.3f} ms')
    else:
        res['csr_skipped_GiB'] = csr_bytes / 2 ** 30
    return res


def run_e2e(name, H):
    from scipy.sparse.linalg import eigsh
    from symmer_amd import exact_gs_energy
    exact_gs_energy(ising(4))                                 # warm-up of the step's kernels
    from scipy.sparse import csr_matrix
    from symmer_amd import kernels

    def median_ms(fn):
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            value = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), value

    n, side = H.n_qubits, 1 << H.n_qubits
    new_ms, (E, psi) = median_ms(lambda: exact_gs_energy(H, return_array=True))
    note(f'  [{name}] exact_gs_energy {new_ms:.1f} ms, E = {E!r}')
    build_ms, A = median_ms(lambda: csr_matrix(kernels.to_csr(H._device(), n), shape=(side, side)))
    eigsh_ms, (w, _) = median_ms(lambda: eigsh(A, k=1, which='SA'))
    eigsh_tol_ms, (w_tol, _) = median_ms(lambda: eigsh(A, k=1, which='SA', tol=1e-10))
    note(f'  [{name}] matrix {build_ms:.1f} ms, eigsh {eigsh_ms:.1f} ms (tol 1e-10: {eigsh_tol_ms:.1f} ms), E = {w[0]!r}')
    return dict(e2e=name, n=n, T=H.n_terms, exact_gs_energy_ms=new_ms, energy=E, csr_build_ms=build_ms, eigsh_ms=eigsh_ms,
                eigsh_energy=float(w[0]), eigsh_tol1e10_ms=eigsh_tol_ms, eigsh_tol1e10_energy=float(w_tol[0]),
                ratio_default_tol=(build_ms + eigsh_ms) / new_ms, ratio_tol1e10=(build_ms + eigsh_tol_ms) / new_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--sizes', default='16,20,24')
    ap.add_argument('--terms', default='1000,10000')
    ap.add_argument('--csr-limit-gib', type=float, default=4.0, help='the CSR baseline runs where the matrix stays below this')
    ap.add_argument('--no-e2e', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matvec_bench.txt'))
    a = ap.parse_args()
    from symmer_amd import _lib
    _lib.init(0)
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(name), 256))
    fill, copy = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.lib().symgpu_membw_probe(1 << 28, ctypes.addressof(fill), ctypes.addressof(copy)))
    text = [f'# tools/bench_matvec.py --reps {a.reps} --sizes {a.sizes} --terms {a.terms} on {name.value.decode()}',
            f'# symgpu_membw_probe over 256 MiB: fill {fill.value:.0f} GB/s, copy {copy.value:.0f} GB/s (read + written)',
            '# apply_ms: HIP events around symgpu_matvec_apply on resident vectors, median; gather_GBps = (G + 1) 2^n 16 bytes / apply_ms',
            '# csr_build_ms: kernels.to_csr + csr_matrix, median of 3 after a warm-up build; csr_host_matvec_ms: SciPy A @ v on the host, median of 3',
            '# end to end: wall clock, median of 3; exact_gs_energy stops at a residual of 1e-10 sum|c|, eigsh at its default tol = 0 and at tol = 1e-10']
    warm = ising(4)                                           # first calls load code objects: not part of any number below
    warm.to_sparse_matrix, warm.matvec(np.ones(16))
    shapes = [('BH', bh())]
    for n in (int(s) for s in a.sizes.split(',') if s):
        for T in (int(t) for t in a.terms.split(',') if t):
            shapes.append((f'n{n}_T{T}', synthetic(n, T, seed=n + T)))
    for shape, H in shapes:
        res = run_shape(shape, H, a.reps, a.csr_limit_gib * 2 ** 30)
        text.append(json.dumps(res))
        line = (f'## {shape}: n = {res["n"]}, T = {res["T"]}, G = {res["G"]}: plan {res["plan_ms"]:.3f} ms, apply {res["apply_ms"]:.3f} ms '
                f'= {res["gather_GBps"]:.0f} GB/s gathered')
        if 'csr_build_ms' in res:
            line += (f'; CSR build {res["csr_build_ms"]:.1f} ms + host A @ v {res["csr_host_matvec_ms"]:.3f} ms = '
                     f'{res["speedup_apply_vs_host_matvec"]:.0f} x the apply')
        else:
            line += f'; CSR of {res["csr_skipped_GiB"]:.1f} GiB not built'
        text.append(line)
        print(line, flush=True)
    if not a.no_e2e:
        for shape, H in (('BH', bh()), ('ising20', ising(20))):
            res = run_e2e(shape, H)
            text.append(json.dumps(res))
            line = (f'## end to end {shape}: exact_gs_energy {res["exact_gs_energy_ms"]:.1f} ms (E = {res["energy"]:.12f}); matrix '
                    f'{res["csr_build_ms"]:.1f} ms + eigsh {res["eigsh_ms"]:.1f} ms at tol = 0 (E = {res["eigsh_energy"]:.12f}) = '
                    f'{res["ratio_default_tol"]:.1f} x, + eigsh {res["eigsh_tol1e10_ms"]:.1f} ms at tol = 1e-10 = {res["ratio_tol1e10"]:.1f} x')
            text.append(line)
            print(line, flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(text) + '\n')


if __name__ == '__main__':
    main()
