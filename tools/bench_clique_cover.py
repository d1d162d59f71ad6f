"""Times ``PauliwordOp.clique_cover`` (both device strategies x the three relations) and ``adjacency_matrix_qwc`` on one MI355X and writes
profiles/clique_cover_bench.txt.  Not part of bench.py.

    python tools/bench_clique_cover.py [--quick]

Shapes (n qubits, T terms): (14, 1086), (30, 10^4), (1000, 10^4); synthetic distinct rows of about four non-identity qubits a term,
Gaussian coefficients.  Each figure: one warm-up call (it uploads the operator), then the median wall time of three calls, the device
drained before the clock stops.  Per shape and relation also the two device calls underneath on the resident handle: the degree pass and
one colouring in magnitude order, with the pair predicates per second they amount to.  Baseline: the host path (``_host=True``: the term-by-term loop of 'sorted_insertion', networkx for
'largest_first') — timed at T = 1086, and at T = 10^4 only where the T = 1086 time scaled by (10^4 / 1086)^2 stays under a minute.  The
QWC table's baseline is the NumPy expression on [N, M, n] temporaries that the device call replaced, timed where the temporaries stay
under 1 GiB.  ``--quick``: the first shape only."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'clique_cover_bench.txt')
RELATIONS = ('C', 'AC', 'QWC')
STRATEGIES = ('sorted_insertion', 'largest_first')


def synthetic(rng, n, T):
    rows = np.unique(rng.random((2 * T, 2 * n)) < min(0.3, 2.0 / n), axis=0)
    rows = rows[rng.permutation(len(rows))[:T]]
    assert len(rows) == T
    return rows, rng.standard_normal(T) + 1j * rng.standard_normal(T)


def timed(fn, repeats=3):
    from symmer_amd import kernels
    fn()
    kernels.sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        kernels.sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), out


def numpy_qwc(P):
    xa, za = P.X_block[:, None, :], P.Z_block[:, None, :]
    xb, zb = P.X_block[None, :, :], P.Z_block[None, :, :]
    both = (xa | za) & (xb | zb)
    return np.all(~both | ((xa == xb) & (za == zb)), axis=2)


def main():
    from symmer_amd import PauliwordOp, kernels, _lib
    _lib.init(0)
    shapes = [(14, 1086), (30, 10000), (1000, 10000)]
    if '--quick' in sys.argv:
        shapes = shapes[:1]
    rng = np.random.default_rng(7)
    lines = ['clique_cover / adjacency_matrix_qwc on one MI355X: wall seconds, median of 3 after a warm-up (tools/bench_clique_cover.py)',
             'host = the path before the device colouring (_host=True; its QWC tests already use the device table); "-" = not timed (over a minute)', '']
    host_at_1086 = {}
    for n, T in shapes:
        symp, coeff = synthetic(rng, n, T)
        P = PauliwordOp(symp, coeff)
        P.symp_matrix
        def qwc():
            P.__dict__.pop('adjacency_matrix_qwc', None)
            return P.adjacency_matrix_qwc
        t_dev, table = timed(qwc)
        t_np = '-'
        if T * T * n <= (1 << 30):
            t0 = time.perf_counter()
            assert np.array_equal(numpy_qwc(P), table)
            t_np = f'{time.perf_counter() - t0:.4f}'
        lines.append(f'n = {n:5d} T = {T:6d}  adjacency_matrix_qwc          device {t_dev:9.4f}   numpy {t_np:>9}')
        # the two device calls under clique_cover on the resident handle: the all-pairs degree pass and one colouring in magnitude order
        dev, by_magnitude = P._device(), np.argsort(-abs(coeff))
        for rel in RELATIONS:
            t_deg, _ = timed(lambda: kernels.relation_degrees_dev(dev, kernels.RELATIONS[rel]))
            t_col, (_, n_col, info) = timed(lambda: kernels.clique_colouring_dev(dev, kernels.RELATIONS[rel], by_magnitude, want_info=True))
            met = T * n_col if info[0] == kernels.CLIQUE_UNIONS else T * T / 2            # predicates of the wide phase, to within a block
            lines.append(f'n = {n:5d} T = {T:6d}  {rel:3s} degrees call {t_deg:9.5f} ({T * T / t_deg:8.2e} pairs/s)   colouring call {t_col:9.5f} '
                         f'({"unions" if info[0] == kernels.CLIQUE_UNIONS else "pairs"}, {info[1]} blocks, {n_col} colours, {met / t_col:8.2e} predicates/s)')
        for rel in RELATIONS:
            for strat in STRATEGIES:
                t_dev, cover = timed(lambda: P.clique_cover(rel, strat))
                t_host = '-'
                scaled = host_at_1086.get((rel, strat), 0.0) * (T / 1086.0) ** 2
                if T == 1086 or scaled < 60.0:
                    t0 = time.perf_counter()
                    ref = P.clique_cover(rel, strat, _host=True)
                    t = time.perf_counter() - t0
                    if T == 1086:
                        host_at_1086[(rel, strat)] = t
                    assert list(ref.keys()) == list(cover.keys())
                    assert all(np.array_equal(ref[k].symp_matrix, cover[k].symp_matrix) and np.array_equal(ref[k].coeff_vec, cover[k].coeff_vec) for k in ref)
                    t_host = f'{t:.4f}'
                lines.append(f'n = {n:5d} T = {T:6d}  {rel:3s} {strat:17s} {len(cover):6d} cliques   device {t_dev:9.4f}   host {t_host:>9}')
                print(lines[-1], flush=True)
        lines.append('')
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
    print(f'wrote {OUT}')


if __name__ == '__main__':
    sys.exit(main())
