"""Writes tests/golden/noncon_sweep.npz: answers of the REFERENCE's noncontextual sweep (symmer/operators/utils.py:592-616
``perform_noncontextual_sweep``) and of the three constructors on it (symmer/operators/noncontextual_op.py:126-226).  Build container
only: the reference is imported through ``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has
neither.  The file holds data only, per case ``NN``:

    NN/kind, NN/symp, NN/coeff          'sweep' or 'dfs'; the operator
    NN/kept                             indices kept by perform_noncontextual_sweep on the operator as it stands
    NN/single_magnitude/{symp,coeff}    _single_sweep_noncontextual_operator(H, 'magnitude')
    NN/single_random/{symp,coeff}       ... (H, 'random') after np.random.seed(NN/random_seed)
    NN/diag_first/{symp,coeff}          _diag_first_noncontextual_op(H)
    NN/dfs_magnitude, NN/dfs_largest    _dfs_noncontextual_op(H, runtime=1e9, strategy=...): every roll ran ('dfs' cases only)

    python tools/gen_golden_noncon_sweep.py

Cases: the B+ and BH Hamiltonians of tests/golden (their rows; B+ with the DFS forms, BH — 631 terms, 631 reference sweeps of 631
steps each — without), random operators of 3 .. 8 qubits with 10 .. 60 terms ('dfs') and with up to 300 terms ('sweep'), half of them
with half of their terms diagonal, the others with three (rows that came out equal or as the identity are dropped, so a case may
hold a few terms fewer than it asked for).  Every operator has distinct rows and coefficients of distinct magnitudes (asserted: the magnitude
order has no ties, so no sorting algorithm's tie order enters the answers); the Hamiltonians' coefficients are scaled by 1 + 1e-3 u_k,
u_k uniform in [-1, 1), to that end.

Checked here: tests/_sweep_oracle.py's ``ref_sweep`` and ``rule_sweep`` both reproduce every ``kept``.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
OUT = os.path.join(GOLDEN, 'noncon_sweep.npz')


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def distinct_magnitudes(coeff):
    mags = np.sort(np.abs(coeff))
    return len(mags) < 2 or float(np.min(np.diff(mags))) > 1e-12 * float(mags[-1])


def main():
    _load('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    oracle = _load('_sweep_oracle', os.path.join(ROOT, 'tests', '_sweep_oracle.py'))
    from symmer.operators import PauliwordOp as RefOp, NoncontextualOp as RefNC
    from symmer.operators.utils import perform_noncontextual_sweep
    rng = np.random.default_rng(20261021)

    specs = []                                                       # (kind, symp, coeff)
    for name, kind in (('B+_STO-3G_SINGLET_JW.json', 'dfs'), ('BH_STO-3G_SINGLET_JW.json', 'sweep')):
        with open(os.path.join(GOLDEN, name)) as f:
            H = RefOp.from_dictionary({k: complex(*v) for k, v in json.load(f)['hamiltonian'].items()})
        coeff = H.coeff_vec.real * (1 + 1e-3 * rng.uniform(-1, 1, H.n_terms))
        specs.append((kind, H.symp_matrix.astype(bool), coeff.astype(np.complex128)))

    def add_random(kind, n, T, half_diagonal):
        codes = rng.choice(1 << (2 * n), size=T, replace=False)      # distinct rows
        symp = ((codes[:, None] >> np.arange(2 * n)) & 1).astype(bool)
        # the reference's diagonal constructor needs a diagonal term other than the identity: three diagonal rows at least, no identity
        symp[: T // 2 if half_diagonal else 3, :n] = False
        symp = np.unique(symp[np.any(symp, axis=1)], axis=0)
        symp = symp[rng.permutation(len(symp))]
        specs.append((kind, symp, rng.standard_normal(len(symp)).astype(np.complex128)))

    for k, (n, T) in enumerate([(3, 10), (3, 40), (4, 25), (4, 60), (5, 33), (5, 60), (6, 48), (6, 60), (7, 57), (8, 60), (8, 17), (5, 12)]):
        add_random('dfs', n, T, half_diagonal=k % 2 == 1)
    for k, (n, T) in enumerate([(5, 100), (5, 300), (6, 129), (6, 300), (7, 200), (7, 65), (8, 300), (8, 256)]):
        add_random('sweep', n, T, half_diagonal=k % 2 == 1)

    out = {'n_cases': np.int64(len(specs))}
    for k, (kind, symp, coeff) in enumerate(specs):
        tag = f'{k:02d}'
        assert len(np.unique(symp, axis=0)) == len(symp), f'case {tag}: repeated rows'
        assert distinct_magnitudes(coeff), f'case {tag}: two coefficients of one magnitude'
        H = RefOp(symp, coeff)
        out[f'{tag}/kind'], out[f'{tag}/symp'], out[f'{tag}/coeff'] = np.str_(kind), symp, coeff
        swept = perform_noncontextual_sweep(H)
        # the kept indices: the rows are distinct, so every kept row names its index
        index_of = {row.tobytes(): i for i, row in enumerate(symp)}
        kept = np.array([index_of[row.astype(bool).tobytes()] for row in swept.symp_matrix], dtype=np.int64)
        assert np.all(np.diff(kept) > 0)
        adj = oracle.adjacency(symp)
        assert np.array_equal(oracle.ref_sweep(adj), kept), f'case {tag}: the restated loop differs from the reference'
        assert np.array_equal(oracle.rule_sweep(adj)[0], kept), f'case {tag}: the rule differs from the reference'
        out[f'{tag}/kept'] = kept
        seed = 1000 + k
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            results = {'single_magnitude': RefNC._single_sweep_noncontextual_operator(H, strategy='magnitude'),
                       'diag_first': RefNC._diag_first_noncontextual_op(H)}
            np.random.seed(seed)
            results['single_random'] = RefNC._single_sweep_noncontextual_operator(H, strategy='random')
            if kind == 'dfs':
                results['dfs_magnitude'] = RefNC._dfs_noncontextual_op(H, runtime=1e9, strategy='magnitude')
                results['dfs_largest'] = RefNC._dfs_noncontextual_op(H, runtime=1e9, strategy='largest')
        out[f'{tag}/random_seed'] = np.int64(seed)
        for name, op in results.items():
            out[f'{tag}/{name}/symp'], out[f'{tag}/{name}/coeff'] = op.symp_matrix.astype(bool), op.coeff_vec.astype(np.complex128)
        print(f'case {tag} {kind:5s}: n = {symp.shape[1] // 2} T = {len(coeff):3d} kept = {len(kept):3d} ' +
              ' '.join(f'{name} = {op.n_terms}' for name, op in results.items()), flush=True)
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(specs)} cases, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
