"""Writes tests/golden/noncon_solve.npz: answers of the REFERENCE's ``NoncontextualOp`` (symmer/operators/noncontextual_op.py) —
its generators, its reconstruction and its brute-force ``solve``.  Build container only: the reference is imported through
``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has neither.  The file holds data only: per case
the operator (symplectic matrix, coefficients), the symmetry generators, the clique representatives, ``G_indices``, ``C_indices``,
``pauli_mult_signs``, the solved ``energy`` and ``nu``, and for the reference-state cases the bit array and the sector it fixes.

    python tools/gen_golden_noncon_solve.py

Cases: ``NoncontextualOp.random`` over 3 .. 13 qubits, 2 .. 5 cliques and 2 .. 300 commuting terms (up to 1,500 terms, up to 11
generators), the three noncontextual lists of the reference's ``test_is_noncontextual``, all-commuting operators (no clique), operators
whose only term outside the cliques is the identity, and five solves with a reference state, one of which fixes every generator.

Checked here and printed: every recorded term has at most one clique bit; tests/_noncon_oracle.py reproduces every energy from the
recorded reconstruction; and the number of cases whose minimiser is unique (gap to the second-best energy above 1e-9 sum|c|) — the
test of ``nu`` needs three quarters of the cases to qualify.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'noncon_solve.npz')


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    _load('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    oracle = _load('_noncon_oracle', os.path.join(ROOT, 'tests', '_noncon_oracle.py'))
    from symmer.operators import PauliwordOp as RefOp, NoncontextualOp as RefNC
    np.random.seed(20261020)
    rng = np.random.default_rng(20261020)

    specs = []                                                       # (kind, symp, coeff, ref_state or None)

    def add_random(kind, n, q, k, clifford=True, ref_state=False):
        H = RefNC.random(n, n_cliques=q, n_commuting_terms=k, apply_clifford=clifford)
        specs.append((kind, H.symp_matrix.astype(bool), H.coeff_vec.astype(np.complex128),
                      rng.integers(0, 2, n).astype(np.int64) if ref_state else None))

    grid = [(3, 2, 2), (3, 3, 4), (4, 2, 8), (4, 3, 5), (5, 3, 10), (5, 4, 6), (5, 5, 8), (6, 2, 20), (6, 3, 16), (6, 4, 12),
            (7, 3, 30), (7, 5, 20), (8, 2, 60), (8, 3, 40), (8, 4, 25), (9, 3, 80), (9, 5, 50), (10, 2, 150), (10, 3, 100),
            (10, 4, 64), (11, 3, 200), (11, 5, 120), (12, 3, 250), (12, 4, 300), (13, 3, 300), (13, 5, 250), (13, 2, 128)]
    for n, q, k in grid:
        add_random('random', n, q, k)
    for labels in (['XZ', 'ZX', 'XX', 'YY'], ['XX', 'YY', 'ZZ', 'II'],
                   ['IZI', 'ZII', 'IIY', 'ZZY', 'XXZ', 'XYZ', 'YXZ', 'YYZ', 'XXX', 'XYX', 'YXX', 'YYX']):
        P = RefOp.from_list(labels, rng.standard_normal(len(labels)))
        specs.append(('list', P.symp_matrix.astype(bool), P.coeff_vec.astype(np.complex128), None))
    add_random('commuting', 6, 0, 20)
    add_random('commuting', 9, 0, 100)
    add_random('no_s0', 5, 3, 0)
    add_random('no_s0', 8, 5, 0)
    # reference states: without the Clifford scrambling part of the generators stay diagonal, so a bit array fixes some and leaves some
    add_random('ref_state', 6, 3, 16, clifford=False, ref_state=True)
    add_random('ref_state', 8, 2, 40, clifford=False, ref_state=True)
    add_random('ref_state', 9, 4, 60, clifford=False, ref_state=True)
    add_random('ref_state', 7, 3, 30, clifford=True, ref_state=True)
    n = 7                                                            # a diagonal operator: every generator is diagonal, every one is fixed
    rows = np.unique(rng.integers(0, 2, (40, n)).astype(bool), axis=0)
    specs.append(('ref_state', np.hstack([np.zeros_like(rows), rows]), rng.standard_normal(len(rows)).astype(np.complex128),
                  rng.integers(0, 2, n).astype(np.int64)))

    out = {'n_cases': np.int64(len(specs))}
    n_unique, n_fixed_all = 0, 0
    for k, (kind, symp, coeff, ref_state) in enumerate(specs):
        tag = f'{k:02d}'
        H = RefNC(symp, coeff)
        sector = None
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if ref_state is not None:
                H.symmetry_generators.update_sector(ref_state)
                sector = np.asarray(H.symmetry_generators.coeff_vec).astype(np.int64).copy()
            H.solve(strategy='brute_force', ref_state=ref_state)
        G, C = np.asarray(H.G_indices).astype(np.int8), np.asarray(H.C_indices).astype(np.int8).reshape(len(coeff), -1)
        assert np.all(C.sum(axis=1) <= 1), f'case {tag}: a term with more than one clique bit'
        signs = np.asarray(H.pauli_mult_signs).astype(np.int8)
        nu = np.asarray(H.symmetry_generators.coeff_vec).astype(np.int64)
        e_or, nu_or, energies = oracle.solve(coeff, G, C, signs, sector)
        tol = oracle.tolerance(coeff.real)
        assert abs(e_or - H.energy) <= tol, f'case {tag}: the restated objective gives {e_or}, the reference {H.energy}'
        unique = oracle.unique_minimum(energies, coeff)
        if unique:
            assert np.array_equal(nu_or, nu), f'case {tag}: the restated tie rule gives {nu_or}, the reference {nu}'
        n_unique += unique
        n_fixed_all += sector is not None and bool(np.all(sector != 0))
        out[f'{tag}/n'] = np.int64(symp.shape[1] // 2)
        out[f'{tag}/symp'], out[f'{tag}/coeff'] = symp, coeff
        out[f'{tag}/generators'] = H.symmetry_generators.symp_matrix.astype(bool)
        out[f'{tag}/cliques'] = H.clique_operator.symp_matrix.astype(bool).reshape(H.n_cliques, symp.shape[1])
        out[f'{tag}/G_indices'], out[f'{tag}/C_indices'], out[f'{tag}/pauli_mult_signs'] = G, C, signs
        out[f'{tag}/energy'], out[f'{tag}/nu'] = np.float64(H.energy), nu
        out[f'{tag}/unique'] = np.bool_(unique)
        if ref_state is not None:
            out[f'{tag}/ref_state'], out[f'{tag}/sector'] = ref_state, sector
        print(f'case {tag} {kind:9s}: n = {symp.shape[1] // 2:2d} T = {len(coeff):4d} generators = {G.shape[1]:2d} cliques = {H.n_cliques} '
              f'free = {G.shape[1] if sector is None else int(np.sum(sector == 0)):2d} energy = {H.energy:+.12f} unique = {unique}')
    assert n_fixed_all >= 1, 'no reference-state case fixes every generator'
    assert 4 * n_unique >= 3 * len(specs), 'fewer than three quarters of the cases have a unique minimiser: pick other seeds'
    np.savez_compressed(OUT, **out)
    print(f'every recorded term has at most one clique bit; unique minimiser in {n_unique} of {len(specs)} cases')
    print(f'wrote {OUT}: {len(specs)} cases, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
