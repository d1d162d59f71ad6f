"""Writes tests/golden/clique_cover.npz: answers of the REFERENCE's ``PauliwordOp.clique_cover`` and ``qubitwise_commutes_termwise``
(symmer/operators/base.py:1266-1364, 985-1009; networkx 3.4.2).  Build container only: the reference is imported through
``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has neither.  The file holds data only: per case
the operator (symplectic matrix, coefficients), the reference's QWC table, and for each of the three relations and both strategies the
clique index of every term and the term indices clique after clique, in the order the clique's own rows have.

    python tools/gen_golden_clique_cover.py

Cases: n in 2 .. 10 and 130, 5 .. 200 terms.  Rows are distinct and so are the magnitudes of the coefficients (no argsort ties, and the
reference's per-term ``+`` neither merges nor drops a term); several cases hold the all-identity row.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'clique_cover.npz')
RELATIONS = ('C', 'AC', 'QWC')
STRATEGIES = ('sorted_insertion', 'largest_first')


def _load_shim():
    spec = importlib.util.spec_from_file_location('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)


def make_operator(rng, n, T, density, identity):
    """T distinct rows (the all-identity row first among them if asked for), Gaussian complex coefficients of distinct magnitude."""
    rows = {}
    if identity:
        rows[bytes(2 * n)] = np.zeros(2 * n, dtype=bool)
    while len(rows) < T:
        r = rng.random(2 * n) < density
        rows.setdefault(r.astype(np.uint8).tobytes(), r)
    symp = np.array(list(rows.values()), dtype=bool)[rng.permutation(T)]
    coeff = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    assert len(np.unique(np.abs(coeff))) == T and np.abs(coeff).min() > 1e-6
    return symp, coeff


def main():
    _load_shim()
    from symmer.operators import PauliwordOp as RefOp
    rng = np.random.default_rng(20261019)
    shapes = [  # (n, T, density, identity row)
        (2, 5, 0.5, False), (2, 16, 0.5, True), (3, 20, 0.5, False), (3, 40, 0.4, True), (4, 60, 0.5, False), (5, 100, 0.3, True),
        (6, 150, 0.3, False), (8, 200, 0.2, False), (8, 64, 0.5, True), (10, 200, 0.3, True), (10, 33, 0.1, False),
        (130, 50, 0.02, True), (130, 200, 0.01, False), (130, 120, 0.3, False)]
    out = {'n_cases': np.int64(len(shapes))}
    n_answers = 0
    for k, (n, T, density, identity) in enumerate(shapes):
        symp, coeff = make_operator(rng, n, T, density, identity)
        tag = f'{k:02d}'
        key_of = {row.astype(np.uint8).tobytes(): t for t, row in enumerate(symp)}
        assert len(key_of) == T
        H = RefOp(symp, coeff)
        out[f'{tag}/n'], out[f'{tag}/symp'], out[f'{tag}/coeff'] = np.int64(n), symp, coeff.astype(np.complex128)
        out[f'{tag}/qwc'] = np.asarray(H.qubitwise_commutes_termwise(H), dtype=bool)
        counts = []
        for rel in RELATIONS:
            for strat in STRATEGIES:
                cover = RefOp(symp, coeff).clique_cover(edge_relation=rel, strategy=strat)
                assert list(cover.keys()) == list(range(len(cover))), 'the reference fills its dict in colour order'
                colour = np.full(T, -1, dtype=np.int32)
                members = []
                for c, clique in cover.items():
                    idx = [key_of[row.astype(np.uint8).tobytes()] for row in clique.symp_matrix]
                    assert np.array_equal(clique.coeff_vec, coeff[idx]), 'a clique is a selection of the terms, coefficients untouched'
                    colour[idx] = c
                    members += idx
                assert sorted(members) == list(range(T)), 'the cliques partition the terms'
                out[f'{tag}/{rel}/{strat}/colour'] = colour
                out[f'{tag}/{rel}/{strat}/members'] = np.array(members, dtype=np.int32)
                counts.append(len(cover))
                n_answers += 1
        print(f'case {tag}: n = {n:3d} T = {T:3d} cliques (C, AC, QWC) x (sorted_insertion, largest_first): {counts}')
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {n_answers} covers of {len(shapes)} operators, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
