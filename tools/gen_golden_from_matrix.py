"""Writes tests/golden/from_matrix.npz: answers of the REFERENCE's ``PauliwordOp.from_matrix(strategy='projector')``
(symmer/operators/base.py:286-425) on small matrices.  Build container only: the reference is imported through
``oracle/tools/ref_shim.py`` (by path), which needs the reference checkout; the GPU box has neither.  The file holds data only:
per case the input (a dense matrix, or the three CSR arrays) and the reference's symplectic matrix and coefficients.

    python tools/gen_golden_from_matrix.py

Cases: dense, n = 1 .. 5, dyadic entries (a + b i) / 8 with about 30 % zeros; dense Gaussian, n = 3, 4, 5; CSR inputs (dyadic
entries) of density 0.3 and 0.8 at n = 2 .. 4.  ``strategy='full_basis'`` cannot run here (the reference's ``to_sparse_matrix`` needs
qiskit, which the shim mocks).  The reference's term order is whatever ``dok_matrix.nonzero()`` yields; the tests compare as sets.
"""
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'from_matrix.npz')


def _load_shim():
    spec = importlib.util.spec_from_file_location('ref_shim', os.path.join(ROOT, 'oracle', 'tools', 'ref_shim.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)


def dyadic(rng, shape):
    return (rng.integers(-8, 9, shape) + 1j * rng.integers(-8, 9, shape)) / 8.0


def main():
    _load_shim()
    from symmer.operators import PauliwordOp as RefOp
    rng = np.random.default_rng(20240607)
    cases = []
    for n in range(1, 6):
        side = 1 << n
        m = dyadic(rng, (side, side))
        m[rng.random((side, side)) < 0.3] = 0
        cases.append(('dense', 'dyadic', n, m))
    for n in (3, 4, 5):
        side = 1 << n
        cases.append(('dense', 'gaussian', n, rng.standard_normal((side, side)) + 1j * rng.standard_normal((side, side))))
    for n in (2, 3, 4):
        for density in (0.3, 0.8):
            side = 1 << n
            m = dyadic(rng, (side, side))
            m[rng.random((side, side)) >= density] = 0
            cases.append(('csr', 'dyadic', n, scipy.sparse.csr_matrix(m)))
    out = {'n_cases': np.int64(len(cases))}
    for k, (layout, kind, n, m) in enumerate(cases):
        ref = RefOp.from_matrix(m, strategy='projector', disable_loading_bar=True)
        tag = f'{k:02d}'
        out[f'{tag}/layout'], out[f'{tag}/kind'], out[f'{tag}/n'] = np.array(layout), np.array(kind), np.int64(n)
        if layout == 'dense':
            out[f'{tag}/matrix'] = m
        else:
            out[f'{tag}/data'], out[f'{tag}/indices'], out[f'{tag}/indptr'] = m.data.astype(np.complex128), m.indices, m.indptr
        out[f'{tag}/symp'] = np.asarray(ref.symp_matrix, dtype=bool)
        out[f'{tag}/coeff'] = np.asarray(ref.coeff_vec, dtype=np.complex128)
        print(f'case {tag}: {layout:5s} {kind:8s} n = {n}: {ref.n_terms} terms')
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    sys.exit(main())
