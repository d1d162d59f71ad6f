"""The NumPy restatement of PauliwordOp.from_matrix's contract (tests/_pauli_decomp_oracle.py) against the REFERENCE's answers
(tests/golden/from_matrix.npz, written by tools/gen_golden_from_matrix.py) and against the definition (a Kronecker-product matrix of a
known operator decomposes into that operator), and the argument errors that are raised before any device call.  No GPU."""
import numpy as np
import pytest
import scipy.sparse

import _pauli_decomp_oracle as po
import _sparse_oracle as so
from symmer_amd import PauliwordOp


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 8.0


@pytest.mark.parametrize('case', range(14))
def test_restatement_matches_the_reference(case):
    cases = po.golden_cases()
    assert len(cases) == 14
    tag, layout, kind, n, dense, csr, ref_symp, ref_coeff = cases[case]
    x, z, c = po.decompose(dense, n)
    assert np.all(np.diff(x * (1 << n) + z) > 0), 'not in ascending (x, z) order'
    po.assert_matches_reference(x, z, c, ref_symp, ref_coeff, kind, n, dense)


def test_goldens_cover_what_they_should():
    kinds = [(layout, kind, n) for _, layout, kind, n, *_ in po.golden_cases()]
    assert [k for k in kinds if k[:2] == ('dense', 'dyadic')] == [('dense', 'dyadic', n) for n in range(1, 6)]
    assert [k for k in kinds if k[1] == 'gaussian'] == [('dense', 'gaussian', n) for n in (3, 4, 5)]
    assert [k for k in kinds if k[0] == 'csr'] == [('csr', 'dyadic', n) for n in (2, 3, 4) for _ in range(2)]


@pytest.mark.parametrize('n', range(1, 6))
def test_restatement_inverts_the_kronecker_definition(n):
    rng = np.random.default_rng(40 + n)
    t = min(4 ** n, 3 * n + 2)
    picked = np.sort(rng.choice(4 ** n, size=t, replace=False))              # distinct terms as (x, z) slots, ascending
    x, z = picked >> n, picked & ((1 << n) - 1)
    c = dyadic(rng, t)
    c[(c.real == 0) & (c.imag == 0)] = 0.125
    symp = po.symp_of(x, z, n)
    gx, gz, gc = po.decompose(so.kron_dense(symp, c), n)
    assert np.array_equal(gx, x) and np.array_equal(gz, z)
    assert np.array_equal(gc, c)
    assert np.array_equal(po.symp_of(gx, gz, n), symp)


def test_tiled_transform_performs_the_same_additions():
    """Low bits inside tiles, then the high bits across tiles: bit-equal to the plain butterfly on Gaussian data."""
    rng = np.random.default_rng(7)
    n, t = 7, 3
    re, im = rng.standard_normal((5, 1 << n)), rng.standard_normal((5, 1 << n))
    want_re, want_im = po.wht_pinned(re.copy(), im.copy())
    a, b = re.copy().reshape(5, 1 << (n - t), 1 << t), im.copy().reshape(5, 1 << (n - t), 1 << t)
    po.wht_pinned(a, b)                                                       # bits [0, t) inside every tile
    a, b = np.ascontiguousarray(a.transpose(0, 2, 1)), np.ascontiguousarray(b.transpose(0, 2, 1))
    po.wht_pinned(a, b)                                                       # bits [t, n) across the tiles
    got_re, got_im = a.transpose(0, 2, 1).reshape(5, -1), b.transpose(0, 2, 1).reshape(5, -1)
    assert np.array_equal(got_re.view(np.uint64), want_re.view(np.uint64)) and np.array_equal(got_im.view(np.uint64), want_im.view(np.uint64))


# ---- errors that need no device ------------------------------------------------------------------------------------------------------
def test_unknown_strategy_is_refused():
    with pytest.raises(ValueError, match='strategy'):
        PauliwordOp.from_matrix(np.eye(2), strategy='magic')


@pytest.mark.parametrize('bad', [[[1, 0], [0, 1]], 'XY', 3.0, None])
def test_only_arrays_and_sparse_matrices_are_taken(bad):
    with pytest.raises(ValueError, match='matrix type'):
        PauliwordOp.from_matrix(bad)


def test_more_than_31_qubits_is_refused():
    with pytest.raises(ValueError, match='32 qubits'):
        PauliwordOp.from_matrix(scipy.sparse.coo_matrix((2 ** 31 + 1, 1), dtype=complex))
    basis = PauliwordOp.from_dictionary({'I' * 32: 1})
    with pytest.raises(ValueError, match='32 qubits'):
        PauliwordOp.from_matrix(scipy.sparse.coo_matrix((1, 2 ** 32), dtype=complex), operator_basis=basis)


def test_31_qubits_without_a_basis_is_refused():
    with pytest.raises(ValueError, match='too large'):
        PauliwordOp.from_matrix(scipy.sparse.coo_matrix((2 ** 30 + 1, 2), dtype=complex))


def test_a_vector_is_not_a_matrix():
    with pytest.raises(ValueError):
        PauliwordOp.from_matrix(np.ones(4))
