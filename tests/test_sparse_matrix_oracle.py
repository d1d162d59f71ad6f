"""CPU: the NumPy restatement of to_sparse_matrix's contract (tests/_sparse_oracle.py) against an explicit Kronecker product."""
import numpy as np
import pytest

import _sparse_oracle as so


def _random_op(rng, n, T, p=0.5, dyadic=True):
    symp = rng.random((T, 2 * n)) < p
    if dyadic:
        c = (rng.integers(-8, 9, T) + 1j * rng.integers(-8, 9, T)) / 8.0
    else:
        c = rng.normal(size=T) + 1j * rng.normal(size=T)
    return symp, c


def _check_canonical(data, indices, indptr, side):
    assert indptr[0] == 0 and indptr[-1] == len(data) == len(indices) and len(indptr) == side + 1
    assert np.all(np.diff(indptr) >= 0)
    for r in range(side):
        cols = indices[indptr[r]:indptr[r + 1]]
        assert np.all(np.diff(cols) > 0)
    assert not np.any((data.real == 0) & (data.imag == 0))


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 6])
def test_oracle_matches_kron_random(n):
    rng = np.random.default_rng(100 + n)
    symp, c = _random_op(rng, n, 3 * n + 2)
    data, indices, indptr = so.to_csr(symp, c)
    _check_canonical(data, indices, indptr, 1 << n)
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))


def test_oracle_all_y_and_duplicates_and_zeros():
    n = 4
    allY = np.ones((1, 2 * n), dtype=bool)
    rng = np.random.default_rng(7)
    symp, c = _random_op(rng, n, 6)
    symp = np.vstack([allY, symp, symp[:3], allY])            # duplicates, including the all-Y term
    c = np.concatenate([[0.5 - 0.25j], c, c[:3] * 2, [0.0]])    # a zero coefficient
    c[2] = 0
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))
    _check_canonical(*so.to_csr(symp, c), 1 << n)


def test_oracle_exact_cancellation_drops_entries():
    # I + Z on qubit 0 (the most significant bit): rows with qubit 0 = 1 cancel to an exact zero
    n = 3
    I = np.zeros(2 * n, dtype=bool)
    Z0 = I.copy(); Z0[n] = True
    data, indices, indptr = so.to_csr(np.vstack([I, Z0]), [1.0, 1.0])
    assert np.array_equal(indptr, [0, 1, 2, 3, 4, 4, 4, 4, 4])
    assert np.array_equal(indices, [0, 1, 2, 3])
    assert np.array_equal(data, [2, 2, 2, 2])
    # X - X cancels everywhere
    X1 = I.copy(); X1[1] = True
    data, indices, indptr = so.to_csr(np.vstack([X1, X1]), [1.0, -1.0])
    assert len(data) == 0 and np.all(indptr == 0)


def test_oracle_qubit_order_single_terms():
    # X on qubit 0 flips the most significant bit; Z on qubit n-1 reads the least significant one; Y = [[0, -i], [i, 0]]
    n = 2
    X0 = np.array([[1, 0, 0, 0]], dtype=bool)
    assert np.array_equal(so.to_dense(X0, [1]), np.kron([[0, 1], [1, 0]], np.eye(2)))
    Z1 = np.array([[0, 0, 0, 1]], dtype=bool)
    assert np.array_equal(so.to_dense(Z1, [1]), np.diag([1, -1, 1, -1]).astype(complex))
    Y0 = np.array([[1, 0, 1, 0]], dtype=bool)
    assert np.array_equal(so.to_dense(Y0, [1]), np.kron([[0, -1j], [1j, 0]], np.eye(2)))


def test_oracle_sums_in_operator_order_and_keeps_nan():
    n = 1
    I = np.zeros((1, 2), dtype=bool)
    big, tiny = 1e16, 3.0
    data, _, _ = so.to_csr(np.vstack([I, I, I]), [big, tiny, -big])
    assert data[0] == (big + tiny) - big == 4.0               # operator order, not a compensated or reordered sum
    data, indices, indptr = so.to_csr(np.vstack([I, I]), [np.nan, 1.0])
    assert len(data) == 2 and np.all(np.isnan(data.real))


@pytest.mark.parametrize('name, n_qubits, n_terms', [('B+_STO-3G_SINGLET_JW.json', 10, 156), ('BH_STO-3G_SINGLET_JW.json', 12, 631)])
def test_golden_molecule_fixtures(name, n_qubits, n_terms):
    import json
    import os
    with open(os.path.join(os.path.dirname(__file__), 'golden', name)) as f:
        d = json.load(f)
    H = d['hamiltonian']
    assert len(H) == n_terms and all(len(k) == n_qubits for k in H)
    assert len(d['data']['hf_array']) == n_qubits
