"""CPU: the NumPy restatement of the matrix-free product (tests/_matvec_oracle.py) against the definition (an explicit Kronecker
product), and QuantumState.from_array (reference base.py:2139-2186), which is host code."""
import warnings

import numpy as np
import pytest

import _matvec_oracle as mo
import _sparse_oracle as so
import test_gpu_xgroups as xg
from symmer_amd import QuantumState


def dyadic(rng, t):
    return (rng.integers(-64, 65, t) + 1j * rng.integers(-64, 65, t)) / 8.0


@pytest.mark.parametrize('n', range(1, 7))
def test_oracle_equals_the_kronecker_definition(n):
    rng = np.random.default_rng(40 + n)
    T = 6 * n + 2
    symp = rng.random((T, 2 * n)) < 0.4
    symp[T // 2:] = symp[:T - T // 2]                       # repeated terms, not cleaned
    c = dyadic(rng, T)
    v = (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / 16.0
    want = so.kron_dense(symp, c) @ v
    assert np.array_equal(mo.matvec(symp, c, v), want)      # dyadic: exact in any order
    g = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    cg = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    assert np.abs(mo.matvec(symp, cg, g) - so.kron_dense(symp, cg) @ g).max() <= mo.error_bound(symp, cg, g)


def test_oracle_no_terms_and_diagonal():
    assert np.array_equal(mo.matvec(np.zeros((0, 6), dtype=bool), np.zeros(0), np.ones(8)), np.zeros(8))
    n = 3
    symp = np.zeros((n + 1, 2 * n), dtype=bool)
    symp[1:, n:] = np.eye(n, dtype=bool)
    c = np.array([n / 2] + [-0.5] * n)                      # sum_q (1 - Z_q) / 2
    assert np.array_equal(mo.diagonal(symp, c), [bin(b).count('1') for b in range(8)])


@pytest.mark.parametrize('n', xg.SIZES)
def test_sparse_oracle_columns_equal_the_matvec_oracle_on_unit_vectors(n):
    """The CPU twin of tests/test_gpu_xgroups.py: the property holds between the two restatements, on the same operators."""
    side = 1 << n
    for name, symp, c in xg.consumer_cases(n):
        A = xg.dense_of_csr(so.to_csr(symp, c), n)
        for j in range(side):
            e = np.zeros(side, dtype=np.complex128)
            e[j] = 1.0
            assert np.array_equal(mo.matvec(symp, c, e), A[:, j]), f'{name}: column {j}'


# ---- QuantumState.from_array ---------------------------------------------------------------------------------------------------------
def test_from_array_reference_example():
    vec = np.array([0.57735027, 0, 0, 0, 0, 0.81649658, 0, 0]).reshape([-1, 1])
    psi = QuantumState.from_array(vec)
    assert psi.vec_type == 'ket' and psi.n_qubits == 3
    assert np.array_equal(psi.state_matrix, [[0, 0, 0], [1, 0, 1]])
    assert np.array_equal(psi.state_op.coeff_vec, [0.57735027, 0.81649658])
    assert str(psi) == ' 0.577+0.000j |000> +\n 0.816+0.000j |101>'
    assert np.array_equal(psi.to_dense_matrix, vec)


def test_from_array_row_vector_is_a_bra():
    vec = np.array([[0, 0.6, 0, -0.8j]])
    psi = QuantumState.from_array(vec)
    assert psi.vec_type == 'bra' and np.array_equal(psi.state_matrix, [[0, 1], [1, 1]])
    assert np.array_equal(psi.to_dense_matrix, vec)


def test_from_array_threshold_and_ordering():
    vec = np.zeros(16, dtype=complex)
    vec[[13, 2, 7, 9]] = [0.5, 1e-16, 1e-15, -0.5j]
    vec[0] = np.sqrt(0.5)
    psi = QuantumState.from_array(vec.reshape(-1, 1))
    assert np.array_equal(so.bits_to_int(psi.state_matrix), [0, 7, 9, 13])          # ascending index; |a| >= 1e-15 kept, 1e-16 not
    assert np.array_equal(psi.state_op.coeff_vec, vec[[0, 7, 9, 13]])
    coarse = QuantumState.from_array(vec.reshape(-1, 1), threshold=0.6)
    assert np.array_equal(so.bits_to_int(coarse.state_matrix), [0])


def test_from_array_refusals_and_warning():
    with pytest.raises(AssertionError):
        QuantumState.from_array(np.ones((6, 1)) / np.sqrt(6))
    with pytest.raises(AssertionError):
        QuantumState.from_array(np.ones(4) / 2)                                     # neither a row nor a column
    with pytest.warns(UserWarning, match='not normalized'):
        QuantumState.from_array(np.ones((4, 1)))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        QuantumState.from_array(np.ones((4, 1)) / 2)
