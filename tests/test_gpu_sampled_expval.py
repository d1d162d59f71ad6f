"""GPU: symmer_amd.utils.sampled_expval — the finite-shot energy: QWC cliques, one layer of H / H S^+ per clique, a sampling plan,
n_shots draws at the clique's offset of the Philox stream, signed sums.  The per-term integers equal the restatement of
tests/_sample_oracle.py run on the host with the same seed and offsets; the energy lies within 6 standard errors of H.expval(psi), the
standard error from the exact per-term variances and the covariances inside a clique (a fixed seed: tests/test_sample_oracle.py runs the
same case on the restatement alone)."""
import numpy as np
import pytest

import _clique_oracle as co
import _sample_oracle as so
from symmer_amd import PauliwordOp, QuantumState
from symmer_amd.utils import sampled_expval

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', (0, 1, 12345))
def test_z_only_operator_on_a_basis_state_is_exact(seed):
    rng = np.random.default_rng(seed)
    n = 7
    z = rng.random((12, n)) < 0.5
    z[3] = False                                                     # the identity
    H = PauliwordOp(np.hstack([np.zeros_like(z), z]), rng.standard_normal(12))
    bits = rng.integers(0, 2, n)
    psi = QuantumState(bits.reshape(1, -1), [1])
    signs = (-1.0) ** (z.astype(int) @ bits)
    value, terms, clique = sampled_expval(H, psi, 50, seed=seed, return_terms=True)
    assert np.array_equal(terms, signs) and terms[3] == 1.0 and np.all(clique == 0)
    assert value == complex(np.sum(H.coeff_vec * signs)).real and abs(value - H.expval(psi).real) <= 1e-12
    assert sampled_expval(H, psi, 50, seed=seed) == value


def test_six_qubit_operator_integers_and_energy():
    symp, coeff, amp = so.expval_case()
    n, shots, seed = so.EXPVAL_QUBITS, so.EXPVAL_SHOTS, so.EXPVAL_SEED
    H, psi = PauliwordOp(symp, coeff), QuantumState.from_array(amp.reshape(-1, 1))
    value, terms, clique = sampled_expval(H, psi, shots, seed=seed, return_terms=True)
    # the cover is the device colouring, which tests/test_gpu_clique.py holds against this restatement
    order = co.term_order(symp, coeff, 'QWC', 'largest_first')
    colours = co.colouring(symp, order, 'QWC')[0]
    members = co.cliques_in_order(colours, order)
    assert np.array_equal(clique, colours)
    want = so.sampled_sums(symp, n, np.asarray(psi.to_dense_matrix).reshape(-1), members, shots, seed)
    assert np.array_equal(np.round(terms * shots).astype(np.int64), want) and np.array_equal(terms, want / shots)
    assert value == complex(np.sum(H.coeff_vec * (want / shots))).real
    exact = H.expval(psi).real
    se = so.energy_standard_error(symp, coeff, n, amp, members, shots)
    print(f'{len(members)} cliques: sampled {value:.6f}, exact {exact:.6f}, standard error {se:.6f}, off by {abs(value - exact) / se:.2f} of them')
    assert abs(exact - so.exact_energy(symp, coeff, n, amp)) <= 1e-12
    assert abs(value - exact) <= 6 * se
    # amplitudes in place of the state; the same seed, the same answer; another strategy is another cover of the same energy
    assert sampled_expval(H, amp, shots, seed=seed) == value
    other = sampled_expval(H, psi, shots, seed=seed, strategy='sorted_insertion')
    assert abs(other - exact) <= 6 * max(se, so.energy_standard_error(
        symp, coeff, n, amp, co.cliques_in_order(co.colouring(symp, co.term_order(symp, coeff, 'QWC', 'sorted_insertion'), 'QWC')[0],
                                                 co.term_order(symp, coeff, 'QWC', 'sorted_insertion')), shots))


def test_seed_none_and_refusals():
    H = PauliwordOp.from_list(['XX', 'ZZ', 'YY'], [0.5, -1.0, 0.25])
    psi = QuantumState([[0, 0], [1, 1]], [np.sqrt(0.5), np.sqrt(0.5)])
    np.random.seed(77)
    first = sampled_expval(H, psi, 1000)
    np.random.seed(77)
    assert sampled_expval(H, psi, 1000) == first
    # a Bell state: XX = 1, ZZ = 1, YY = -1 in every shot
    assert first == 0.5 - 1.0 - 0.25
    with pytest.raises(ValueError, match='normalized'):
        sampled_expval(H, QuantumState([[0, 0], [1, 1]], [1, 1]), 10)
    with pytest.raises(ValueError):
        sampled_expval(H, psi, 0)
    with pytest.raises(ValueError):
        sampled_expval(H, psi, 10, strategy='random_sequential')
    with pytest.raises(TypeError):
        sampled_expval(np.eye(4), psi, 10)
