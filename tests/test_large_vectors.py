"""CPU: the closed forms of tests/_large_vectors.py, which tests/test_gpu_statevector_large.py holds the device to at 27 and 28 qubits,
against the oracles the project already has, at 8 .. 12 qubits where psi is materialised.  Everything is exact (==) except the basis
change, which is held to its stated bound.  The same functions run at the large sizes with n as their only difference."""
from fractions import Fraction

import numpy as np
import pytest

import _ansatz_oracle as ao
import _evolve_oracle as evo
import _large_vectors as lv
import _matvec_oracle as mo
import _rdm_oracle as ro
import _sample_oracle as so

SIZES = [8, 9, 10, 11, 12]
SEEDS = list(lv.SEEDS)
CASES = [(n, seed) for n in SIZES for seed in SEEDS]


@pytest.fixture(scope='module')
def psi():
    cache = {}

    def get(n, seed):
        if (n, seed) not in cache:
            cache[(n, seed)] = lv.materialise(n, seed)
            cache[(n, seed)].setflags(write=False)
        return cache[(n, seed)]
    return get


@pytest.mark.parametrize('n, seed', CASES + [(15, 1), (26, 3)])
def test_factor_rules(n, seed):
    phase, half = lv.factors(n, seed)
    phi = lv.factor_values(n, seed)
    assert half.sum() <= lv.MAX_HALF and np.all(phi[:, 0] != phi[:, 1])
    assert all(tuple(phi[q]) != tuple(phi[q - 1]) for q in range(1, n))
    assert np.all(np.abs(phi[:, 0]) == 1) and np.all(np.isin(np.abs(phi[:, 1]), [1.0, 0.5]))
    assert np.array_equal(lv.factors(n, seed)[0], phase)                       # seeded: the same list again
    assert not np.array_equal(lv.factor_values(n, SEEDS[0]), lv.factor_values(n, SEEDS[1])) # two assignments


@pytest.mark.parametrize('n, seed', CASES)
def test_amplitudes_are_the_kronecker_product_and_the_pieces_tile_it(n, seed, psi):
    phi = lv.factor_values(n, seed)
    want = np.ones(1, dtype=np.complex128)
    for q in range(n):
        want = np.kron(want, phi[q])
    assert np.array_equal(psi(n, seed), want)
    assert np.array_equal(lv.amplitudes(n, seed, np.arange(1 << n)), want)
    idx = np.random.default_rng(n).integers(0, 1 << n, 300)
    assert np.array_equal(lv.amplitudes(n, seed, idx), want[idx])


def test_pieces_above_one_piece_are_outer_products_at_their_offsets():
    """25 qubits: two pieces of 2^24; checked on indices through `amplitudes`, which the test above holds to the Kronecker product."""
    n, seed = 25, 1
    rng = np.random.default_rng(5)
    firsts = []
    for first, piece in lv.pieces(n, seed):
        firsts.append(first)
        at = np.concatenate([[0, piece.shape[0] - 1, (1 << lv.LOW_BITS) - 1, 1 << lv.LOW_BITS], rng.integers(0, piece.shape[0], 500)])
        assert piece.shape[0] == 1 << 24 and piece.nbytes <= 256 << 20
        assert np.array_equal(piece[at], lv.amplitudes(n, seed, first + at))
    assert firsts == [0, 1 << 24]


@pytest.mark.parametrize('n', SIZES + [16, 27, 28])
def test_windows_lie_inside_do_not_repeat_and_straddle_the_middle(n):
    w = lv.windows(n)
    N = 1 << n
    assert all(0 <= first and count > 0 and first + count <= N for first, count in w)
    assert all(w[i][0] + w[i][1] <= w[i + 1][0] for i in range(len(w) - 1)), 'two windows overlap or repeat'
    idx = lv.window_indices(n)
    assert np.unique(idx).shape[0] == idx.shape[0]
    for point in (N // 4, N // 2, 3 * N // 4):
        assert point - 1 in idx and point in idx
    assert 0 in idx and N - 1 in idx
    if n >= 16:
        assert sum(c == 4096 for _, c in w) >= 5 and sum(c == 256 for _, c in w) == 64
    if n == 28:
        assert (1 << 27) - 1 in idx and 1 << 27 in idx                          # byte 2^31
    assert w == lv.windows(n)


def test_budget_rejects_one_half_magnitude_qubit_too_many():
    lv.assert_exact_budget(28, lv.MAX_HALF, 8)
    with pytest.raises(AssertionError):
        lv.assert_exact_budget(28, lv.MAX_HALF + 1, 8)
    with pytest.raises(AssertionError):
        lv.assert_exact_budget(28, lv.MAX_HALF, 9)                               # 28 + 16 + 9 = 53 bits
    with pytest.raises(AssertionError):
        lv.bits_of([0.3])                                                        # not an integer over 8
    for n in (27, 28):                                                           # the large cases themselves fit
        symp, coeff = lv.matvec_operator(n)
        lv.assert_exact_budget(n, lv.MAX_HALF, lv.bits_of(coeff) + 1)
        lv.assert_exact_budget(n, lv.MAX_HALF, lv.cheb_bits(coeff, -0.125, CHEB_C[:6]), whole_vector=False)


CHEB_C = np.array([0.5, -0.25j, 0.125, 0.25 + 0.125j, -0.125, 0.125j], dtype=np.complex128)


@pytest.mark.parametrize('n, seed', CASES)
def test_apply_terms_is_the_matvec_oracle(n, seed, psi):
    idx = np.arange(1 << n)
    for symp, coeff in (lv.matvec_operator(n), lv.aligned_operator(n, seed), lv.number_operator(n)):
        got = lv.apply_terms(symp, coeff, lambda b: lv.amplitudes(n, seed, b))(idx)
        assert np.array_equal(got, mo.matvec(symp, coeff, psi(n, seed)))
    twice = lv.apply_terms(symp, coeff, lv.apply_terms(symp, coeff, lambda b: lv.amplitudes(n, seed, b)))(idx)
    assert np.array_equal(twice, mo.matvec(symp, coeff, mo.matvec(symp, coeff, psi(n, seed))))


@pytest.mark.parametrize('n, seed', CASES)
def test_cheb_window_is_the_chebyshev_oracle_bit_for_bit(n, seed, psi):
    symp, coeff = lv.matvec_operator(n)
    idx = lv.window_indices(n)
    for K in (0, 1, 2, 3, 5):
        for centre, half_width in ((-0.125, 4.0), (0.0, 1.0)):
            want = evo.cheb_apply(symp, coeff, centre, half_width, CHEB_C[:K + 1], psi(n, seed))
            got = lv.cheb_window(symp, coeff, centre, half_width, CHEB_C[:K + 1], n, seed, idx)
            assert np.array_equal(got, want[idx]), f'K = {K}, interval {(centre, half_width)}'
    sums = lv.cheb_window(symp, coeff, -0.125, 4.0, CHEB_C, n, seed, idx, every_order=True)
    assert all(np.array_equal(sums[K], lv.cheb_window(symp, coeff, -0.125, 4.0, CHEB_C[:K + 1], n, seed, idx)) for K in range(6))
    got = lv.cheb_window(symp, coeff, 0.0, 1.0, [0, 1], n, seed, idx)
    assert np.array_equal(got, mo.matvec(symp, coeff, psi(n, seed))[idx])


@pytest.mark.parametrize('n, seed', CASES)
def test_expectations_norm_and_energy(n, seed, psi):
    v = psi(n, seed)
    assert lv.norm2(n, seed) == float(np.vdot(v, v).real)
    for symp, coeff in (lv.matvec_operator(n), lv.aligned_operator(n, seed)):
        assert lv.energy(symp, coeff, n, seed) == ao.energy(symp, coeff, v)
        for row in symp:
            assert lv.pauli_expectation(row, n, seed) == ao.energy(row[None, :], [1.0], v)
    assert all(lv.pauli_expectation(row, n, seed) != 0 for row in lv.aligned_operator(n, seed)[0])


@pytest.mark.parametrize('n, seed', [(8, 1), (8, 3), (9, 1), (10, 3)])
def test_commutator_expectation_is_the_dense_pool_gradient(n, seed, psi):
    pool = np.vstack([lv.pool_strings(n), lv.ansatz_generators(n)[0]])
    nonzero = 0
    for symp, coeff in (lv.hermitian_operator(n, seed), lv.aligned_operator(n, seed)):
        want = ao.pool_grad(ao.dense_operator(symp, coeff), pool, psi(n, seed))
        got = np.array([lv.commutator_expectation(symp, coeff, row, n, seed) for row in pool])
        assert np.array_equal(got, want)
        nonzero += np.count_nonzero(got)
    assert nonzero, 'every gradient of the case is zero: it would not notice a dropped term'


@pytest.mark.parametrize('n, seed', CASES)
def test_rotate_window_is_the_ansatz_oracle(n, seed, psi):
    symp, cos_t, sin_t = lv.ansatz_generators(n)
    x, z, y = ao.gens_of(symp)
    v = psi(n, seed)
    for k in range(len(x)):
        v = ao.rotate(x[k], z[k], y[k], cos_t[k], sin_t[k], v)
    idx = lv.window_indices(n)
    assert np.array_equal(lv.rotate_window(symp, cos_t, sin_t, n, seed, idx), v[idx])
    assert set(zip(cos_t, sin_t)) == {(0.0, 1.0), (0.0, -1.0), (-1.0, 0.0), (0.5, 0.5)}


@pytest.mark.parametrize('n, seed', CASES)
def test_rdm_exact_is_the_deposit_oracle(n, seed, psi):
    for kept in ([0], [n - 1], [0, n // 2, n - 1], [0, 2, 3, n - 3, n - 2, n - 1], []):
        assert np.array_equal(lv.rdm_exact(n, seed, kept), ro.rdm_deposit(psi(n, seed), n, kept)), kept


@pytest.mark.parametrize('n, seed', CASES)
def test_basis_window_within_its_bound_of_the_butterfly_oracle(n, seed, psi):
    xq, yq = [0, 5, n - 1], [1, n - 2]
    want = so.basis_change(psi(n, seed), n, xq, yq)
    got, bound = lv.basis_window(n, seed, xq, yq, np.arange(1 << n))
    assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
    exact = so.layer_matrix(n, xq, yq, dtype=np.clongdouble) @ psi(n, seed).astype(np.clongdouble) if n <= 10 else None
    if exact is not None:                                    # and the closed form itself is the layer: r against 1 / sqrt 2, 2^-53 a layer
        assert np.all(np.abs(got - exact) <= 5 * 2.0 ** -52 * np.abs(exact) + 2.0 ** -58 * np.abs(exact).max())
    assert np.count_nonzero(bound) > 0


@pytest.mark.parametrize('n, seed', CASES)
def test_index_of_uniform_is_the_tree_walk_and_the_exact_inverse_cdf(n, seed, psi):
    v = psi(n, seed)
    w = so.weights(v)
    levels = so.tree_build(w)
    assert len(levels) - 1 == lv.tree_depth(n) and levels[-1][0] == lv.norm2(n, seed)
    u = sampling_uniforms(n, seed, 512)
    assert u[0] == 0 and u.max() == 1 - 2.0 ** -20 and (seed != 3 or lv.boundary_uniforms(n, seed).shape[0] >= 16)
    got = lv.index_of_uniform(n, seed, u)
    assert np.array_equal(got, so.tree_walk(levels, u))
    total = Fraction(lv.norm2(n, seed))
    want, prefix = so.exact_inverse_cdf(w, [Fraction(float(x)) * total for x in u])
    assert np.array_equal(got, want)
    edge = lv.boundary_uniforms(n, seed)
    for x, i in zip(edge[:6], lv.index_of_uniform(n, seed, edge[:6])):          # on the boundary exactly, and in the interval above it
        assert Fraction(float(x)) * total == lv.cumulative_below(n, seed, int(i)) == prefix[int(i) - 1]
    for i in (0, 1, (1 << n) // 2, (1 << n) - 1, int(got[7])):
        assert lv.cumulative_below(n, seed, i) == (prefix[i - 1] if i else 0)
    philox = so.philox_uniforms(3, 1 << 40, 256)
    assert np.array_equal(lv.index_of_uniform(n, seed, philox), so.tree_walk(levels, philox))


def sampling_uniforms(n, seed, count):
    """count uniforms k / 2^20: 0, the largest below 1, values that hit a cumulative boundary exactly, the rest seeded."""
    return lv.sampling_uniforms(n, seed, count)


def test_a_flipped_phase_in_the_factor_list_is_noticed(monkeypatch):
    """The closed forms are tied to the factor list: with one phase of it flipped behind their back, the materialised vector no longer
    matches them."""
    n, seed = 9, 1
    v = lv.materialise(n, seed)
    real = lv.factors

    def flipped(n_, seed_):
        phase, half = real(n_, seed_)
        phase = phase.copy()
        phase[4, 1] = (phase[4, 1] + 2) & 3
        return phase, half
    monkeypatch.setattr(lv, 'factors', flipped)
    assert not np.array_equal(lv.amplitudes(n, seed, np.arange(1 << n)), v)
    symp, coeff = lv.aligned_operator(n, seed)
    assert lv.energy(symp, coeff, n, seed) != ao.energy(symp, coeff, v)
    assert not np.array_equal(lv.rdm_exact(n, seed, [4]), ro.rdm_deposit(v, n, [4]))
