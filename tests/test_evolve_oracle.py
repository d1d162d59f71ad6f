"""No device: the NumPy restatement of symgpu_cheb_apply (tests/_evolve_oracle.py) and the host half of evolve_state
(symmer_amd/evolution/time_evolution.py: chebyshev_coefficients, spectral_interval 'norm1') against things that do not share their text —
scipy.linalg.expm of the dense matrix, numpy.polynomial.chebyshev.chebval of the exponential itself, numpy.linalg.eigvalsh.

THE ROUNDING ALLOWANCE R.  The truncation error of a step is bounded by the dropped tail that chebyshev_coefficients returns; what is left
is rounding — of the recurrence, and of scipy's expm on the other side.  Over ACCURACY_CASES (the Hermitian draws of
_evolve_oracle.hermitian_case on 1, 3 and 6 qubits, sum|c| = 4, t in {0.1, 1, 5}, real and imaginary time, tol = 1e-10, unit vectors)
the worst ||oracle - expm psi||_2 - tail was measured as

    MEASURED_EXCESS = -4.9e-14     (every deviation stayed BELOW its tail; the largest deviation, 9.2e-11, belongs to an imaginary-time
                                    case with an eigenvalue at the lower edge, where the dropped terms all have one sign)

R = max(8 * MEASURED_EXCESS, 1e-13) = 1e-13.  It is measured against scipy's expm, never against the device, and every accuracy assertion
here and in tests/test_gpu_evolve.py is `<= tail + R`, errors as 2-norms of unit states."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb
from scipy.linalg import expm

import _ansatz_oracle as ao
import _evolve_oracle as evo
import _statevector_families as sf
from symmer_amd import PauliwordOp
from symmer_amd.evolution import chebyshev_coefficients, spectral_interval

MEASURED_EXCESS = -4.9e-14
R = max(8 * MEASURED_EXCESS, 1e-13)
TOL = 1e-10
ACCURACY_CASES = [(seed, n, t, imaginary) for n in (1, 3, 6) for seed in (0, 1, 2) for t in (0.1, 1.0, 5.0) for imaginary in (False, True)]


def exact_step(symp, coeff, interval, t, imaginary, psi):
    """expm of the dense matrix on psi: exp(-i H t) psi, or exp(-t (H - E_low)) psi, E_low = centre - half_width (the scaling of the
    imaginary-time coefficients)."""
    H = ao.dense_operator(symp, coeff)
    if imaginary:
        return expm(-t * (H - (interval[0] - interval[1]) * np.eye(H.shape[0]))) @ psi
    return expm(-1j * t * H) @ psi


def oracle_step(symp, coeff, t, imaginary, psi, tol=TOL):
    """(the oracle's state, the exact one, tail) of one step with the 'norm1' interval of the operator as given."""
    interval = spectral_interval(PauliwordOp(symp, coeff), None, 'norm1')
    coeffs, tail = chebyshev_coefficients(interval[1] * t, tol, imaginary)
    got = evo.propagate(symp, coeff, interval, coeffs, psi, None if imaginary else t)
    return got, exact_step(symp, coeff, interval, t, imaginary, psi), tail


def excess(seed, n, t, imaginary):
    symp, coeff = evo.hermitian_case(seed, n)
    got, want, tail = oracle_step(symp, coeff, t, imaginary, sf.vector(seed, n, 'gaussian'))
    return float(np.linalg.norm(got - want)), tail


def test_the_recorded_rounding_allowance_covers_every_accuracy_case():
    worst_excess, worst_deviation = -np.inf, 0.0
    for case in ACCURACY_CASES:
        deviation, tail = excess(*case)
        assert tail <= TOL
        assert deviation <= tail + R, f'{case}: deviation {deviation:.3e}, tail {tail:.3e}'
        worst_excess, worst_deviation = max(worst_excess, deviation - tail), max(worst_deviation, deviation)
    print(f'worst deviation - tail = {worst_excess:.3e}, worst deviation = {worst_deviation:.3e}')


@pytest.mark.parametrize('n', [1, 3, 6])
def test_oracle_is_expm_when_the_series_is_carried_to_rounding(n):
    """With tol = 1e-15 the truncation is below rounding: the oracle IS the propagator, within R alone."""
    symp, coeff = evo.hermitian_case(3, n)
    for t, imaginary in ((0.7, False), (2.0, True)):
        got, want, tail = oracle_step(symp, coeff, t, imaginary, sf.vector(7, n, 'gaussian'), tol=1e-15)
        assert tail <= 1e-15 and np.linalg.norm(got - want) <= tail + R


def test_oracle_identity_and_single_term_by_hand():
    """H = 3 I: centre 3, half_width 1, H~ = 0, so T_k psi = (1, 0, -1, 0, ...) psi; H = Z with c = (1, 2, 4, 8): even orders keep psi, odd
    ones apply Z."""
    psi = np.array([0.5 + 0.25j, -0.125 + 1j])
    c = np.array([1, 2, 4, 8, 16], dtype=np.complex128)
    identity = np.zeros((1, 2), dtype=bool)
    assert np.array_equal(evo.cheb_apply(identity, [3.0], 3.0, 1.0, c, psi), (1 - 4 + 16) * psi)
    z = np.array([[False, True]])
    assert np.array_equal(evo.cheb_apply(z, [1.0], 0.0, 1.0, c[:4], psi), (1 + 4) * psi + (2 + 8) * psi * [1, -1])
    assert np.array_equal(evo.cheb_apply(np.zeros((0, 2), dtype=bool), [], 0.0, 1.0, c[:3], psi), (1 - 4) * psi)       # H = 0


@pytest.mark.parametrize('imaginary', [False, True])
@pytest.mark.parametrize('z', [0, 0.3, 5, 80])
def test_coefficients_reproduce_the_exponential_within_the_tail_and_K_is_minimal(z, imaginary):
    x = np.linspace(-1.0, 1.0, 201)
    for tol in (1e-6, 1e-10, 1e-13):
        c, tail = chebyshev_coefficients(z, tol, imaginary)
        want = np.exp(-z * (x + 1.0)) if imaginary else np.exp(-1j * z * x)
        # chebval's own rounding: K additions of terms bounded by |c_k|, a few ulp each
        assert np.abs(npcheb.chebval(x, c) - want).max() <= tail + 8 * len(c) * 2.0 ** -53 * max(1.0, np.abs(c).sum())
        assert 0 <= tail <= tol
        if z == 0:
            assert np.array_equal(c, [1]) and tail == 0
            continue
        K = len(c) - 1
        assert K >= 1 and tail + abs(c[K]) > tol, 'one order fewer would have done'
        longer, _ = chebyshev_coefficients(z, tol * 1e-3, imaginary)
        assert np.array_equal(longer[:K + 1], c)
    assert c.dtype == np.complex128


def test_coefficients_refuse_what_they_cannot_deliver():
    with pytest.raises(ValueError):
        chebyshev_coefficients(5.0, 1e-300)              # no order of the window has so small a tail
    with pytest.raises(ValueError):
        chebyshev_coefficients(-1.0, 1e-10)
    with pytest.raises(ValueError):
        chebyshev_coefficients(np.inf, 1e-10)
    with pytest.raises(ValueError):
        chebyshev_coefficients(1.0, 0.0)


def test_orders_grow_as_the_issue_measured():
    """K = a t plus a slowly growing margin: 46 at a t = 21 and 706 at a t = 630 for a tail of 1e-12 (the trial that motivated the design)."""
    assert len(chebyshev_coefficients(21.0, 1e-12)[0]) - 1 == pytest.approx(46, abs=3)
    assert len(chebyshev_coefficients(630.0, 1e-12)[0]) - 1 == pytest.approx(706, abs=8)


@pytest.mark.parametrize('seed', range(24))
def test_norm1_interval_contains_the_spectrum(seed):
    """A containment: the interval gets no tolerance.  The REFERENCE does: a draw whose terms all share one X-part, or a single term,
    attains the bound exactly (seed 3: eigvalsh returned the edge plus 4e-16), and the eigenvalues compared are those of a matrix built
    with T rounded additions per entry by a backward-stable solver, so they are the exact ones only within (T + 2^n) 2^-52 ||H||."""
    op = sf.operator(seed, hermitian=True, n_max=7, t_max=40)
    centre, half_width = spectral_interval(PauliwordOp(op.symp, op.coeff), None, 'norm1')
    ev = np.linalg.eigvalsh(ao.dense_operator(op.symp, op.coeff))
    reference_error = (op.symp.shape[0] + (1 << op.n)) * 2.0 ** -52 * np.abs(op.coeff).sum()
    assert centre - half_width <= ev[0] + reference_error and ev[-1] - reference_error <= centre + half_width


def test_interval_edge_cases():
    assert spectral_interval(PauliwordOp.from_list(['II'], [2.5]), None, 'norm1') == (2.5, 1.0)           # H = 2.5 I: no width, half_width 1
    assert spectral_interval(PauliwordOp.from_list(['XI', 'II', 'ZZ'], [-0.5, 1.25, 2.0]), None) == (1.25, 2.5)
    assert spectral_interval(PauliwordOp.from_list(['XI'], [3.0]), None, (0.5, 4)) == (0.5, 4.0)          # a pair is passed through
    for bad in ((0.0, 0.0), (np.nan, 1.0), (0.0, np.inf), (0.0, -1.0)):
        with pytest.raises(ValueError):
            spectral_interval(PauliwordOp.from_list(['XI'], [3.0]), None, bad)
    with pytest.raises(ValueError):
        spectral_interval(PauliwordOp.from_list(['XI'], [3.0]), None, 'gershgorin')
