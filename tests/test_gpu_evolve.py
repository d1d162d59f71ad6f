"""GPU: symgpu_cheb_apply (csrc/evolve.hip; MatvecPlan.chebyshev) and evolve_state (symmer_amd/evolution/time_evolution.py).

1. bit for bit against the NumPy restatement of the f11 arithmetic (tests/_evolve_oracle.py), at the sizes where the kernel can go
   wrong: 2 and 4 rows (less than a wavefront), 2^8 (one full workgroup), 2^9 (two, with gathers across them), 2^10; the orders 0 (its
   own launch), 1 (order 0 folded in), 2 (T_{k-2} is the caller's psi), 3 and 4 (both in-place roles of the two scratch vectors), 17.
2. known answers without the oracle: for H = P, T_k(P) is I or P, and with dyadic data the sum is exact.
3. physics: a single rotation against the ansatz kernel, a diagonal chain against its phases, random Hermitian operators against expm,
   the norm, the conserved energy.
4. first-order Trotter on the ansatz kernel: the derived commutator bound, and the error halves with the step.
5. imaginary time against the normalised expm, the energy never rising.
6. the 'lanczos' interval: contains the spectrum, needs no more orders, gives the same state.
7. refusals, with the device allocator's balance.
8. exponentiation.py against dense matrices and against the device Trotter product.
Every accuracy assertion is `<= tail + R` with R of tests/test_evolve_oracle.py (measured there against scipy's expm), errors as 2-norms
of unit states."""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
from scipy.linalg import expm

import _ansatz_oracle as ao
import _evolve_oracle as evo
import _matvec_oracle as mo
import _statevector_families as sf
from test_evolve_oracle import R, TOL
from symmer_amd import PauliwordOp, QuantumState, kernels, packing, _lib
from symmer_amd._lib import SymgpuError
from symmer_amd.evolution import (EvolutionResult, chebyshev_coefficients, evolve_state, exponentiate_single_Pop, spectral_interval, trotter,
                                  truncated_exponential)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')
ORDERS = [0, 1, 2, 3, 4, 17]
INTERVALS = [(0.0, 1.0), (-0.75, 3.0), (0.37, 2.7)]          # the last half_width is not a power of two: 1 / 2.7 is rounded


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.float64).view(np.uint64)


def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


def upload_operator(symp, coeff):
    if symp.shape[0] == 0:
        op = kernels.DeviceOp.alloc(1, 1, True)
        op.set_rows(0)
        return op
    return kernels.DeviceOp.upload(packing.pack_rows(symp), np.asarray(coeff, dtype=complex))


def device_cheb(symp, coeff, n, centre, half_width, coeffs, psi):
    """(out, out of a second call, psi as it is afterwards, form) through the kernels layer; every handle freed."""
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan, kernels.DeviceBuffer.upload(psi) as x, \
            kernels.DeviceBuffer(16 << n) as y, kernels.DeviceBuffer(16 << n) as y2:
        form = plan.chebyshev(centre, half_width, coeffs, x, y)
        plan.chebyshev(centre, half_width, coeffs, x, y2)
        return y.download(np.complex128, 1 << n), y2.download(np.complex128, 1 << n), x.download(np.complex128, 1 << n), form


def family(name, n, rng):
    """(symp bool[T, 2n], complex Gaussian coefficients) of the operator family `name`."""
    if name == 'y_terms':                                   # X, Y and Z everywhere, a Y string planted, repeated X-parts
        symp = rng.random((12, 2 * n)) < 0.4
        symp[0] = True
        symp[7, :n] = symp[3, :n]
    elif name == 'one_x':                                   # one group, x != 0, no diagonal group
        symp = rng.random((5, 2 * n)) < 0.5
        symp[:, :n] = False
        symp[:, int(rng.integers(n))] = True
    elif name == 'diagonal':
        symp = np.hstack([np.zeros((6, n), dtype=bool), rng.random((6, n)) < 0.5])
    elif name == 'identity':
        symp = np.zeros((1, 2 * n), dtype=bool)
    elif name == 'none':
        symp = np.zeros((0, 2 * n), dtype=bool)
    else:
        raise KeyError(name)
    return symp, gaussian(rng, symp.shape[0])


FAMILIES = ['y_terms', 'one_x', 'diagonal', 'identity', 'none']


@pytest.fixture(scope='module', autouse=True)
def plans_and_buffers_are_balanced():
    """DEV_BLOCKS_LIVE is the same before and after the module's tests (after one warm-up of every call the module makes)."""
    rng = np.random.default_rng(0)
    device_cheb(*family('y_terms', 5, rng), 5, 0.0, 1.0, gaussian(rng, 4), gaussian(rng, 32))
    H = PauliwordOp.from_list(['XZ', 'ZI', 'II'], [0.5, -0.25, 0.125])
    evolve_state(H, np.array([1, 0, 0, 0]), [0.5], observables=[H], spectral_bounds='lanczos')
    evolve_state(H, np.array([1, 0, 0, 0]), [0.5], imaginary=True)
    before = kernels.counters(BALANCE)
    yield
    gc.collect()                                             # operators a failed test's traceback kept alive hold device copies
    assert np.array_equal(kernels.counters(BALANCE), before)


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 8, 9, 10])
def test_chebyshev_equals_the_oracle_bit_for_bit(n):
    case = 0
    for name in FAMILIES:
        for K in ORDERS:
            rng = np.random.default_rng(100000 * n + 100 * case)
            symp, coeff = family(name, n, rng)
            centre, half_width = INTERVALS[case % len(INTERVALS)]
            case += 1
            c, psi = gaussian(rng, K + 1), gaussian(rng, 1 << n)
            got, again, psi_after, form = device_cheb(symp, coeff, n, centre, half_width, c, psi)
            want = evo.cheb_apply(symp, coeff, centre, half_width, c, psi)
            assert form == kernels.CHEB_DIRECT
            assert np.array_equal(bits(got), bits(want)), f'{name}, K = {K}, interval {(centre, half_width)}: not bit-equal to the oracle'
            assert np.array_equal(bits(got), bits(again)), f'{name}, K = {K}: two calls differ'
            assert np.array_equal(bits(psi_after), bits(psi)), f'{name}, K = {K}: psi was written'


# ---- 2. known answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 2.0])
@pytest.mark.parametrize('string', ['Z', 'X', 'Y', 'XYZ'])
def test_single_pauli_known_answer(string, scale):
    """H = scale P, half_width = scale, centre 0: T_k(P) = I (k even), P (k odd), and everything is a small integer over a power of two."""
    n = len(string)
    rng = np.random.default_rng(len(string) + ord(string[0]))
    P = PauliwordOp.from_list([string], [scale])
    c = (rng.integers(-8, 9, 6) + 1j * rng.integers(-8, 9, 6)) / 8.0
    psi = sf.vector(3, n, 'dyadic')
    x, z, y = ao.gens_of(P.symp_matrix)
    want = c[0::2].sum() * psi + c[1::2].sum() * ao.apply_pauli(x[0], z[0], y[0], psi)
    got, _, _, _ = device_cheb(np.asarray(P.symp_matrix, dtype=bool), [scale], n, 0.0, scale, c, psi)
    assert np.array_equal(got, want)


# ---- 3. physics ------------------------------------------------------------------------------------------------------------------------------
def evolve(symp, coeff, psi, times, **kw):
    res = evolve_state(PauliwordOp(symp, coeff), psi, list(np.atleast_1d(times)), tol=TOL, **kw)
    assert isinstance(res, EvolutionResult)
    return res


def dense_state(state):
    return np.asarray(state.to_dense_matrix).reshape(-1)


@pytest.mark.parametrize('string', ['Y', 'XZY', 'IZZ', 'XYZXYZXYZ', 'IIIIIIIIX'])
def test_one_term_is_a_rotation_of_the_ansatz_kernel(string):
    """exp(-i theta t P) = exp(i (-theta t) P): csrc/ansatz.hip applies it with the host's cos and sin, each within an ulp or two."""
    n, theta, t = len(string), 0.7, 1.3
    P = PauliwordOp.from_list([string], [theta])
    psi = sf.vector(11, n, 'gaussian')
    res = evolve(np.asarray(P.symp_matrix, dtype=bool), [theta], psi, t)
    with kernels.DeviceOp.upload(packing.pack_rows(np.asarray(P.symp_matrix, dtype=bool))) as gen, kernels.AnsatzPlan(gen, n) as ans, \
            kernels.DeviceBuffer.upload(psi) as buf:
        ans.apply([-theta * t], buf)
        want = buf.download(np.complex128, 1 << n)
    err = np.linalg.norm(dense_state(res.states[0]) - want)
    assert err <= res.tails[0] + R + 4 * 2.0 ** -52, f'{err:.3e}'
    assert res.interval == (0.0, theta) and res.orders[0] >= 1


def test_diagonal_chain_gives_the_exact_phases():
    n, t = 9, 2.0
    symp = np.zeros((n - 1, 2 * n), dtype=bool)
    for q in range(n - 1):
        symp[q, [n + q, n + q + 1]] = True
    coeff = np.linspace(0.3, 0.8, n - 1)
    psi = sf.vector(5, n, 'gaussian')
    res = evolve(symp, coeff, psi, t)
    want = np.exp(-1j * mo.diagonal(symp, coeff).real * t) * psi
    assert np.linalg.norm(dense_state(res.states[0]) - want) <= res.tails[0] + R


@pytest.mark.parametrize('t', [0.1, 1.0, 5.0])
@pytest.mark.parametrize('n', [3, 4, 5, 6])
def test_random_hermitian_operators_against_expm(n, t):
    symp, coeff = evo.hermitian_case({3: 24, 4: 27, 5: 24, 6: 27}[n], n)      # repeated terms, shared X-parts, 13 to 22 terms once cleaned
    psi = sf.vector(n, n, 'gaussian')
    res = evolve(symp, coeff, psi, t)
    got = dense_state(res.states[0])
    want = expm(-1j * t * ao.dense_operator(symp, coeff)) @ psi
    bound = res.tails[0] + R
    assert res.tails[0] <= TOL and np.linalg.norm(got - want) <= bound and abs(np.linalg.norm(got) - 1) <= bound
    interval = spectral_interval(PauliwordOp(symp, coeff).cleanup(), None, 'norm1')
    assert res.interval == pytest.approx(interval, rel=1e-14) and res.orders[0] == len(chebyshev_coefficients(res.interval[1] * t, TOL)[0]) - 1


def test_an_operator_that_cancels_to_nothing_leaves_the_state():
    symp, coeff = evo.hermitian_case(25, 4)                   # two terms, c P - c P: H = 0 once cleaned, a plan without groups
    psi = sf.vector(2, 4, 'gaussian')
    res = evolve(symp, coeff, psi, 3.0)
    assert res.interval == (0.0, 1.0) and res.orders[0] >= 1
    assert np.linalg.norm(dense_state(res.states[0]) - psi) <= res.tails[0] + R


def test_energy_is_conserved_on_a_time_grid_and_states_need_not_come_back():
    n = 6
    symp, coeff = evo.hermitian_case(31, n)
    H = PauliwordOp(symp, coeff)
    psi = sf.vector(9, n, 'gaussian')
    times = [0.0, 0.4, 0.4, 1.5]
    res = evolve_state(H, psi, times, tol=TOL, observables=[H, PauliwordOp.from_list(['I' * n], [1])])
    exact = float(np.vdot(psi, ao.dense_operator(symp, coeff) @ psi).real)
    tails = np.cumsum(res.tails)
    for i in range(len(times)):
        assert abs(res.expvals[i, 0] - exact) <= 2 * (tails[i] + R) * np.abs(coeff).sum()
        assert abs(res.expvals[i, 1] - 1) <= 2 * (tails[i] + R)
    assert res.orders[0] == 0 and res.orders[2] == 0 and res.states[2] is res.states[1] and np.array_equal(res.expvals[2], res.expvals[1])
    assert np.array_equal(bits(dense_state(res.states[0])), bits(psi))
    lean = evolve_state(H, psi, times, tol=TOL, observables=[H, PauliwordOp.from_list(['I' * n], [1])], return_states=False)
    assert lean.states is None and np.array_equal(lean.expvals, res.expvals) and lean.orders == res.orders
    # a scalar time without observables returns the state itself, the same bits as the grid's
    alone = evolve_state(H, QuantumState.from_array(psi.reshape(-1, 1)), 0.4, tol=TOL)
    assert isinstance(alone, QuantumState) and np.array_equal(bits(dense_state(alone)), bits(dense_state(res.states[1])))


# ---- 4. Trotter on the device ----------------------------------------------------------------------------------------------------------------
def device_trotter(symp, coeff, psi, t, r, reverse=False):
    """r first-order steps prod_k exp(-i c_k P_k t / r) on the ansatz kernel, term 0 applied first (reverse: last term first)."""
    n = symp.shape[1] // 2
    order = np.arange(symp.shape[0])[::-1] if reverse else np.arange(symp.shape[0])
    gens, theta = np.tile(symp[order], (r, 1)), np.tile(-np.asarray(coeff)[order] * t / r, r)
    with kernels.DeviceOp.upload(packing.pack_rows(gens)) as op, kernels.AnsatzPlan(op, n) as ans, kernels.DeviceBuffer.upload(psi) as buf:
        ans.apply(theta, buf)
        return buf.download(np.complex128, 1 << n)


def commutator_bound(symp, coeff, t, r):
    """(t^2 / 2 r) sum_{j < k} ||[c_j P_j, c_k P_k]||: the first-order product formula's error; the norm is 2 |c_j c_k| for a pair that
    anticommutes and 0 otherwise."""
    n = symp.shape[1] // 2
    x, z = symp[:, :n].astype(int), symp[:, n:].astype(int)
    anti = (x @ z.T + z @ x.T) % 2 == 1
    c = np.abs(np.asarray(coeff, dtype=np.float64))
    return t * t / (2 * r) * float(np.sum(np.triu(anti, 1) * 2 * np.outer(c, c)))


def test_trotter_steps_converge_to_the_propagator_at_first_order():
    n, t = 6, 0.5
    symp, coeff = evo.hermitian_case(40, n)
    psi = sf.vector(13, n, 'gaussian')
    res = evolve(symp, coeff, psi, t)
    exact = dense_state(res.states[0])
    err = {}
    for r in (64, 128):
        err[r] = np.linalg.norm(device_trotter(symp, coeff, psi, t, r) - exact)
        bound = commutator_bound(symp, coeff, t, r)
        assert bound > 0 and err[r] <= bound + res.tails[0] + R, f'r = {r}: {err[r]:.3e} > {bound:.3e}'
    assert err[64] > 1e3 * (res.tails[0] + R), 'the case has no Trotter error to halve'
    assert err[128] < 0.6 * err[64]


# ---- 5. imaginary time -----------------------------------------------------------------------------------------------------------------------
def test_imaginary_time_against_the_normalised_expm_and_the_energy_never_rises():
    n, tau = 6, 5.0                                          # sum|c| = 4 at least half of which is width: half_width * tau about 20
    symp, coeff = evo.hermitian_case(52, n)
    H = PauliwordOp(symp, coeff)
    dense = ao.dense_operator(symp, coeff)
    psi = sf.vector(17, n, 'gaussian')
    res = evolve(symp, coeff, psi, tau, imaginary=True)
    assert 10 <= res.interval[1] * tau <= 20.000001
    want = expm(-tau * (dense - (res.interval[0] - res.interval[1]) * np.eye(1 << n))) @ psi
    assert res.norms[0] == pytest.approx(np.linalg.norm(want), abs=res.tails[0] + R)
    got = dense_state(res.states[0])
    assert np.linalg.norm(got - want / np.linalg.norm(want)) <= (res.tails[0] + R) / res.norms[0]
    assert abs(np.linalg.norm(got) - 1) <= 2.0 ** -50
    grid = evolve_state(H, psi, [0.0, 1.0, 2.5, 5.0, 5.0], imaginary=True, tol=TOL, observables=[H], return_states=False)
    energies = grid.expvals[:, 0]
    for i in range(1, len(energies)):
        allowance = (grid.tails[i] + R) / grid.norms[i]
        assert energies[i] <= energies[i - 1] + allowance * np.abs(coeff).sum(), f'step {i}: {energies[i - 1]!r} -> {energies[i]!r}'
    assert energies[-1] >= np.linalg.eigvalsh(dense)[0] - (grid.tails[-2] + R) / grid.norms[-2] * np.abs(coeff).sum()
    assert energies[3] < energies[0]


# ---- 6. the Lanczos interval -----------------------------------------------------------------------------------------------------------------
def _bh():
    with open(os.path.join(GOLDEN, 'BH_STO-3G_SINGLET_JW.json')) as f:
        d = json.load(f)
    return PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()})


def _ising(n=8):
    symp = np.zeros((2 * n - 1, 2 * n), dtype=bool)
    for q in range(n - 1):
        symp[q, [n + q, n + q + 1]] = True
    for q in range(n):
        symp[n - 1 + q, q] = True
    return PauliwordOp(symp, np.concatenate([-np.ones(n - 1), -0.7 * np.ones(n)]))


@pytest.mark.parametrize('make, t', [(_ising, 1.0), (_bh, 0.5)])
def test_lanczos_interval_contains_the_spectrum_and_costs_no_more(make, t):
    H = make()
    n = H.n_qubits
    dense = H.to_sparse_matrix.toarray()
    assert not np.any(dense.imag)
    ev = np.linalg.eigvalsh(np.ascontiguousarray(dense.real))
    centre, half_width = spectral_interval(H, None, 'lanczos')
    c1, h1 = spectral_interval(H, None, 'norm1')
    assert centre - half_width <= ev[0] and ev[-1] <= centre + half_width
    assert c1 - h1 <= centre - half_width and centre + half_width <= c1 + h1 and half_width < h1
    psi = sf.vector(21, n, 'gaussian')
    a = evolve_state(H, psi, [t], tol=TOL, spectral_bounds='lanczos')
    b = evolve_state(H, psi, [t], tol=TOL, spectral_bounds='norm1')
    assert a.interval == (centre, half_width) and b.interval == (c1, h1)
    assert a.orders[0] <= b.orders[0]
    assert np.linalg.norm(dense_state(a.states[0]) - dense_state(b.states[0])) <= 2 * (max(a.tails[0], b.tails[0]) + R)
    via_pair = evolve_state(H, psi, [t], tol=TOL, spectral_bounds=(centre, half_width))
    assert np.array_equal(bits(dense_state(via_pair.states[0])), bits(dense_state(a.states[0])))


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_stays_allocated():
    n = 4
    rng = np.random.default_rng(3)
    symp, coeff = family('y_terms', n, rng)
    c = gaussian(rng, 4)
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan, kernels.DeviceBuffer.upload(gaussian(rng, 1 << n)) as x, \
            kernels.DeviceBuffer(16 << n) as y:
        y.write(np.full(1 << n, 7.0 + 0j))
        before = kernels.counters(BALANCE)

        def refused(call):
            with pytest.raises(SymgpuError) as e:
                call()
            assert e.value.code == _lib.E_INVALID
            assert np.array_equal(kernels.counters(BALANCE), before)

        refused(lambda: plan.chebyshev(0.0, 1.0, c, x, x))                                   # psi == out
        refused(lambda: plan.chebyshev(0.0, 1.0, np.zeros(0, dtype=complex), x, y))          # K = -1
        for half_width in (0.0, -1.0, np.inf, np.nan):
            refused(lambda: plan.chebyshev(0.0, half_width, c, x, y))
        for centre in (np.nan, np.inf):
            refused(lambda: plan.chebyshev(centre, 1.0, c, x, y))
        refused(lambda: plan.chebyshev(0.0, 1.0, c, None, y))
        refused(lambda: plan.chebyshev(0.0, 1.0, c, x, None))
        form = ctypes.c_int(5)
        args = (0.0, 1.0, _lib.addr(np.ascontiguousarray(c)), 3, x.ptr, y.ptr, ctypes.addressof(form))
        refused(lambda: _lib.check(_lib.lib().symgpu_cheb_apply(None, *args)))
        refused(lambda: _lib.check(_lib.lib().symgpu_cheb_apply(plan.handle, 0.0, 1.0, None, 3, x.ptr, y.ptr, ctypes.addressof(form))))
        assert np.array_equal(y.download(np.complex128, 1 << n), np.full(1 << n, 7.0 + 0j)), 'a refused call wrote its output'
        assert plan.chebyshev(0.0, 1.0, c, x, y) == kernels.CHEB_DIRECT and np.array_equal(kernels.counters(BALANCE), before)


def test_evolve_state_refuses_bad_input():
    H = PauliwordOp.from_list(['XZ', 'ZI'], [0.5, -0.25])
    psi = np.array([1, 0, 0, 0], dtype=complex)
    assert isinstance(evolve_state(H, psi, 0.25), QuantumState)       # H keeps its device copy from here on, as every PauliwordOp does
    before = kernels.counters(BALANCE)
    with pytest.raises(ValueError):
        evolve_state(PauliwordOp.from_list(['XZ', 'ZI'], [0.5, 0.25j]), psi, 1.0)
    with pytest.raises(ValueError):
        evolve_state(H, psi, [0.5, 0.2])
    with pytest.raises(ValueError):
        evolve_state(H, psi, -0.1)
    with pytest.raises(ValueError):
        evolve_state(H, psi, [0.1, np.nan])
    with pytest.raises(ValueError):
        evolve_state(H, np.ones(8, dtype=complex), 1.0)
    with pytest.raises(ValueError):
        evolve_state(H, QuantumState([[0, 0, 1]]), 1.0)
    with pytest.raises(ValueError):
        evolve_state(H, psi, 1.0, observables=[PauliwordOp.from_list(['XZI'], [1])])
    with pytest.raises(ValueError):
        evolve_state(H, psi, 1.0, spectral_bounds='exact')
    with pytest.raises(TypeError):
        evolve_state(H.to_sparse_matrix, psi, 1.0)
    gc.collect()                                             # the refused operators, which the tracebacks above may have kept alive
    assert np.array_equal(kernels.counters(BALANCE), before), 'a refused evolve_state left a plan or a buffer behind'


# ---- 8. exponentiation.py --------------------------------------------------------------------------------------------------------------------
def test_exponentiate_single_pauli_term():
    theta = 0.83
    for string in ('Y', 'XZY', 'III'):
        P = PauliwordOp.from_list([string], [1])
        dense = ao.dense_operator(np.asarray(P.symp_matrix, dtype=bool), [1.0])
        got = exponentiate_single_Pop(P.multiply_by_constant(1j * theta)).to_sparse_matrix.toarray()
        assert np.abs(got - (np.cos(theta) * np.eye(dense.shape[0]) + 1j * np.sin(theta) * dense)).max() <= 4 * 2.0 ** -53
    with pytest.raises(AssertionError):
        exponentiate_single_Pop(PauliwordOp.from_list(['XZ', 'ZI'], [0.5, -0.25]))
    with pytest.raises(NotImplementedError):
        truncated_exponential(PauliwordOp.from_list(['XZ'], [0.5]))


def test_trotter_of_a_commuting_operator_is_its_exponential():
    op = PauliwordOp.from_list(['XXI', 'ZZI', 'YYI', 'IIZ', 'XXZ'], [0.4, -0.7, 0.2 + 0.3j, 1.1, -0.5j])
    dense = ao.dense_operator(np.asarray(op.symp_matrix, dtype=bool), np.asarray(op.coeff_vec))
    scale = np.exp(np.abs(np.asarray(op.coeff_vec)).sum())
    for trotnum in (1, 3):
        assert np.abs(trotter(op, trotnum).to_sparse_matrix.toarray() - expm(dense)).max() <= 1e-12 * scale


def test_operator_trotter_is_the_device_trotter_product():
    """trotter(-i H t, r) is F_0 F_1 ... F_{T-1} repeated r times, so applied to a state its LAST term acts first: the ansatz sequence in
    reverse term order is the same product."""
    n, t, r = 3, 0.6, 2
    symp, coeff = evo.hermitian_case(61, n)
    H = PauliwordOp(symp, coeff)
    psi = sf.vector(19, n, 'gaussian')
    got = trotter(H.multiply_by_constant(-1j * t), r).to_sparse_matrix @ psi
    want = device_trotter(symp, coeff, psi, t, r, reverse=True)
    assert np.abs(got - want).max() <= ao.bound(n, r * symp.shape[0], symp.shape[0], np.ones(1))
