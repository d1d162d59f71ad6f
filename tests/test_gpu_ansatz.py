"""GPU: rotations exp(i theta P) on a resident statevector, <psi|H|psi>, the adjoint-sweep gradient and the pool gradient (csrc/ansatz.hip,
kernels.AnsatzPlan / kernels.pool_gradient), and VQE_Driver / ADAPT_VQE on top of them, against the NumPy restatement of the contract
(tests/_ansatz_oracle.py): the prepared state bit for bit, energies and gradients within the a-priori bound R of the oracle's `bound`.
A slot owns two amplitudes and a workgroup 256 slots: n = 9 is exactly one workgroup, n = 10 two."""
import gc
import itertools
import json
import os

import numpy as np
import pytest

import _ansatz_oracle as ao
from symmer_amd import PauliwordOp, QuantumState, kernels, packing
from symmer_amd._lib import SymgpuError
from symmer_amd.evolution import VQE_Driver, ADAPT_VQE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def symp_of(strings):
    n = len(strings[0])
    out = np.zeros((len(strings), 2 * n), dtype=bool)
    for r, s in enumerate(strings):
        for q, ch in enumerate(s):
            out[r, q], out[r, n + q] = ch in 'XY', ch in 'ZY'
    return out


def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


def unit(v):
    return v / np.linalg.norm(v)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.float64).view(np.uint64)


def upload_rows(symp):
    """The rows of bool[K, 2n] as a device operator without coefficients; K = 0 is an operator of no rows."""
    if symp.shape[0] == 0:
        op = kernels.DeviceOp.alloc(1, 1, True)
        op.set_rows(0)
        return op
    return kernels.DeviceOp.upload(packing.pack_rows(symp))


def expected_form(symp, k_begin, k_end):
    """The forms the plan's segments give the range (tests/_ansatz_oracle.py plan_runs), or DIRECT alone when it is forced."""
    segs = [seg for seg in ao.plan_runs(symp)]
    if k_end <= k_begin:
        return 0
    if os.environ.get('SYMGPU_ANSATZ_FORM') == 'direct' or not any(seg[3] for seg in segs):
        return kernels.ANSATZ_DIRECT
    form = 0
    for k0, k1, _, tiled in segs:
        if max(k0, k_begin) < min(k1, k_end):
            form |= kernels.ANSATZ_TILED if tiled else kernels.ANSATZ_DIRECT
    return form


@pytest.fixture(params=['default', 'direct'])
def either_form(request, monkeypatch):
    """The test runs once as the library chooses and once with direct passes forced."""
    if request.param == 'direct':
        monkeypatch.setenv('SYMGPU_ANSATZ_FORM', 'direct')
    return request.param


def device_state(symp, theta, ref, k_begin=0, k_end=None, inverse=False):
    """(amplitudes, form) of the rotations on `ref` through the kernels layer; the form is the planned one; every handle freed."""
    n = symp.shape[1] // 2
    with upload_rows(symp) as op, kernels.AnsatzPlan(op, n) as plan, kernels.DeviceBuffer.upload(np.asarray(ref, dtype=np.complex128)) as psi:
        runs = sum(1 for seg in ao.plan_runs(symp) if seg[3])
        assert plan.info() == (n, symp.shape[0], runs, (32 if runs else 16) * symp.shape[0])
        form = plan.apply(theta, psi, k_begin, k_end, inverse)
        assert form == expected_form(symp, k_begin, symp.shape[0] if k_end is None else k_end)
        return psi.download(np.complex128, 1 << n), form


def device_energy_grad(h_symp, h_coeff, symp, theta, ref, want_psi=False, want_grad=True):
    n = symp.shape[1] // 2
    with upload_rows(symp) as op, kernels.AnsatzPlan(op, n) as plan, PauliwordOp(h_symp, h_coeff)._matvec_plan() as plan_h, \
            kernels.DeviceBuffer.upload(np.asarray(ref, dtype=np.complex128)) as ref_dev, kernels.DeviceBuffer(16 << n) as out:
        e, g = plan.energy_grad(plan_h, theta, ref_dev, psi_out=out if want_psi else None, want_grad=want_grad)
        assert np.array_equal(bits(ref_dev.download(np.complex128, 1 << n)), bits(ref)), 'the reference state was changed'
        return e, g, (out.download(np.complex128, 1 << n) if want_psi else None)


def device_pool_gradient(h_symp, h_coeff, pool, psi, want_energy=False):
    n = h_symp.shape[1] // 2
    with upload_rows(pool) as op, PauliwordOp(h_symp, h_coeff)._matvec_plan() as plan_h, \
            kernels.DeviceBuffer.upload(np.asarray(psi, dtype=np.complex128)) as psi_dev:
        return kernels.pool_gradient(plan_h, op, psi_dev, want_energy)


@pytest.fixture(scope='module', autouse=True)
def plans_and_buffers_are_balanced():
    """DEV_BLOCKS_LIVE is the same before and after the module's tests (after one warm-up call: the context keeps its sort state)."""
    rng = np.random.default_rng(0)
    h = symp_of(['XYZ', 'ZZI', 'IXX'])
    device_energy_grad(h, np.ones(3), symp_of(['XYI', 'IZY']), [0.1, 0.2], unit(gaussian(rng, 8)))
    device_pool_gradient(h, np.ones(3), symp_of(['XYI']), unit(gaussian(rng, 8)))
    device_pool_gradient(rng.random((300, 10)) < 0.4, np.ones(300), symp_of(['XYIZI']), unit(gaussian(rng, 32)))       # the sort of a longer operator
    warm = VQE_Driver(PauliwordOp(h, np.ones(3)), excitation_ops=PauliwordOp(symp_of(['XYI', 'IZY']), [1, 1]), ref_state=unit(gaussian(rng, 8)))
    warm.expectation_eval = 'observable_rotation'                                                                         # rotation and cleanup state
    warm.f([0.1, 0.2])
    del warm
    gc.collect()
    before = kernels.counters(('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN'))
    yield
    gc.collect()
    assert np.array_equal(kernels.counters(('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')), before)


class Molecule:
    def __init__(self, name):
        with open(os.path.join(GOLDEN, name)) as f:
            d = json.load(f)
        self.data = d['data']
        self.n = self.data['n_qubits']
        ham = d['hamiltonian']
        self.h_symp, self.h_coeff = symp_of(list(ham)), np.array([complex(*v).real for v in ham.values()])
        self.gens = symp_of(list(self.data['auxiliary_operators']['UCCSD_operator']))
        self.hf = np.zeros(1 << self.n, dtype=np.complex128)
        self.hf[int(''.join(map(str, self.data['hf_array'])), 2)] = 1.0
        self.energies = {k: v['energy'] for k, v in self.data['calculated_properties'].items()}
        self.R = ao.bound(self.n, self.gens.shape[0], self.h_symp.shape[0], self.h_coeff)

    def operators(self):
        """(H, the UCCSD generators, the Hartree-Fock state), new objects: nothing of the device outlives the test that asked."""
        return PauliwordOp(self.h_symp, self.h_coeff), PauliwordOp(self.gens, np.ones(len(self.gens))), QuantumState([self.data['hf_array']], [1.0])


@pytest.fixture(scope='module')
def bplus():
    m = Molecule('B+_STO-3G_SINGLET_JW.json')
    assert (m.n, m.gens.shape[0], m.h_symp.shape[0]) == (10, 96, 156)
    return m


@pytest.fixture(scope='module')
def bplus_dense(bplus):
    return ao.dense_operator(bplus.h_symp, bplus.h_coeff)


# ---- 1. the state, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3])
def test_every_string_of_small_registers(n, either_form):
    strings = [''.join(s) for s in itertools.product('IXYZ', repeat=n)][1:]
    symp = symp_of(strings)
    rng = np.random.default_rng(n)
    theta, ref = rng.uniform(-np.pi, np.pi, len(strings)), gaussian(rng, 1 << n)
    with upload_rows(symp) as op, kernels.AnsatzPlan(op, n) as plan, kernels.DeviceBuffer(16 << n) as psi:
        for k, s in enumerate(strings):
            psi.write(ref)
            assert plan.apply(theta, psi, k, k + 1) == expected_form(symp, k, k + 1)
            assert np.array_equal(bits(psi.download(np.complex128, 1 << n)), bits(ao.state(symp, theta, ref, k, k + 1))), s
    got, _ = device_state(symp, theta, ref)
    assert np.array_equal(bits(got), bits(ao.state(symp, theta, ref)))


def edge_strings(n):
    """X-part on qubit 0 only (partner 2^(n-1) away), on qubit n-1 only (neighbours), on every qubit; x = 0 with z != 0; the identity;
    0 .. 4 Y's; a repeated generator."""
    pad = lambda s: s + 'I' * (n - len(s))
    return ['X' + 'I' * (n - 1), 'Y' + 'Z' * (n - 1), 'I' * (n - 1) + 'X', 'Z' * (n - 1) + 'Y', 'X' * n, 'XY' * (n // 2) + 'X' * (n % 2),
            'Z' * n, pad('IZIIZ'), 'I' * n, pad('XZXI'), pad('IYXZ'), pad('YIYX'), pad('ZYYYX'), pad('YYXYY'), pad('XZXI')]


@pytest.mark.parametrize('n', [9, 10])
def test_edges_one_and_two_workgroups(n, either_form):
    strings = edge_strings(n)
    assert {s.count('Y') % 8 for s in strings} >= {0, 1, 2, 3, 4}
    symp = symp_of(strings)
    rng = np.random.default_rng(10 + n)
    theta, ref = rng.uniform(-np.pi, np.pi, len(strings)), gaussian(rng, 1 << n)
    for k, s in enumerate(strings):
        got, form = device_state(symp[k:k + 1], theta[k:k + 1], ref)
        assert np.array_equal(bits(got), bits(ao.state(symp[k:k + 1], theta[k:k + 1], ref))), s
    got, _ = device_state(symp, theta, ref)
    assert np.array_equal(bits(got), bits(ao.state(symp, theta, ref)))
    got, _ = device_state(symp, np.zeros(len(strings)), ref)
    assert np.array_equal(bits(got), bits(ref)), 'theta = 0 changed the state'


def test_random_sequence_and_its_inverse(either_form):
    n, K = 10, 30
    rng = np.random.default_rng(77)
    symp = rng.random((K, 2 * n)) < 0.4
    theta, ref = rng.uniform(-np.pi, np.pi, K), unit(gaussian(rng, 1 << n))
    fwd, _ = device_state(symp, theta, ref)
    want = ao.state(symp, theta, ref)
    assert np.array_equal(bits(fwd), bits(want))
    back, form = device_state(symp, theta, fwd, inverse=True)
    assert np.array_equal(bits(back), bits(ao.state(symp, theta, want, inverse=True)))
    part, _ = device_state(symp, theta, ref, 7, 19)
    assert np.array_equal(bits(part), bits(ao.state(symp, theta, ref, 7, 19)))
    none, form = device_state(symp, theta, ref, 5, 5)
    assert form == 0 and np.array_equal(bits(none), bits(ref))


# ---- 2. the two forms ------------------------------------------------------------------------------------------------------------------
def on_qubits(n, letters):
    """The string with the given {qubit: letter}, I elsewhere."""
    return ''.join(letters.get(q, 'I') for q in range(n))


def form_cases():
    """name -> (strings, tiled runs, forms) at n = 14 (index bit of qubit q: 13 - q; the 4 low tile bits are qubits 10 .. 13), one at n = 6."""
    n = 14
    shared = [on_qubits(n, {**dict(zip((0, 3, 5, 7), letters)), 9: 'Z', 12: 'Z'}) for letters in
              ('XXXY', 'XXYX', 'XYXX', 'YXXX', 'XYYY', 'YXYY', 'YYXY', 'YYYX')]                     # a double excitation: 8 strings on 4 positions
    wide = 'XY' * 7                                                                                 # 14 X/Y positions: no tile holds it
    return {
        'one_run': (shared, 1, kernels.ANSATZ_TILED),
        'cut_by_the_budget': ([on_qubits(n, {0: 'X', 1: 'Y', 2: 'X', 3: 'X'}), on_qubits(n, {4: 'Y', 5: 'X', 6: 'X', 7: 'Z', 8: 'Z'}),
                               on_qubits(n, {4: 'X', 5: 'X', 6: 'X', 7: 'Y'}), on_qubits(n, {8: 'X', 9: 'Y'}), on_qubits(n, {9: 'X', 0: 'Z'})], 2,
                              kernels.ANSATZ_TILED),
        'run_of_one': ([on_qubits(n, {2: 'X', 6: 'Y', 11: 'Z'})], 1, kernels.ANSATZ_TILED),
        'diagonal_inside': ([shared[0], on_qubits(n, {0: 'Z', 5: 'Z', 13: 'Z'}), 'I' * n, shared[5]], 1, kernels.ANSATZ_TILED),
        'first_and_last_qubit': ([on_qubits(n, {0: 'X', 13: 'Y'}), on_qubits(n, {0: 'Y', 13: 'X', 6: 'Z'}), on_qubits(n, {13: 'X'})], 1,
                                 kernels.ANSATZ_TILED),
        'too_wide_between_runs': (shared[:3] + [wide, on_qubits(n, {q: 'X' for q in range(10)})] + shared[3:6], 2,
                                  kernels.ANSATZ_TILED | kernels.ANSATZ_DIRECT),
        'whole_vector_one_tile': (['XYZIXY', 'ZZIIZZ', 'YYYYYY', 'IIXIII'], 1, kernels.ANSATZ_TILED),
    }


@pytest.mark.parametrize('name', ['one_run', 'cut_by_the_budget', 'run_of_one', 'diagonal_inside', 'first_and_last_qubit', 'too_wide_between_runs',
                                  'whole_vector_one_tile'])
def test_forms_agree_bit_for_bit(name, monkeypatch):
    strings, runs, forms = form_cases()[name]
    symp = symp_of(strings)
    n = symp.shape[1] // 2
    rng = np.random.default_rng(len(name))
    theta, ref = rng.uniform(-np.pi, np.pi, len(strings)), unit(gaussian(rng, 1 << n))
    with upload_rows(symp) as op, kernels.AnsatzPlan(op, n) as plan:
        assert plan.info()[:3] == (n, len(strings), runs)
    tiled, form = device_state(symp, theta, ref)
    assert form == forms
    back, _ = device_state(symp, theta, tiled, inverse=True)
    part, _ = device_state(symp, theta, ref, 1, len(strings))                                       # a range clips the first run
    e_tiled, _, psi_tiled = device_energy_grad(symp_of([strings[0], 'Z' * n]), np.array([0.5, -0.25]), symp, theta, ref, want_psi=True, want_grad=False)
    monkeypatch.setenv('SYMGPU_ANSATZ_FORM', 'direct')
    direct, form = device_state(symp, theta, ref)
    assert form == kernels.ANSATZ_DIRECT
    want = ao.state(symp, theta, ref)
    assert np.array_equal(bits(tiled), bits(direct)) and np.array_equal(bits(tiled), bits(want))
    assert np.array_equal(bits(back), bits(device_state(symp, theta, direct, inverse=True)[0]))
    assert np.array_equal(bits(back), bits(ao.state(symp, theta, want, inverse=True)))
    assert np.array_equal(bits(part), bits(ao.state(symp, theta, ref, 1, len(strings))))
    e_direct, _, psi_direct = device_energy_grad(symp_of([strings[0], 'Z' * n]), np.array([0.5, -0.25]), symp, theta, ref, want_psi=True, want_grad=False)
    assert e_tiled == e_direct and np.array_equal(bits(psi_tiled), bits(psi_direct)) and np.array_equal(bits(psi_tiled), bits(want))


# ---- 3. energy and gradient ------------------------------------------------------------------------------------------------------------
def check_energy_grad(h_symp, h_coeff, symp, theta, ref):
    n, K = symp.shape[1] // 2, symp.shape[0]
    R = ao.bound(n, K, h_symp.shape[0], h_coeff)
    e, g, psi = device_energy_grad(h_symp, h_coeff, symp, theta, ref, want_psi=True)
    e_o, g_o = ao.energy_at(h_symp, h_coeff, symp, theta, ref), ao.grad_shift(h_symp, h_coeff, symp, theta, ref)
    print(f'n={n} K={K}: |E - E_o| = {abs(e - e_o):.3e}, max|g - g_o| = {np.abs(g - g_o).max() if K else 0.0:.3e}, R = {R:.3e}')
    assert abs(e - e_o) <= R
    assert g.shape == (K,) and (K == 0 or np.abs(g - g_o).max() <= 2 * R)
    assert np.array_equal(bits(psi), bits(ao.state(symp, theta, ref))), 'psi_out is not the state of apply'
    e2, g2, _ = device_energy_grad(h_symp, h_coeff, symp, theta, ref)
    assert np.array_equal(np.float64(e).view(np.uint64), np.float64(e2).view(np.uint64)) and np.array_equal(g.view(np.uint64), g2.view(np.uint64))
    e3, g3, _ = device_energy_grad(h_symp, h_coeff, symp, theta, ref, want_grad=False)
    assert g3 is None and e3 == e
    return e, g


def test_energy_and_gradient_of_the_molecule(bplus):
    rng = np.random.default_rng(5)
    theta = rng.uniform(-np.pi, np.pi, 96)
    check_energy_grad(bplus.h_symp, bplus.h_coeff, bplus.gens, theta, bplus.hf)


def test_energy_and_gradient_small_cases():
    rng = np.random.default_rng(6)
    h_symp, h_coeff = rng.random((12, 6)) < 0.5, rng.standard_normal(12)
    ref = unit(gaussian(rng, 8))
    gens = symp_of(['XYZ', 'ZZI', 'YIY', 'XYZ', 'IIX'])
    check_energy_grad(h_symp, h_coeff, gens, rng.uniform(-np.pi, np.pi, 5), ref)
    check_energy_grad(h_symp, h_coeff, gens[:1], [0.4], ref)                                        # K = 1
    e, g = check_energy_grad(h_symp, h_coeff, gens[:0], [], ref)                                    # K = 0
    assert g.shape == (0,) and abs(e - ao.energy(h_symp, h_coeff, ref)) <= ao.bound(3, 0, 12, h_coeff)
    check_energy_grad(np.zeros((0, 6), dtype=bool), np.zeros(0), gens, rng.uniform(-1, 1, 5), ref)  # H = 0


def test_driver_gradient_against_its_partial_derivatives():
    rng = np.random.default_rng(8)
    n, K = 6, 8
    h_symp, h_coeff = rng.random((20, 2 * n)) < 0.4, rng.standard_normal(20)
    gens = rng.random((K, 2 * n)) < 0.5
    gens[:, 0] = True                                                                               # no identity row
    vqe = VQE_Driver(PauliwordOp(h_symp, h_coeff), excitation_ops=PauliwordOp(gens, np.ones(K)), ref_state=unit(gaussian(rng, 1 << n)))
    x = rng.uniform(-np.pi, np.pi, K)
    g = vqe.gradient(x)
    R = ao.bound(n, K, 20, h_coeff)
    assert g.shape == (K,) and isinstance(vqe.f(x), float)
    for i in range(K):
        assert abs(g[i] - vqe.partial_derivative(x, i)) <= 2 * R


def test_driver_statevector_against_observable_rotation():
    """The second route rotates H itself: every rotation scales the 1-norm of its coefficients by at most |cos| + |sin| <= sqrt 2, so its
    error is bounded by R of the rotated operator's term count times 2^(K/2)."""
    rng = np.random.default_rng(9)
    n, K = 4, 5
    h_symp, h_coeff = rng.random((10, 2 * n)) < 0.5, rng.standard_normal(10)
    gens = symp_of(['XYII', 'IXYZ', 'YZXI', 'XYII', 'ZIIY'])                                        # they do not commute: the order counts
    ref = QuantumState(rng.integers(0, 2, (6, n)), gaussian(rng, 6)).cleanup().normalize
    vqe = VQE_Driver(PauliwordOp(h_symp, h_coeff), excitation_ops=PauliwordOp(gens, np.ones(K)), ref_state=ref)
    x = rng.uniform(-np.pi, np.pi, K)
    direct = vqe.f(x)
    assert abs(direct - ao.energy_at(h_symp, h_coeff, gens, x, ref.to_dense_matrix.reshape(-1))) <= ao.bound(n, K, 10, h_coeff)
    vqe.expectation_eval = 'observable_rotation'
    rotated = vqe.f(x)
    assert isinstance(rotated, float) and abs(direct - rotated) <= ao.bound(n, K, 4 ** n, h_coeff) * 2 ** (K / 2)
    g = vqe.gradient(x)
    vqe.expectation_eval = 'statevector'
    assert np.abs(g - vqe.gradient(x)).max() <= 4 * ao.bound(n, K, 4 ** n, h_coeff) * 2 ** (K / 2)


def test_driver_states_and_no_parameters():
    rng = np.random.default_rng(12)
    n = 4
    h_symp, h_coeff = rng.random((10, 2 * n)) < 0.5, rng.standard_normal(10)
    ref = unit(gaussian(rng, 1 << n))
    gens = symp_of(['XYII', 'IIII', 'YZXI', 'XYII'])                                                # the identity row is dropped
    vqe = VQE_Driver(PauliwordOp(h_symp, h_coeff), excitation_ops=PauliwordOp(gens, [2, 3, 4, 5]), ref_state=ref)
    assert vqe.excitation_generators.n_terms == 3 and np.array_equal(vqe.excitation_generators.symp_matrix, gens[[0, 2, 3]])
    x = rng.uniform(-1, 1, 3)
    want = ao.state(gens[[0, 2, 3]], x, ref)
    assert np.array_equal(bits(vqe.get_state(vqe.excitation_generators, x, as_array=True)), bits(want))
    state = vqe.get_state(vqe.excitation_generators, x)
    assert isinstance(state, QuantumState) and np.array_equal(state.to_dense_matrix.reshape(-1), want)
    other = PauliwordOp(symp_of(['IIII', 'ZZXY']), [1, 1])                                          # any generators; the identity: a phase
    assert np.array_equal(bits(vqe.get_state(other, [0.3, -0.2], as_array=True)), bits(ao.state(other.symp_matrix, [0.3, -0.2], ref)))
    none = VQE_Driver(PauliwordOp(h_symp, h_coeff), excitation_ops=PauliwordOp.empty(n), ref_state=ref)
    assert abs(none.f([]) - ao.energy(h_symp, h_coeff, ref)) <= ao.bound(n, 0, 10, h_coeff) and none.gradient([]).shape == (0,)


# ---- 4. the pool gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['hartree_fock', 'prepared'])
def test_pool_gradient_of_the_molecule(bplus, bplus_dense, which):
    rng = np.random.default_rng(13)
    psi = bplus.hf if which == 'hartree_fock' else ao.state(bplus.gens[:5], rng.uniform(-1, 1, 5), bplus.hf)
    got, e = device_pool_gradient(bplus.h_symp, bplus.h_coeff, bplus.gens, psi, want_energy=True)
    want = ao.pool_grad(bplus_dense, bplus.gens, psi)
    print(f'pool ({which}): max|g - g_o| = {np.abs(got - want).max():.3e}, R = {bplus.R:.3e}')
    assert got.shape == (96,) and np.abs(got - want).max() <= 2 * bplus.R
    assert abs(e - ao.energy(bplus.h_symp, bplus.h_coeff, psi)) <= bplus.R
    again = device_pool_gradient(bplus.h_symp, bplus.h_coeff, bplus.gens, psi)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    if which == 'hartree_fock':
        assert abs(np.abs(got).max() - 0.2255428783) <= 2 * bplus.R


def test_pool_gradient_small_pools(bplus):
    assert device_pool_gradient(bplus.h_symp, bplus.h_coeff, bplus.gens[:0], bplus.hf).shape == (0,)
    one = device_pool_gradient(bplus.h_symp, bplus.h_coeff, bplus.gens[7:8], bplus.hf)
    assert one.shape == (1,) and one[0] == device_pool_gradient(bplus.h_symp, bplus.h_coeff, bplus.gens, bplus.hf)[7]
    # a diagonal pool element on a state of real amplitudes: <psi| i [H, P] |psi> is the expectation of an imaginary-antisymmetric matrix
    rng = np.random.default_rng(14)
    real_state = unit(rng.standard_normal(1 << bplus.n)).astype(np.complex128)
    diag = symp_of(['IZIIZIIIII', 'ZZZZZZZZZZ', 'IIIIIIIIII'])
    assert np.abs(device_pool_gradient(bplus.h_symp, bplus.h_coeff, diag, real_state)).max() <= bplus.R


# ---- 5. VQE end to end -----------------------------------------------------------------------------------------------------------------
def test_vqe_reaches_the_uccsd_energy(bplus):
    H, gens, hf = bplus.operators()
    vqe = VQE_Driver(H, excitation_ops=gens, ref_state=hf)
    vqe.verbose = False
    assert abs(vqe.f(np.zeros(96)) - bplus.energies['HF']) <= 1e-6
    out, history = vqe.run(x0=np.zeros(96), method='BFGS', options={'gtol': 1e-6})
    print(f"VQE: E = {out['fun']:.10f} after nit = {out['nit']}, nfev = {out['nfev']}")
    assert out['success']
    assert bplus.energies['FCI'] - bplus.R <= out['fun'] <= bplus.energies['CCSD']
    assert set(history) == {'params', 'energy', 'gradient'} and set(out) == {'message', 'success', 'status', 'fun', 'x', 'jac', 'nit', 'nfev', 'njev'}
    assert sorted(history['energy']) == list(range(out['nfev'])) and sorted(history['params']) == list(range(out['nfev']))
    assert 1 <= len(history['gradient']) <= out['njev'] and set(history['gradient']) <= set(history['energy'])
    assert all(len(g) == 96 for g in history['gradient'].values())
    assert history['energy'][0] == vqe.f(np.zeros(96)) and len(out['x']) == 96 and isinstance(out['x'], tuple)


# ---- 6. ADAPT end to end ---------------------------------------------------------------------------------------------------------------
def test_adapt_grows_the_ansatz(bplus):
    H, pool, hf = bplus.operators()
    adapt = ADAPT_VQE(H, excitation_pool=pool, ref_state=hf)
    adapt.verbose = False
    for name in ('param_shift', 'commutators'):
        adapt.derivative_eval = name
        assert abs(adapt.pool_score().max() - 0.2255428783) <= 2 * bplus.R
    out = adapt.optimize(max_cycles=4, gtol=1e-3)
    data = out['interim_data']
    assert abs(data[1]['gmax'] - 0.2255428783) <= 2 * bplus.R
    history = data['history']
    print('ADAPT energies:', history)
    assert len(history) == 4 and all(b < a for a, b in zip(history, history[1:])) and history[-1] < bplus.energies['MP2']
    pool_strings = set(bplus.data['auxiliary_operators']['UCCSD_operator'])
    assert len(out['adapt_operator']) == 4 and set(out['adapt_operator']) <= pool_strings
    assert out['result'] is data[4]['output'] and out['ref_state'] == {''.join(map(str, bplus.data['hf_array'])): (1.0, 0.0)}
    assert set(out) == {'result', 'interim_data', 'ref_state', 'adapt_operator'}


def test_adapt_tetris_adds_disjoint_strings(bplus):
    H, pool, hf = bplus.operators()
    adapt = ADAPT_VQE(H, excitation_pool=pool, ref_state=hf)
    adapt.verbose, adapt.TETRIS = False, True
    out = adapt.optimize(max_cycles=1, gtol=1e-3)
    picked = out['interim_data'][1]['excitation']
    assert len(picked) >= 1 and picked == out['adapt_operator']
    support = np.array([[ch != 'I' for ch in s] for s in picked])
    assert support.sum(axis=0).max() == 1, 'two selected strings share a qubit'


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_usable():
    rng = np.random.default_rng(15)
    n = 3
    gens, ref = symp_of(['XYZ', 'ZIX']), unit(gaussian(rng, 8))
    h_symp, h_coeff = symp_of(['ZZI', 'XIX']), np.array([0.5, -1.5])

    def good():
        got, _ = device_state(gens, [0.3, 0.4], ref)
        assert np.array_equal(bits(got), bits(ao.state(gens, [0.3, 0.4], ref)))
        e, g, _ = device_energy_grad(h_symp, h_coeff, gens, [0.3, 0.4], ref)
        assert abs(e - ao.energy_at(h_symp, h_coeff, gens, [0.3, 0.4], ref)) <= ao.bound(n, 2, 2, h_coeff)

    import ctypes
    from symmer_amd import _lib
    lib = _lib.lib()
    with upload_rows(gens) as op:
        for bad_n in (0, 33):
            with pytest.raises(ValueError):
                kernels.AnsatzPlan(op, bad_n)
            handle = ctypes.c_void_p()
            assert lib.symgpu_ansatz_plan(op.handle, bad_n, ctypes.byref(handle)) == _lib.E_INVALID and not handle.value
            good()
    wide = np.zeros((2, 2 * 70), dtype=bool)
    wide[:, 3] = True
    with kernels.DeviceOp.upload(packing.pack_rows(wide)) as op:
        with pytest.raises(SymgpuError):
            kernels.AnsatzPlan(op, 32)
        good()
        with PauliwordOp(h_symp, h_coeff)._matvec_plan() as plan_h, kernels.DeviceBuffer.upload(ref) as psi:
            with pytest.raises(SymgpuError):
                kernels.pool_gradient(plan_h, op, psi)
        good()
    with upload_rows(gens) as op, kernels.AnsatzPlan(op, n) as plan, PauliwordOp(h_symp, h_coeff)._matvec_plan() as plan_h, \
            kernels.DeviceBuffer.upload(ref) as psi:
        cs = np.ones(2)
        e = ctypes.c_double(0)
        assert lib.symgpu_ansatz_apply(plan.handle, cs.ctypes.data, cs.ctypes.data, 0, 2, 0, None, None) == _lib.E_INVALID
        assert lib.symgpu_ansatz_apply(plan.handle, None, None, 0, 2, 0, psi.ptr, None) == _lib.E_INVALID
        assert lib.symgpu_ansatz_apply(plan.handle, cs.ctypes.data, cs.ctypes.data, 1, 3, 0, psi.ptr, None) == _lib.E_INVALID
        assert lib.symgpu_ansatz_energy_grad(plan.handle, plan_h.handle, cs.ctypes.data, cs.ctypes.data, None, None, ctypes.addressof(e), None) == _lib.E_INVALID
        assert lib.symgpu_ansatz_energy_grad(plan.handle, plan_h.handle, cs.ctypes.data, cs.ctypes.data, psi.ptr, None, None, None) == _lib.E_INVALID
        assert lib.symgpu_ansatz_energy_grad(plan.handle, None, cs.ctypes.data, cs.ctypes.data, psi.ptr, None, ctypes.addressof(e), None) == _lib.E_INVALID
        assert lib.symgpu_pool_gradient(plan_h.handle, op.handle, None, None, cs.ctypes.data) == _lib.E_INVALID
        assert lib.symgpu_pool_gradient(plan_h.handle, op.handle, psi.ptr, None, None) == _lib.E_INVALID
        assert np.array_equal(bits(psi.download(np.complex128, 8)), bits(ref)), 'a refused call changed the state'
        with pytest.raises(ValueError):
            plan.apply([0.1], psi)                                                                   # one angle for two generators
        with PauliwordOp(symp_of(['ZZIZ']), [1.0])._matvec_plan() as plan_4:                         # another qubit count
            with pytest.raises(SymgpuError):
                plan.energy_grad(plan_4, [0.1, 0.2], psi)
    good()


def test_driver_refusals():
    rng = np.random.default_rng(16)
    H = PauliwordOp(symp_of(['ZZI', 'XIX']), [0.5, -1.5])
    gens, ref = PauliwordOp(symp_of(['XYZ']), [1]), unit(gaussian(rng, 8))
    with pytest.raises(NotImplementedError):
        VQE_Driver(H, ansatz_circuit=object(), ref_state=ref)
    with pytest.raises(AssertionError):
        VQE_Driver(PauliwordOp(symp_of(['ZZI', 'XIX']), [0.5, 1j]), excitation_ops=gens, ref_state=ref)
    vqe = VQE_Driver(H, excitation_ops=gens, ref_state=ref)
    for name in ('symbolic_direct', 'symbolic_projector', 'sparse_array', 'dense_array'):
        vqe.expectation_eval = name
        with pytest.raises(NotImplementedError, match='observable_rotation'):
            vqe.f([0.1])
    vqe.expectation_eval = 'nonsense'
    with pytest.raises(ValueError):
        vqe.gradient([0.1])
    vqe.expectation_eval = 'statevector'
    assert abs(vqe.f([0.1]) - ao.energy_at(H.symp_matrix, H.coeff_vec.real, gens.symp_matrix, [0.1], ref)) <= ao.bound(3, 1, 2, [0.5, 1.5])
    adapt = ADAPT_VQE(H, excitation_pool=gens, ref_state=ref)
    adapt.topology_aware = True
    with pytest.raises(NotImplementedError):
        adapt.pool_score()
    adapt.topology_aware, adapt.derivative_eval = False, 'nonsense'
    with pytest.raises(ValueError):
        adapt.pool_gradient()
    adapt.derivative_eval = 'commutators'
    assert adapt.pool_score().shape == (1,)
