"""GPU: the dense-statevector kernels (csrc/matvec.hip, lanczos.hip, evolve.hip, ansatz.hip, rdm.hip, basis.hip, sample.hip) at 27 and 28
qubits, held to EXACT answers.

What happens only here: a vector of 2 GiB (27 qubits) is the first that leaves the allocator's arena for a device allocation of its own,
and every scratch vector follows it; byte counts reach 2^31 at 27 qubits and 2^32 at 28; grids reach 2^19 .. 2^20 workgroups and the
two-level reductions their largest chunks; the sampling tree gets its 7th level (completely full at 28 qubits); partner indices carry
the top index bit.

The vectors are the product states of tests/_large_vectors.py, whose every property has a closed form that tests/test_large_vectors.py
proves against the project's oracles on the CPU.  All data are dyadic and within the exactness budget asserted there, so every comparison
is == — except the basis change (1 / sqrt 2: its stated bound) and evolve_state (the truncation bound of tests/test_gpu_evolve.py).
Whole vectors never come back: results are read in the windows of `lv.windows`, and whole-vector coverage comes from device reductions
with exact expected values and from device-against-device differences of norm 0.

Sizes: 27 qubits for everything, 28 for upload/download, matvec, Chebyshev (orders 0 .. 3), the basis change and sampling.  Every test
checks `mem_info` for the bytes it needs (counted from the library's own allocations) and skips with the figure when they are not there."""
import ctypes
import gc
import math
import time

import numpy as np
import pytest

import _large_vectors as lv
from test_evolve_oracle import R, TOL
from symmer_amd import PauliwordOp, kernels, packing, _lib
from symmer_amd.evolution import evolve_state

pytestmark = pytest.mark.gpu

BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')
SEED_A, SEED_B = lv.SEEDS
STAR = [27, 28]
MiB, GiB = 1 << 20, 1 << 30
UPLOAD_SECONDS = {}


def vec(n):
    return 16 << n


def need(nbytes, what):
    free = kernels.mem_info()[0]
    if free < nbytes:
        pytest.skip(f'{what}: {nbytes / GiB:.2f} GiB needed, {free / GiB:.2f} GiB free on the device')


def upload_operator(symp, coeff=None):
    rows = packing.pack_rows(np.asarray(symp, dtype=bool))
    return kernels.DeviceOp.upload(rows) if coeff is None else kernels.DeviceOp.upload(rows, np.asarray(coeff, dtype=complex))


def identity_plan(n):
    with upload_operator(lv.rows_of(n, [{}]), [1.0]) as op:
        return kernels.MatvecPlan(op, n)


def expectation(plan, buf):
    """Re <v| O |v> of the plan's operator on the vector as it is: alpha of a Lanczos step on a basis of one slot (scratch: one vector)."""
    return plan.lanczos_step(None, buf, 1, 0)[0]


class Slot:
    """Vector j of a DeviceBuffer that holds several: the `ptr` the kernels layer passes on, and `download` at the slot's offset."""

    def __init__(self, buf, j, n):
        self.buf, self.base, self.nbytes = buf, j * vec(n), vec(n)
        self.ptr = ctypes.c_void_p(buf.ptr.value + self.base)

    def download(self, dtype, count, offset_bytes=0):
        return self.buf.download(dtype, count, self.base + offset_bytes)


def read_windows(buf, n, dtype=np.complex128):
    size = np.dtype(dtype).itemsize
    return np.concatenate([buf.download(dtype, count, first * size) for first, count in lv.windows(n)])


def copy_of(psi, n):
    out = kernels.DeviceBuffer(vec(n))
    kernels.vec_combine(psi, 1, n, [1.0], out=out)
    return out


@pytest.fixture(scope='module', autouse=True)
def plans_and_buffers_are_balanced():
    """DEV_BLOCKS_LIVE is the same before and after the module (after one warm-up of evolve_state, whose operators keep device copies
    until collected); the resident vectors are freed by their own fixture, which is torn down before this one."""
    H = PauliwordOp.from_list(['ZI', 'IZ'], [0.5, -0.25])
    evolve_state(H, np.array([1, 0, 0, 0]), [0.5], observables=[H], return_states=False)
    evolve_state(H, np.array([1, 0, 0, 0]), [0.5], imaginary=True, return_states=False)
    del H
    gc.collect()
    before = kernels.counters(BALANCE)
    yield
    gc.collect()
    assert np.array_equal(kernels.counters(BALANCE), before)
    print('\nupload seconds per (n, seed):', {k: round(v, 2) for k, v in UPLOAD_SECONDS.items()})


@pytest.fixture(scope='module')
def resident():
    """get(n, seed): psi on the device, uploaded once per (n, seed), read-only for every test, freed when the module ends."""
    cache = {}

    def get(n, seed):
        if (n, seed) not in cache:
            need(vec(n), f'psi of {n} qubits')
            t0 = time.perf_counter()
            cache[(n, seed)] = lv.upload(n, seed)
            kernels.sync()
            UPLOAD_SECONDS[(n, seed)] = time.perf_counter() - t0
        return cache[(n, seed)]
    yield get
    for buf in cache.values():
        buf.free()


# ---- upload and download ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', STAR)
def test_upload_and_download_at_large_offsets(n, resident):
    need(2 * vec(n), 'psi and one more vector')
    psi = resident(n, SEED_A)
    assert np.array_equal(read_windows(psi, n), lv.amplitudes(n, SEED_A, lv.window_indices(n)))
    rng = np.random.default_rng(n)
    with kernels.DeviceBuffer(vec(n)) as buf:
        assert buf.nbytes == 1 << (n + 4) and buf.nbytes >= 1 << 31
        ends = [buf.nbytes] + ([(1 << 31) + 5 * 65536 + 48] if n == 28 else [])          # ending at byte 2^31 (27) / 2^32 (28); from above 2^31
        for end in ends:
            sent = rng.standard_normal(4096) + 1j * rng.standard_normal(4096)
            at = end - sent.nbytes
            assert n == 27 or at > 1 << 31
            _lib.check(_lib.lib().symgpu_dev_upload(ctypes.c_void_p(buf.ptr.value + at), _lib.addr(sent), sent.nbytes))
            assert np.array_equal(buf.download(np.complex128, 4096, at), sent)


# ---- matvec ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, seed', [(27, SEED_A), (27, SEED_B), (28, SEED_A)])
def test_matvec_windows_energy_and_norm(n, seed, resident):
    need(3 * vec(n), 'psi, H psi and the vector of a Lanczos step')
    psi = resident(n, seed)
    idx = lv.window_indices(n)
    symp, coeff = lv.matvec_operator(n)
    psi_at = lambda b: lv.amplitudes(n, seed, b)
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan, kernels.DeviceBuffer(vec(n)) as y:
        assert plan.apply(psi, y) == kernels.MATVEC_DIRECT
        assert np.array_equal(read_windows(y, n), lv.apply_terms(symp, coeff, psi_at)(idx))
        assert expectation(plan, psi) == lv.energy(symp, coeff, n, seed)
    symp, coeff = lv.aligned_operator(n, seed)                 # every term with an expectation that is not zero
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan:
        want = lv.energy(symp, coeff, n, seed)
        assert want != 0 and expectation(plan, psi) == want
    with identity_plan(n) as unit:
        assert expectation(unit, psi) == lv.norm2(n, seed)


def test_sector_mask_of_the_number_operator_at_27_qubits(resident):
    n = 27
    need((1 << n) + 64 * MiB, 'the mask')
    symp, coeff = lv.number_operator(n)
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan, kernels.DeviceBuffer(1 << n) as keep:
        assert plan.sector_mask(13, keep) == math.comb(27, 13) == 20_058_300
        idx = lv.window_indices(n)
        popcount = np.array([bin(int(b)).count('1') for b in idx])
        assert np.array_equal(read_windows(keep, n, np.uint8), (popcount == 13).astype(np.uint8))
        assert (popcount == 13).any()


# ---- Chebyshev -------------------------------------------------------------------------------------------------------------------------------
CHEB_C = np.array([0.5, -0.25j, 0.125, 0.25 + 0.125j, -0.125, 0.125j], dtype=np.complex128)
CENTRE, HALF_WIDTH = -0.125, 4.0


@pytest.mark.parametrize('n', STAR)
def test_chebyshev_orders_against_the_recurrence_on_index_functions(n, resident):
    """Orders 0 (its own launch), 1, 2 (T_{k-2} is psi), 3 (both in-place roles of the two scratch vectors), and 5 at 27 qubits."""
    need(5 * vec(n) + vec(n), 'psi, two outputs, two scratch vectors of cheb_apply, the vector of a Lanczos step')
    seed = SEED_A
    psi = resident(n, seed)
    idx = lv.window_indices(n)
    symp, coeff = lv.matvec_operator(n)
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan, identity_plan(n) as unit, kernels.DeviceBuffer(2 * vec(n)) as pair:
        out, again = Slot(pair, 0, n), Slot(pair, 1, n)
        orders = [0, 1, 2, 3] + ([5] if n == 27 else [])
        want = lv.cheb_window(symp, coeff, CENTRE, HALF_WIDTH, CHEB_C[:orders[-1] + 1], n, seed, idx, every_order=True)
        for K in orders:
            c = CHEB_C[:K + 1]
            assert plan.chebyshev(CENTRE, HALF_WIDTH, c, psi, out) == kernels.CHEB_DIRECT
            got = read_windows(out, n)
            assert np.array_equal(got, want[K]), f'K = {K}'
            if K == orders[-1]:                                # the repeat at the highest order only: every call allocates two vectors
                plan.chebyshev(CENTRE, HALF_WIDTH, c, psi, again)
                assert np.array_equal(read_windows(again, n), got), f'K = {K}: two calls differ'
        # T_1 of the unscaled operator IS the matvec, over the whole vector: the difference has norm 0
        plan.chebyshev(0.0, 1.0, [0, 1], psi, out)
        plan.apply(psi, again)
        assert np.array_equal(read_windows(out, n), lv.apply_terms(symp, coeff, lambda b: lv.amplitudes(n, seed, b))(idx))
        kernels.vec_combine(pair, 2, n, [1.0, -1.0], out=out)
        assert expectation(unit, out) == 0.0
        # psi is as it was
        assert np.array_equal(read_windows(psi, n), lv.amplitudes(n, seed, idx))
        assert expectation(unit, psi) == lv.norm2(n, seed)


# ---- evolve_state ------------------------------------------------------------------------------------------------------------------------------
def test_evolve_state_keeps_the_product_form_under_a_diagonal_field():
    """H = sum_q w_q Z_q: qubit q goes to (a_q e^{-i w_q t}, b_q e^{+i w_q t}), in imaginary time to (a_q e^{-w_q tau}, b_q e^{+w_q tau}), so
    <X_q>(t), <Z_q>(t) and the norms are products of single-qubit numbers.  The state is psi itself, NOT normalised (its amplitudes
    stay exact on the host): the bound 2 (sum tails + R) ||O|| of a unit state scales with |psi|^2, and the first imaginary-time norm
    with |psi|.  Only observables come back (return_states=False)."""
    n, seed = 27, SEED_A
    need(4 * vec(n) + vec(n), 'two state buffers, two scratch vectors of cheb_apply, the vector of a Lanczos step')
    w = (1.0 + np.arange(n) % 3) / 32.0
    H = PauliwordOp(lv.rows_of(n, [{q: 'Z'} for q in range(n)]), w)
    qubits = [0, n // 2, n - 1]
    obs = [PauliwordOp(lv.rows_of(n, [{q: p}]), [1.0]) for q in qubits for p in 'XZ']
    phi = lv.factor_values(n, seed)
    norms_q = (np.abs(phi) ** 2).sum(axis=1)
    s2 = lv.norm2(n, seed)
    host = np.concatenate([piece for _, piece in lv.pieces(n, seed)])
    times = [0.5, 1.5, 3.0]
    res = evolve_state(H, host, times, tol=TOL, observables=obs, return_states=False)
    assert res.states is None and min(res.orders) >= 1
    tails = np.cumsum(res.tails)
    for i, t in enumerate(times):
        bound = 2 * (tails[i] + R) * s2
        for j, q in enumerate(qubits):
            rest = s2 / norms_q[q]
            want_x = 2 * (phi[q, 0].conjugate() * phi[q, 1] * np.exp(2j * w[q] * t)).real * rest
            want_z = (abs(phi[q, 0]) ** 2 - abs(phi[q, 1]) ** 2) * rest
            assert abs(res.expvals[i, 2 * j] - want_x) <= bound, f'<X_{q}>({t}): {res.expvals[i, 2 * j]!r} against {want_x!r}'
            assert abs(res.expvals[i, 2 * j + 1] - want_z) <= bound, f'<Z_{q}>({t})'
    assert abs(res.expvals[2, 0] - res.expvals[0, 0]) > 1e3 * 2 * (tails[-1] + R) * s2, 'the case has no dynamics to get wrong'

    taus = [0.05, 0.1, 0.15]
    res = evolve_state(H, host, taus, imaginary=True, tol=TOL, return_states=False)
    del host
    e_low = res.interval[0] - res.interval[1]
    assert res.interval == pytest.approx((0.0, float(np.abs(w).sum())), rel=1e-14)

    def norm_at(tau):                                        # |exp(-tau (H - E_low)) psi|
        per_qubit = np.abs(phi[:, 0]) ** 2 * np.exp(-2 * tau * w) + np.abs(phi[:, 1]) ** 2 * np.exp(2 * tau * w)
        return float(np.sqrt(np.prod(per_qubit)) * np.exp(tau * e_low))
    tails = np.cumsum(res.tails)
    assert abs(res.norms[0] - norm_at(taus[0])) <= 2 * (tails[0] + R) * np.sqrt(s2)
    for i in (1, 2):                                          # from a unit state on; every norm is above 1/2, so the division costs at most 2
        want = norm_at(taus[i]) / norm_at(taus[i - 1])
        assert want > 0.5 and abs(res.norms[i] - want) <= 2 * (tails[i] + R), f'norms[{i}] = {res.norms[i]!r} against {want!r}'


# ---- ansatz ------------------------------------------------------------------------------------------------------------------------------------
def ansatz_apply_exact(plan, cos_t, sin_t, psi):
    """symgpu_ansatz_apply with the caller's (cos, sin) arrays, which the C ABI takes as they are."""
    cos_t, sin_t = np.ascontiguousarray(cos_t, dtype=np.float64), np.ascontiguousarray(sin_t, dtype=np.float64)
    form = ctypes.c_int(0)
    _lib.check(_lib.lib().symgpu_ansatz_apply(plan.handle, _lib.addr(cos_t), _lib.addr(sin_t), 0, cos_t.shape[0], 0, psi.ptr, ctypes.addressof(form)))
    return form.value


def test_ansatz_rotations_tiled_and_direct_at_27_qubits(resident, monkeypatch):
    n, seed = 27, SEED_A
    need(2 * vec(n), 'psi and its copy')
    psi = resident(n, seed)
    idx = lv.window_indices(n)
    symp, cos_t, sin_t = lv.ansatz_generators(n)
    x_count = symp[:, :n].sum(axis=1)
    assert x_count.max() >= 13 and symp[:, 0].any()
    want = lv.rotate_window(symp, cos_t, sin_t, n, seed, idx)
    with upload_operator(symp) as gens, kernels.AnsatzPlan(gens, n) as plan:
        monkeypatch.delenv('SYMGPU_ANSATZ_FORM', raising=False)
        with copy_of(psi, n) as work:
            form = ansatz_apply_exact(plan, cos_t, sin_t, work)
            print(f'\nansatz forms at n = {n}: {form} (runs: {plan.info()[2]})')
            assert form == kernels.ANSATZ_DIRECT | kernels.ANSATZ_TILED
            assert np.array_equal(read_windows(work, n), want)
        monkeypatch.setenv('SYMGPU_ANSATZ_FORM', 'direct')
        with copy_of(psi, n) as work:
            ansatz_apply_exact(plan, cos_t, sin_t, work)
            assert np.array_equal(read_windows(work, n), want)
        monkeypatch.delenv('SYMGPU_ANSATZ_FORM')


def test_energy_gradient_and_pool_gradient_at_27_qubits(resident):
    """At x = 0 the prepared state is psi: E = <psi|H|psi> and dE/dx_k = <psi| i [H, P_k] |psi>, sums of products of single-qubit numbers
    (H Hermitian: the kernels form -2 Im <H psi, P_k psi>)."""
    n, seed = 27, SEED_A
    need(4 * vec(n), 'psi, the two vectors of energy_grad and H psi')
    psi = resident(n, seed)
    symp, coeff = lv.hermitian_operator(n, seed)
    gens = lv.ansatz_generators(n)[0]
    pool = lv.pool_strings(n)
    want_e = lv.energy(symp, coeff, n, seed)
    with upload_operator(symp, coeff) as op, kernels.MatvecPlan(op, n) as plan_h:
        with upload_operator(gens) as g, kernels.AnsatzPlan(g, n) as ans:
            energy, grad = ans.energy_grad(plan_h, np.zeros(gens.shape[0]), psi)
        want_g = np.array([lv.commutator_expectation(symp, coeff, row, n, seed) for row in gens])
        assert energy == want_e and np.array_equal(grad, want_g)
        with upload_operator(pool) as p:
            grad, energy = kernels.pool_gradient(plan_h, p, psi, want_energy=True)
        want_p = np.array([lv.commutator_expectation(symp, coeff, row, n, seed) for row in pool])
        assert energy == want_e and np.array_equal(grad, want_p)
        assert np.count_nonzero(want_g) >= 2 and np.count_nonzero(want_p) >= 3, 'the gradients of the case are mostly zero'


# ---- RDM ---------------------------------------------------------------------------------------------------------------------------------------
def test_reduced_density_matrices_at_27_qubits(resident, monkeypatch):
    n, seed = 27, SEED_A
    need(vec(n) + 256 * MiB, 'psi and the chunk sums')
    psi = resident(n, seed)
    seen = []
    for kept in ([0], [n - 1], [0, 13, n - 1]):
        for force, form in ((None, kernels.RDM_STREAM), ('tiled', kernels.RDM_TILED)):
            if force is None:
                monkeypatch.delenv('SYMGPU_RDM_FORM', raising=False)
            else:
                monkeypatch.setenv('SYMGPU_RDM_FORM', force)
            rho, info = kernels.rdm_dev(psi, n, kept, want_info=True)
            seen.append((kept, int(info[0]), int(info[2])))
            assert info[0] == form and info[2] > 1, f'kept = {kept}: form {info[0]}, {info[2]} chunks'
            assert np.array_equal(rho, lv.rdm_exact(n, seed, kept)), f'kept = {kept}, form {form}'
    monkeypatch.delenv('SYMGPU_RDM_FORM')
    kept = [0, 2, 13, 14, n - 2, n - 1]
    rho, info = kernels.rdm_dev(psi, n, kept, want_info=True)
    seen.append((kept, int(info[0]), int(info[2])))
    assert info[0] == kernels.RDM_TILED and info[2] > 1
    assert np.array_equal(rho, lv.rdm_exact(n, seed, kept))
    print(f'\nrdm (kept, form, chunks) at n = {n}: {seen}')


# ---- basis change ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', STAR)
def test_basis_change_keeps_the_product_form(n, resident, monkeypatch):
    need(3 * vec(n) + vec(n), 'psi, two copies, the vector of a Lanczos step')
    seed = SEED_A
    psi = resident(n, seed)
    xq, yq = [0, 5, n - 1], [1, n - 2]
    idx = lv.window_indices(n)
    want, bound = lv.basis_window(n, seed, xq, yq, idx)
    monkeypatch.delenv('SYMGPU_BASIS_FORM', raising=False)
    with copy_of(psi, n) as tiled, identity_plan(n) as unit:
        form = kernels.basis_change_dev(tiled, n, xq, yq)
        assert form == kernels.BASIS_TILED
        got = read_windows(tiled, n)
        worst = max(np.max(np.abs(got.real - want.real) - bound), np.max(np.abs(got.imag - want.imag) - bound))
        print(f'\nbasis change at n = {n}: form {form}, largest deviation less its bound {float(worst):.3e}')
        assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound)
        norm = expectation(unit, tiled)
        s2 = lv.norm2(n, seed)
        print(f'basis change at n = {n}: |psi\'|^2 / |psi|^2 - 1 = {norm / s2 - 1:.3e}')
        assert abs(norm - s2) <= 2 * 5 * 2 * 2.0 ** -52 * s2                 # a squared amplitude: twice the relative bound of an amplitude
        monkeypatch.setenv('SYMGPU_BASIS_FORM', 'direct')
        with copy_of(psi, n) as direct:
            assert kernels.basis_change_dev(direct, n, xq, yq) == kernels.BASIS_DIRECT
            assert np.array_equal(read_windows(direct, n), got)
    monkeypatch.delenv('SYMGPU_BASIS_FORM')


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', STAR)
def test_sampling_tree_walk_and_counting_forms(n, resident, monkeypatch):
    seed = SEED_B                                             # the assignment with cumulative boundaries at dyadic uniforms
    m = 1 << n
    need(vec(n) + m // 15 * 8 + 8 * m + 64 * MiB, 'psi, the tree, the two counter arrays of the histogram form')
    psi = resident(n, seed)
    S = 4096
    u = lv.sampling_uniforms(n, seed, S)
    assert u[0] == 0 and u[1] == 1 - 2.0 ** -20 and lv.boundary_uniforms(n, seed).shape[0] >= 16
    want = lv.index_of_uniform(n, seed, u)
    assert want[0] == 0 and want[1] == want.max() and want[1] > m - (m >> 12)
    want_idx, want_count = np.unique(want, return_counts=True)
    z_rows = lv.rows_of(n, [{0: 'Z'}, {1: 'Z', n // 2: 'Z', n - 1: 'Z'}, {q: 'Z' for q in range(n)}])
    with kernels.SamplePlan(psi) as plan, upload_operator(z_rows) as zop:
        assert plan.total == lv.norm2(n, seed)
        assert plan.info()[0] == m and plan.info()[1] == 7
        results = {}
        for name, form in (('hist', kernels.SAMPLE_HIST), ('sort', kernels.SAMPLE_SORT)):
            monkeypatch.setenv('SYMGPU_SAMPLE_COUNT', name)
            idx, count, order = plan.draw(S, u=u, want_order=True)
            assert plan.info()[4] == form
            assert np.array_equal(order, want), name
            results[name] = (idx, count)
        monkeypatch.delenv('SYMGPU_SAMPLE_COUNT')
        assert results['hist'][0].tobytes() == results['sort'][0].tobytes() and results['hist'][1].tobytes() == results['sort'][1].tobytes()
        idx, count = results['sort']
        assert np.array_equal(idx, want_idx) and np.array_equal(count, want_count)
        masks = [sum(1 << (n - 1 - q) for q in range(n) if row[n + q]) for row in z_rows]
        host = [int(sum(int(c) * (-1 if bin(mask & int(b)).count('1') & 1 else 1) for b, c in zip(idx, count))) for mask in masks]
        assert kernels.counts_signed_sums(zop, n, idx, count).tolist() == host
        # the library's own stream, far along it
        first = 1 << 40
        _, _, order = plan.draw(S, seed=7, first_draw=first, want_order=True)
        print(f'\nsampling at n = {n}: depth {plan.info()[1]}, counting form of the free choice {plan.info()[4]}')
        assert np.array_equal(order, lv.index_of_uniform(n, seed, kernels.philox_uniforms(7, first, S)))
