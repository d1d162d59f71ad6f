"""GPU: the dense-statevector features under concurrent host threads.  tests/test_gpu_threads.py pins the context lock (DeviceScope,
CTX_MAX_THREADS, CTX_UNLOCKED_USES, CTX_WAITS) with the operator calls; here the same lock is held to everything that came after them:
plans that live between calls and lock their own device (matvec, ansatz, sample), raw-buffer calls that lock the thread's current
device (rdm, basis_change, philox_uniform, vec_combine, sample_plan), plans and buffers freed from whichever thread collects them, and
the unlocked Python state on top (PauliwordOp._device, _matvec_plan, QuantumState.to_dense_matrix, _clique_members_device).

The bar.  Every feature is bit-reproducible by contract, so a concurrent call must return the BYTES of the serial call.  The builders of
tests/_thread_tasks.py make every call once on the main thread before any worker starts, hold it to the feature's own oracle as its
single-thread test does (equality for dyadic inputs, else the a-priori bound of the oracle module; no tolerance is defined here), and
keep the bytes.  No worker touches os.environ: the form switches are read with getenv on every call, and setting one from a thread would
race inside libc; the main thread removes them before the workers start, and forms are reached by shape alone
(tests/test_thread_tasks.py holds the shapes to the restated rules without a GPU).

Forms that run under threads here, and forms only an environment switch reaches at these sizes (not run here):
  expval       LDS (S <= 2048 rows at Wq = 1) and GLOBAL (S > 2048).                          SYMGPU_EXPVAL_FORM=global on a small state.
  matvec       DIRECT, the one form; exact_gs_energy with and without a sector mask, max_basis explicit (restarts included).
  ansatz       TILED runs, and DIRECT passes for a generator of 13 X/Y positions at n = 13.    SYMGPU_ANSATZ_FORM=direct (all passes direct).
  rdm          STREAM (k <= 3) and TILED (k >= 4).                                            SYMGPU_RDM_FORM=tiled at k <= 3.
  sample       HIST and SORT by the byte rule.                                                SYMGPU_SAMPLE_COUNT=hist|sort against the rule.
  basis        TILED with one tile group and with two (n = 13, every qubit measured).         SYMGPU_BASIS_FORM=direct.
  from_matrix  ONE_PASS.                 TWO_PASS: SYMGPU_PAULI_TILE_BITS, or more than 13 qubits (12 where the large-LDS attribute is refused).
  to_csr       is not a task here (tests/test_gpu_threads.py has it); SYMGPU_CSR_SCRATCH / SYMGPU_CSR_SCRATCH_MIB size its scratch.
  clique       UNIONS (QWC) and PAIRS (C, AC), one block of the order and two.
  noncon       one block of assignments (n_free below the library's L low bits; more blocks need n_free >= 10).

A refusal's text: SG_REQUIRE prefixes every message with 'invalid argument: ', so "starts with the name of the call" is held after that
prefix.  Times are printed by every test (run with -s)."""
import ctypes
import gc
import time

import numpy as np
import pytest

import _ansatz_oracle as ao
import _matvec_oracle as mo
import _sample_oracle as so
import _thread_tasks as tt
from symmer_amd import PauliwordOp, QuantumState, kernels, packing, _lib
from symmer_amd.kernels import DeviceBuffer, DeviceOp
from test_gpu_exact_gs import TOL as GS_TOL
from test_gpu_threads import run_workers, assert_serialised, dyadic

pytestmark = pytest.mark.gpu
ITERATIONS = 10                 # passes of every worker over all thirteen tasks: about 1 s for 8 workers on an MI355X, beside 1 s of oracles
FORM_SWITCHES = ('SYMGPU_EXPVAL_FORM', 'SYMGPU_ANSATZ_FORM', 'SYMGPU_RDM_FORM', 'SYMGPU_SAMPLE_COUNT', 'SYMGPU_BASIS_FORM', 'SYMGPU_CSR_SCRATCH',
                 'SYMGPU_CSR_SCRATCH_MIB', 'SYMGPU_PAULI_TILE_BITS')
BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')
SHARED_ITERATIONS, FIRST_TOUCH_ROUNDS, REFUSAL_ITERATIONS = 20, 5, 25       # each loop stays well below a second


@pytest.fixture(autouse=True)
def no_form_switches(monkeypatch):
    """The main thread removes the switches before any worker starts; no worker reads or writes os.environ."""
    for name in FORM_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    _lib.init()


def balance():
    gc.collect()
    return kernels.counters(BALANCE)


def upload_rows(symp, coeff=None):
    return DeviceOp.upload(packing.pack_rows(np.asarray(symp, dtype=bool)), coeff)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. every task from every worker ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_workers', [4, 8])
def test_threads_share_one_device_statevector(n_workers):
    assert tt.GS_TOL == GS_TOL
    t0 = time.perf_counter()
    checks = [{name: make(tt.worker_rng(n_workers, w, name), w) for name, make in tt.TASKS.items()} for w in range(n_workers)]
    t1 = time.perf_counter()
    for per_worker in checks:                                       # the single-thread warm-up of all tasks: the contexts' scratch has its size
        for name in sorted(tt.TASKS):
            per_worker[name]()
    before = balance()
    waited = kernels.counter('CTX_WAITS')
    seen = [set() for _ in range(n_workers)]
    t2 = time.perf_counter()

    def work(w):
        order = np.random.default_rng(w)

        def go():
            for it in range(ITERATIONS):
                for name in order.permutation(sorted(tt.TASKS)):
                    try:
                        seen[w] |= checks[w][name]()
                    except Exception as e:
                        raise AssertionError(f'worker {w}, iteration {it}, task {name}: {e}') from e
        return go
    run_workers([work(w) for w in range(n_workers)])
    t3 = time.perf_counter()
    print(f'{n_workers} workers x {ITERATIONS} passes x {len(tt.TASKS)} tasks: serial calls and oracles {t1 - t0:.2f} s, warm-up {t2 - t1:.2f} s, threads {t3 - t2:.2f} s; '
          f'CTX_MAX_THREADS = {kernels.counter("CTX_MAX_THREADS")}, CTX_UNLOCKED_USES = {kernels.counter("CTX_UNLOCKED_USES")}, '
          f'CTX_WAITS grew by {kernels.counter("CTX_WAITS") - waited}; forms {sorted(set().union(*seen))}')
    assert_serialised()
    assert kernels.counter('CTX_WAITS') > waited, 'no call ever waited for another: the workers did not overlap'
    assert set().union(*seen) == tt.REQUIRED_FORMS, f'forms never run under threads: {sorted(tt.REQUIRED_FORMS - set().union(*seen))}'
    assert np.array_equal(balance(), before), 'device blocks are not balanced after the threads'


# ---- 2. shared plans, one reference state --------------------------------------------------------------------------------------------
class Shared:
    """The data of test_shared_plans_and_reference, and its oracle answers per worker."""
    n, T, K, J, m, n_workers = 10, 60, 8, 12, 700, 6

    def __init__(self):
        rng = np.random.default_rng(5151)
        n = self.n
        self.h_symp, self.h_coeff = rng.random((self.T, 2 * n)) < 0.3, dyadic(rng, self.T).real * 4
        self.gens = tt.excitation_rows(rng, n, self.K)
        self.pool = rng.random((self.J, 2 * n)) < 0.4
        self.ref = tt.unit(tt.gaussian(rng, 1 << n))
        self.amp = so.dyadic_amplitudes(rng, self.m)
        self.x = [rng.uniform(-np.pi, np.pi, self.K) for _ in range(self.n_workers)]
        self.S = [400 + 37 * w for w in range(self.n_workers)]

    def objects(self):
        """New host objects of the same value, nothing on the device yet: (H, G, P, the reference as a QuantumState)."""
        return (PauliwordOp(self.h_symp, self.h_coeff), PauliwordOp(self.gens, np.ones(self.K)), PauliwordOp(self.pool, np.ones(self.J)),
                QuantumState.from_array(self.ref.reshape(-1, 1)))

    def check_against_oracles(self, w, got):
        hv, e, g, psi, pg, idx, count, order = got
        want_hv = mo.matvec(self.h_symp, self.h_coeff, self.ref)
        assert np.abs(hv - want_hv).max() <= mo.error_bound(self.h_symp, self.h_coeff, self.ref)
        R = ao.bound(self.n, self.K, self.T, self.h_coeff)
        state = ao.state(self.gens, self.x[w], self.ref)
        assert np.array_equal(bits(psi), bits(state)), 'psi_out is not the oracle state'
        assert abs(e - ao.energy(self.h_symp, self.h_coeff, state)) <= R
        assert np.abs(g - ao.grad_shift(self.h_symp, self.h_coeff, self.gens, self.x[w], self.ref)).max() <= 2 * R
        if w == 0:
            self.h_dense = ao.dense_operator(self.h_symp, self.h_coeff)
        assert np.abs(pg - ao.pool_grad(self.h_dense, self.pool, state)).max() <= 2 * ao.bound(self.n, self.J, self.T, self.h_coeff)
        want_order = so.tree_walk(so.tree_build(so.weights(self.amp)), so.philox_uniforms(w, w * self.S[w], self.S[w]))
        assert np.array_equal(order, want_order) and np.array_equal(idx, so.counts_of(want_order)[0]) and np.array_equal(count, so.counts_of(want_order)[1])


def shared_calls(d, w, plan_h, ansatz, ref, pool, sample):
    """The four calls of one worker on the shared objects, with buffers of its own: the bytes of everything they return."""
    side = 1 << d.n
    with DeviceBuffer(16 * side) as y, DeviceBuffer(16 * side) as own:
        plan_h.apply(ref, y)
        hv = y.download(np.complex128, side)
        e, g = ansatz.energy_grad(plan_h, d.x[w], ref, psi_out=own)
        psi = own.download(np.complex128, side)
        pg = kernels.pool_gradient(plan_h, pool, own)
    idx, count, order = sample.draw(d.S[w], seed=w, first_draw=w * d.S[w], want_order=True)
    return hv, e, g, psi, pg, idx, count, order


def as_bytes(got):
    return tuple(np.ascontiguousarray(a).tobytes() for a in got)


def test_shared_plans_and_reference():
    """Six workers on ONE MatvecPlan of H, one AnsatzPlan, one reference buffer, one pool operator and one SamplePlan over one amplitude
    buffer — a plan of H shared by every energy evaluation is the expected use.  Once with the plans built before the threads start;
    once with the host objects (H, G, P, the QuantumState) first touched by all workers together, every worker building its plans from
    them: _device() and to_dense_matrix may then run twice, and the blocks still balance.  No worker reads the shared sample plan's
    info()[4:6]: those are last-writer words."""
    d = Shared()
    side = 1 << d.n
    t0 = time.perf_counter()

    def build(H, G, P, state):
        return SimpleShared(H._matvec_plan(), kernels.AnsatzPlan(G._device(), d.n), DeviceBuffer.upload(np.asarray(state.to_dense_matrix).reshape(-1)),
                            P._device(), DeviceBuffer.upload(d.amp))

    class SimpleShared:
        def __init__(self, plan_h, ansatz, ref, pool, amp):
            self.plan_h, self.ansatz, self.ref, self.pool, self.amp = plan_h, ansatz, ref, pool, amp
            self.sample = kernels.SamplePlan(amp)

        def calls(self, w):
            return shared_calls(d, w, self.plan_h, self.ansatz, self.ref, self.pool, self.sample)

        def free(self):
            for thing in (self.sample, self.plan_h, self.ansatz, self.ref, self.amp):
                thing.free()

    # serial, on the main thread: the oracle checks and the bytes; it also warms the context before the blocks are counted
    host = d.objects()
    warm = build(*host)
    expected = []
    for w in range(d.n_workers):
        got = warm.calls(w)
        d.check_against_oracles(w, got)
        expected.append(as_bytes(got))
    warm.free()
    del warm, host
    before = balance()
    waited = kernels.counter('CTX_WAITS')
    t1 = time.perf_counter()

    # (a) the plans exist before the threads start
    host = d.objects()
    shared = build(*host)

    def work_shared(w):
        def go():
            for it in range(SHARED_ITERATIONS):
                assert as_bytes(shared.calls(w)) == expected[w], f'worker {w}, iteration {it}: shared plans gave other bytes than the serial calls'
        return go
    run_workers([work_shared(w) for w in range(d.n_workers)])
    assert shared.ref.download(np.complex128, side).tobytes() == d.ref.tobytes(), 'the shared reference state was written'
    assert shared.amp.download(np.complex128, d.m).tobytes() == d.amp.tobytes(), 'the shared amplitudes were written'
    shared.free()
    del shared, host
    t2 = time.perf_counter()

    # (b) nothing of the host objects is on the device, and the dense vector of the state is not cached, when the workers start;
    # a first touch happens once per object, so the round is repeated with new objects
    for round_ in range(FIRST_TOUCH_ROUNDS):
        H, G, P, state = d.objects()
        assert H._dev is None and G._dev is None and P._dev is None and 'to_dense_matrix' not in state.__dict__

        def work_first_touch(w):
            def go():
                mine = build(H, G, P, state)
                try:
                    for it in range(2):
                        assert as_bytes(mine.calls(w)) == expected[w], f'round {round_}, worker {w}, iteration {it}: plans of first-touched objects gave other bytes'
                finally:
                    mine.free()
            return go
        run_workers([work_first_touch(w) for w in range(d.n_workers)])
        assert H._dev is not None and G._dev is not None and P._dev is not None
        assert np.array_equal(H.packed, packing.pack_rows(d.h_symp)) and np.array_equal(H._c(), d.h_coeff), 'the shared operator changed'
        assert np.array_equal(np.asarray(state.to_dense_matrix).reshape(-1), d.ref)
        del H, G, P, state
    t3 = time.perf_counter()
    print(f'shared plans: serial calls and oracles {t1 - t0:.2f} s, shared plans {t2 - t1:.2f} s, first touch {t3 - t2:.2f} s; '
          f'CTX_WAITS grew by {kernels.counter("CTX_WAITS") - waited}')
    assert_serialised()
    assert kernels.counter('CTX_WAITS') > waited
    assert np.array_equal(balance(), before), 'device blocks are not balanced'


# ---- 3. the contract the threads rely on: a plan holds nothing of its operator -----------------------------------------------------------
def test_plans_outlive_their_operators():
    """Single thread.  A matvec and an ansatz plan are built from device operators; the operators are freed and their parked blocks are
    handed out again with other contents — or the operators are scaled and given other coefficients in place — and the plans return the
    bytes from before."""
    t0 = time.perf_counter()
    rng = np.random.default_rng(6161)
    n, T, K = 9, 80, 7
    side = 1 << n
    h_symp, h_coeff = rng.random((T, 2 * n)) < 0.3, dyadic(rng, T)
    h_rows, g_symp = packing.pack_rows(h_symp), tt.excitation_rows(rng, n, K)
    g_rows, theta, ref = packing.pack_rows(g_symp), rng.uniform(-np.pi, np.pi, K), tt.unit(tt.gaussian(rng, side))
    before = balance()

    def results(plan_h, ansatz):
        with DeviceBuffer.upload(ref) as x, DeviceBuffer(16 * side) as y, DeviceBuffer(16 * side) as out:
            form = plan_h.apply(x, y)
            e, g = ansatz.energy_grad(plan_h, theta, x, psi_out=out)
            return as_bytes((y.download(np.complex128, side), np.float64(e), g, out.download(np.complex128, side))) + (form, plan_h.info(), ansatz.info())

    def others():
        """Operators of the same byte sizes with other contents: the allocator hands the parked blocks out again."""
        return [DeviceOp.upload(packing.pack_rows(rng.random((T, 2 * n)) < 0.5), dyadic(rng, T)) for _ in range(3)] + \
               [DeviceOp.upload(packing.pack_rows(rng.random((K, 2 * n)) < 0.5), dyadic(rng, K)) for _ in range(3)]

    first = None
    for change in ('free', 'scale and set_coeff'):
        h_op, g_op = DeviceOp.upload(h_rows, h_coeff), DeviceOp.upload(g_rows, np.ones(K, dtype=complex))
        plan_h, ansatz = kernels.MatvecPlan(h_op, n), kernels.AnsatzPlan(g_op, n)
        at_first = results(plan_h, ansatz)
        if first is None:
            first = at_first
            hv = np.frombuffer(first[0], dtype=np.complex128)
            assert np.abs(hv - mo.matvec(h_symp, h_coeff, ref)).max() <= mo.error_bound(h_symp, h_coeff, ref)
            assert np.array_equal(bits(np.frombuffer(first[3], dtype=np.complex128)), bits(ao.state(g_symp, theta, ref)))
        assert at_first == first, 'a second plan of the same operator gives other bytes'
        if change == 'free':
            h_op.free()
            g_op.free()
        else:
            h_op.scale(3 - 2j)
            h_op.set_coeff(dyadic(rng, T))
            g_op.scale(-1j)
            g_op.set_coeff(dyadic(rng, K))
        reused = others()
        assert results(plan_h, ansatz) == first, f'after {change}: the plan read its source operator'
        for op in reused:
            op.free()
        assert results(plan_h, ansatz) == first
        if change != 'free':
            assert np.array_equal(h_op.download()[0], h_rows)
            h_op.free()
            g_op.free()
        plan_h.free()
        ansatz.free()
    print(f'plans outlive their operators: {time.perf_counter() - t0:.2f} s')
    assert np.array_equal(balance(), before)


# ---- 4. refusals are the caller's own ---------------------------------------------------------------------------------------------------
def test_each_thread_reads_its_own_refusal():
    """Workers alternate good calls with host-side refusals (argument checks: nothing is launched) of five entry points, each worker
    starting at another one, so different calls are refused at the same time.  The error text is thread-local: a worker reads the name
    of the call IT just made.  The good results stay byte-equal, and no block is lost on a refusal path."""
    t0 = time.perf_counter()
    L = _lib.lib()
    n_workers, n = 6, 8
    side = 1 << n
    rng = np.random.default_rng(7171)
    data = []
    for w in range(n_workers):
        T, K, m, S = 30 + w, 4, 150 + w, 200 + w
        data.append(dict(h_symp=rng.random((T, 2 * n)) < 0.3, h_coeff=dyadic(rng, T), gens=tt.excitation_rows(rng, n, K), theta=rng.uniform(-1, 1, K),
                         v=tt.dyadic_vector(rng, side), amp=so.dyadic_amplitudes(rng, m), S=S,
                         z=np.hstack([np.zeros((5 + w, n), dtype=bool), rng.random((5 + w, n)) < 0.5]), xs=[0, 3], ys=[1, n - 1]))

    class Own:
        """One worker's plans and buffers, and its five (good call, refused call) pairs."""

        def __init__(self, d):
            self.d = d
            with upload_rows(d['h_symp'], d['h_coeff']) as h, upload_rows(d['gens']) as g:
                self.plan_h, self.ansatz = kernels.MatvecPlan(h, n), kernels.AnsatzPlan(g, n)
            self.sample, self.zop = kernels.SamplePlan(d['amp']), upload_rows(d['z'])
            self.x, self.y, self.small_a, self.small_b = DeviceBuffer.upload(d['v']), DeviceBuffer(16 * side), DeviceBuffer(64), DeviceBuffer(64)
            self.idx, self.count = self.sample.draw(d['S'], seed=3)
            self.cos, self.sin = np.ascontiguousarray(np.cos(d['theta'])), np.ascontiguousarray(np.sin(d['theta']))

        def good(self, which):
            d = self.d
            if which == 'matvec_apply':
                self.plan_h.apply(self.x, self.y)
                return self.y.download(np.complex128, side).tobytes()
            with DeviceBuffer.upload(d['v']) as psi:
                if which == 'basis_change':
                    kernels.basis_change_dev(psi, n, d['xs'], d['ys'])
                elif which == 'ansatz_apply':
                    self.ansatz.apply(d['theta'], psi)
                elif which == 'sample_draw':
                    return as_bytes(self.sample.draw(d['S'], seed=3, want_order=True))
                else:
                    return kernels.counts_signed_sums(self.zop, n, self.idx, self.count).tobytes()
                return psi.download(np.complex128, side).tobytes()

        def refused(self, which):
            """The call's return code; nothing else enters the library between the refusal and the caller's look at the error text."""
            nd, out = ctypes.c_int64(7), np.zeros(self.d['z'].shape[0], dtype=np.int64)
            if which == 'matvec_apply':
                return L.symgpu_matvec_apply(self.plan_h.handle, self.x.ptr, self.x.ptr, None)                        # x is y
            if which == 'basis_change':
                return L.symgpu_basis_change(self.x.ptr, n, 0b0110, 0b0100, None)                                   # qubit 2 in both masks
            if which == 'sample_draw':
                return L.symgpu_sample_draw(self.sample.handle, -1, 0, 0, None, None, self.small_a.ptr, self.small_b.ptr, ctypes.addressof(nd))
            if which == 'counts_signed_sums':
                return L.symgpu_counts_signed_sums(self.zop.handle, 33, self.small_a.ptr, self.small_b.ptr, 1, _lib.addr(out))
            return L.symgpu_ansatz_apply(self.ansatz.handle, _lib.addr(self.cos), _lib.addr(self.sin), 3, 2, 0, self.x.ptr, None)      # k_begin > k_end

        def free(self):
            for thing in (self.plan_h, self.ansatz, self.sample, self.zop, self.x, self.y, self.small_a, self.small_b):
                thing.free()

    calls = ('matvec_apply', 'basis_change', 'sample_draw', 'counts_signed_sums', 'ansatz_apply')
    # serial: the good results against their oracles, the refusals once, the bytes kept; it also warms the context
    expected = []
    for w, d in enumerate(data):
        own = Own(d)
        good = {which: own.good(which) for which in calls}
        assert np.array_equal(bits(np.frombuffer(good['matvec_apply'], dtype=np.complex128)), bits(mo.matvec(d['h_symp'], d['h_coeff'], d['v'])))
        assert good['basis_change'] == so.basis_change(d['v'], n, d['xs'], d['ys']).tobytes()
        assert good['ansatz_apply'] == ao.state(d['gens'], d['theta'], d['v']).tobytes()
        order = so.tree_walk(so.tree_build(so.weights(d['amp'])), so.philox_uniforms(3, 0, d['S']))
        assert good['sample_draw'] == as_bytes(so.counts_of(order) + (order,))
        assert good['counts_signed_sums'] == so.signed_sums(d['z'][:, n:], n, *so.counts_of(order)).tobytes()
        for which in calls:
            assert own.refused(which) == _lib.E_INVALID and _lib.last_error().startswith(f'invalid argument: {which}:'), (which, _lib.last_error())
        assert np.array_equal(own.x.download(np.complex128, side), d['v']), 'a refused call wrote its buffer'
        expected.append(good)
        own.free()
    before = balance()
    t1 = time.perf_counter()

    def work(w):
        def go():
            own = Own(data[w])
            try:
                for it in range(REFUSAL_ITERATIONS):
                    for step in range(len(calls)):
                        which = calls[(step + w) % len(calls)]
                        assert own.good(which) == expected[w][which], f'worker {w}, iteration {it}: {which} gave other bytes than the serial call'
                        rc, text = own.refused(which), _lib.last_error()
                        assert rc == _lib.E_INVALID, f'worker {w}, iteration {it}: {which} returned {rc}'
                        assert text.startswith(f'invalid argument: {which}:'), f'worker {w}, iteration {it}: after a refused {which} the error reads {text!r}'
            finally:
                own.free()
        return go
    run_workers([work(w) for w in range(n_workers)])
    print(f'refusals: serial calls and oracles {t1 - t0:.2f} s, threads {time.perf_counter() - t1:.2f} s')
    assert_serialised()
    assert np.array_equal(balance(), before), 'a refusal path lost or double-freed a block'


# ---- 5. plans of another device --------------------------------------------------------------------------------------------------------
OTHER_DEVICE_WORKERS, OTHER_DEVICE_QUBITS = 6, 8


class SimpleData:
    def __init__(self, **fields):
        self.__dict__.update(fields)


def other_device_data():
    n, side = OTHER_DEVICE_QUBITS, 1 << OTHER_DEVICE_QUBITS
    rng = np.random.default_rng(8181)
    data = []
    for w in range(OTHER_DEVICE_WORKERS):
        T, K, J, m, S = 30 + w, 5, 4 + w, 200 + w, 300 + w
        data.append(SimpleData(h_symp=rng.random((T, 2 * n)) < 0.3, h_coeff=dyadic(rng, T).real, gens=tt.excitation_rows(rng, n, K),
                               theta=rng.uniform(-np.pi, np.pi, K), ref=tt.unit(tt.gaussian(rng, side)), pool=rng.random((J, 2 * n)) < 0.4,
                               amp=so.dyadic_amplitudes(rng, m), m=m, S=S, z=np.hstack([np.zeros((6, n), dtype=bool), rng.random((6, n)) < 0.5])))
    return data


def other_device_calls(d, build_on, hop_to):
    """Everything is built — and every raw-buffer call made — with `build_on` the thread's current device; the plan- and handle-taking
    calls follow with `hop_to` current; the buffers are read back and freed with `build_on` current again.  Returns what the calls
    returned, arrays as bytes."""
    n, side = OTHER_DEVICE_QUBITS, 1 << OTHER_DEVICE_QUBITS
    L = _lib.lib()
    _lib.set_device(build_on)
    h, g, pool, zop = upload_rows(d.h_symp, d.h_coeff.astype(complex)), upload_rows(d.gens), upload_rows(d.pool), upload_rows(d.z)
    plan_h, ansatz = kernels.MatvecPlan(h, n), kernels.AnsatzPlan(g, n)
    x, y, psi, out = DeviceBuffer.upload(d.ref), DeviceBuffer(16 * side), DeviceBuffer.upload(d.ref), DeviceBuffer(16 * side)
    basis = DeviceBuffer(4 * 16 * side)
    basis.write(d.ref)                                               # slot 0 of a Lanczos basis of four vectors
    amp = DeviceBuffer.upload(d.amp)
    sample = kernels.SamplePlan(amp)                                 # symgpu_sample_plan takes a raw buffer: made here, not after the hop
    order, idx, count = DeviceBuffer(8 * d.S), DeviceBuffer(8 * min(d.m, d.S)), DeviceBuffer(8 * min(d.m, d.S))
    _lib.set_device(hop_to)
    got = [plan_h.apply(x, y), plan_h.lanczos_step(None, basis, 4, 0), ansatz.apply(d.theta, psi)]
    e, grad = ansatz.energy_grad(plan_h, d.theta, x, psi_out=out)
    got += [np.float64(e), grad, kernels.pool_gradient(plan_h, pool, psi)]
    nd = ctypes.c_int64(0)
    _lib.check(L.symgpu_sample_draw(sample.handle, d.S, 11, 5, None, order.ptr, idx.ptr, count.ptr, ctypes.addressof(nd)))
    got += [nd.value, kernels.counts_signed_sums(zop, n, idx, count, nd.value)]
    got += [plan_h.info(), ansatz.info(), sample.info().tobytes(), sample.total, h.info(), zop.n_terms]
    for thing in (plan_h, ansatz, sample, h, g, pool, zop):          # *_free of plans and handles: on their own device
        thing.free()
    _lib.set_device(build_on)
    got += [b.download(np.complex128, side) for b in (y, psi, out)] + [basis.download(np.complex128, side, 16 * side),
            order.download(np.int64, d.S), idx.download(np.int64, nd.value), count.download(np.int64, nd.value)]
    for b in (x, y, psi, out, basis, amp, order, idx, count):
        b.free()
    return tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in got)


def check_other_device_oracles(d, got):
    n = OTHER_DEVICE_QUBITS
    hv, prepared = np.frombuffer(got[-7], dtype=np.complex128), np.frombuffer(got[-5], dtype=np.complex128)
    assert np.abs(hv - mo.matvec(d.h_symp, d.h_coeff, d.ref)).max() <= mo.error_bound(d.h_symp, d.h_coeff, d.ref)
    assert np.array_equal(bits(prepared), bits(ao.state(d.gens, d.theta, d.ref))), 'psi_out is not the oracle state'
    assert got[-6] == got[-5], 'apply and energy_grad prepared different states'
    R = ao.bound(n, len(d.theta), d.h_symp.shape[0], d.h_coeff)
    assert abs(got[3] - ao.energy(d.h_symp, d.h_coeff, prepared)) <= R
    assert np.abs(np.frombuffer(got[4]) - ao.grad_shift(d.h_symp, d.h_coeff, d.gens, d.theta, d.ref)).max() <= 2 * R
    want_order = so.tree_walk(so.tree_build(so.weights(d.amp)), so.philox_uniforms(11, 5, d.S))
    want_idx, want_count = so.counts_of(want_order)
    assert got[6] == len(want_idx) and (got[-3], got[-2], got[-1]) == (want_order.tobytes(), want_idx.tobytes(), want_count.tobytes())
    assert got[7] == so.signed_sums(d.z[:, n:], n, want_idx, want_count).tobytes()


def test_plans_of_another_device():
    """Workers build buffers, operators and plans on device 1; half of them then make device 0 their current device, and all call only
    entry points that take a plan or a handle, which by contract run on — and lock — the plan's or handle's device.  A guard that locked
    the thread's device instead would leave the device-0 threads inside device 1's context without its lock (CTX_UNLOCKED_USES,
    CTX_MAX_THREADS).  Raw-buffer calls (rdm, basis_change, philox_uniform, vec_combine, sample_plan, and the up- and downloads of a
    DeviceBuffer) lock the thread's CURRENT device: every one of them is made while that is device 1, never from device 0."""
    if _lib.device_count() < 2:
        pytest.skip('needs two devices')
    _lib.check(_lib.load().symgpu_init_all(2))
    data = other_device_data()
    try:
        expected = []
        for d in data:                                               # serial, all on device 0: the same hardware gives the same bytes
            expected.append(other_device_calls(d, 0, 0))
            check_other_device_oracles(d, expected[-1])
        other_device_calls(data[0], 1, 1)                            # device 1's context has its scratch before the blocks are counted
        before = balance()
        waited = kernels.counter('CTX_WAITS')

        def work(w):
            def go():
                try:
                    for it in range(3):
                        assert other_device_calls(data[w], 1, 0 if w % 2 == 0 else 1) == expected[w], f'worker {w}, iteration {it}: other bytes on device 1'
                finally:
                    _lib.set_device(0)
            return go
        run_workers([work(w) for w in range(OTHER_DEVICE_WORKERS)])
    finally:
        _lib.set_device(0)
    assert_serialised()
    assert kernels.counter('CTX_WAITS') > waited
    assert np.array_equal(balance(), before)
