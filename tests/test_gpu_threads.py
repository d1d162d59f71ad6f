"""GPU: calls from several host threads on one device.  ctypes releases the GIL, so threads that use the drop-in classes on one GPU run
inside the library at the same time; every call holds its device's context lock (DeviceScope, csrc/context.hip) for its whole duration.
Each worker runs every hot path on operators of its own, in its own shuffled order, and checks every result against the C oracle or the
NumPy restatement, exactly as the single-thread tests of the same path do.  All expected results are computed on the main thread before
any worker starts.  Every task has a shape of its own, and the shapes differ by worker, so two calls never read back equal counts by
accident.  The library records where a call USES a context's state, whichever lock the call took: the counter CTX_MAX_THREADS (most
threads seen using one context at once) must stay 1 and CTX_UNLOCKED_USES (uses of a context by a call that does not hold its lock) must
stay 0, and CTX_WAITS (calls that waited for a busy context) must grow, which shows that the calls did overlap."""
import ctypes
import threading

import numpy as np
import pytest

import _sparse_oracle as so
from symmer_amd import PauliwordOp, IndependentOp, QuantumState, kernels, packing, _lib
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
from oracle import oracle_c as oc
from _golden import assert_op_equal

pytestmark = pytest.mark.gpu
TOL = 1e-12
JOIN_TIMEOUT_S = 300
ITERATIONS = 6                 # passes of every worker over all tasks: the whole file takes about 10 s on an MI355X


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 16.0


def assert_serialised():
    assert kernels.counter('CTX_UNLOCKED_USES') == 0, f'{kernels.counter("CTX_UNLOCKED_USES")} uses of a context by calls that did not hold its lock'
    assert kernels.counter('CTX_MAX_THREADS') == 1, f'{kernels.counter("CTX_MAX_THREADS")} threads used one context at once'


def run_workers(works, timeout=JOIN_TIMEOUT_S):
    """Runs works[w]() on thread w, all started together.  A worker that has not ended after `timeout` seconds fails the test as a
    deadlock or hang; otherwise the first failure of any worker is raised, naming the worker."""
    n = len(works)
    failures = [[] for _ in range(n)]
    start = threading.Barrier(n)

    def body(w):
        try:
            start.wait(timeout=60)
            works[w]()
        except BaseException as e:          # noqa: BLE001 (reported below, on the main thread)
            failures[w].append(e)

    threads = [threading.Thread(target=body, args=(w,), daemon=True, name=f'symgpu-worker-{w}') for w in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    alive = [w for w, t in enumerate(threads) if t.is_alive()]
    assert not alive, f'deadlock or hang: workers {alive} still running after {timeout} s'
    failed = [(w, f) for w in range(n) for f in failures[w]]
    if failed:
        w, first = failed[0]
        raise AssertionError(f'{len(failed)} worker(s) failed; first: worker {w}: {first!r}') from first


# ---- the tasks: make_X(rng, w) computes the expected result on the calling (main) thread and returns the check to run on a worker ----
def make_product(rng, w):
    n, NA, NB = 100, 400 + 3 * w, 300 + 5 * w
    sa, ca = rng.random((NA, 2 * n)) < 0.3, dyadic(rng, NA)
    sb, cb = rng.random((NB, 2 * n)) < 0.3, dyadic(rng, NB)
    er, ec = oc.mul(packing.pack_rows(sa), ca, packing.pack_rows(sb), cb)

    def run():
        R = PauliwordOp(sa, ca) * PauliwordOp(sb, cb)
        assert np.array_equal(R.packed, er) and np.array_equal(R.coeff_vec, ec), 'P * Q differs from the oracle'
    return run


def make_square(rng, w):
    n, T = 70, 500 + 7 * w
    pool = rng.random((6, 2 * n)) < 0.3
    symp, c = pool[rng.integers(0, 6, T)], dyadic(rng, T)
    p = packing.pack_rows(symp)
    er, ec = oc.mul(p, c, p, c)

    def run():
        P = PauliwordOp(symp, c)
        R = P * P
        assert np.array_equal(R.packed, er) and np.array_equal(R.coeff_vec, ec), 'P * P differs from the oracle'
    return run


def make_cleanup(rng, w):
    n, T = 130, 60000 + 101 * w
    base = packing.pack_rows(rng.random((int(T * 0.4) + 1, 2 * n)) < 0.3)
    rows, coeff = base[rng.integers(0, base.shape[0], T)], dyadic(rng, T)
    er, ec = oc.cleanup(rows, coeff, 1e-15)

    def run():
        r, c = kernels.cleanup(rows, coeff, 1e-15)
        assert np.array_equal(r, er) and np.array_equal(c, ec), 'cleanup differs from the oracle'
    return run


def make_resident_rotation(rng, w):
    n, T = 1000, 20000 + 11 * w
    symp, c = onp.cleanup_op(rng.random((T, 2 * n)) < 0.3, dyadic(rng, T))
    q = rng.random(2 * n) < 0.3
    er, ec = onp.rotate_by_single_pword(symp, c, q, 0.37)

    def run():
        P = PauliwordOp(symp, c).cleanup()                  # a cleaned handle: known free of duplicates, so the one-launch kernel takes it
        R = P._rotate_by_single_Pword(PauliwordOp(q.reshape(1, -1), [1]), 0.37)
        assert_op_equal(R.symp_matrix, R.coeff_vec, er, ec, exact=False, tol=TOL)
    return run


def make_clifford_chain(rng, w):
    n, T = 130, 1500 + 13 * w
    symp, c = onp.cleanup_op(rng.random((T, 2 * n)) < 0.3, dyadic(rng, T))
    rots = [(rng.random(2 * n) < 0.4, float(rng.integers(-2, 6)) * np.pi / 2) for _ in range(30)]
    er, ec = onp.perform_rotations(symp, c, rots)

    def run():
        P = PauliwordOp(symp, c).cleanup()
        R = P.perform_rotations([(PauliwordOp(q.reshape(1, -1), [1]), a) for q, a in rots])
        assert_op_equal(R.symp_matrix, R.coeff_vec, er, ec, exact=True)
    return run


def make_commutation(rng, w):
    n, N, M = 200, 700 + 3 * w, 2600 + 17 * w
    sa, sb = rng.random((N, 2 * n)) < 0.3, rng.random((M, 2 * n)) < 0.3
    expect = oc.commutes(packing.pack_rows(sa), packing.pack_rows(sb))

    def run():
        A, B = PauliwordOp(sa, np.ones(N)), PauliwordOp(sb, np.ones(M))
        assert np.array_equal(A.commutes_termwise(B), expect), 'commutes_termwise differs from the oracle'
        assert np.array_equal(kernels.commutes_handles(A._device(rows_only=True), B._device(rows_only=True)), expect), \
            'commutes_handles differs from the oracle'
    return run


def make_gf2(rng, w):
    n, M, k = 64, 300 + 5 * w, 3 + w % 5
    symp = rng.random((M, 2 * n)) < 0.3
    symp[:, :k] = False                                     # planted: Z_0 .. Z_{k-1} commute with every term
    e_sym = onp.symmetry_generators_symp(symp)
    assert e_sym.shape[0] == k
    e_gen = onp.generators(symp)
    R, C = 300 + w, 2000 + 64 * w
    mat = packing.pack_bits(rng.random((R, C)) < 0.5)
    e_red, e_xor, e_piv = oc.rref(mat, want_pivots=True)

    def run():
        H = PauliwordOp(symp, np.ones(M))
        S = IndependentOp.symmetry_generators(H, commuting_override=True)
        assert np.array_equal(S.symp_matrix, e_sym), 'symmetry generators differ from the oracle'
        assert np.array_equal(H.generators.symp_matrix, e_gen), 'generators differ from the oracle'
        red, n_xor, piv = kernels.rref(mat, want_pivots=True)
        assert np.array_equal(red, e_red) and n_xor == e_xor and np.array_equal(piv, e_piv), 'rref differs from the oracle'
    return run


def make_sparse_matrix(rng, w):
    n, T = 10, 600 + 9 * w
    x_parts = rng.random((150, n)) < 0.3
    xs = x_parts[rng.integers(0, 150, T)]
    xs[: T // 3] = False
    symp, c = np.hstack([xs, rng.random((T, n)) < 0.4]), dyadic(rng, T)
    want = so.to_csr(symp, c)

    def run():
        A = PauliwordOp(symp, c).to_sparse_matrix
        assert np.array_equal(A.indptr, want[2]) and np.array_equal(A.indices, want[1]), 'sparse matrix structure differs from the oracle'
        assert np.array_equal(A.data, want[0]), 'sparse matrix entries differ from the oracle'
    return run


def make_state_inner(rng, w):
    nq, Na, Nb = 70, 300 + 3 * w, 500 + 7 * w
    base = rng.integers(0, 2, (Na + Nb, nq))
    a_m = np.vstack([base[:Na], base[: Na // 3]]); b_m = np.vstack([base[Na // 2:], base[Na // 2: Na // 2 + 7]])
    a_c, b_c = dyadic(rng, a_m.shape[0]), dyadic(rng, b_m.shape[0])

    def summed(m, c):                                       # the cleaned state as {basis string: amplitude}
        d = {}
        for row, x in zip(m, c):
            key = row.tobytes()
            d[key] = d.get(key, 0) + x
        return d
    da, db = summed(a_m, a_c), summed(b_m, b_c)
    expect = sum((x * db[k] for k, x in da.items() if k in db), 0j)   # dyadic amplitudes: exact in any order

    def run():
        got = QuantumState(a_m, a_c, vec_type='bra') * QuantumState(b_m, b_c)
        assert got == expect, f'bra * ket = {got}, expected {expect}'
    return run


def make_handle_churn(rng, w):
    n, T = 90, 3000 + 29 * w
    rows, coeff = packing.pack_rows(rng.random((T, 2 * n)) < 0.3), dyadic(rng, T)
    const = (1 + 2 * (w % 3)) / 4 - 0.5j
    e_scaled = coeff * const

    def run():
        keep = []
        for _ in range(4):
            up = DeviceOp.upload(rows, coeff)
            cl = up.clone()
            cl.scale(const)
            r, c = cl.download()
            assert np.array_equal(r, rows) and np.array_equal(c, e_scaled), 'upload -> clone -> scale -> download'
            up.free()
            junk = {'op': cl}
            junk['self'] = junk                             # a reference cycle: the garbage collector frees it, on whichever thread runs it
            keep.append(junk)
        r, c = keep[-1]['op'].download()
        assert np.array_equal(c, e_scaled)
        keep.clear()
    return run


TASKS = {'product': make_product, 'square': make_square, 'cleanup': make_cleanup, 'resident_rotation': make_resident_rotation,
         'clifford_chain': make_clifford_chain, 'commutation': make_commutation, 'gf2': make_gf2, 'sparse_matrix': make_sparse_matrix,
         'state_inner': make_state_inner, 'handle_churn': make_handle_churn}


@pytest.mark.parametrize('n_workers', [4, 8])
def test_threads_share_one_device(n_workers):
    _lib.init()
    checks = []
    for w in range(n_workers):                               # expected results first, on this thread only
        rng = np.random.default_rng(9000 + 100 * n_workers + w)
        checks.append({name: make(rng, w) for name, make in TASKS.items()})
    waited, resident = kernels.counter('CTX_WAITS'), kernels.counter('RESIDENT_DONE')

    def work(w):
        order = np.random.default_rng(w)

        def go():
            for it in range(ITERATIONS):
                for name in order.permutation(sorted(TASKS)):
                    try:
                        checks[w][name]()
                    except Exception as e:
                        raise AssertionError(f'worker {w}, iteration {it}, task {name}: {e}') from e
        return go
    run_workers([work(w) for w in range(n_workers)])
    print(f'{n_workers} workers: CTX_MAX_THREADS = {kernels.counter("CTX_MAX_THREADS")}, CTX_UNLOCKED_USES = {kernels.counter("CTX_UNLOCKED_USES")}, '
          f'CTX_WAITS grew by {kernels.counter("CTX_WAITS") - waited}, one-launch rotations: {kernels.counter("RESIDENT_DONE") - resident}')
    assert_serialised()
    assert kernels.counter('CTX_WAITS') > waited, 'no call ever waited for another: the workers did not overlap'
    assert kernels.counter('RESIDENT_DONE') > resident, 'the one-launch rotation never ran'


def test_shared_read_only_operand():
    """One Hamiltonian multiplied, commuted against and used to rotate from every worker, each with a partner of its own: once resident
    before the threads start, once first touched by the workers together (PauliwordOp._device may then upload it twice)."""
    _lib.init()
    n, T, n_workers = 100, 900, 6
    rng = np.random.default_rng(4242)
    h_symp, h_c = onp.cleanup_op(rng.random((T, 2 * n)) < 0.3, dyadic(rng, T))
    h2_symp, h2_c = onp.cleanup_op(rng.random((T + 37, 2 * n)) < 0.3, dyadic(rng, T + 37))
    H, H2 = PauliwordOp(h_symp, h_c), PauliwordOp(h2_symp, h2_c)
    H._device()                                             # resident before the threads start; H2 is not
    assert H._dev is not None and H2._dev is None
    plans = []
    for w in range(n_workers):
        m = 150 + 13 * w
        ps, pc = rng.random((m, 2 * n)) < 0.3, dyadic(rng, m)
        q = rng.random(2 * n) < 0.3
        ang = 0.2 + 0.1 * w
        exp = {}
        for name, (hs, hc) in (('H', (h_symp, h_c)), ('H2', (h2_symp, h2_c))):
            exp[name] = (oc.mul(packing.pack_rows(hs), hc, packing.pack_rows(ps), pc),
                         oc.commutes(packing.pack_rows(hs), packing.pack_rows(ps)),
                         onp.rotate_by_single_pword(hs, hc, q, ang))
        plans.append((ps, pc, q, ang, exp))

    def work(w, op, name):
        ps, pc, q, ang, exp = plans[w]
        (er, ec), ecomm, (rr, rc) = exp[name]

        def go():
            for it in range(3):
                P = PauliwordOp(ps, pc)
                R = op * P
                assert np.array_equal(R.packed, er) and np.array_equal(R.coeff_vec, ec), f'worker {w}, iteration {it}: {name} * P'
                assert np.array_equal(op.commutes_termwise(P), ecomm), f'worker {w}, iteration {it}: {name}.commutes_termwise(P)'
                R = op._rotate_by_single_Pword(PauliwordOp(q.reshape(1, -1), [1]), ang)
                assert_op_equal(R.symp_matrix, R.coeff_vec, rr, rc, exact=False, tol=TOL)
        return go
    for op, name in ((H, 'H'), (H2, 'H2')):
        run_workers([work(w, op, name) for w in range(n_workers)])
    assert np.array_equal(H.packed, packing.pack_rows(h_symp)) and np.array_equal(H._c(), h_c), 'the shared operand changed'
    assert np.array_equal(H2.packed, packing.pack_rows(h2_symp)) and np.array_equal(H2._c(), h2_c), 'the shared operand changed'
    assert_serialised()


def test_threads_on_handles_of_another_device():
    """Threads whose current device is 0 work on handles of device 1 while other threads work on device 1 directly: a call runs on, and
    locks, its handles' device.  A guard that locked the thread's device instead would leave the device-0 threads using device 1's
    context without its lock: CTX_UNLOCKED_USES would count every such call, and CTX_MAX_THREADS would see two threads on device 1 at once."""
    if _lib.device_count() < 2:
        pytest.skip('needs two devices')
    rc = _lib.load().symgpu_init_all(2)
    _lib.check(rc)
    n, n_workers = 130, 6
    plans = []
    rng = np.random.default_rng(777)
    for w in range(n_workers):
        T = 5000 + 31 * w
        base = packing.pack_rows(rng.random((T // 2, 2 * n)) < 0.3)
        rows, coeff = base[rng.integers(0, base.shape[0], T)], dyadic(rng, T)
        plans.append((rows, coeff, oc.cleanup(rows, coeff, 1e-15)))
    waited = kernels.counter('CTX_WAITS')

    def work(w):
        rows, coeff, (er, ec) = plans[w]

        def go():
            _lib.set_device(1)
            op = DeviceOp.upload(rows, coeff)                    # a handle of device 1
            if w % 2 == 0:
                _lib.set_device(0)                               # half of the workers go on from device 0
            for it in range(4):
                out = ctypes.c_void_p()
                _lib.check(_lib.lib().symgpu_cleanup_dev(op.handle, 1e-15, 1, ctypes.byref(out)))
                r, c = DeviceOp(out).download()
                assert np.array_equal(r, er) and np.array_equal(c, ec), f'worker {w}, iteration {it}: cleanup on device 1'
                clone = op.clone()
                clone.free()
            op.free()
            _lib.set_device(0)
        return go
    try:
        run_workers([work(w) for w in range(n_workers)])
    finally:
        _lib.set_device(0)
    assert_serialised()
    assert kernels.counter('CTX_WAITS') > waited
