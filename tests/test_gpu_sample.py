"""GPU: csrc/sample.hip — the Philox uniforms, the sampling plan (a radix-16 sum tree over the weights), the draws, the two counting
forms and the signed sums — and what stands on them: kernels.SamplePlan / philox_uniforms / counts_signed_sums,
QuantumState.sample_state / sample_counts.  Everything is compared for equality: uniforms with NumPy's own Philox, the sample of every
draw with the restatement of tests/_sample_oracle.py (held against exact inverse CDFs by tests/test_sample_oracle.py), counts with
np.unique, signed sums with Python integers."""
import ctypes
import os

import numpy as np
import pytest

import _sample_oracle as so
from symmer_amd import QuantumState, _lib, kernels, packing

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, (1 << 63) + 5)
OFFSETS = (0, 3, (1 << 40) + 1)
SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097, 65537, (1 << 20) + 3)          # the edges of every tree level
FAMILIES = ('gaussian', 'dyadic', 'zeros99', 'one_hot_first', 'one_hot_last', 'zero_blocks')
TOP = 1.0 - 2.0 ** -53


class counting:
    """``with counting('sort'):`` — SYMGPU_SAMPLE_COUNT for the calls inside; None leaves the choice to the library."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.before = os.environ.pop('SYMGPU_SAMPLE_COUNT', None)
        if self.form is not None:
            os.environ['SYMGPU_SAMPLE_COUNT'] = self.form

    def __exit__(self, *exc):
        os.environ.pop('SYMGPU_SAMPLE_COUNT', None)
        if self.before is not None:
            os.environ['SYMGPU_SAMPLE_COUNT'] = self.before
        return False


def amplitudes(family, m, rng):
    gauss = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    if family == 'gaussian':
        return gauss
    if family == 'dyadic':
        return so.dyadic_amplitudes(rng, m) if m >= 3 else (rng.integers(1, 9, m) + 1j * rng.integers(-8, 9, m)) / 8.0
    if family == 'zeros99':
        keep = rng.random(m) < 0.01
        keep[rng.integers(0, m)] = True
        return np.where(keep, gauss, 0)
    if family in ('one_hot_first', 'one_hot_last'):
        out = np.zeros(m, dtype=np.complex128)
        out[0 if family == 'one_hot_first' else m - 1] = 0.6 - 0.8j
        return out
    out = gauss.copy()                                               # a leading and a trailing block of zeros
    out[:m // 3] = 0
    out[m - m // 3:] = 0
    return out


@pytest.fixture(scope='module', autouse=True)
def blocks_are_balanced():
    """DEV_BLOCKS_LIVE is the same before and after the module's tests (after one warm-up of both counting forms: the context keeps
    its scan and sort state)."""
    for form in ('hist', 'sort'):
        with counting(form), kernels.SamplePlan(np.ones(300, dtype=np.complex128)) as plan:
            plan.draw(5000, 1)
    before = kernels.counters(('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN'))
    yield
    assert np.array_equal(kernels.counters(('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')), before)


# ---- uniforms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('first_draw', OFFSETS)
def test_uniforms_are_numpys(seed, first_draw):
    for count in (0, 1, 4099):
        got = kernels.philox_uniforms(seed, first_draw, count)
        assert got.shape == (count,) and np.array_equal(got.view(np.uint64), so.numpy_uniforms(seed, first_draw, count).view(np.uint64))


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('m', SIZES)
def test_every_draw_is_the_restatements(m, family):
    rng = np.random.default_rng(7 * m + FAMILIES.index(family))
    amp = np.ascontiguousarray(amplitudes(family, m, rng), dtype=np.complex128)
    w = so.weights(amp)
    levels = so.tree_build(w)
    u = [so.philox_uniforms(11, 0, 1500), [0.0, TOP]]
    if family == 'dyadic' and m >= 3:                                # exactly on boundaries: they belong to the upper interval
        total, prefix = levels[-1][0], np.cumsum(w)
        at = np.unique(np.concatenate([np.arange(min(m - 1, 40)), rng.integers(0, m - 1, 200), np.arange(max(0, m - 41), m - 1)]))
        on = prefix[at] / total
        assert np.array_equal(on * total, prefix[at])
        u.append(on)
        assert np.array_equal(so.tree_walk(levels, on), [np.flatnonzero(w[a + 1:] > 0)[0] + a + 1 for a in at])
    u = np.concatenate(u)
    with kernels.DeviceBuffer.upload(amp) as buf, kernels.SamplePlan(buf) as plan:
        assert plan.total == levels[-1][0] and plan.info()[0] == m and plan.info()[1] == len(levels) - 1
        assert plan.info()[2] == 8 * sum(lev.shape[0] for lev in levels[1:])
        idx, count, order = plan.draw(u.shape[0], u=u, want_order=True)
        want = so.tree_walk(levels, u)
        assert np.array_equal(order, want), np.flatnonzero(order != want)[:5]
        assert np.all(w[order] > 0), 'a sample of weight zero'
        want_idx, want_count = so.counts_of(want)
        assert np.array_equal(idx, want_idx) and np.array_equal(count, want_count)
        # the generator inside the sampler: the same uniforms, the same samples
        gen = plan.draw(1500, seed=11, first_draw=0, want_order=True)
        assert np.array_equal(gen[2], want[:1500])
        again = plan.draw(u.shape[0], u=u, want_order=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((idx, count, order), again)), 'a second call returns other bytes'
        assert buf.download(np.complex128, m).tobytes() == amp.tobytes(), 'the amplitudes were written'


@pytest.mark.parametrize('m', (17, 4097, 65537))
def test_both_counting_forms_give_the_same_bytes(m):
    rng = np.random.default_rng(m)
    amp = amplitudes('zero_blocks', m, rng)
    levels = so.tree_build(so.weights(amp))
    with kernels.SamplePlan(amp) as plan:
        for n_samples in (0, 1, 255, 4096, 100_003):
            want = so.counts_of(so.tree_walk(levels, so.philox_uniforms(3, 17, n_samples)))
            got = {}
            for form, code in (('hist', kernels.SAMPLE_HIST), ('sort', kernels.SAMPLE_SORT)):
                with counting(form):
                    got[form] = plan.draw(n_samples, seed=3, first_draw=17, want_order=True)
                assert plan.info()[4] == (code if n_samples else 0), (form, plan.info())
            for a, b in zip(got['hist'], got['sort']):
                assert a.dtype == np.int64 and a.tobytes() == b.tobytes()
            idx, count, order = got['hist']
            assert np.array_equal(idx, want[0]) and np.array_equal(count, want[1]) and int(count.sum()) == n_samples
            assert np.array_equal(np.unique(order, return_counts=True)[0], idx) and np.array_equal(np.unique(order, return_counts=True)[1], count)
            with counting(None):
                free = plan.draw(n_samples, seed=3, first_draw=17)
            assert np.array_equal(free[0], idx) and np.array_equal(free[1], count)


def test_stream_offsets_concatenate():
    amp = amplitudes('gaussian', 4097, np.random.default_rng(5))
    s1, s2 = 1003, 2501
    with kernels.SamplePlan(amp) as plan:
        whole = plan.draw(s1 + s2, seed=9, first_draw=0, want_order=True)[2]
        head, tail = plan.draw(s1, seed=9, first_draw=0, want_order=True)[2], plan.draw(s2, seed=9, first_draw=s1, want_order=True)[2]
        far = plan.draw(64, seed=9, first_draw=(1 << 40) + 1, want_order=True)[2]
    assert np.array_equal(whole, np.concatenate([head, tail]))
    assert np.array_equal(far, so.draw(amp, so.numpy_uniforms(9, (1 << 40) + 1, 64)))


# ---- refusals and state ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind():
    lib = _lib.lib()
    live = lambda: kernels.counters(('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN'))
    good = np.ones(40, dtype=np.complex128)
    with kernels.DeviceBuffer.upload(good) as buf, kernels.DeviceBuffer(8 * 64) as out, kernels.DeviceBuffer(8 * 64) as out2:
        before = live()
        handle, nd = ctypes.c_void_p(), ctypes.c_int64(7)
        assert lib.symgpu_sample_plan(None, 40, ctypes.byref(handle)) == _lib.E_INVALID and not handle.value
        assert lib.symgpu_sample_plan(buf.ptr, 40, None) == _lib.E_INVALID
        assert lib.symgpu_sample_plan(buf.ptr, 0, ctypes.byref(handle)) == _lib.E_INVALID and not handle.value
        assert lib.symgpu_sample_plan(buf.ptr, -3, ctypes.byref(handle)) == _lib.E_INVALID and not handle.value
        for bad in (np.where(np.arange(40) == 13, np.nan, good), np.zeros(40, dtype=np.complex128), np.where(np.arange(40) == 39, np.inf, good)):
            with kernels.DeviceBuffer.upload(np.ascontiguousarray(bad, dtype=np.complex128)) as bad_buf:
                assert lib.symgpu_sample_plan(bad_buf.ptr, 40, ctypes.byref(handle)) == _lib.E_INVALID and not handle.value
                with pytest.raises(ValueError):
                    kernels.SamplePlan(bad_buf)
        assert np.array_equal(live(), before), 'a refused plan left a block behind'
        assert lib.symgpu_sample_free(None) == _lib.E_INVALID and lib.symgpu_sample_info(None, None, None) == _lib.E_INVALID
        assert lib.symgpu_sample_draw(None, 5, 0, 0, None, None, out.ptr, out2.ptr, ctypes.addressof(nd)) == _lib.E_INVALID
        assert lib.symgpu_philox_uniform(1, 0, 4, None) == _lib.E_INVALID
        assert lib.symgpu_philox_uniform(1, -1, 4, out.ptr) == _lib.E_INVALID and lib.symgpu_philox_uniform(1, 0, -4, out.ptr) == _lib.E_INVALID
        assert lib.symgpu_philox_uniform(1, (1 << 63) - 4, 4, out.ptr) == _lib.E_INVALID                  # first_draw + count = 2^63
        assert lib.symgpu_philox_uniform(1, (1 << 63) - 5, 4, out.ptr) == _lib.OK
        plan = kernels.SamplePlan(buf)
        during = live()
        assert during[0] == before[0] + 1, 'a plan is one block: the stored levels'
        for args in ((-1, 0, 0, None, None, out.ptr, out2.ptr, ctypes.addressof(nd)), (5, 0, 0, None, None, None, out2.ptr, ctypes.addressof(nd)),
                     (5, 0, 0, None, None, out.ptr, None, ctypes.addressof(nd)), (5, 0, 0, None, None, out.ptr, out2.ptr, None),
                     (5, 0, -1, None, None, out.ptr, out2.ptr, ctypes.addressof(nd)), (5, 0, (1 << 63) - 5, None, None, out.ptr, out2.ptr, ctypes.addressof(nd)),
                     (1 << 31, 0, 0, None, None, out.ptr, out2.ptr, ctypes.addressof(nd))):
            assert lib.symgpu_sample_draw(plan.handle, *args) == _lib.E_INVALID, args
            assert np.array_equal(live(), during), 'a refused draw left a block behind'
        assert lib.symgpu_sample_draw(plan.handle, 5, 0, (1 << 63) - 6, None, None, out.ptr, out2.ptr, ctypes.addressof(nd)) == _lib.OK and nd.value >= 1
        assert np.array_equal(live(), during), 'a draw left scratch behind'
        plan.free()
        assert np.array_equal(live(), before), 'free did not return the plan'


# ---- signed sums ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 31, 32))
def test_signed_sums_are_numpys_integers(n):
    rng = np.random.default_rng(n)
    T, D = 37, 1 if n == 1 else 700
    z = rng.random((T, n)) < 0.4
    z[0] = False                                                     # the identity: the plain sum of the counts
    z[1] = True
    idx = np.unique(np.concatenate([rng.integers(0, 1 << n, D, dtype=np.int64), [0, (1 << n) - 1]]))
    count = rng.integers(1, (1 << 40) + 1, idx.shape[0], dtype=np.int64)
    count[0] = 1 << 40
    rows = packing.pack_rows(np.hstack([np.zeros_like(z), z]))
    with kernels.DeviceOp.upload(rows) as op:
        got = kernels.counts_signed_sums(op, n, idx, count)
        assert got.dtype == np.int64 and np.array_equal(got, so.signed_sums(z, n, idx, count)) and got[0] == count.sum()
        assert np.array_equal(kernels.counts_signed_sums(op, n, idx[:0], count[:0]), np.zeros(T, dtype=np.int64))
    mixed = np.hstack([np.zeros_like(z), z])
    mixed[5, 0] = True                                               # one X
    with kernels.DeviceOp.upload(packing.pack_rows(mixed)) as op:
        before = kernels.counters(('DEV_BLOCKS_LIVE',))
        with pytest.raises(ValueError, match='X-part'):
            kernels.counts_signed_sums(op, n, idx, count)
        assert np.array_equal(kernels.counters(('DEV_BLOCKS_LIVE',)), before)
        assert _lib.lib().symgpu_counts_signed_sums(op.handle, 33, None, None, 0, _lib.addr(np.zeros(T, dtype=np.int64))) == _lib.E_INVALID
        assert _lib.lib().symgpu_counts_signed_sums(op.handle, n, None, None, 3, _lib.addr(np.zeros(T, dtype=np.int64))) == _lib.E_INVALID


# ---- QuantumState -------------------------------------------------------------------------------------------------------------------------------
def test_sample_state_and_sample_counts():
    # a repeated row (0 and 3) and a row of zero weight (2); the state as given sums to one and so does its cleaned form
    bits = np.array([[0, 1, 1], [1, 0, 0], [1, 1, 1], [0, 1, 1], [0, 0, 0]])
    coeff = np.array([0.3, 0.5j, 0.0, 0.3, np.sqrt(1 - 0.36 - 0.25)])
    psi = QuantumState(bits, coeff)
    n_samples = 10_000
    got = psi.sample_state(n_samples, seed=42)
    counts = got.state_op.coeff_vec
    assert np.array_equal(got.state_matrix, bits) and got.vec_type == 'ket' and got.n_terms == 5
    assert counts[2] == 0 and np.all(counts.imag == 0) and np.all(counts.real == np.round(counts.real)) and counts.real.sum() == n_samples
    order = so.draw(coeff, so.philox_uniforms(42, 0, n_samples))
    assert np.array_equal(counts.real, np.bincount(order, minlength=5))
    assert np.array_equal(psi.sample_state(n_samples, seed=42).state_op.coeff_vec, counts)
    assert not np.array_equal(psi.sample_state(n_samples, seed=43).state_op.coeff_vec, counts)
    normalized = psi.sample_state(n_samples, return_normalized=True, seed=42)
    assert np.array_equal(normalized.state_op.coeff_vec, np.sqrt(counts.real / n_samples))
    assert np.allclose(got.normalize_counts.state_op.coeff_vec, np.sqrt(counts / counts.sum()), rtol=0, atol=0)
    bra = psi.dagger.sample_state(100, seed=1)
    assert bra.vec_type == 'bra' and np.array_equal(bra.state_matrix, bits)
    # np.random.seed governs seed=None
    np.random.seed(123)
    first = psi.sample_state(500).state_op.coeff_vec
    np.random.seed(123)
    assert np.array_equal(psi.sample_state(500).state_op.coeff_vec, first)
    np.random.seed(123)
    expect_seed = int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64))
    assert np.array_equal(psi.sample_state(500, seed=expect_seed).state_op.coeff_vec, first)
    with pytest.raises(ValueError, match='should not sample state that is not normalized'):
        QuantumState(bits, 2 * coeff).sample_state(10)
    with pytest.raises(ValueError, match='should not sample state that is not normalized'):
        QuantumState(bits, 2 * coeff).sample_counts(10)
    # the dense route agrees with the sparse one on a state given both ways (distinct rows in ascending index order: the same weights
    # in the same order, up to the zero-weight entries the dense vector has in between)
    rng = np.random.default_rng(3)
    rows = np.sort(rng.choice(1 << 6, size=16, replace=False))
    amp = rng.choice(np.array([0.25, -0.25, 0.25j, -0.25j]), size=16)       # 16 weights of 1/16: every partial sum of both trees is exact
    state = QuantumState(((rows[:, None] >> np.arange(5, -1, -1)) & 1), amp)
    idx, count = state.sample_counts(20_000, seed=8)
    dense = np.zeros(64, dtype=np.complex128)
    dense[rows] = amp
    want_idx, want_count = so.counts_of(so.draw(dense, so.philox_uniforms(8, 0, 20_000)))
    assert np.array_equal(idx, want_idx) and np.array_equal(count, want_count) and set(idx) <= set(rows)
    sparse = state.sample_state(20_000, seed=8).state_op.coeff_vec.real
    # both walk trees over the same positive weights in the same order, and with exact sums both are the exact inverse CDF
    assert np.array_equal(sparse[np.searchsorted(rows, idx)], count) and sparse.sum() == count.sum()
