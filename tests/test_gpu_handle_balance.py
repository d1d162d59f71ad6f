"""GPU: every call that builds operators inside the library returns what it took from the device allocator.

The allocator counts the blocks it has handed out and not got back (DEV_BLOCKS_LIVE, a gauge) and the frees of pointers it does not
hold (DEV_FREE_UNKNOWN, a double free).  A case is one call with its operands: it is run once as a warm-up (the context keeps hash
tables, join tables and sort state after first use), then twice more on the same shapes, each run creating its operands and freeing
every operand and result; both counters must read the same before and after.  Every run also checks the call's result against the
oracle or the known answer that the call's own tests use, so a conversion that hands out the wrong handle fails here too.  Operators of
4 to 12 terms on 5 qubits (one word per half row) and on 70 (two)."""
import ctypes

import numpy as np
import pytest

from symmer_amd import _lib, kernels
from symmer_amd.kernels import DeviceOp, rotation_args
from oracle import oracle_np as onp
from oracle import oracle_c as oc
from _golden import assert_op_equal, rotate_empty_cases
from _f3_f4_families import projection_expected
import _pauli_decomp_oracle as pdo

pytestmark = pytest.mark.gpu
TOL = 1e-12                      # non-Clifford coefficients against the NumPy oracle, as tests/test_gpu_parity.py compares them
BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')
STAGES = ('RESIDENT_DONE', 'ROTATE_HASH_JOIN', 'ROTATE_CLIFFORD_FAST', 'ROTATE_GENERAL', 'ROTATE_GENERAL_BY_DUP_CHECK')
CHAIN_FORMS = ('CHAIN_REGISTERS', 'CHAIN_LDS', 'CHAIN_SINGLE_WORKGROUP', 'CHAIN_TWO_LAUNCHES', 'CHAIN_FOUR_LAUNCHES')
I64, DBL, byref = ctypes.c_int64, ctypes.c_double, ctypes.byref
addr = _lib.addr


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 16.0


def operator(n, T=8, seed=5, duplicates=False):
    """bool[T, 2n] and dyadic coefficients without a zero; `duplicates`: the last three rows repeat the first three."""
    rng = np.random.default_rng(seed + n)
    symp = rng.random((T, 2 * n)) < 0.4
    symp[0, 0] = True                                # never the identity alone
    if duplicates:
        symp[T - 3:] = symp[:3]
    coeff = dyadic(rng, T)
    coeff[coeff == 0] = 0.5
    return symp, coeff


def cleaned(n, T=8, seed=5):
    return onp.cleanup_op(*operator(n, T, seed, duplicates=True))


def generator(n, seed=11):
    """A row that anticommutes with the first term of operator(n) and is not the identity."""
    symp, _ = operator(n)
    rng = np.random.default_rng(seed + n)
    while True:
        q = rng.random(2 * n) < 0.4
        if not onp.commutes_termwise(symp[:1], q.reshape(1, -1))[0, 0]:
            return q


def strings(strs, n):
    """bool[T, 2n] of Pauli strings on the first qubits, identities behind them."""
    m = np.zeros((len(strs), 2 * n), dtype=bool)
    for t, s in enumerate(strs):
        for j, ch in enumerate(s):
            m[t, j], m[t, n + j] = ch in 'XY', ch in 'ZY'
    return m


def up(symp, coeff=None):
    return DeviceOp.upload(onp.pack_rows(np.asarray(symp, dtype=bool)), coeff)


def up_clean(symp, coeff):
    """The cleanup of the operator, as a handle the library knows to hold no two equal rows."""
    with up(symp, coeff) as raw:
        return kernels.cleanup_dev(raw)


def down(h, n):
    rows, coeff = h.download()
    return onp.unpack_rows(rows, n), coeff


def same(h, n, exp_rows, exp_coeff, exact=True):
    rows, coeff = down(h, n)
    assert_op_equal(rows, coeff, exp_rows, exp_coeff, exact=exact, tol=TOL)


def stage_counts(fn, names=STAGES):
    before = kernels.counters(names)
    out = fn()
    return out, dict(zip(names, (kernels.counters(names) - before).tolist()))


# ---- the cases: name -> builder(n) -> run() ---------------------------------------------------------------------------------------
CASES = {}


def case(name, env=None, ns=(5, 70)):
    def register(builder):
        for n in ns:
            CASES[f'{name}-n{n}'] = (builder, n, env or {})
        return builder
    return register


# -- cleanups
@case('cleanup_dev-duplicates')
def _(n):
    symp, coeff = operator(n, duplicates=True)
    er, ec = onp.cleanup_op(symp, coeff)

    def run():
        with up(symp, coeff) as a, kernels.cleanup_dev(a) as res:
            assert res.info() == (er.shape[0], (n + 63) // 64, max(1, er.shape[0]))
            same(res, n, er, ec)
    return run


@case('cleanup_dev-no-rows')
def _(n):
    def run():
        with up(np.zeros((0, 2 * n), dtype=bool), np.zeros(0, dtype=complex)) as a, kernels.cleanup_dev(a) as res:
            assert res.info() == (0, (n + 63) // 64, 1)
    return run


@case('cleanup_indexed_dev-duplicates')
def _(n):
    symp, coeff = operator(n, duplicates=True)
    er, ec = onp.cleanup_op(symp, coeff)
    first = np.array([next(t for t in range(symp.shape[0]) if np.array_equal(symp[t], row)) for row in er], dtype=np.int64)

    def run():
        rows, c, f = kernels.cleanup_indexed(onp.pack_rows(symp), coeff)
        assert_op_equal(onp.unpack_rows(rows, n), c, er, ec)
        assert np.array_equal(f, first)
    return run


@case('cleanup_indexed_dev-no-rows')
def _(n):
    def run():
        out = ctypes.c_void_p()
        with up(np.zeros((0, 2 * n), dtype=bool), np.zeros(0, dtype=complex)) as a:
            _lib.check(_lib.lib().symgpu_cleanup_indexed_dev(a.handle, 1e-15, 1, byref(out)))
            with DeviceOp(out) as res:
                assert res.n_terms == 0 and kernels.op_first_index(res).shape == (0,)
    return run


# -- fused product + cleanup
def product_operands(n):
    (sa, ca), (sb, cb) = operator(n, 3, seed=21), operator(n, 4, seed=22)
    sb[3] = sb[0] ^ sa[0] ^ sa[1]                    # a planted merge: a0 b3 = a1 b0
    return onp.pack_rows(sa), ca, onp.pack_rows(sb), cb


def product_expected(A, a, B, b):
    """inner * outer as the device orders it (pair o * Ni + i; oracle_c.mul would make the operand with fewer terms the outer one)."""
    return oc.cleanup(*oc.mul_allpairs(A, a, B, b, True), 1e-15)


@case('mul_cleanup_dev-3x4')
def _(n):
    A, a, B, b = product_operands(n)
    er, ec = product_expected(A, a, B, b)

    def run():
        with DeviceOp.upload(A, a) as x, DeviceOp.upload(B, b) as y, kernels.mul_cleanup_handles(x, y) as res:
            rows, c = res.download()
            assert np.array_equal(rows, er) and np.array_equal(c, ec)
    return run


@case('mul_cleanup_dev-squared')
def _(n):
    _, _, B, b = product_operands(n)
    er, ec = product_expected(B, b, B, b)

    def run():
        with DeviceOp.upload(B, b) as y, kernels.mul_cleanup_handles(y, y) as res:
            rows, c = res.download()
            assert np.array_equal(rows, er) and np.array_equal(c, ec)
    return run


@case('mul_cleanup_dev-empty-operand')
def _(n):
    A, a, _, _ = product_operands(n)

    def run():
        with DeviceOp.upload(A, a) as x, DeviceOp.upload(A[:0], a[:0]) as none:
            for l, r in ((x, none), (none, x)):
                with kernels.mul_cleanup_handles(l, r) as res:
                    assert res.info() == (0, A.shape[1] // 2, 1)
    return run


@case('mul_cleanup_indexed_dev-3x4')
def _(n):
    A, a, B, b = product_operands(n)
    er, ec = product_expected(A, a, B, b)

    def run():
        rows, c, i_first, o_first = kernels.mul_cleanup_indexed(A, a, B, b, True, 1e-15)
        assert np.array_equal(rows, er) and np.array_equal(c, ec) and np.array_equal(A[i_first] ^ B[o_first], rows)
        assert np.all(np.diff(o_first * A.shape[0] + i_first) > 0)
    return run


# -- the calls that take and return host arrays
def host_cleanup(rows, coeff, capacity):
    W = rows.shape[1]
    out_r, out_c, n_out = np.zeros((max(capacity, 1), W), dtype='<u8'), np.zeros(max(capacity, 1), dtype=np.complex128), I64(-1)
    rc = _lib.lib().symgpu_cleanup(addr(rows), addr(coeff), rows.shape[0], W, 1e-15, 1, addr(out_r), addr(out_c), capacity, ctypes.addressof(n_out))
    return rc, out_r[:capacity], out_c[:capacity], n_out.value


@case('symgpu_cleanup')
def _(n):
    symp, coeff = operator(n, duplicates=True)
    rows = onp.pack_rows(symp)
    er, ec = oc.cleanup(rows, coeff, 1e-15)

    def run():
        rc, r, c, n_out = host_cleanup(rows, coeff, er.shape[0])
        assert rc == _lib.OK and n_out == er.shape[0] and np.array_equal(r, er) and np.array_equal(c, ec)
    return run


@case('symgpu_cleanup-capacity-one-short')
def _(n):
    symp, coeff = operator(n, duplicates=True)
    rows = onp.pack_rows(symp)
    count = oc.cleanup(rows, coeff, 1e-15)[0].shape[0]

    def run():
        rc, r, c, n_out = host_cleanup(rows, coeff, count - 1)
        assert rc == _lib.E_CAPACITY and n_out == count and not r.any() and not c.any()
    return run


@case('symgpu_mul_cleanup')
def _(n):
    A, a, B, b = product_operands(n)
    er, ec = product_expected(A, a, B, b)

    def run():
        cap = A.shape[0] * B.shape[0]
        out_r, out_c, n_out = np.zeros((cap, A.shape[1]), dtype='<u8'), np.zeros(cap, dtype=np.complex128), I64(-1)
        _lib.check(_lib.lib().symgpu_mul_cleanup(addr(A), addr(a), A.shape[0], addr(B), addr(b), B.shape[0], A.shape[1] // 2, 1, 1e-15, 1,
                                                 addr(out_r), addr(out_c), cap, ctypes.addressof(n_out)))
        assert n_out.value == er.shape[0] and np.array_equal(out_r[:n_out.value], er) and np.array_equal(out_c[:n_out.value], ec)
    return run


@case('symgpu_mul_allpairs')
def _(n):
    A, a, B, b = product_operands(n)
    er, ec = oc.mul_allpairs(A, a, B, b, True)

    def run():
        rows, c = kernels.mul_allpairs(A, a, B, b, True)
        assert np.array_equal(rows, er) and np.array_equal(c, ec)
    return run


def host_rotate(rows, coeff, q_row, angle, capacity):
    N, W = rows.shape
    cos_t, sin_t, k = rotation_args(angle)
    out_r, out_c = np.zeros((max(capacity, 1), W), dtype='<u8'), np.zeros(max(capacity, 1), dtype=np.complex128)
    n_out, allc = I64(-1), ctypes.c_int(-1)
    rc = _lib.lib().symgpu_rotate_single(addr(rows), addr(coeff), N, W // 2, addr(q_row), cos_t, sin_t, k, 1e-15, addr(out_r), addr(out_c), capacity,
                                         ctypes.addressof(n_out), ctypes.addressof(allc))
    return rc, out_r[:capacity], out_c[:capacity], n_out.value, allc.value


@case('symgpu_rotate_single')
def _(n):
    symp, coeff = cleaned(n)
    q = generator(n)
    er, ec = onp.rotate_by_single_pword(symp, coeff, q, 0.3)
    rows, q_row = onp.pack_rows(symp), onp.pack_rows(q.reshape(1, -1))

    def run():
        rc, r, c, n_out, allc = host_rotate(rows, coeff, q_row, 0.3, 2 * rows.shape[0])
        assert rc == _lib.OK and allc == 0 and n_out == er.shape[0] > rows.shape[0]
        assert_op_equal(onp.unpack_rows(r[:n_out], n), c[:n_out], er, ec, exact=False, tol=TOL)
    return run


@case('symgpu_rotate_single-capacity-one-short')
def _(n):
    symp, coeff = cleaned(n)
    q = generator(n)
    count = onp.rotate_by_single_pword(symp, coeff, q, 0.3)[0].shape[0]
    rows, q_row = onp.pack_rows(symp), onp.pack_rows(q.reshape(1, -1))

    def run():
        rc, r, c, n_out, allc = host_rotate(rows, coeff, q_row, 0.3, count - 1)
        assert rc == _lib.E_CAPACITY and n_out == count and allc == 0 and not r.any() and not c.any()
    return run


@case('symgpu_symmetry_kernel')
def _(n):
    symp, _ = operator(n, 6, seed=31)
    symp[:, [1, 3]] = False                          # two qubits without X or Y: at least two symmetries
    symp[:, [n + 1, n + 3]] = False
    H = onp.pack_rows(symp)
    eg, e_xor = oc.symmetry_generators(H, n)
    assert eg.shape[0] >= 2

    def run():
        gens, xor = kernels.symmetry_kernel(H, n)
        assert np.array_equal(gens, eg) and xor == e_xor
    return run


# -- a single rotation through each stage that can complete it
def rotation_case(name, angle, stage, env=None, clean=True, duplicates=False, commuting=False, extra=None):
    @case(f'rotate_single_dev-{name}', env)
    def _(n):
        symp, coeff = operator(n, duplicates=duplicates)
        if commuting:
            symp[:, :n] = False                      # Z and I only, and so is Q: everything commutes
            symp[:, n] = True
        if clean:
            symp, coeff = onp.cleanup_op(symp, coeff)
        q = strings(['Z'], n)[0] if commuting else generator(n)
        er, ec = onp.rotate_by_single_pword(symp, coeff, q, angle)
        q_row = onp.pack_rows(q.reshape(1, -1))[0]
        want = dict.fromkeys(STAGES, 0)
        want.update({stage: 1}, **(extra or {}))

        def run():
            with (up_clean if clean else up)(symp, coeff) as a:
                (res, allc), ran = stage_counts(lambda: kernels.rotate_single_dev(a, q_row, angle))
                assert ran == want, ran
                assert allc == commuting and (res is None) == commuting
                if res is not None:
                    with res:
                        same(res, n, er, ec, exact=False)
        return run


rotation_case('one-launch', 0.3, 'RESIDENT_DONE')
rotation_case('hash-join', 0.3, 'ROTATE_HASH_JOIN', {'SYMGPU_ROT_RESIDENT': '0'})
rotation_case('clifford-fast-k1', np.pi / 2, 'ROTATE_CLIFFORD_FAST', {'SYMGPU_ROT_RESIDENT': '0'})
rotation_case('clifford-fast-k2', np.pi, 'ROTATE_CLIFFORD_FAST', {'SYMGPU_ROT_RESIDENT': '0'})
rotation_case('general-non-clifford', 0.3, 'ROTATE_GENERAL', {'SYMGPU_ROTATE_GENERAL': '1'})
rotation_case('general-even-k', np.pi, 'ROTATE_GENERAL', {'SYMGPU_ROTATE_GENERAL': '1'})
rotation_case('general-odd-k-merge', np.pi / 2, 'ROTATE_GENERAL', {'SYMGPU_ROTATE_GENERAL': '1'}, clean=False, duplicates=True)
rotation_case('dup-check-to-general', np.pi / 2, 'ROTATE_GENERAL', clean=False, duplicates=True, extra={'ROTATE_GENERAL_BY_DUP_CHECK': 1})
rotation_case('all-commute', 0.3, 'RESIDENT_DONE', commuting=True)


# -- runs of Clifford rotations
def chain_case(K, env, registers):
    @case(f'rotate_clifford_chain_dev-K{K}-{"registers" if registers else "chain-reg-off"}', env)
    def _(n):
        symp, coeff = cleaned(n)
        rng = np.random.default_rng(41 + n)
        qs = np.vstack([generator(n), rng.random(2 * n) < 0.4])[:K]
        ks = [1, 3][:K]
        er, ec = onp.perform_rotations(symp, coeff, [(q, k * np.pi / 2) for q, k in zip(qs, ks)])

        def run():
            with up_clean(symp, coeff) as a:
                res, ran = stage_counts(lambda: kernels.rotate_clifford_chain_dev(a, onp.pack_rows(qs), ks), CHAIN_FORMS)
                with res:
                    assert sum(ran.values()) == 1 and ran['CHAIN_REGISTERS'] == int(registers), ran
                    assert res.info()[2] == symp.shape[0]
                    same(res, n, er, ec)
        return run


for K in (1, 2):                                     # the result is taken after an odd and after an even number of steps
    chain_case(K, {}, True)
    chain_case(K, {'SYMGPU_CHAIN_REG': '0'}, False)


def perform(a, qs, angles, clean):
    """symgpu_perform_rotations_dev as PauliwordOp.perform_rotations drives it -> the final handle (`a` itself if nothing changed)."""
    args = [rotation_args(float(t)) for t in angles]
    q_rows = onp.pack_rows(np.asarray(qs, dtype=bool))
    cos_t, sin_t, ks = (np.array([v[j] for v in args]) for j in range(3))
    res, n_done, _, _ = kernels.perform_rotations_dev(a, q_rows, cos_t, sin_t, ks.astype(np.int32), clean)
    assert n_done == len(angles)
    return a if res is None else res


@case('perform_rotations_dev-mixed')
def _(n):
    symp, coeff = cleaned(n)
    rng = np.random.default_rng(51 + n)
    qs = np.vstack([generator(n)] + [rng.random(2 * n) < 0.4 for _ in range(4)])
    angles = [np.pi / 2, 3 * np.pi / 2, 0.3, np.pi, np.pi / 2]            # Clifford run, non-Clifford step, Clifford run
    er, ec = onp.perform_rotations(symp, coeff, list(zip(qs, angles)))

    def run():
        with up_clean(symp, coeff) as a:
            res = perform(a, qs, angles, True)
            assert res is not a
            with res:
                same(res, n, er, ec, exact=False)
    return run


@case('perform_rotations_dev-through-no-terms-and-zero-identity', ns=(2,))
def _(n):
    cases = [c for c in rotate_empty_cases() if c['kind'] != 'single' and len(c['angles']) <= 3]
    assert len(cases) > 50 and all(c['in_symp'].shape[1] == 2 * n for c in cases)
    assert any(c['out_symp'].shape[0] == 0 for c in cases) and any(c['out_symp'].shape[0] == 1 and not c['out_symp'].any() for c in cases)

    def run():
        for c in cases:
            with up(c['in_symp'], c['in_coeff']) as a:
                res = perform(a, c['q'], c['angles'], False)
                rows, coeff = down(res, n)
                if res is not a:
                    res.free()
                assert rows.shape == c['out_symp'].shape and np.array_equal(rows, c['out_symp']), c
                assert np.allclose(coeff, c['out_coeff'], rtol=0, atol=1e-15), c
    return run


# -- the pieces of the hash-partitioned cleanup
@case('op_gather')
def _(n):
    symp, coeff = operator(n)
    idx = np.array([5, 0, 5, 7], dtype=np.int64)

    def run():
        with up(symp, coeff) as a:
            with kernels.op_gather(a, idx) as res:
                same(res, n, symp[idx], coeff[idx])
            with kernels.op_gather(a, idx[:0]) as none:
                assert none.info() == (0, (n + 63) // 64, 1)
    return run


def indexed(symp, coeff, keys):
    h = up(symp, coeff)
    kernels.op_set_first_index(h, np.asarray(keys, dtype='<u8'))
    return h


@case('merge_indexed_dev')
def _(n):
    symp, coeff = operator(n)
    keys = np.array([5, 1, 9, 12, 2, 7, 3, 20], dtype=np.int64)
    order = np.argsort(keys)
    shared = symp.copy()
    shared[[4, 6]] = symp[[1, 0]]                    # the second part repeats rows of the first: they merge at the smaller key
    sr, sc = onp.cleanup_op(shared[order], coeff[order])
    s_first = np.array([min(k for k, row in zip(keys, shared) if np.array_equal(row, r)) for r in sr], dtype=np.int64)

    def run():
        with indexed(symp[:4], coeff[:4], keys[:4]) as p0, indexed(symp[4:], coeff[4:], keys[4:]) as p1:
            with kernels.merge_indexed_dev([p0, p1], 0, False) as res:
                same(res, n, symp[order], coeff[order])
                assert np.array_equal(kernels.op_first_index(res).astype(np.int64), keys[order])
        with indexed(shared[:4], coeff[:4], keys[:4]) as p0, indexed(shared[4:], coeff[4:], keys[4:]) as p1:
            with kernels.merge_indexed_dev([p0, p1], 0, True) as res:
                same(res, n, sr, sc)
                assert np.array_equal(kernels.op_first_index(res).astype(np.int64), s_first)
        with up(symp[:0], coeff[:0]) as e0, up(symp[:0], coeff[:0]) as e1, kernels.merge_indexed_dev([e0, e1], 0, True) as res:
            assert res.info() == (0, (n + 63) // 64, 1)
    return run


# -- generators, projection, noncontextuality, Pauli decomposition
@case('generators_dev')
def _(n):
    symp, coeff = operator(n, duplicates=True)
    eg = onp.generators(symp)
    assert 0 < eg.shape[0] < symp.shape[0]

    def run():
        with up(symp, coeff) as a, kernels.generators_dev(a) as res:
            same(res, n, eg, np.ones(eg.shape[0]))
        with up(np.zeros((4, 2 * n), dtype=bool), coeff[:4]) as identities, kernels.generators_dev(identities) as res:
            assert res.info() == (0, (n + 63) // 64, 1)                   # rank 0
    return run


@case('project_dev')
def _(n):
    stab, eig, keep = strings(['Z'], n), np.array([-1]), np.arange(1, n)
    symp, coeff = operator(n)
    symp[:, 0] = False                               # no X or Y on the stabilised qubit: every term survives ...
    symp[4:, 1:n], symp[4:, n + 1:] = symp[:4, 1:n], symp[:4, n + 1:]       # ... and the last four fall onto the first four
    symp[:, n] = np.arange(8) % 2 == 0
    er, ec, n_s = projection_expected(symp, coeff, stab, eig, keep)
    assert n_s == 8 and 0 < er.shape[0] <= 4
    killed = symp.copy()
    killed[:, 0] = True                              # X or Y on the stabilised qubit: nothing survives

    def run():
        with up(symp, coeff) as a:
            res, survived = kernels.project_dev(a, onp.pack_rows(stab), eig, keep, n)
            with res:
                assert survived == n_s
                same(res, n - 1, er, ec)
        with up(killed, coeff) as a:
            res, survived = kernels.project_dev(a, onp.pack_rows(stab), eig, keep, n)
            with res:
                assert survived == 0 and res.info() == (0, (n - 1 + 63) // 64, 1)
        with up(symp[:0], coeff[:0]) as a:
            res, survived = kernels.project_dev(a, onp.pack_rows(stab), eig, keep, n)
            with res:
                assert survived == 0 and res.info() == (0, (n - 1 + 63) // 64, 1)
    return run


@case('noncontextual_dev')
def _(n):
    yes, no = strings(['ZII', 'IZI', 'ZZI', 'IIZ', 'XXI', 'YYI'], n), strings(['XI', 'IX', 'ZI', 'IZ', 'XX', 'ZZ'], n)
    assert onp.is_noncontextual(yes) and not onp.is_noncontextual(no)

    def run():
        with up(yes, np.ones(6)) as a, up(no, np.ones(6)) as b:
            assert kernels.noncontextual_dev(a) is True and kernels.noncontextual_dev(b) is False
    return run


@case('from_matrix_dense', ns=(1, 2))
def _(n):
    rng = np.random.default_rng(61)
    side = 1 << n
    matrix = np.zeros((2, 2), dtype=complex) if n == 1 else (rng.integers(-8, 9, (side, side)) + 1j * rng.integers(-8, 9, (side, side))) / 16.0
    ex, ez, ec = pdo.decompose(matrix, n)
    assert (ex.shape[0] == 0) == (n == 1)

    def run():
        res, n_terms, _ = kernels.pauli_decompose_dense(matrix, n)
        with res:
            assert n_terms == ex.shape[0] and res.info() == (n_terms, 1, n_terms)
            rows, coeff = down(res, n)
            assert np.array_equal(rows, pdo.symp_of(ex, ez, n)) and pdo.bits_equal(coeff, ec)
    return run


# -- the handle primitives that make a fresh operator
@case('op_clone-upload_bool-random')
def _(n):
    symp, coeff = operator(n, duplicates=True)

    def run():
        with DeviceOp.upload_bool(symp, coeff) as a, a.clone() as b:
            for h in (a, b):
                assert h.info() == (8, (n + 63) // 64, 8)
                same(h, n, symp, coeff)
        with DeviceOp.random(12, n, 0.3, 77) as r, DeviceOp.random(12, n, 0.3, 77) as again, DeviceOp.random(0, n, 0.3, 77) as none:
            rows, c = r.download()
            assert r.info() == (12, (n + 63) // 64, 12) and none.info()[0] == 0
            assert np.array_equal(onp.pack_rows(onp.unpack_rows(rows, n)), rows)          # no bit beyond qubit n - 1
            assert rows.any() and np.all(np.isfinite(c.view(float))) and all(np.array_equal(x, y) for x, y in zip(again.download(), (rows, c)))
    return run


@pytest.mark.parametrize('name', list(CASES))
def test_a_call_returns_every_block_it_took(name, monkeypatch):
    builder, n, env = CASES[name]
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    run = builder(n)
    run()                                            # warm-up: what the context keeps after first use
    before = kernels.counters(BALANCE)
    run()
    run()
    after = kernels.counters(BALANCE)
    print(name, dict(zip(BALANCE, before.tolist())), '->', dict(zip(BALANCE, after.tolist())))
    assert np.array_equal(after, before), dict(zip(BALANCE, (after - before).tolist()))
