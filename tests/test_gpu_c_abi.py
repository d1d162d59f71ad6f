"""GPU: the C ABI as INTEGRATION.md binds it — host-array calls, the capacity contract, refusals, handle primitives, and the
instruments (checksums, popcounts, the synthetic-operator generator) the full-size tests and bench.py trust.

The binding is INDEPENDENT of symmer_amd.kernels and the drop-in classes: (a) the ctypes stub of INTEGRATION.md §1, extracted from the
document and executed with the library name replaced by the built library's path; (b) plain ctypes calls in the stub's style — P(...),
I64(...), c_double(...), bare ints, on a CDLL object of this file's own without argtypes.  Expected values come from oracle/oracle_np.py
on bool matrices, oracle/oracle_c.py, plain NumPy and the committed goldens, never from another path of the library.

Bar (tests/test_gpu_parity.py): rows, row order, tables and GF(2) words bit-exact; coefficients bit-exact for dyadic inputs
and Clifford rotations, within 1e-12 for Gaussian inputs (assert_op_equal(..., exact=False, tol=1e-12)).

symgpu_op_scale is held to the kernel's claim, "plain IEEE products, no contraction": bit for bit NumPy's complex128 SCALAR multiply.
NumPy's ARRAY multiply is no bit reference on x86-64: its SIMD loop contracts with FMA ("Product coefficients"; 487 of
2,000 components of 1,000 Gaussian products differ from the plain product by an ulp on an AVX-512 host), so it is NumPy that contracts.

Refusals: only conditions the source decides on the host before any allocation, copy or launch (the SG_REQUIRE lines at the top of the
entry points).  No wild, misaligned-and-dereferenced or freed pointer is ever passed."""
import ctypes
import types

import numpy as np
import pytest

from symmer_amd import _lib as _pkg_lib
from symmer_amd.kernels import rotation_args          # pure host arithmetic
from oracle import oracle_np as onp
from oracle import oracle_c as oc
from _golden import family, as_bool, assert_op_equal, GOLDEN
from _integration_doc import stub_source

pytestmark = pytest.mark.gpu
TOL = 1e-12
OK, E_INVALID, E_CAPACITY = 0, -1, -4
P, I64, U64, DBL = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
byref = ctypes.byref
SENT_ROW = np.uint64(0xA5A5A5A5A5A5A5A5)
SENT_C = complex(-7.25, 3.5)


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 16.0


# ---------------------------------------------------------------- the two bindings ---------------------------------------------
@pytest.fixture(scope='module')
def stub():
    """INTEGRATION.md §1 as a module.  The package's loader runs first so that the library is bound to the HIP runtime it was linked
    against (RTLD_DEEPBIND); the stub's own CDLL of the same path is then the same library instance."""
    _pkg_lib.load()
    src = stub_source()
    assert "'libsymgpu.so'" in src
    mod = types.ModuleType('_symgpu_stub')
    exec(compile(src.replace("'libsymgpu.so'", repr(_pkg_lib.LIB_PATH)), 'INTEGRATION.md:stub', 'exec'), mod.__dict__)
    return mod


@pytest.fixture(scope='module')
def L(stub):
    lib = ctypes.CDLL(_pkg_lib.LIB_PATH)              # this file's own object: no argtypes anywhere
    lib.symgpu_last_error.restype = ctypes.c_char_p
    assert lib.symgpu_init(0) == OK                   # idempotent
    return lib


def ptr(a):
    return None if a is None else P(a.ctypes.data)


def err(L):
    return L.symgpu_last_error().decode()


def ok(L, rc):
    assert rc == OK, (rc, err(L))


def c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def upload(L, rows, coeff=None):
    rows = np.ascontiguousarray(rows, dtype='<u8')
    h = ctypes.c_void_p()
    c = None if coeff is None else c128(coeff)
    ok(L, L.symgpu_op_upload(ptr(rows), ptr(c), I64(rows.shape[0]), rows.shape[1] // 2, byref(h)))
    assert h.value
    return h


def info(L, h):
    T, Wq, cap = I64(-1), ctypes.c_int(-1), I64(-1)
    ok(L, L.symgpu_op_info(h, byref(T), byref(Wq), byref(cap)))
    return T.value, Wq.value, cap.value


def download(L, h, coeff=True):
    T, Wq, _ = info(L, h)
    rows = np.full((T, 2 * Wq), SENT_ROW, dtype='<u8')
    c = np.full(T, SENT_C, dtype=np.complex128) if coeff else None
    ok(L, L.symgpu_op_download(h, ptr(rows), ptr(c), I64(T)))
    return rows, c


def free(L, *handles):
    for h in handles:
        ok(L, L.symgpu_op_free(h))


def sanity(L):
    """A valid call after a refusal: the library still answers, and answers right."""
    rng = np.random.default_rng(5)
    a, b = rng.random((9, 140)) < 0.4, rng.random((6, 140)) < 0.4
    A, B = onp.pack_rows(a), onp.pack_rows(b)
    out = np.full((9, 6), 7, dtype=np.uint8)
    ok(L, L.symgpu_commutes(ptr(A), I64(9), ptr(B), I64(6), 2, ptr(out)))
    assert np.array_equal(out.astype(bool), onp.commutes_termwise(a, b))


def with_duplicates(rng, T, n, p=0.3, frac=0.5):
    """bool[T, 2n] whose rows repeat often enough that segments of several rows occur."""
    base = rng.random((max(1, int(T * (1 - frac)) // 2 + 1), 2 * n)) < p
    return base[rng.integers(0, base.shape[0], T)]


def thr_on_a_sum(coeff):
    """|c| of one merged coefficient, exactly: a sum with a zero component, whose modulus is its other component (strict > decides)."""
    for c in coeff:
        if c != 0 and (c.real == 0 or c.imag == 0):
            return float(abs(c.real) + abs(c.imag))
    return float(np.abs(coeff[0]))


# ---------------------------------------------------------------- 2a. the stub, as written ---------------------------------------
def test_stub_pack_unpack_match_the_oracle(stub):
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, 128, 130):
        symp = rng.random((37, 2 * n)) < 0.5
        symp[0] = True                                                   # every qubit set: padding must stay zero
        packed = stub.pack(symp)
        assert packed.dtype == np.dtype('<u8') and np.array_equal(packed, onp.pack_rows(symp)), n
        assert np.array_equal(stub.unpack(packed, n), symp) and np.array_equal(onp.unpack_rows(packed, n), symp), n


def test_stub_cleanup_golden(stub):
    for i, case in enumerate(family('cleanup')):
        s, c, thr = as_bool(case['in_symp']), case['in_coeff'], float(case['thr'])
        rows, coeff = stub.cleanup(s, c, None if thr < 0 else thr)
        if s.shape[0] == 0:
            # the fixture records PauliwordOp.cleanup, whose 0 * I for an operator without terms is made on the Python side
            # (base.py:631-632); symplectic_cleanup itself, which the stub replaces, returns no row
            assert rows.shape == (0, s.shape[1]) and coeff.shape == (0,)
            continue
        exact = bool(np.all(np.asarray(c) * 16 == np.round(np.asarray(c) * 16)))
        try:
            assert_op_equal(rows, coeff, case['out_symp'], case['out_coeff'], exact=exact, tol=TOL)
        except AssertionError as e:
            raise AssertionError(f'cleanup golden case {i}: {e}')


def test_stub_mul_cleanup_golden(stub):
    """Operand choice as test_mul_golden: the operand with fewer terms is outer.  The family holds both orientations, so both values
    of inner_is_left meet the reference's output; the opposite flag on the same operands is held against the C oracle."""
    seen = set()
    for i, case in enumerate(family('mul')):
        a, ca, b, cb = as_bool(case['a_symp']), case['a_coeff'], as_bool(case['b_symp']), case['b_coeff']
        inner, ci, outer, co, left = (b, cb, a, ca, False) if a.shape[0] < b.shape[0] else (a, ca, b, cb, True)
        exact = bool(case['exact'])
        n = a.shape[1] // 2
        try:
            rows, coeff = stub.mul_cleanup(inner, ci, outer, co, left, 1e-15)
            assert_op_equal(rows, coeff, case['out_symp'], case['out_coeff'], exact=exact, tol=TOL)
            if inner.shape[0] and outer.shape[0]:
                seen.add(left)
                rows, coeff = stub.mul_cleanup(inner, ci, outer, co, not left, 1e-15)
                er, ec = oc.mul_allpairs(onp.pack_rows(inner), ci, onp.pack_rows(outer), co, inner_is_left=not left)
                er, ec = oc.cleanup(er, ec, 1e-15)
                assert_op_equal(rows, coeff, onp.unpack_rows(er, n), ec, exact=exact, tol=TOL)
        except AssertionError as e:
            raise AssertionError(f'mul golden case {i} (inner_is_left={left}): {e}')
    assert seen == {True, False}


def test_stub_commutes_golden(stub):
    for i, case in enumerate(family('commute')):
        out = stub.commutes(as_bool(case['a_symp']), as_bool(case['b_symp']))
        assert out.dtype == bool and out.shape == case['out'].shape and np.array_equal(out, as_bool(case['out'])), i


@pytest.mark.parametrize('n', [1, 3, 64, 65, 130, 1000])
def test_stub_cleanup_vs_oracle(stub, n):
    rng = np.random.default_rng(100 + n)
    for T in (1, 2, 65, 700, 3000):
        symp = with_duplicates(rng, T, n)
        coeff = dyadic(rng, T)
        _, merged = onp.symplectic_cleanup(symp, coeff, None)
        assert T < 60 or merged.shape[0] < 0.8 * T                       # segments of several rows do occur
        for thr in (None, 1e-15, thr_on_a_sum(merged)):
            rows, c = stub.cleanup(symp, coeff, thr)
            er, ec = onp.symplectic_cleanup(symp, coeff, thr)
            assert_op_equal(rows, c, er, ec, exact=True)
            if thr is not None and thr > 1e-15:
                assert er.shape[0] < merged.shape[0]                     # the sum that lies on the threshold is dropped: strict >


@pytest.mark.parametrize('n', [1, 3, 64, 65, 130, 1000])
def test_stub_mul_cleanup_vs_oracle(stub, n):
    """Operands drawn from a small group, so products collide and segments of several pairs occur.  The stub binds use_thr = 1, so
    thr is 1e-15, 0, or a value that lies on a merged sum."""
    rng = np.random.default_rng(200 + n)
    gens = rng.random((5, 2 * n)) < 0.4

    def group_rows(t):
        pick = rng.random((t, 5)) < 0.5
        return (pick.astype(np.uint8) @ gens.astype(np.uint8) % 2).astype(bool)

    for Ni, No in ((1, 1), (7, 3), (64, 40), (300, 10)):
        inner, outer, ci, co = group_rows(Ni), group_rows(No), dyadic(rng, Ni), dyadic(rng, No)
        for left in (True, False):
            def expected(thr):
                if left:
                    return onp.multiply_by_operator(inner, ci, outer, co, thr)
                er, ec = onp.multiply_by_operator(inner, ci.conjugate(), outer, co.conjugate(), thr)   # the dagger swap, base.py:847-852
                return er, ec.conjugate()
            _, merged = expected(None)
            for thr in (1e-15, 0.0, thr_on_a_sum(merged)):
                rows, c = stub.mul_cleanup(inner, ci, outer, co, left, thr)
                er, ec = expected(thr)
                assert_op_equal(rows, c, er, ec, exact=True)


@pytest.mark.parametrize('n', [1, 3, 64, 65, 130, 1000])
def test_stub_commutes_vs_oracle(stub, n):
    rng = np.random.default_rng(300 + n)
    for N, M in ((1, 1), (65, 130), (300, 257)):
        a, b = rng.random((N, 2 * n)) < 0.4, rng.random((M, 2 * n)) < 0.4
        assert np.array_equal(stub.commutes(a, b), onp.commutes_termwise(a, b)), (N, M)


# ---------------------------------------------------------------- 2b. host-array entry points beside the stub ------------------------
def rotate_single(L, symp, coeff, q, angle, clifford_thr=1e-18, capacity=None):
    """symgpu_rotate_single through raw ctypes -> (rc, rows bool or None, coeff, n_out, all_commute, untouched)."""
    symp = np.asarray(symp, dtype=bool)
    n = symp.shape[1] // 2
    rows, c = onp.pack_rows(symp), c128(coeff)
    N, W = rows.shape
    qrow = onp.pack_rows(np.asarray(q, dtype=bool).reshape(1, -1))
    cos_t, sin_t, k = rotation_args(angle, clifford_thr)
    cap = 2 * N if capacity is None else capacity
    out_r = np.full((max(cap, 1), W), SENT_ROW, dtype='<u8')
    out_c = np.full(max(cap, 1), SENT_C, dtype=np.complex128)
    n_out, allc = I64(-1), ctypes.c_int(-1)
    rc = L.symgpu_rotate_single(ptr(rows), ptr(c), I64(N), W // 2, ptr(qrow), DBL(cos_t), DBL(sin_t), k, DBL(1e-15),
                                ptr(out_r), ptr(out_c), I64(cap), byref(n_out), byref(allc))
    untouched = bool(np.all(out_r == SENT_ROW) and np.all(out_c == SENT_C))
    res = None
    if rc == OK and not allc.value:
        res = onp.unpack_rows(out_r[:n_out.value], n)
        assert np.all(out_r[n_out.value:] == SENT_ROW) and np.all(out_c[n_out.value:] == SENT_C)
    return rc, res, out_c[:max(n_out.value, 0)], n_out.value, allc.value, untouched


def check_rotation_case(L, symp, coeff, q, angle, clifford_thr, exp_rows, exp_coeff):
    symp = as_bool(symp)
    rc, rows, c, n_out, allc, untouched = rotate_single(L, symp, coeff, q, angle, clifford_thr)
    assert rc == OK, err(L)
    if np.all(onp.commutes_termwise(symp, as_bool(q).reshape(1, -1))):
        assert allc == 1 and untouched and n_out == symp.shape[0]        # `return self` (base.py:1131-1133): the result is the input
        rows, c = symp, np.asarray(coeff)
    else:
        assert allc == 0
    clifford = rotation_args(angle, clifford_thr)[2] >= 0
    assert_op_equal(rows, c, exp_rows, exp_coeff, exact=clifford, tol=TOL)


def test_rotate_single_golden(L):
    done = 0
    for i, case in enumerate(family('rotate')):
        if int(case['chain']):
            continue
        try:
            check_rotation_case(L, case['in_symp'], case['in_coeff'], case['q'], float(case['angle']), 1e-18, case['out_symp'], case['out_coeff'])
        except AssertionError as e:
            raise AssertionError(f'rotate golden case {i}: {e}')
        done += 1
    assert done > 200


def test_rotate_single_duplicate_rows_and_threshold_golden(L):
    for i, case in enumerate(family('rotate_dup')):
        try:
            check_rotation_case(L, case['in_symp'], case['in_coeff'], case['q'], float(case['angle']), float(case['threshold']),
                                case['out_symp'], case['out_coeff'])
        except AssertionError as e:
            raise AssertionError(f'rotate_dup golden case {i}: {e}')


@pytest.mark.parametrize('n,N', [(1, 4), (65, 300), (130, 2000), (1000, 500)])
def test_rotate_single_vs_oracle(L, n, N):
    rng = np.random.default_rng(400 + n)
    symp = rng.random((N, 2 * n)) < 0.3 if n > 1 else np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=bool)      # I, X, Z, Y
    symp, coeff = onp.symplectic_cleanup(symp, dyadic(rng, N) + 1 / 32, 1e-15)
    q = rng.random(2 * n) < 0.4
    q[0] = q[n] = True
    for angle in (0.0, np.pi / 2, np.pi, 3 * np.pi / 2, 0.3, -1.1):
        rc, rows, c, n_out, allc, _ = rotate_single(L, symp, coeff, q, angle)
        er, ec = onp.rotate_by_single_pword(symp, coeff, q, angle)
        assert rc == OK and allc == 0 and n_out == er.shape[0], (angle, err(L))
        clifford = rotation_args(angle)[2] >= 0
        assert_op_equal(rows, c, er, ec, exact=clifford, tol=TOL)


def test_rotate_single_all_commute_and_empty(L):
    rng = np.random.default_rng(41)
    n, N = 70, 50
    symp, coeff = rng.random((N, 2 * n)) < 0.3, dyadic(rng, N)
    identity = np.zeros(2 * n, dtype=bool)
    for angle in (0.3, np.pi / 2):
        rc, rows, _, n_out, allc, untouched = rotate_single(L, symp, coeff, identity, angle)
        assert rc == OK and allc == 1 and untouched and rows is None
        assert n_out == N                                              # the header's sentence: the result is the input
    q = rng.random(2 * n) < 0.5
    for angle in (0.3, np.pi / 2):
        rc, rows, _, n_out, allc, untouched = rotate_single(L, symp[:0], coeff[:0], q, angle)
        assert rc == OK and allc == 1 and n_out == 0 and untouched


def growing_rotation(rng, n=100, N=400):
    symp = rng.random((N, 2 * n)) < 0.3
    symp, coeff = onp.symplectic_cleanup(symp, rng.standard_normal(N) + 1j * rng.standard_normal(N), 1e-15)
    q = rng.random(2 * n) < 0.5
    er, ec = onp.rotate_by_single_pword(symp, coeff, q, 0.3)
    assert er.shape[0] > symp.shape[0] + 20                              # the anticommuting rows split in two
    return symp, coeff, q, er, ec


def test_rotate_single_result_longer_than_the_input(L):
    symp, coeff, q, er, ec = growing_rotation(np.random.default_rng(42))
    N = symp.shape[0]
    rc, _, _, n_out, allc, untouched = rotate_single(L, symp, coeff, q, 0.3, capacity=N)
    assert rc == E_CAPACITY and n_out == er.shape[0] and allc == 0 and untouched and err(L)
    rc, rows, c, n_out, allc, _ = rotate_single(L, symp, coeff, q, 0.3, capacity=2 * N)
    assert rc == OK and n_out == er.shape[0]
    assert_op_equal(rows, c, er, ec, exact=False, tol=TOL)


def test_empty_inputs_of_cleanup_and_mul_cleanup(L):
    rows = onp.pack_rows(np.random.default_rng(1).random((4, 140)) < 0.5)
    c = c128(np.ones(4))
    out_r, out_c = np.full((4, 4), SENT_ROW, dtype='<u8'), np.full(4, SENT_C)
    n_out = I64(-1)
    ok(L, L.symgpu_cleanup(ptr(rows), ptr(c), I64(0), 4, DBL(1e-15), 1, ptr(out_r), ptr(out_c), I64(4), byref(n_out)))
    assert n_out.value == 0
    n_out = I64(-1)
    ok(L, L.symgpu_cleanup(None, None, I64(0), 4, DBL(0.0), 0, None, None, I64(0), byref(n_out)))
    assert n_out.value == 0
    for Ni, No in ((0, 4), (4, 0), (0, 0)):
        n_out = I64(-1)
        ok(L, L.symgpu_mul_cleanup(ptr(rows), ptr(c), I64(Ni), ptr(rows), ptr(c), I64(No), 2, 1, DBL(1e-15), 1,
                                   ptr(out_r), ptr(out_c), I64(4), byref(n_out)))
        assert n_out.value == 0
    assert np.all(out_r == SENT_ROW) and np.all(out_c == SENT_C)


def dev_buffer(L, host):
    d = ctypes.c_void_p()
    ok(L, L.symgpu_dev_alloc(I64(max(host.nbytes, 16)), byref(d)))
    if host.nbytes:
        ok(L, L.symgpu_dev_upload(d, ptr(host), I64(host.nbytes)))
    return d


@pytest.mark.parametrize('R,Wc', [(40, 1), (64, 3), (300, 12), (130, 70)])
def test_rref_dev_matches_rref_and_the_oracle(L, R, Wc):
    rng = np.random.default_rng(500 + R)
    m = rng.integers(0, 1 << 63, (R, Wc), dtype=np.uint64) & rng.integers(0, 1 << 63, (R, Wc), dtype=np.uint64)
    m[R // 2] = 0
    m[R - 1] = m[0]
    er, e_xor, e_piv = oc.rref(m, want_pivots=True)
    host = m.copy()
    xor_h, piv_h = I64(-1), np.full(R, -7, dtype=np.int64)
    ok(L, L.symgpu_rref(ptr(host), I64(R), I64(Wc), byref(xor_h), ptr(piv_h)))
    d = dev_buffer(L, m)
    xor_d, piv_d = I64(-1), np.full(R, -7, dtype=np.int64)
    ok(L, L.symgpu_rref_dev(d, I64(R), I64(Wc), byref(xor_d), ptr(piv_d)))
    got = np.empty_like(m)
    ok(L, L.symgpu_dev_download(d, ptr(got), I64(got.nbytes)))
    ok(L, L.symgpu_dev_free(d))
    assert np.array_equal(got, er) and np.array_equal(host, er)
    assert xor_d.value == xor_h.value == e_xor
    assert np.array_equal(piv_d, e_piv) and np.array_equal(piv_h, e_piv)


def test_rref_dev_without_rows(L):
    xor = I64(-1)
    ok(L, L.symgpu_rref_dev(None, I64(0), I64(3), byref(xor), None))
    assert xor.value == 0
    xor = I64(-1)
    ok(L, L.symgpu_rref(None, I64(0), I64(3), byref(xor), None))
    assert xor.value == 0


def symmetry_kernel(L, h_symp, capacity):
    h_symp = as_bool(h_symp)
    n = h_symp.shape[1] // 2
    H = onp.pack_rows(h_symp)
    out = np.full((max(capacity, 1), H.shape[1]), SENT_ROW, dtype='<u8')
    k, xor = I64(-1), I64(-1)
    rc = L.symgpu_symmetry_kernel(ptr(H), I64(H.shape[0]), n, H.shape[1] // 2, ptr(out), I64(capacity), byref(k), byref(xor))
    return rc, out, k.value, xor.value, n, H


def test_symmetry_kernel_golden_through_raw_ctypes(L):
    for case in family('symgen')[2:4]:
        n2 = case['h_symp'].shape[1]
        rc, out, k, xor, n, H = symmetry_kernel(L, case['h_symp'], n2)
        assert rc == OK, err(L)
        assert k == case['symgen'].shape[0] and np.array_equal(onp.unpack_rows(out[:k], n), as_bool(case['symgen']))
        assert np.all(out[k:] == SENT_ROW)
        eg, e_xor = oc.symmetry_generators(H, n)
        assert np.array_equal(out[:k], eg) and xor == e_xor


# ---------------------------------------------------------------- 2c. the capacity contract -----------------------------------------
def test_capacity_contract_of_cleanup(L):
    rng = np.random.default_rng(61)
    symp, coeff = with_duplicates(rng, 500, 130), dyadic(rng, 500)
    er, ec = onp.symplectic_cleanup(symp, coeff, 1e-15)
    cnt = er.shape[0]
    rows, c = onp.pack_rows(symp), c128(coeff)
    assert 10 < cnt < 400
    for cap in (0, cnt - 1, cnt):
        out_r, out_c = np.full((cnt, rows.shape[1]), SENT_ROW, dtype='<u8'), np.full(cnt, SENT_C)
        n_out = I64(-1)
        rc = L.symgpu_cleanup(ptr(rows), ptr(c), I64(500), rows.shape[1], DBL(1e-15), 1, ptr(out_r), ptr(out_c), I64(cap), byref(n_out))
        assert n_out.value == cnt
        if cap < cnt:
            assert rc == E_CAPACITY and err(L) and np.all(out_r == SENT_ROW) and np.all(out_c == SENT_C)
        else:
            assert rc == OK, err(L)
            assert_op_equal(onp.unpack_rows(out_r, 130), out_c, er, ec, exact=True)
    n_out = I64(-1)                                                      # asking needs no buffer
    assert L.symgpu_cleanup(ptr(rows), ptr(c), I64(500), rows.shape[1], DBL(1e-15), 1, None, None, I64(0), byref(n_out)) == E_CAPACITY
    assert n_out.value == cnt


def test_capacity_contract_of_mul_cleanup(L):
    rng = np.random.default_rng(62)
    n = 70
    gens = rng.random((6, 2 * n)) < 0.4
    rows_of = lambda t: ((rng.random((t, 6)) < 0.5).astype(np.uint8) @ gens.astype(np.uint8) % 2).astype(bool)
    inner, outer, ci, co = rows_of(60), rows_of(20), dyadic(rng, 60), dyadic(rng, 20)
    er, ec = onp.multiply_by_operator(inner, ci, outer, co, 1e-15)
    cnt = er.shape[0]
    assert 4 < cnt <= 64
    A, B, ca, cb = onp.pack_rows(inner), onp.pack_rows(outer), c128(ci), c128(co)
    for cap in (0, cnt - 1, cnt):
        out_r, out_c = np.full((cnt, A.shape[1]), SENT_ROW, dtype='<u8'), np.full(cnt, SENT_C)
        n_out = I64(-1)
        rc = L.symgpu_mul_cleanup(ptr(A), ptr(ca), I64(60), ptr(B), ptr(cb), I64(20), A.shape[1] // 2, 1, DBL(1e-15), 1,
                                  ptr(out_r), ptr(out_c), I64(cap), byref(n_out))
        assert n_out.value == cnt
        if cap < cnt:
            assert rc == E_CAPACITY and err(L) and np.all(out_r == SENT_ROW) and np.all(out_c == SENT_C)
        else:
            assert rc == OK, err(L)
            assert_op_equal(onp.unpack_rows(out_r, n), out_c, er, ec, exact=True)


def test_capacity_contract_of_rotate_single(L):
    symp, coeff, q, er, ec = growing_rotation(np.random.default_rng(63))
    cnt = er.shape[0]
    for cap in (0, cnt - 1):
        rc, _, _, n_out, allc, untouched = rotate_single(L, symp, coeff, q, 0.3, capacity=cap)
        assert rc == E_CAPACITY and n_out == cnt and allc == 0 and untouched and err(L)
    rc, rows, c, n_out, _, _ = rotate_single(L, symp, coeff, q, 0.3, capacity=cnt)
    assert rc == OK and n_out == cnt
    assert_op_equal(rows, c, er, ec, exact=False, tol=TOL)


def test_capacity_contract_of_symmetry_kernel(L):
    case = family('symgen')[3]
    expect = as_bool(case['symgen'])
    cnt = expect.shape[0]
    assert cnt >= 2
    for cap in (0, cnt - 1):
        rc, out, k, _, n, _ = symmetry_kernel(L, case['h_symp'], cap)
        assert rc == E_CAPACITY and k == cnt and err(L) and np.all(out == SENT_ROW)
    rc, out, k, _, n, _ = symmetry_kernel(L, case['h_symp'], cnt)
    assert rc == OK and k == cnt and np.array_equal(onp.unpack_rows(out[:k], n), expect)


def test_capacity_contract_of_the_downloads(L):
    rng = np.random.default_rng(64)
    n, T = 100, 90
    symp, coeff = with_duplicates(rng, T, n), dyadic(rng, T)
    rows = onp.pack_rows(symp)
    h = upload(L, rows, coeff)
    out_r, out_c = np.full((T, rows.shape[1]), SENT_ROW, dtype='<u8'), np.full(T, SENT_C)
    assert L.symgpu_op_download(h, ptr(out_r), ptr(out_c), I64(T - 1)) == E_CAPACITY and 'op_download' in err(L)
    assert np.all(out_r == SENT_ROW) and np.all(out_c == SENT_C)
    r, c = download(L, h)
    assert np.array_equal(r, rows) and np.array_equal(c, coeff)
    out_b = np.full((T, 2 * n), 9, dtype=np.uint8)
    assert L.symgpu_op_download_bool(h, n, ptr(out_b), I64(T - 1)) == E_CAPACITY and 'op_download_bool' in err(L)
    assert np.all(out_b == 9)
    ok(L, L.symgpu_op_download_bool(h, n, ptr(out_b), I64(T)))
    assert np.array_equal(out_b.astype(bool), symp) and out_b.max() <= 1
    cleaned = ctypes.c_void_p()
    ok(L, L.symgpu_cleanup_indexed_dev(h, DBL(1e-15), 1, byref(cleaned)))
    first, inverse = onp.first_occurrence_unique(symp.astype(np.uint8))
    sums = np.zeros(first.shape[0], dtype=complex)
    np.add.at(sums, inverse, coeff)
    e_first = first[np.abs(sums) > 1e-15].astype(np.uint64)
    Tc = info(L, cleaned)[0]
    assert Tc == e_first.shape[0] and Tc > 2
    got = np.full(Tc, SENT_ROW, dtype='<u8')
    assert L.symgpu_op_first_index(cleaned, ptr(got), I64(Tc - 1)) == E_CAPACITY and 'op_first_index' in err(L)
    assert np.all(got == SENT_ROW)
    ok(L, L.symgpu_op_first_index(cleaned, ptr(got), I64(Tc)))
    assert np.array_equal(got, e_first)
    er, ec = onp.symplectic_cleanup(symp, coeff, 1e-15)
    r, c = download(L, cleaned)
    assert_op_equal(onp.unpack_rows(r, n), c, er, ec, exact=True)
    free(L, h, cleaned)


# ---------------------------------------------------------------- 2d. refusals decided on the host -----------------------------------
@pytest.fixture(scope='module')
def ops(L):
    """Handles for the refusal cases: a (Wq = 2, coefficients), b (Wq = 2, none), w1 (Wq = 1, coefficients), big1 / big2 (Wq = 1, 65,536
    rows each, so Ni * No = 2^32), wide (Wq = 4,097, no rows).  Their contents never matter: every case is refused before the device."""
    rng = np.random.default_rng(70)
    o = types.SimpleNamespace()
    o.rows2 = onp.pack_rows(rng.random((12, 200)) < 0.4)
    o.c = c128(dyadic(rng, 12))
    o.a = upload(L, o.rows2, o.c)
    o.b = upload(L, o.rows2, None)
    o.w1 = upload(L, onp.pack_rows(rng.random((12, 40)) < 0.4), o.c)
    zeros = np.zeros((65536, 2), dtype='<u8')
    o.big1 = upload(L, zeros, np.zeros(65536, dtype=complex))
    o.big2 = upload(L, zeros, np.zeros(65536, dtype=complex))
    o.wide = ctypes.c_void_p()
    ok(L, L.symgpu_op_alloc(I64(0), 4097, 0, byref(o.wide)))
    o.dev = ctypes.c_void_p()
    ok(L, L.symgpu_dev_alloc(I64(4096), byref(o.dev)))
    yield o
    free(L, o.a, o.b, o.w1, o.big1, o.big2, o.wide)
    ok(L, L.symgpu_dev_free(o.dev))


def refusal_cases():
    """(id, names the call, call(L, o) -> rc).  Every condition is an SG_REQUIRE that its entry point evaluates before it allocates,
    copies or launches anything."""
    R = lambda o: ptr(o.rows2)
    C = lambda o: ptr(o.c)
    buf = np.zeros(4096, dtype=np.uint8)
    B = P(buf.ctypes.data)
    out = ctypes.c_void_p()
    n64, i32 = I64(0), ctypes.c_int(0)
    idx_bad = np.array([0, 12], dtype=np.int64)
    idx_neg = np.array([-1], dtype=np.int64)
    keep_bad = np.array([3, 3], dtype=np.int32)
    keep_ok = np.array([0, 1], dtype=np.int32)
    parts = (ctypes.c_void_p * 1)()
    keepalive = (buf, idx_bad, idx_neg, keep_bad, keep_ok, parts)
    cases = [
        # context.hip
        ('debug_counter/which', 'debug_counter', lambda L, o: L.symgpu_debug_counter(61, byref(n64))),
        ('current_device/null', 'current_device', lambda L, o: L.symgpu_current_device(None)),
        ('n_initialised/null', 'n_initialised', lambda L, o: L.symgpu_n_initialised(None)),
        # alloc.hip
        ('dev_alloc/negative', 'dev_alloc', lambda L, o: L.symgpu_dev_alloc(I64(-1), byref(out))),
        # transfer.hip
        ('dev_upload/null-host', 'dev_upload', lambda L, o: L.symgpu_dev_upload(o.dev, None, I64(16))),
        ('dev_download/negative', 'dev_download', lambda L, o: L.symgpu_dev_download(o.dev, B, I64(-1))),
        # op_handles.hip
        ('op_copy_rows/same-handle', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.a, I64(0), o.a, I64(0), I64(1))),
        ('op_copy_rows/Wq-mismatch', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.a, I64(0), o.w1, I64(0), I64(1))),
        ('op_copy_rows/null-dst', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(None, I64(0), o.a, I64(0), I64(1))),
        ('op_copy_rows/beyond-capacity', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.b, I64(8), o.a, I64(0), I64(5))),
        ('op_copy_rows/beyond-T', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.b, I64(0), o.a, I64(8), I64(5))),
        ('op_copy_rows/negative-count', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.b, I64(0), o.a, I64(0), I64(-1))),
        ('op_copy_rows/negative-offset', 'op_copy_rows', lambda L, o: L.symgpu_op_copy_rows(o.b, I64(-1), o.a, I64(0), I64(1))),
        ('op_write/beyond-capacity', 'op_write', lambda L, o: L.symgpu_op_write(o.a, I64(8), R(o), C(o), I64(5))),
        ('op_write/negative-offset', 'op_write', lambda L, o: L.symgpu_op_write(o.a, I64(-1), R(o), C(o), I64(1))),
        ('op_write/null-rows', 'op_write', lambda L, o: L.symgpu_op_write(o.a, I64(0), None, None, I64(1))),
        ('op_write/null-handle', 'op_write', lambda L, o: L.symgpu_op_write(None, I64(0), R(o), None, I64(1))),
        ('op_set_rows/beyond-capacity', 'op_set_rows', lambda L, o: L.symgpu_op_set_rows(o.a, I64(13))),
        ('op_set_rows/negative', 'op_set_rows', lambda L, o: L.symgpu_op_set_rows(o.a, I64(-1))),
        ('op_upload/Wq-0', 'op_upload', lambda L, o: L.symgpu_op_upload(R(o), None, I64(12), 0, byref(out))),
        ('op_upload/negative-T', 'op_upload', lambda L, o: L.symgpu_op_upload(R(o), None, I64(-1), 2, byref(out))),
        ('op_upload/null-rows', 'op_upload', lambda L, o: L.symgpu_op_upload(None, None, I64(12), 2, byref(out))),
        ('op_upload/null-out', 'op_upload', lambda L, o: L.symgpu_op_upload(R(o), None, I64(12), 2, None)),
        ('op_alloc/Wq-0', 'op_alloc', lambda L, o: L.symgpu_op_alloc(I64(4), 0, 1, byref(out))),
        ('op_alloc/negative-capacity', 'op_alloc', lambda L, o: L.symgpu_op_alloc(I64(-4), 1, 1, byref(out))),
        ('op_upload_bool/n-0', 'op_upload_bool', lambda L, o: L.symgpu_op_upload_bool(B, None, I64(4), 0, byref(out))),
        ('op_upload_bool/null-symp', 'op_upload_bool', lambda L, o: L.symgpu_op_upload_bool(None, None, I64(4), 5, byref(out))),
        ('op_download_bool/n-mismatch', 'op_download_bool', lambda L, o: L.symgpu_op_download_bool(o.a, 40, B, I64(12))),
        ('op_download/null-handle', 'op_download', lambda L, o: L.symgpu_op_download(None, B, None, I64(12))),
        ('op_info/null-handle', 'op_info', lambda L, o: L.symgpu_op_info(None, byref(n64), byref(i32), byref(n64))),
        ('op_clone/null-out', 'op_clone', lambda L, o: L.symgpu_op_clone(o.a, None)),
        ('op_set_coeff/null', 'op_set_coeff', lambda L, o: L.symgpu_op_set_coeff(o.a, None)),
        ('op_scale/no-coefficients', 'op_scale', lambda L, o: L.symgpu_op_scale(o.b, DBL(2.0), DBL(0.0), 0)),
        ('op_ycount/null-out', 'op_ycount', lambda L, o: L.symgpu_op_ycount(o.a, None)),
        ('op_random/density', 'op_random', lambda L, o: L.symgpu_op_random(I64(4), 10, DBL(1.5), U64(1), byref(out))),
        ('op_random/negative-density', 'op_random', lambda L, o: L.symgpu_op_random(I64(4), 10, DBL(-0.1), U64(1), byref(out))),
        ('op_random/n-0', 'op_random', lambda L, o: L.symgpu_op_random(I64(4), 0, DBL(0.5), U64(1), byref(out))),
        # checksum.hip
        ('op_popcount/null-sum', 'op_popcount', lambda L, o: L.symgpu_op_popcount(o.a, None)),
        ('op_checksum/null-handle', 'op_checksum', lambda L, o: L.symgpu_op_checksum(None, B, B)),
        ('op_checksum/too-wide', 'op_checksum', lambda L, o: L.symgpu_op_checksum(o.wide, B, None)),
        # the pointer is inside a live block and is never dereferenced: the alignment is a host-side comparison
        ('dev_checksum_u8/alignment', 'dev_checksum_u8', lambda L, o: L.symgpu_dev_checksum_u8(P(o.dev.value + 1), I64(16), byref(n64))),
        ('dev_checksum_u8/negative-n', 'dev_checksum_u8', lambda L, o: L.symgpu_dev_checksum_u8(o.dev, I64(-1), byref(n64))),
        ('dev_checksum_u8/null-sum', 'dev_checksum_u8', lambda L, o: L.symgpu_dev_checksum_u8(o.dev, I64(16), None)),
        ('dev_popcount_u64/null-sum', 'dev_popcount_u64', lambda L, o: L.symgpu_dev_popcount_u64(o.dev, I64(2), None)),
        # rotate_driver.hip
        ('debug_rotation_trace/null-out', 'debug_rotation_trace', lambda L, o: L.symgpu_debug_rotation_trace(None, 0, byref(i32))),
        # cleanup_driver.hip
        ('cleanup/W-odd', 'cleanup', lambda L, o: L.symgpu_cleanup(R(o), C(o), I64(12), 3, DBL(0.0), 0, B, B, I64(12), byref(n64))),
        ('cleanup/W-0', 'cleanup', lambda L, o: L.symgpu_cleanup(R(o), C(o), I64(12), 0, DBL(0.0), 0, B, B, I64(12), byref(n64))),
        ('cleanup/negative-T', 'cleanup', lambda L, o: L.symgpu_cleanup(R(o), C(o), I64(-1), 4, DBL(0.0), 0, B, B, I64(12), byref(n64))),
        ('cleanup/negative-capacity', 'cleanup', lambda L, o: L.symgpu_cleanup(R(o), C(o), I64(12), 4, DBL(0.0), 0, B, B, I64(-1), byref(n64))),
        ('cleanup/null-coeff', 'cleanup', lambda L, o: L.symgpu_cleanup(R(o), None, I64(12), 4, DBL(0.0), 0, B, B, I64(12), byref(n64))),
        ('mul_cleanup/Wq-0', 'mul_cleanup', lambda L, o: L.symgpu_mul_cleanup(R(o), C(o), I64(12), R(o), C(o), I64(12), 0, 1, DBL(0.0), 1, B, B, I64(144), byref(n64))),
        ('mul_cleanup/negative-Ni', 'mul_cleanup', lambda L, o: L.symgpu_mul_cleanup(R(o), C(o), I64(-1), R(o), C(o), I64(12), 2, 1, DBL(0.0), 1, B, B, I64(144), byref(n64))),
        ('mul_cleanup/null-outer', 'mul_cleanup', lambda L, o: L.symgpu_mul_cleanup(R(o), C(o), I64(12), None, C(o), I64(12), 2, 1, DBL(0.0), 1, B, B, I64(144), byref(n64))),
        ('mul_cleanup_dev/Wq-mismatch', 'mul_cleanup_dev', lambda L, o: L.symgpu_mul_cleanup_dev(o.a, o.w1, 1, DBL(0.0), 1, byref(out))),
        ('mul_cleanup_dev/no-coefficients', 'mul_cleanup_dev', lambda L, o: L.symgpu_mul_cleanup_dev(o.a, o.b, 1, DBL(0.0), 1, byref(out))),
        ('mul_cleanup_dev/2^32-pairs', 'mul_cleanup_dev', lambda L, o: L.symgpu_mul_cleanup_dev(o.big1, o.big2, 1, DBL(0.0), 1, byref(out))),
        ('mul_cleanup_dev/null-out', 'mul_cleanup_dev', lambda L, o: L.symgpu_mul_cleanup_dev(o.a, o.a, 1, DBL(0.0), 1, None)),
        ('mul_cleanup_indexed_dev/Wq-mismatch', 'mul_cleanup_indexed_dev', lambda L, o: L.symgpu_mul_cleanup_indexed_dev(o.a, o.w1, 1, DBL(0.0), 1, byref(out))),
        ('mul_cleanup_indexed_dev/2^32-pairs', 'mul_cleanup_indexed_dev', lambda L, o: L.symgpu_mul_cleanup_indexed_dev(o.big1, o.big2, 1, DBL(0.0), 1, byref(out))),
        ('cleanup_dev/no-coefficients', 'cleanup_dev', lambda L, o: L.symgpu_cleanup_dev(o.b, DBL(0.0), 1, byref(out))),
        ('cleanup_dev/null-out', 'cleanup_dev', lambda L, o: L.symgpu_cleanup_dev(o.a, DBL(0.0), 1, None)),
        ('cleanup_indexed_dev/no-coefficients', 'cleanup_indexed_dev', lambda L, o: L.symgpu_cleanup_indexed_dev(o.b, DBL(0.0), 1, byref(out))),
        ('op_first_index/not-indexed', 'op_first_index', lambda L, o: L.symgpu_op_first_index(o.a, B, I64(12))),
        ('op_first_index/null', 'op_first_index', lambda L, o: L.symgpu_op_first_index(o.a, None, I64(12))),
        # rotate_driver.hip
        ('rotate_single/Wq-0', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), C(o), I64(12), 0, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), byref(n64), byref(i32))),
        ('rotate_single/negative-N', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), C(o), I64(-1), 2, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), byref(n64), byref(i32))),
        ('rotate_single/null-q', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), C(o), I64(12), 2, None, DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), byref(n64), byref(i32))),
        ('rotate_single/null-n_out', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), C(o), I64(12), 2, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), None, byref(i32))),
        ('rotate_single/null-all_commute', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), C(o), I64(12), 2, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), byref(n64), None)),
        ('rotate_single/null-coeff', 'rotate_single', lambda L, o: L.symgpu_rotate_single(R(o), None, I64(12), 2, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), B, B, I64(24), byref(n64), byref(i32))),
        ('rotate_single_dev/null-q', 'rotate_single_dev', lambda L, o: L.symgpu_rotate_single_dev(o.a, None, DBL(0.0), DBL(0.0), 1, DBL(0.0), byref(out), byref(i32))),
        ('rotate_single_dev/no-coefficients', 'rotate_single_dev', lambda L, o: L.symgpu_rotate_single_dev(o.b, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), byref(out), byref(i32))),
        ('rotate_single_dev_n/null-n_out', 'rotate_single_dev_n', lambda L, o: L.symgpu_rotate_single_dev_n(o.a, R(o), DBL(0.0), DBL(0.0), 1, DBL(0.0), byref(out), byref(i32), None)),
        ('rotate_clifford_chain_dev/not-clean', 'rotate_clifford_chain_dev', lambda L, o: L.symgpu_rotate_clifford_chain_dev(o.a, R(o), ptr(keep_ok), I64(2), byref(out))),
        ('rotate_clifford_chain_dev/null-ks', 'rotate_clifford_chain_dev', lambda L, o: L.symgpu_rotate_clifford_chain_dev(o.a, R(o), None, I64(2), byref(out))),
        ('perform_rotations_dev/null-out', 'perform_rotations_dev', lambda L, o: L.symgpu_perform_rotations_dev(o.a, R(o), B, B, ptr(keep_ok), I64(1), DBL(1e-15), 0, None, None, byref(n64), byref(i32))),
        # ycount.hip
        ('ycount/Wq-0', 'ycount', lambda L, o: L.symgpu_ycount(R(o), I64(12), 0, B)),
        ('ycount/null-out', 'ycount', lambda L, o: L.symgpu_ycount(R(o), I64(12), 2, None)),
        # commute_driver.hip
        ('commutes/Wq-0', 'commutes', lambda L, o: L.symgpu_commutes(R(o), I64(12), R(o), I64(12), 0, B)),
        ('commutes/negative-M', 'commutes', lambda L, o: L.symgpu_commutes(R(o), I64(12), R(o), I64(-1), 2, B)),
        ('commutes/null-out', 'commutes', lambda L, o: L.symgpu_commutes(R(o), I64(12), R(o), I64(12), 2, None)),
        ('commutes_dev/Wq-mismatch', 'commutes_dev', lambda L, o: L.symgpu_commutes_dev(o.a, I64(0), I64(12), o.w1, o.dev)),
        ('commutes_dev/row-range', 'commutes_dev', lambda L, o: L.symgpu_commutes_dev(o.a, I64(0), I64(13), o.b, o.dev)),
        ('commutes_dev/reversed-range', 'commutes_dev', lambda L, o: L.symgpu_commutes_dev(o.a, I64(5), I64(4), o.b, o.dev)),
        ('commutes_dev/null-out', 'commutes_dev', lambda L, o: L.symgpu_commutes_dev(o.a, I64(0), I64(12), o.b, None)),
        ('commutes_bits_dev/Wq-mismatch', 'commutes_bits_dev', lambda L, o: L.symgpu_commutes_bits_dev(o.a, I64(0), I64(12), o.w1, o.dev)),
        ('commutes_bits_dev/row-range', 'commutes_bits_dev', lambda L, o: L.symgpu_commutes_bits_dev(o.a, I64(-1), I64(12), o.b, o.dev)),
        # product.hip
        ('mul_allpairs/Wq-0', 'mul_allpairs', lambda L, o: L.symgpu_mul_allpairs(R(o), C(o), I64(12), R(o), C(o), I64(12), 0, 1, B, B)),
        ('mul_allpairs/null-out', 'mul_allpairs', lambda L, o: L.symgpu_mul_allpairs(R(o), C(o), I64(12), R(o), C(o), I64(12), 2, 1, None, B)),
        ('mul_allpairs_dev/Wq-mismatch', 'mul_allpairs_dev', lambda L, o: L.symgpu_mul_allpairs_dev(o.a, o.a, I64(0), I64(1), 1, o.w1)),
        ('mul_allpairs_dev/outer-range', 'mul_allpairs_dev', lambda L, o: L.symgpu_mul_allpairs_dev(o.a, o.a, I64(0), I64(13), 1, o.b)),
        ('mul_allpairs_dev/null-out', 'mul_allpairs_dev', lambda L, o: L.symgpu_mul_allpairs_dev(o.a, o.a, I64(0), I64(1), 1, None)),
        # the rows would be read out of the buffer being written (and the handle's caches are dropped first): refused before anything is touched
        ('mul_allpairs_dev/out-is-inner', 'mul_allpairs_dev', lambda L, o: L.symgpu_mul_allpairs_dev(o.a, o.b, I64(0), I64(1), 1, o.a)),
        ('mul_allpairs_dev/out-is-outer', 'mul_allpairs_dev', lambda L, o: L.symgpu_mul_allpairs_dev(o.b, o.a, I64(0), I64(1), 1, o.a)),
        # gf2_driver.hip
        ('rref/negative-R', 'rref', lambda L, o: L.symgpu_rref(R(o), I64(-1), I64(4), None, None)),
        ('rref/null-rows', 'rref', lambda L, o: L.symgpu_rref(None, I64(12), I64(4), None, None)),
        ('rref_dev/negative-Wc', 'rref_dev', lambda L, o: L.symgpu_rref_dev(o.dev, I64(4), I64(-1), None, None)),
        ('rref_dev/null-rows', 'rref_dev', lambda L, o: L.symgpu_rref_dev(None, I64(4), I64(4), None, None)),
        # gf2_symmetry.hip
        ('symmetry_kernel/n-does-not-match-Wq', 'symmetry_kernel', lambda L, o: L.symgpu_symmetry_kernel(R(o), I64(12), 100, 1, B, I64(8), byref(n64), None)),
        ('symmetry_kernel/null-k', 'symmetry_kernel', lambda L, o: L.symgpu_symmetry_kernel(R(o), I64(12), 100, 2, B, I64(8), None, None)),
        ('symmetry_kernel/null-H', 'symmetry_kernel', lambda L, o: L.symgpu_symmetry_kernel(None, I64(12), 100, 2, B, I64(8), byref(n64), None)),
        ('symmetry_kernel/negative-M', 'symmetry_kernel', lambda L, o: L.symgpu_symmetry_kernel(R(o), I64(-1), 100, 2, B, I64(8), byref(n64), None)),
        ('symmetry_kernel_dev/n-does-not-match-Wq', 'symmetry_kernel_dev', lambda L, o: L.symgpu_symmetry_kernel_dev(o.a, 40, B, I64(8), byref(n64), None)),
        ('symmetry_kernel_dev/null-k', 'symmetry_kernel_dev', lambda L, o: L.symgpu_symmetry_kernel_dev(o.a, 100, B, I64(8), None, None)),
        # partition.hip
        ('op_gather/index-beyond-T', 'op_gather', lambda L, o: L.symgpu_op_gather(o.a, ptr(idx_bad), I64(2), byref(out))),
        ('op_gather/negative-index', 'op_gather', lambda L, o: L.symgpu_op_gather(o.a, ptr(idx_neg), I64(1), byref(out))),
        ('op_gather/null-indices', 'op_gather', lambda L, o: L.symgpu_op_gather(o.a, None, I64(1), byref(out))),
        ('op_gather/negative-n', 'op_gather', lambda L, o: L.symgpu_op_gather(o.a, ptr(idx_bad), I64(-1), byref(out))),
        ('part_global_index/not-indexed', 'part_global_index', lambda L, o: L.symgpu_part_global_index(o.a, ptr(idx_bad), I64(2), ptr(idx_bad), I64(2), I64(12))),
        ('part_global_index/no-inner', 'part_global_index', lambda L, o: L.symgpu_part_global_index(o.a, ptr(idx_bad), I64(0), ptr(idx_bad), I64(2), I64(12))),
        ('op_set_first_index/null', 'op_set_first_index', lambda L, o: L.symgpu_op_set_first_index(o.a, None)),
        ('merge_indexed_dev/no-parts', 'merge_indexed_dev', lambda L, o: L.symgpu_merge_indexed_dev(ctypes.cast(parts, P), 0, 0, 1, DBL(0.0), 1, byref(out))),
        ('merge_indexed_dev/key-bits', 'merge_indexed_dev', lambda L, o: L.symgpu_merge_indexed_dev(ctypes.cast(parts, P), 1, 65, 1, DBL(0.0), 1, byref(out))),
        ('merge_indexed_dev/null-parts', 'merge_indexed_dev', lambda L, o: L.symgpu_merge_indexed_dev(None, 1, 0, 1, DBL(0.0), 1, byref(out))),
        # genrec.hip
        ('op_gf2_rank/null-rank', 'op_gf2_rank', lambda L, o: L.symgpu_op_gf2_rank(o.a, None)),
        ('generators_dev/null-out', 'generators_dev', lambda L, o: L.symgpu_generators_dev(o.a, None)),
        ('generator_reconstruction_dev/Wq-mismatch', 'generator_reconstruction_dev', lambda L, o: L.symgpu_generator_reconstruction_dev(o.a, o.w1, 100, B, B)),
        ('generator_reconstruction_dev/n-mismatch', 'generator_reconstruction_dev', lambda L, o: L.symgpu_generator_reconstruction_dev(o.a, o.b, 40, B, B)),
        ('generator_reconstruction_dev/null-recon', 'generator_reconstruction_dev', lambda L, o: L.symgpu_generator_reconstruction_dev(o.a, o.b, 100, None, B)),
        ('generator_reconstruction_dev/too-many-generators', 'generator_reconstruction_dev', lambda L, o: L.symgpu_generator_reconstruction_dev(o.big1, o.big2, 1, B, B)),
        # project.hip
        ('project_dev/n-mismatch', 'project_dev', lambda L, o: L.symgpu_project_dev(o.a, R(o), 1, R(o), ptr(keep_ok), 2, 40, DBL(0.0), 1, byref(out), None)),
        ('project_dev/no-keep', 'project_dev', lambda L, o: L.symgpu_project_dev(o.a, R(o), 1, R(o), ptr(keep_ok), 0, 100, DBL(0.0), 1, byref(out), None)),
        ('project_dev/no-coefficients', 'project_dev', lambda L, o: L.symgpu_project_dev(o.b, R(o), 1, R(o), ptr(keep_ok), 2, 100, DBL(0.0), 1, byref(out), None)),
        ('project_dev/keep-not-ascending', 'project_dev', lambda L, o: L.symgpu_project_dev(o.a, R(o), 1, R(o), ptr(keep_bad), 2, 100, DBL(0.0), 1, byref(out), None)),
        ('noncontextual_dev/null-flag', 'noncontextual_dev', lambda L, o: L.symgpu_noncontextual_dev(o.a, None)),
        ('state_inner_dev/Wq-mismatch', 'state_inner_dev', lambda L, o: L.symgpu_state_inner_dev(o.a, o.w1, B)),
        ('state_inner_dev/not-clean', 'state_inner_dev', lambda L, o: L.symgpu_state_inner_dev(o.a, o.a, B)),
        # sparse_matrix.hip
        ('to_csr_count/Wq-2', 'to_csr_count', lambda L, o: L.symgpu_to_csr_count(o.a, 20, byref(n64), byref(n64), byref(out))),
        ('to_csr_count/32-qubits', 'to_csr_count', lambda L, o: L.symgpu_to_csr_count(o.w1, 32, byref(n64), byref(n64), byref(out))),
        ('to_csr_fill/null-plan', 'to_csr_fill', lambda L, o: L.symgpu_to_csr_fill(None, None, None, None, 4)),
    ]
    return [pytest.param(name, fn, keepalive, id=cid) for cid, name, fn in cases]


@pytest.mark.parametrize('name,call,keepalive', refusal_cases())
def test_refusal(L, ops, name, call, keepalive):
    L.symgpu_op_set_rows(ops.a, I64(12))                                  # a valid call in between: the error text below is this refusal's
    rc = call(L, ops)
    assert rc == E_INVALID, (rc, err(L))
    assert name + ':' in err(L) or name + ' ' in err(L) or f'{name} (' in err(L), err(L)
    assert info(L, ops.a) == (12, 2, 12) and info(L, ops.b) == (12, 2, 12)
    sanity(L)
    r, c = download(L, ops.a)
    assert np.array_equal(r, ops.rows2) and np.array_equal(c, ops.c)


def test_context_queries(L):
    d, n, cnt = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    ok(L, L.symgpu_current_device(byref(d)))
    ok(L, L.symgpu_n_initialised(byref(n)))
    ok(L, L.symgpu_device_count(byref(cnt)))
    assert d.value == 0 and 1 <= n.value <= cnt.value
    buf = ctypes.create_string_buffer(256)
    ok(L, L.symgpu_device_name(buf, 256))
    assert b'gfx950' in buf.value
    ok(L, L.symgpu_set_device(0))
    ok(L, L.symgpu_sync())
    ok(L, L.symgpu_device_sync())
    free_b, total_b = I64(-1), I64(-1)
    ok(L, L.symgpu_mem_info(byref(free_b), byref(total_b)))
    assert 0 < free_b.value <= total_b.value
    ok(L, L.symgpu_degraded(buf, 256))
    assert L.symgpu_device_name(None, 256) == E_INVALID and L.symgpu_degraded(buf, 0) == E_INVALID
    assert L.symgpu_set_device(-1) == E_INVALID and 'device -1' in err(L)
    ok(L, L.symgpu_current_device(byref(d)))
    assert d.value == 0
    sanity(L)


# ---------------------------------------------------------------- 2e. handle primitives against NumPy mirrors ------------------------
class Mirror:
    """A handle and the NumPy arrays it must hold: rows[capacity], coeff[capacity] (or None), T.  `known` marks the coefficient rows
    whose value the ABI defines (a copy between an operator with and one without coefficients leaves the copied range undefined)."""

    def __init__(self, L, capacity, Wq, with_coeff):
        self.L, self.Wq, self.cap, self.T = L, Wq, capacity, 0
        self.h = ctypes.c_void_p()
        ok(L, L.symgpu_op_alloc(I64(capacity), Wq, int(with_coeff), byref(self.h)))
        self.rows = np.zeros((capacity, 2 * Wq), dtype='<u8')
        self.rows_known = np.zeros(capacity, dtype=bool)
        self.coeff = np.zeros(capacity, dtype=complex) if with_coeff else None
        self.known = np.zeros(capacity, dtype=bool)

    def check(self):
        L = self.L
        assert info(L, self.h) == (self.T, self.Wq, self.cap)
        rows = np.full((self.T, 2 * self.Wq), SENT_ROW, dtype='<u8')
        c = np.full(self.T, SENT_C) if self.coeff is not None else None
        ok(L, L.symgpu_op_download(self.h, ptr(rows), ptr(c), I64(self.T)))
        k = self.rows_known[:self.T]
        assert np.array_equal(rows[k], self.rows[:self.T][k])
        if c is not None:
            k = self.known[:self.T]
            assert np.array_equal(c[k], self.coeff[:self.T][k])

    def write(self, off, rows, coeff):
        rows = np.ascontiguousarray(rows, dtype='<u8')
        c = None if coeff is None else c128(coeff)
        ok(self.L, self.L.symgpu_op_write(self.h, I64(off), ptr(rows), ptr(c), I64(len(rows))))
        self.rows[off:off + len(rows)] = rows
        self.rows_known[off:off + len(rows)] = True
        if c is not None and self.coeff is not None:
            self.coeff[off:off + len(rows)] = c
            self.known[off:off + len(rows)] = True
        self.T = max(self.T, off + len(rows))
        self.check()

    def set_rows(self, T):
        ok(self.L, self.L.symgpu_op_set_rows(self.h, I64(T)))
        self.T = T
        self.check()

    def copy_from(self, dst_off, src, src_off, count):
        ok(self.L, self.L.symgpu_op_copy_rows(self.h, I64(dst_off), src.h, I64(src_off), I64(count)))
        self.rows[dst_off:dst_off + count] = src.rows[src_off:src_off + count]
        self.rows_known[dst_off:dst_off + count] = src.rows_known[src_off:src_off + count]
        if self.coeff is not None:
            if src.coeff is not None:
                self.coeff[dst_off:dst_off + count] = src.coeff[src_off:src_off + count]
                self.known[dst_off:dst_off + count] = src.known[src_off:src_off + count]
            else:
                self.known[dst_off:dst_off + count] = False             # "if both have them": not asserted
        self.T = max(self.T, dst_off + count)
        self.check()
        src.check()

    def free(self):
        free(self.L, self.h)


def test_alloc_write_set_rows_copy_rows_against_mirrors(L):
    rng = np.random.default_rng(80)
    cap, Wq = 40, 2
    data = lambda t: (rng.integers(0, 1 << 63, (t, 2 * Wq), dtype=np.uint64), dyadic(rng, t))
    for with_coeff in (True, False):
        m = Mirror(L, cap, Wq, with_coeff)
        m.check()                                                        # a fresh handle holds no row
        r, c = data(7)
        m.write(15, r, c)                                                # middle: T grows to 22
        assert m.T == 22
        r, c = data(5)
        m.write(0, r, None)                                              # offset 0, no coefficient argument: T stays
        assert m.T == 22
        r, c = data(6)
        m.write(cap - 6, r, c)                                           # the last rows of the capacity
        assert m.T == cap
        r, c = data(3)
        m.write(4, r, c)                                                 # never shrinks
        assert m.T == cap
        m.write(9, r[:0], c[:0])                                         # nothing
        m.set_rows(10)
        m.set_rows(cap)
        m.set_rows(0)
        m.set_rows(21)
        m.free()
    # copies with non-zero offsets on both sides, between operators with and without coefficients
    a, b, nc = Mirror(L, cap, Wq, True), Mirror(L, 30, Wq, True), Mirror(L, 30, Wq, False)
    for m, t in ((a, 35), (b, 30), (nc, 30)):
        r, c = data(t)
        m.write(0, r, c)
    b.copy_from(3, a, 11, 9)
    b.copy_from(20, a, 0, 10)                                            # up to the capacity
    b.copy_from(5, a, 7, 0)                                              # count = 0
    b.copy_from(8, nc, 2, 6)                                             # source without coefficients: rows move, coefficients outside the range stay
    assert b.known.sum() == 24
    nc.copy_from(4, a, 20, 12)                                           # the reverse: rows only
    nc.set_rows(12)
    nc.copy_from(14, a, 1, 3)                                            # beyond T, inside the capacity: T grows to 17
    assert nc.T == 17
    for m in (a, b, nc):
        m.free()


def test_clone_is_independent(L):
    rng = np.random.default_rng(81)
    rows, c = onp.pack_rows(rng.random((50, 260)) < 0.3), dyadic(rng, 50)
    for coeff in (c, None):
        h = upload(L, rows, coeff)
        k = ctypes.c_void_p()
        ok(L, L.symgpu_op_clone(h, byref(k)))
        assert info(L, k)[:2] == (50, 3)
        other, doubled = np.ascontiguousarray(rows[::-1][:20]), c128(c[:20] * 2)
        ok(L, L.symgpu_op_write(h, I64(5), ptr(other), ptr(doubled) if coeff is not None else None, I64(20)))
        r2, c2 = download(L, k, coeff is not None)
        assert np.array_equal(r2, rows) and (coeff is None or np.array_equal(c2, c))
        if coeff is not None:
            ok(L, L.symgpu_op_scale(k, DBL(0.0), DBL(1.0), 0))
            r1, c1 = download(L, h)
            exp_c = c.copy(); exp_c[5:25] = c[:20] * 2
            exp_r = rows.copy(); exp_r[5:25] = other
            assert np.array_equal(r1, exp_r) and np.array_equal(c1, exp_c)
        free(L, h, k)
    e = upload(L, rows[:0], c[:0])
    k = ctypes.c_void_p()
    ok(L, L.symgpu_op_clone(e, byref(k)))
    assert info(L, k)[0] == 0
    free(L, e, k)


def test_set_coeff_allocates_and_replaces(L):
    rng = np.random.default_rng(82)
    rows = onp.pack_rows(rng.random((300, 100)) < 0.3)
    c1, c2 = c128(rng.standard_normal(300) + 1j * rng.standard_normal(300)), c128(dyadic(rng, 300))
    h = upload(L, rows, None)                                            # no coefficients: set_coeff allocates them
    assert L.symgpu_op_scale(h, DBL(1.0), DBL(0.0), 0) == E_INVALID
    ok(L, L.symgpu_op_set_coeff(h, ptr(c1)))
    r, c = download(L, h)
    assert np.array_equal(r, rows) and np.array_equal(c, c1)
    ok(L, L.symgpu_op_set_coeff(h, ptr(c2)))                             # has them: replaced
    r, c = download(L, h)
    assert np.array_equal(r, rows) and np.array_equal(c, c2)
    cleaned = ctypes.c_void_p()                                          # and they are real coefficients to the kernels
    ok(L, L.symgpu_cleanup_dev(h, DBL(1e-15), 1, byref(cleaned)))
    er, ec = onp.symplectic_cleanup(onp.unpack_rows(rows, 50), c2, 1e-15)
    r, c = download(L, cleaned)
    assert_op_equal(onp.unpack_rows(r, 50), c, er, ec, exact=True)
    free(L, h, cleaned)
    # an operator allocated with spare capacity and no coefficients: the new array covers the capacity
    m = Mirror(L, 20, 1, False)
    m.write(0, rows[:8, :2], None)
    ok(L, L.symgpu_op_set_coeff(m.h, ptr(c1)))
    m.coeff = np.zeros(20, dtype=complex); m.coeff[:8] = c1[:8]; m.known[:8] = True
    m.check()
    m.write(8, rows[8:20, :2], c2[8:20])
    assert m.T == 20
    m.free()


def plain_product(c, s, conjugate_first):
    """(conj?(c)) * s with NumPy's complex128 SCALAR multiply: every partial product and the sum rounded once (no FMA) — and the
    same thing spelled out in float64 array arithmetic.  The two must agree, or this host contracts where it should not."""
    c = np.conj(c) if conjugate_first else c
    s = np.complex128(s)
    with np.errstate(all='ignore'):
        scalar = np.array([ci * s for ci in c], dtype=np.complex128)
        re = c.real * s.real - c.imag * s.imag
        im = c.real * s.imag + c.imag * s.real
    spelled = np.empty(len(c), dtype=np.complex128)
    spelled.real, spelled.imag = re, im
    assert same_bits(scalar, spelled)
    return scalar


def same_bits(a, b):
    """Equal as numbers with NaNs in the same places, and the same sign bit wherever the value is not a NaN."""
    a, b = c128(a).view(np.float64), c128(b).view(np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    num = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[num]), np.signbit(b[num])))


@pytest.mark.parametrize('T', [1, 255, 256, 257, 3000])
def test_scale_is_the_plain_ieee_product(L, T):
    rng = np.random.default_rng(830 + T)
    rows = onp.pack_rows(rng.random((T, 10)) < 0.5)
    c = c128(rng.standard_normal(T) + 1j * rng.standard_normal(T))
    for s, conj in ((0.37 - 1.21j, 0), (0.37 - 1.21j, 1), (-2.5 + 0j, 0), (1j, 1), (rng.standard_normal() + 1j * rng.standard_normal(), 1)):
        h = upload(L, rows, c)
        ok(L, L.symgpu_op_scale(h, DBL(s.real), DBL(s.imag), conj))
        r, got = download(L, h)
        free(L, h)
        assert np.array_equal(r, rows)
        exp = plain_product(c, s, conj)
        assert same_bits(got, exp), (T, s, conj, int(np.sum(got.view(np.float64) != exp.view(np.float64))))
        assert np.allclose(got, (np.conj(c) if conj else c) * s, rtol=0, atol=TOL)     # NumPy's (contracting) array multiply: the project's bar


def test_scale_with_non_finite_and_signed_zero_coefficients(L):
    z = np.load(f'{GOLDEN}/coeff_edges.npz')
    pool = np.concatenate([z[k] for k in z.files if k.endswith('/in_coeff')])
    special = pool[~np.isfinite(pool.view(np.float64).reshape(-1, 2)).all(axis=1)]
    zeros = np.array([complex(0.0, -0.0), complex(-0.0, 0.0), complex(-0.0, -0.0), complex(0.0, 0.0), complex(-0.0, 1.5), complex(2.0, -0.0)])
    c = c128(np.concatenate([special, zeros, pool[:200]]))
    assert np.isnan(c.view(np.float64)).any() and np.isinf(c.view(np.float64)).any()
    rows = np.zeros((len(c), 2), dtype='<u8')
    for s, conj in ((0.5 + 0.25j, 0), (0.5 + 0.25j, 1), (-1 + 0j, 0), (0 - 1j, 1), (complex(0.0, -0.0), 0), (1 + 0j, 1)):
        h = upload(L, rows, c)
        ok(L, L.symgpu_op_scale(h, DBL(s.real), DBL(s.imag), conj))
        _, got = download(L, h)
        free(L, h)
        assert same_bits(got, plain_product(c, s, conj)), (s, conj)
    e = upload(L, rows[:0], c[:0])
    ok(L, L.symgpu_op_scale(e, DBL(2.0), DBL(0.0), 1))
    free(L, e)


def test_gather(L):
    rng = np.random.default_rng(84)
    rows, c = onp.pack_rows(rng.random((70, 130)) < 0.3), dyadic(rng, 70)
    for coeff in (c, None):
        h = upload(L, rows, coeff)
        for idx in (np.array([5, 5, 5, 0, 69, 5]), np.arange(69, -1, -1), np.arange(0), rng.integers(0, 70, 500)):
            idx = np.ascontiguousarray(idx, dtype=np.int64)
            g = ctypes.c_void_p()
            ok(L, L.symgpu_op_gather(h, ptr(idx) if len(idx) else None, I64(len(idx)), byref(g)))
            assert info(L, g)[:2] == (len(idx), 2)
            r, cc = download(L, g, coeff is not None)
            assert np.array_equal(r, rows[idx]) and (coeff is None or np.array_equal(cc, c[idx]))
            free(L, g)
        free(L, h)


def upload_bool(L, symp, coeff, n):
    symp = np.ascontiguousarray(symp, dtype=np.uint8)
    c = None if coeff is None else c128(coeff)
    h = ctypes.c_void_p()
    ok(L, L.symgpu_op_upload_bool(ptr(symp) if symp.size else None, ptr(c), I64(symp.shape[0]), n, byref(h)))
    return h


def test_upload_bool_download_bool(L):
    rng = np.random.default_rng(85)
    for n, T in ((1, 3), (63, 70), (64, 70), (65, 70), (130, 257), (1000, 40)):
        symp = rng.random((T, 2 * n)) < 0.5
        symp[0] = True
        c = dyadic(rng, T)
        for coeff in (c, None):
            h = upload_bool(L, symp, coeff, n)
            r, cc = download(L, h, coeff is not None)
            assert np.array_equal(r, onp.pack_rows(symp)) and (coeff is None or np.array_equal(cc, c))
            out = np.full((T, 2 * n), 9, dtype=np.uint8)
            ok(L, L.symgpu_op_download_bool(h, n, ptr(out), I64(T)))
            assert np.array_equal(out, symp.astype(np.uint8))
            free(L, h)
    # bytes other than 0 / 1 are true
    loud = np.array([[0, 255, 2, 0, 1, 128]], dtype=np.uint8)
    h = upload_bool(L, loud, None, 3)
    assert np.array_equal(download(L, h, False)[0], onp.pack_rows(loud != 0))
    free(L, h)
    e = upload_bool(L, np.zeros((0, 20), dtype=np.uint8), None, 10)
    assert info(L, e) == (0, 1, 0)
    ok(L, L.symgpu_op_download_bool(e, 10, None, I64(0)))
    free(L, e)


def test_upload_bool_beyond_one_pass_of_the_grid(L):
    """k_pack_bool / k_unpack_bool take 4 words per workgroup and cap the grid at 65536 * 16 workgroups: above 4 * 65536 * 16 words
    the grid-stride loop runs again.  n = 1, so the rows are 2 words and the buffers stay small (4.4 MB of bools, 35 MB packed)."""
    T = 2_200_000
    assert T * 2 > 4 * 65536 * 16
    rng = np.random.default_rng(86)
    symp = rng.integers(0, 2, (T, 2), dtype=np.uint8)
    h = upload_bool(L, symp, None, 1)
    r, _ = download(L, h, False)
    assert r.shape == (T, 2) and np.array_equal(r, symp.astype('<u8'))
    out = np.full((T, 2), 9, dtype=np.uint8)
    ok(L, L.symgpu_op_download_bool(h, 1, ptr(out), I64(T)))
    assert np.array_equal(out, symp)
    free(L, h)


@pytest.mark.parametrize('Wq', [1, 2, 16])
def test_ycount(L, Wq):
    rng = np.random.default_rng(87 + Wq)
    n = 64 * Wq - (0 if Wq == 2 else 3)
    for T in (1, 65, 1000):
        symp = rng.random((T, 2 * n)) < 0.5
        rows = onp.pack_rows(symp)
        assert rows.shape[1] == 2 * Wq
        expect = onp.y_count(symp).astype(np.int64)
        got = np.full(T, -1, dtype=np.int64)
        ok(L, L.symgpu_ycount(ptr(rows), I64(T), Wq, ptr(got)))
        assert np.array_equal(got, expect)
        h = upload(L, rows, None)
        got = np.full(T, -1, dtype=np.int64)
        ok(L, L.symgpu_op_ycount(h, ptr(got)))
        assert np.array_equal(got, expect)
        free(L, h)
    ok(L, L.symgpu_ycount(None, I64(0), Wq, None))


# ---------------------------------------------------------------- 2f. the instruments ------------------------------------------------
def checksum(L, h, W, want_xor=True, want_sum=True):
    x = np.full(W, SENT_ROW, dtype='<u8') if want_xor else None
    s = np.full(2, -123.0) if want_sum else None
    ok(L, L.symgpu_op_checksum(h, ptr(x), ptr(s)))
    return x, s


@pytest.mark.parametrize('W', [2, 4, 6, 32])
def test_op_checksum(L, W):
    rng = np.random.default_rng(900 + W)
    wrap = 1024 * 256 // W + 1001                                        # rows * words above the grid: the grid-stride loop wraps
    for T in (0, 1, 63, 64, 65, 255, 257, wrap):
        rows = rng.integers(0, 1 << 63, (T, W), dtype=np.uint64) | (rng.integers(0, 2, (T, W), dtype=np.uint64) << np.uint64(63))
        c = c128(dyadic(rng, T))
        e_xor = np.bitwise_xor.reduce(rows, axis=0) if T else np.zeros(W, dtype=np.uint64)
        h = upload(L, rows, c)
        x, s = checksum(L, h, W)
        assert np.array_equal(x, e_xor), T
        assert complex(s[0], s[1]) == c.sum(), T                         # dyadic: exact in any order
        x, s = checksum(L, h, W, want_sum=False)
        assert np.array_equal(x, e_xor) and s is None
        x, s = checksum(L, h, W, want_xor=False)
        assert x is None and complex(s[0], s[1]) == c.sum()
        free(L, h)
        h = upload(L, rows, None)                                        # no coefficients: a zero sum
        x, s = checksum(L, h, W)
        assert np.array_equal(x, e_xor) and s[0] == 0 and s[1] == 0
        free(L, h)


def test_op_checksum_at_the_widest_row_it_is_defined_for(L):
    W = 8192                                                             # 64 KiB of LDS: the header's limit
    rng = np.random.default_rng(91)
    rows = rng.integers(0, 1 << 63, (3, W), dtype=np.uint64)
    h = upload(L, rows, None)
    x, _ = checksum(L, h, W, want_sum=False)
    assert np.array_equal(x, np.bitwise_xor.reduce(rows, axis=0))
    free(L, h)


SIZES = (0, 1, 15, 16, 17, 4095, 4096 + 5, 2048 * 256 * 16 + 16 * 777 + 13)


@pytest.mark.parametrize('n', SIZES)
def test_dev_checksum_u8(L, n):
    rng = np.random.default_rng(920 + n % 1000)
    arr = (rng.random(n) < 0.4).astype(np.uint8)
    if n:
        arr[-1] = 1
        arr[n - 1 - (n - 1) % 16:] = 1                                   # the whole ragged tail counts
    d = dev_buffer(L, arr)
    got = U64(12345)
    ok(L, L.symgpu_dev_checksum_u8(d, I64(n), byref(got)))
    ok(L, L.symgpu_dev_free(d))
    assert got.value == int(arr.sum(dtype=np.uint64))


@pytest.mark.parametrize('n', [0, 1, 15, 16, 17, 4095, 4096 + 5, 2048 * 256 + 64 * 777 + 13])
def test_popcounts(L, n):
    rng = np.random.default_rng(940 + n % 1000)
    words = rng.integers(0, 1 << 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    if n:
        words[-1] |= np.uint64(1) << np.uint64(63)
        words[0] |= np.uint64(1) << np.uint64(63)
    expect = int(np.unpackbits(words.view(np.uint8)).sum(dtype=np.uint64))
    d = dev_buffer(L, words)
    got = U64(12345)
    ok(L, L.symgpu_dev_popcount_u64(d, I64(n), byref(got)))
    ok(L, L.symgpu_dev_free(d))
    assert got.value == expect
    for W in (2, 6):                                                     # the same words as an operator's rows
        T = n // W
        h = upload(L, words[:T * W].reshape(T, W), None)
        got = U64(12345)
        ok(L, L.symgpu_op_popcount(h, byref(got)))
        free(L, h)
        assert got.value == int(np.unpackbits(words[:T * W].view(np.uint8)).sum(dtype=np.uint64))


def random_op(L, T, n, density, seed):
    h = ctypes.c_void_p()
    ok(L, L.symgpu_op_random(I64(T), n, DBL(density), U64(seed), byref(h)))
    rows, c = download(L, h)
    free(L, h)
    return rows, c


def bits_of(rows, n):
    """bool[T, 2n] of packed rows, and True iff every padding bit is zero (judged on the words, not through an unpack that drops them)."""
    wq = rows.shape[1] // 2
    full = np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder='little').reshape(rows.shape[0], 2, wq * 64)
    return np.concatenate([full[:, 0, :n], full[:, 1, :n]], axis=1).astype(bool), not full[:, :, n:].any()


def test_bernoulli_bounds_hold_for_a_true_source():
    """The 6-sigma bands below, on NumPy's generator (no device): a true Bernoulli source stays inside them."""
    rng = np.random.default_rng(2024)
    n, T, p = 1000, 20000, 0.3
    bits = rng.random((T, 2 * n)) < p
    check_bernoulli(bits, n, p)


def check_bernoulli(bits, n, p):
    T = bits.shape[0]
    q = 2.0 ** -17                                                       # the kernel compares 16-bit slices with round(p * 65536)
    sig = np.sqrt(p * (1 - p) / (2 * n * T))
    assert abs(bits.mean() - p) <= 6 * sig + q
    col = bits.mean(axis=0)
    sig_col = np.sqrt(p * (1 - p) / T)
    assert np.all(np.abs(col - p) <= 6 * sig_col + q), float(np.abs(col - p).max())
    # X and Z bit of one qubit, and one column in adjacent rows: products of independent bits, mean p^2, inside the same band
    xz = (bits[:, :n] & bits[:, n:]).mean()
    adj = (bits[1:] & bits[:-1]).mean()
    assert abs(xz - p * p) <= 6 * sig_col + q and abs(adj - p * p) <= 6 * sig_col + q, (xz, adj)


@pytest.mark.parametrize('n,T', [(100, 20000), (1000, 20000)])
def test_op_random(L, n, T):
    seed = 0x5eed0000 + n
    for p in (0.1, 0.3, 0.5):
        rows, c = random_op(L, T, n, p, seed)
        bits, padding_zero = bits_of(rows, n)
        assert padding_zero, 'padding bits MUST be zero'
        check_bernoulli(bits, n, p)
        assert np.isfinite(c.view(np.float64)).all()
        for part in (c.real, c.imag):
            assert abs(part.mean()) <= 6 / np.sqrt(T)
            assert abs(part.var() - 1) <= 6 * np.sqrt(2 / T)
        if p == 0.3:
            again, c_again = random_op(L, T, n, p, seed)
            assert np.array_equal(again, rows) and np.array_equal(c_again, c)
            other, c_other = random_op(L, T, n, p, seed + 1)
            assert not np.array_equal(other, rows) and not np.array_equal(c_other, c)
            assert np.mean(bits_of(other, n)[0] == bits) < 0.7           # unrelated, not a shifted copy: agreement near p^2 + (1-p)^2 = 0.58
            if n == 1000:
                assert np.unique(rows, axis=0).shape[0] == T              # no two rows equal
    rows, c = random_op(L, 500, n, 0.0, seed)
    assert not rows.any() and np.isfinite(c.view(np.float64)).all()
    rows, _ = random_op(L, 500, n, 1.0, seed)
    bits, padding_zero = bits_of(rows, n)
    assert padding_zero and bits.all()                                   # exactly n bits in each half of every row
    assert int(np.unpackbits(rows.view(np.uint8)).sum()) == 500 * 2 * n
    h = ctypes.c_void_p()
    ok(L, L.symgpu_op_random(I64(0), n, DBL(0.3), U64(seed), byref(h)))
    assert h.value and info(L, h)[0] == 0
    x, s = checksum(L, h, 2 * ((n + 63) // 64))
    assert not x.any() and s[0] == 0 and s[1] == 0
    free(L, h)
