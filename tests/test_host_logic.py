"""CPU: host-side logic of the drop-in classes (no kernel is launched), the packing convention, and the C-ABI
library: it must load here and export every symbol ``include/symgpu.h`` declares; compute calls must fail
loudly without a GPU (there is no CPU fallback)."""
import os, re, ctypes
import numpy as np
import pytest
import symmer_amd
from symmer_amd import PauliwordOp, IndependentOp, SymgpuError, _lib, packing
from symmer_amd.operators.utils import string_to_symplectic, symplectic_to_string
from oracle import oracle_np as onp
from _golden import known, as_bool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_GPU = _lib.device_count() > 0 if os.path.exists(_lib.LIB_PATH) else False


# ---- constructor validation: mirrors tests/test_operators/test_base.py:26-110 of the reference -------------
def test_init_symplectic_float_type():
    with pytest.raises(AssertionError):
        PauliwordOp([[0., 1., 0., 1., 0., 1.]], [1])


def test_init_symplectic_nonbinary_ints_type():
    with pytest.raises(AssertionError):
        PauliwordOp([[0, 1, 2, 3, 4, 5]], [1])


def test_init_symplectic_str_type():
    with pytest.raises(AssertionError):
        PauliwordOp([['0', '1', '1', '0', '1', '1']], [1])


def test_incompatible_length_of_symp_matrix_and_coeff_vec():
    with pytest.raises(AssertionError):
        PauliwordOp([[0, 1, 0, 1, 0, 1], [1, 0, 1, 0, 1, 0]], [1])


def test_init_symplectic_incorrect_dimension():
    with pytest.raises(AssertionError):
        PauliwordOp([[[[0, 1, 1, 0, 1, 1]]]], [1])


def test_init_symplectic_2D_but_odd_columns():
    with pytest.raises(AssertionError):
        PauliwordOp([[0, 0, 1], [1, 0, 1]], [1, 1])


def test_init_symplectic_int_coeff():
    with pytest.raises(TypeError):
        PauliwordOp([[0, 0, 1, 1]], 1)


def test_from_list_incorrect_str():
    with pytest.raises(AssertionError):
        PauliwordOp.from_list(['ixi', 'zzi'], [0, 1])


def test_empty_and_constructors():
    P = PauliwordOp.empty(3)
    assert P.n_terms == 1 and P.n_qubits == 3 and np.array_equal(P.coeff_vec, [0])
    k = known()
    P1 = PauliwordOp.from_list(['III', 'XXX', 'YYY', 'ZZZ'])
    assert np.array_equal(P1.symp_matrix, as_bool(k['pl1_symp']))
    D = PauliwordOp.from_dictionary({'XZ': 1 + 2j, 'YI': 3})
    assert D.n_terms == 2 and D.coeff_vec[0] == 1 + 2j
    T = PauliwordOp.from_list(['XZ', 'YI'], [(1, 2), (3, 0)])
    assert np.array_equal(T.coeff_vec, [1 + 2j, 3])
    R = PauliwordOp.random(7, 5)
    assert R.symp_matrix.shape == (5, 14) and R.coeff_vec.dtype == complex
    assert str(PauliwordOp.from_list(['XY'], [1])) == ' 1.000+0.000j XY'


def test_strings_roundtrip():
    for s in ('IXYZ', 'YYII', 'Z'):
        assert symplectic_to_string(string_to_symplectic(s, len(s)).astype(bool)) == s


def test_getitem_iter_sort_dagger_append():
    P = PauliwordOp.from_list(['ZXZ', 'XZX', 'XYZ', 'ZIX'], [1, 2j, -3, 4])
    assert all(np.array_equal(P[i].symp_matrix[0], P.symp_matrix[i]) for i in range(-4, 4))
    assert [q.coeff_vec[0] for q in P] == list(P.coeff_vec)
    assert P[1:3].n_terms == 2 and P[[0, 3]].n_terms == 2 and P[np.array([True, False, True, False])].n_terms == 2
    with pytest.raises(ValueError):
        P['a']
    lex = P.sort('lex')
    assert np.array_equal(lex.symp_matrix, P.symp_matrix[onp.lex_order(P.symp_matrix)])
    assert np.array_equal(P.sort('magnitude').coeff_vec, [4, -3, 2j, 1])
    with pytest.raises(ValueError):
        P.sort('nope')
    assert np.array_equal(P.dagger.coeff_vec, np.conj(P.coeff_vec))
    A = P.append(P)
    assert A.n_terms == 8
    with pytest.raises(AssertionError):
        P.append(PauliwordOp.from_list(['XX']))
    assert np.array_equal(P.multiply_by_constant(2).coeff_vec, 2 * P.coeff_vec)
    assert np.array_equal((P * 2).coeff_vec, 2 * P.coeff_vec) and np.array_equal((2 * P).coeff_vec, 2 * P.coeff_vec)
    C = P.copy(); C.coeff_vec[:] = 0
    assert P.coeff_vec[0] == 1


def test_qubit_mismatch_asserts_before_any_kernel():
    P, Q = PauliwordOp.from_list(['XX']), PauliwordOp.from_list(['XXX'])
    with pytest.raises(AssertionError):
        P * Q
    with pytest.raises(AssertionError):
        P.commutes_termwise(Q)
    with pytest.raises(AssertionError):
        P._multiply_by_operator(Q)
    with pytest.raises(AssertionError):
        P._rotate_by_single_Pword(Q, 0.3)


def test_packing_convention():
    rng = np.random.default_rng(3)
    for n in (1, 5, 63, 64, 65, 130, 1000):
        s = rng.random((6, 2 * n)) < 0.4
        p = packing.pack_rows(s)
        wq = packing.words_per_block(n)
        assert p.shape == (6, 2 * wq) and p.dtype == np.dtype('<u8')
        assert np.array_equal(p, onp.pack_rows(s))
        assert np.array_equal(packing.unpack_rows(p, n), s)
        q = 64 * (wq - 1) + (n - 1) % 64                           # bit j of word w <-> qubit 64 w + j
        assert bool((p[0, (n - 1) // 64] >> np.uint64((n - 1) % 64)) & np.uint64(1)) == bool(s[0, n - 1])
        if n % 64:
            assert not np.any(p[:, wq - 1] >> np.uint64(n % 64))    # padding bits zero
    m = rng.random((5, 70)) < 0.5
    assert np.array_equal(packing.unpack_bits(packing.pack_bits(m), 70), m)


# ---- the C-ABI library ---------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'symgpu.h')).read()
    declared = set(re.findall(r'\b(symgpu_[a-z0-9_]+)\s*\(', hdr))
    assert len(declared) >= 40
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/symgpu.h but not exported by libsymgpu.so'
    assert declared == set(_lib.SIGNATURES) | {'symgpu_last_error'}, 'ctypes prototypes out of sync with the header'


@pytest.mark.skipif(HAVE_GPU, reason='this container has a GPU')
def test_compute_fails_loudly_without_gpu():
    P = PauliwordOp.from_list(['XX', 'ZZ'], [1, 2])
    for call in (lambda: P * P, lambda: P.cleanup(), lambda: P.commutes_termwise(P),
                 lambda: IndependentOp.symmetry_generators(P), lambda: P + P):
        with pytest.raises(SymgpuError):
            call()
    n = ctypes.c_int(-1)
    assert _lib.load().symgpu_device_count(ctypes.addressof(n)) == 0 and n.value == 0
    assert _lib.load().symgpu_sync() == _lib.E_NODEVICE


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'symmer_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in src.replace('ORACLE', ''), f'{f} mentions the oracle'


def test_packed_results_are_not_expanded_until_asked():
    """Kernel results arrive packed; the one-byte-per-bit matrix is only built on access, and row selection / scaling /
    appending keep working on the packed layout alone."""
    from symmer_amd.operators import PauliwordOp
    from symmer_amd import packing
    rng = np.random.default_rng(0)
    symp = rng.random((7, 2 * 70)) < 0.4
    coeff = rng.standard_normal(7) + 0j
    op = PauliwordOp._from_packed(packing.pack_rows(symp), 70, coeff)
    assert op._symp is None and op.n_terms == 7 and op.n_qubits == 70
    sub = (op[[4, 1]] * 2.0).append(op[2:5])
    assert sub._symp is None and op._symp is None
    assert np.array_equal(sub.symp_matrix, symp[[4, 1, 2, 3, 4]]) and np.array_equal(sub.coeff_vec, np.hstack([2 * coeff[[4, 1]], coeff[2:5]]))
    assert np.array_equal(op.symp_matrix, symp) and np.array_equal(op.X_block, symp[:, :70]) and np.array_equal(op.Z_block, symp[:, 70:])
    assert np.array_equal(op.dagger.coeff_vec, coeff.conjugate())


def test_circuit_rotation_string_last_write_wins_and_negative_indices():
    """reference evolution/circuit_symmerlator.py:38-40 fills a list of characters: a repeated index keeps the LAST letter and
    negative indices count from the end."""
    from symmer_amd.evolution import CircuitSymmerlator
    C = CircuitSymmerlator(70)

    def letters(op):
        m = np.asarray(op.symp_matrix)[0]
        return ''.join('IXZY'[int(m[i]) + 2 * int(m[70 + i])] for i in range(70))
    assert letters(C.get_rotation_string('XZ', [0, 0])) == 'Z' + 'I' * 69
    assert letters(C.get_rotation_string('YX', [3, 3])) == 'III' + 'X' + 'I' * 66
    assert letters(C.get_rotation_string('ZI', [65, 65])) == 'I' * 70
    assert letters(C.get_rotation_string('Y', [-1])) == 'I' * 69 + 'Y'
    assert letters(C.get_rotation_string('XZ', [-70, 64])) == 'X' + 'I' * 63 + 'Z' + 'I' * 5
    with pytest.raises(AssertionError):
        C.get_rotation_string('X', [70])
    with pytest.raises(AssertionError):
        C.get_rotation_string('X', [-71])


def test_hash_partition_classes_are_linear_and_shares_partition_the_product():
    """symmer_amd/sharding.py, hash-partitioned multi-GPU cleanup (no GPU: checker kernels built on the oracle): the row class is GF(2)-linear
    (class of a product row = XOR of the operands' classes), every pair has exactly one owner for any world size, and the shares of
    G = 1 .. 8 ranks merged by first pair index are the single-process result — rows, order and sums (dyadic: bit for bit)."""
    from symmer_amd import sharding
    from oracle import oracle_c as oc, oracle_np as onp
    rng = np.random.default_rng(11)
    n, Ni, No = 70, 90, 57
    A = onp.pack_rows(rng.random((Ni, 2 * n)) < 0.3); B = onp.pack_rows(rng.random((No, 2 * n)) < 0.3)
    A[40:50] = A[:10]; B[30:35] = B[:5]
    a = (rng.integers(-8, 9, Ni) + 1j * rng.integers(-8, 9, Ni)) / 16.0; b = (rng.integers(-8, 9, No) + 1j * rng.integers(-8, 9, No)) / 16.0
    for bits in (1, 3, 5):
        ca, cb = sharding.linear_row_classes(A, bits), sharding.linear_row_classes(B, bits)
        prod = (A[:, None, :] ^ B[None, :, :]).reshape(-1, A.shape[1])
        assert np.array_equal(sharding.linear_row_classes(prod, bits), (ca[:, None] ^ cb[None, :]).ravel())
        assert ca.max() < (1 << bits)

    def indexed_cleanup(r, c, thr):
        first, inv = onp.first_occurrence_unique(np.ascontiguousarray(r).view(np.uint8).reshape(r.shape[0], -1))
        sums = np.zeros(first.shape[0], dtype=complex)
        np.add.at(sums, inv, c)
        keep = np.ones(first.shape[0], dtype=bool) if thr is None else np.abs(sums) > thr
        return r[first][keep], sums[keep], first[keep]

    def indexed_mul(inner, ci, outer, co, left):
        r, c = oc.mul_allpairs(inner, ci, outer, co, left)
        rr, cc, first = indexed_cleanup(r, c, None)
        return rr, cc, first % inner.shape[0], first // inner.shape[0]
    for X, x, Y, y, left in ((A, a, B, b, True), (A, a, A, a, True), (B, b, A, a, False)):
        pr, pc = oc.mul_allpairs(X, x, Y, y, left)
        er, ec = oc.cleanup(pr, pc, 1e-15)
        for G in range(1, 9):
            shares, owned = [], 0
            for rank in range(G):
                st = {}
                shares.append(sharding.hash_partition_local(X, x, Y, y, rank, G, left, 1e-15, indexed_mul, indexed_cleanup, st))
                owned += st['pairs_owned']
            assert owned == X.shape[0] * Y.shape[0]
            g = np.concatenate([s[2] for s in shares])
            order = np.argsort(g, kind='stable')
            assert np.unique(g).size == g.size
            assert np.array_equal(np.concatenate([s[0] for s in shares], axis=0)[order], er)
            assert np.array_equal(np.concatenate([s[1] for s in shares])[order], ec)


def test_host_operators_pickle_and_constructor_owns_its_coefficients():
    """A host-only operator pickles as plain arrays (the reference's objects are NumPy and travel through its process pool); the
    constructor copies the coefficient array it is given (mutations reach an operator through `op.coeff_vec` only)."""
    import pickle
    c = np.array([1 + 2j, -0.5, 3j])
    P = PauliwordOp.from_list(['XZ', 'YI', 'ZZ'], c)
    c[0] = 99
    assert P.coeff_vec[0] == 1 + 2j
    Q = pickle.loads(pickle.dumps(P))
    assert np.array_equal(Q.symp_matrix, P.symp_matrix) and np.array_equal(Q.coeff_vec, P.coeff_vec) and Q.n_qubits == 2 and Q._dev is None
    Z = pickle.loads(pickle.dumps(PauliwordOp(np.zeros((1, 0), dtype=bool), [2.5])))          # a 0-qubit scalar has no packed rows
    assert Z.n_qubits == 0 and Z.coeff_vec[0] == 2.5


def test_sector_values_are_checked_with_an_exception():
    """anything but -1, 0, +1 as a stabiliser eigenvalue is a ValueError (not an assert that `python -O` removes),
    raised before the values are used; float noise within 1e-12 is rounded."""
    from symmer_amd import kernels
    assert list(kernels.sector_signs([1, -1, 0, 1.0000000000000002, -0.9999999999999999 + 0j])) == [1, -1, 0, 1, -1]
    for bad in ([2], [0.5], [1j], [1 + 1e-6]):
        with pytest.raises(ValueError, match='eigenvalues'):
            kernels.sector_signs(bad)


def test_bench_summary_carries_every_config():
    """`summary_of` on a line shaped like the full default run: cfg1-cfg5 + the strong-scaling shard within 1.5 KB, in the last 4 KB."""
    import json, sys, importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module('bench')
    roof = {'kernel': 'k_some_kernel_name', 'frac': 0.812345, 'lds': {'frac': 0.6012}}
    api = {'a_result_object_seconds': 0.0023456, 'b_host_arrays_out_seconds': 0.165432}
    line = {'metric': 'pauli_term_pairs_per_sec', 'value': 2.52e10, 'unit': 'pairs/s', 'ms_per_step': 396.5, 'config': {'workload': 'allpairs_product'},
            'roofline': roof, 'cpu_baseline': {'value': 1.1e6, 'other_configs': {'cfg1_mul_cleanup': {'pairs_per_s': 3e5}, 'cfg2_rotation': {'term_pairs_per_s': 2e4},
                                                                                 'cfg3_sample_mul_cleanup': {'pairs_per_s': 1e5}, 'cfg4_sample_rref': {'row_xors_per_s': 1e4},
                                                                                 'cfg5_sample_commutation': {'pairs_per_s': 5e6}}},
            'extras': {'cfg1_api_mul': {'pairs_per_s': 1.4e8, 'seconds': 1.8e-3, 'api': api},
                       'cfg2_rotation': {'term_pairs_per_s': 3.5e9, 'seconds_per_rotation': 2.8e-5, 'roofline': roof, 'api': api, 'clifford': {'run_of_200_seconds_per_rotation': 5e-6},
                                         'saturated_chain': {'seconds_per_rotation': 3e-5}},
                       'cfg3_mul_cleanup': {'pairs_per_s': 4.2e10, 'seconds': 2.36e-3, 'roofline': roof, 'api': api},
                       'cfg4_symmetry_kernel': {'row_xors_per_s': 4.1e9, 'seconds': 1.95e-3, 'roofline': roof, 'api': api},
                       'cfg5_adjacency': {'pairs_per_s': 1.28e12, 'seconds': 0.0312, 'roofline': roof, 'api': {'full': api, 'rank_share': api},
                                          'rank_share_25000_rows': {'seconds': 4.2e-3, 'predicted_8gpu_strong_speedup_before_allgather': 7.43}},
                       'strong_scaling_shard': {'ms_per_step': 49.9, 'roofline': roof, 'predicted_8gpu_strong_speedup_before_allgather': 7.95},
                       'broken_section': {'error': 'X'}}}
    sm = bench.summary_of(line)
    text = json.dumps(sm)
    assert len(text) <= 1500, len(text)
    for key in ('product_1e5x1e5', 'cfg1_mul_500t_100q', 'cfg2_rotation', 'cfg3_mul_cleanup', 'cfg4_gf2', 'cfg5_adjacency', 'strong_scaling_shard'):
        assert key in sm, key
    assert sm['cfg5_adjacency']['predicted_8gpu_x'] == 7.43 and sm['cfg3_mul_cleanup']['api'] == [0.002346, 0.1654] and sm['failed_sections'] == ['broken_section']


def test_bench_plain_run_leaves_the_other_measurements_to_full(monkeypatch):
    """A plain `bench.py --gpus 1 --steps N --warmup W` measures its contract line only: the CPU baselines, the `api` objects and `extras`
    run with `--full`, where `--no-cpu` / `--no-api` / `--no-extras` still switch them off one by one; steps and warm-up are untouched."""
    import sys, importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    monkeypatch.delenv('BENCH_CPU_FULL', raising=False)

    def parse(*argv):
        monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
        return bench.parse()
    a = parse('--gpus', '1', '--steps', '5', '--warmup', '2')
    assert not a.full and a.no_cpu and a.no_api and a.no_extras and (a.steps, a.warmup) == (5, 2)
    a = parse('--gpus', '1', '--steps', '5', '--warmup', '2', '--full')
    assert a.full and not (a.no_cpu or a.no_api or a.no_extras) and (a.steps, a.warmup) == (5, 2)
    a = parse('--full', '--no-cpu', '--workload', 'gf2')
    assert a.no_cpu and not (a.no_api or a.no_extras) and (a.steps, a.warmup) == (10, 2)
    a = parse('--workload', 'rotation')
    assert a.no_cpu and a.no_api and a.no_extras and (a.steps, a.warmup) == (3, 1)


def test_lexicographic_order_from_packed_rows_equals_numpy_lexsort_of_the_columns():
    """``sort('lex')`` and ``==`` (base.py:455-492, 640-662) order the rows by ``np.lexsort(symp_matrix.T)`` (last column = primary key); the
    drop-in takes the order from the packed rows — 2 Wq sort keys instead of 2n — which must be the SAME permutation, ties included."""
    rng = np.random.default_rng(321)
    for n in (1, 5, 63, 64, 65, 130):
        m = rng.random((300, 2 * n)) < 0.5
        m[10] = m[3]; m[200] = m[3]                               # equal rows: a stable sort keeps their order
        P = PauliwordOp(m, np.arange(300, dtype=complex))
        assert np.array_equal(P._lex_order(), np.lexsort(m.T)), n
        Q = P.sort('lex')
        assert np.array_equal(Q.symp_matrix, m[np.lexsort(m.T)]) and np.array_equal(Q.coeff_vec, np.lexsort(m.T).astype(complex))
    assert PauliwordOp(np.zeros((0, 6), dtype=bool), [])._lex_order().size == 0


@pytest.mark.parametrize('angle', [np.pi / 2, -np.pi / 2, np.pi, -np.pi, 3 * np.pi / 2, -3 * np.pi / 2, 2 * np.pi, 0.0, -0.0, 0.3, -1.1,
                                   np.pi / 2 * 1e-18, np.pi / 2 * 0.9e-18, np.pi / 2 * 2e-18, -np.pi / 2 * 1e-18, -np.pi / 2 * 2e-18])
def test_rotation_args_clifford_detection(angle):
    """The reference's Clifford branch (base.py:1146-1154): multiple = 2 angle / pi, int_part = round(multiple); Clifford iff
    |int_part - multiple| <= 1e-18; odd int_part multiplies by Q; int_part in [2, 3] negates.  rotation_args must decide the same for the
    float _rotate_by_single_Pword hands it, whether the caller's angle was a float, a 0-d ndarray or a complex 0-d ndarray."""
    from symmer_amd import kernels
    for given in (angle, np.array(angle), np.array(complex(angle, 0.0)), np.float64(angle)):
        assert kernels.rotation_args(float(np.real(given))) == kernels.rotation_args(angle)
    cos_t, sin_t, k = kernels.rotation_args(angle)
    multiple = angle * 2 / np.pi
    int_part = round(multiple)
    if abs(int_part - multiple) <= 1e-18:
        assert k >= 0
        assert (k & 1) == (int_part % 2)                    # multiplies by Q
        assert (k in (2, 3)) == (int_part in (2, 3))        # negates
    else:
        assert k == -1 and cos_t == np.cos(angle) and sin_t == np.sin(angle)


# ---- the debug counters: one table (SYMGPU_COUNTER_LIST, include/symgpu.h), ids frozen ----------------------------------------------
# The freeze: the ids are part of the C ABI (outside binders pass the numbers).  A name may only ever be ADDED here, at the end.
COUNTER_IDS = [
    (0, 'HASH_RESEEDS'), (1, 'RESIDENT_DONE'), (2, 'RESIDENT_FAILED'), (3, 'DEV_MALLOC_CALLS'), (4, 'RESIDENT_NS_PREPARE'),
    (5, 'RESIDENT_NS_LAUNCH'), (6, 'RESIDENT_NS_WAIT'), (7, 'H2D_BYTES'), (8, 'D2H_BYTES'), (9, 'OP_UPLOADS'), (10, 'OP_DOWNLOADS'),
    (11, 'CANARY_HITS'), (12, 'CTX_MAX_THREADS'), (13, 'CTX_WAITS'), (14, 'CTX_UNLOCKED_USES'), (15, 'GF2_BLOCKS_PANELLED'),
    (16, 'GF2_PANEL_FULL_ROWS'), (17, 'GF2_PANEL_WINDOW'), (18, 'COMMUTE_REGISTER_TILE'), (19, 'COMMUTE_WIDE_ROWS'), (20, 'COMMUTE_M4R_TILE'),
    (21, 'COMMUTE_M4R_STREAMK'), (22, 'CHAIN_REGISTERS'), (23, 'CHAIN_LDS'), (24, 'CHAIN_SINGLE_WORKGROUP'), (25, 'CHAIN_TWO_LAUNCHES'),
    (26, 'CHAIN_FOUR_LAUNCHES'), (27, 'CHAIN_SORT_ONE_LAUNCH'), (28, 'CHAIN_SORT_LAUNCHES'), (29, 'ROTATE_HASH_JOIN'),
    (30, 'ROTATE_CLIFFORD_FAST'), (31, 'ROTATE_GENERAL'), (32, 'ROTATE_GENERAL_BY_DUP_CHECK'), (33, 'RESIDENT_LDS'), (34, 'RESIDENT_REGISTERS'),
    (35, 'RESIDENT_ROWS_IN_MEMORY'), (36, 'FLOW_COMPLETE_SORT'), (37, 'FLOW_FLAGS_HASH_TABLES'), (38, 'FLOW_FLAGS_PARTIAL_SORT'),
    (39, 'FLOW_FLAGS_GAVE_UP'), (40, 'GIVEUP_PRODUCT_BUCKET'), (41, 'GIVEUP_COUNTER_SATURATED'), (42, 'GIVEUP_LIST_OVERFLOW'),
    (43, 'GIVEUP_OPERAND_BUCKET'), (44, 'FLOW_SORTED_WHOLE'), (45, 'FLOW_SORTED_FLAGGED'), (46, 'FLOW_MARKED_FROM_BYTES'),
    (47, 'FLOW_FULL_SORT_REPEAT'), (48, 'PRODUCT_ROWS_ONLY'), (49, 'PRODUCT_PHASE_STREAM'), (50, 'PRODUCT_WIDE_COEFF_THEN_ROWS'),
    (51, 'PRODUCT_WORD_MAJOR_THEN_ROWS'), (52, 'PRODUCT_WORD_MAJOR_BESIDE_ROWS'), (53, 'CSR_FILL_LDS'), (54, 'CSR_FILL_SCRATCH'),
    (55, 'DEV_BLOCKS_LIVE'), (56, 'DEV_FREE_UNKNOWN'), (57, 'OP_WORD_MAJOR_BUILDS'), (58, 'OP_BIT_MAJOR_BUILDS'), (59, 'OP_YCOUNT_BUILDS'),
    (60, 'OP_ROW_HASH_BUILDS'),
]


def test_debug_counter_ids_and_names_are_frozen():
    """symgpu_debug_counter_name spells exactly the table above (so does the map the Python side builds from it), NULL outside it; every id
    reads without a device and 61 is the first that does not; an unknown name is a KeyError that names it."""
    from symmer_amd import kernels
    lib = _lib.load()
    assert [i for i, _ in COUNTER_IDS] == list(range(61)) and len({name for _, name in COUNTER_IDS}) == 61
    got = [(i, lib.symgpu_debug_counter_name(i)) for i in range(61)]
    assert [(i, name.decode('ascii') if name is not None else None) for i, name in got] == COUNTER_IDS
    assert lib.symgpu_debug_counter_name(-1) is None and lib.symgpu_debug_counter_name(61) is None
    assert _lib.counter_ids() == {name: i for i, name in COUNTER_IDS}
    v = ctypes.c_int64(-1)
    for i, name in COUNTER_IDS:
        assert lib.symgpu_debug_counter(i, ctypes.addressof(v)) == _lib.OK and v.value >= 0, name
        assert kernels.counter(name) == v.value
    assert lib.symgpu_debug_counter(61, ctypes.addressof(v)) == _lib.E_INVALID and lib.symgpu_debug_counter(-1, ctypes.addressof(v)) == _lib.E_INVALID
    assert kernels.counters(['H2D_BYTES', 'CSR_FILL_SCRATCH']).dtype == np.int64
    with pytest.raises(KeyError, match='no_such'):
        kernels.counter('no_such')


# ---- every exported entry point that touches a device context holds that context's lock (SG_ENTER, common.h) ------------------------
# The calls that deliberately take no lock, each with its reason.  Every name here must still be defined (the list cannot rot).
UNLOCKED_ENTRY_POINTS = {
    'symgpu_comm_available': 'loads librccl only; touches no context',
    'symgpu_comm_unique_id': 'RCCL bring-up: no lock may be held inside RCCL (a watchdog may give up on it)',
    'symgpu_comm_init': 'RCCL bring-up on a watchdog thread that may never return; the device must stay usable meanwhile',
    'symgpu_comm_init_all': 'RCCL bring-up: no lock may be held inside RCCL',
    'symgpu_comm_abandon': 'disowns a bring-up a watchdog gave up on; must not wait for anything',
    'symgpu_comm_destroy': 'RCCL teardown: no lock may be held inside RCCL',
    'symgpu_comm_allgather_op': 'RCCL collective: the first one runs on a watchdog thread while the main thread goes on',
    'symgpu_comm_allgather_ops': 'RCCL collective over all devices: no lock may be held inside RCCL',
    'symgpu_comm_barrier': 'RCCL collective: no lock may be held inside RCCL',
    'symgpu_init': 'creates a context; documented as before the threads start',
    'symgpu_init_all': 'creates the contexts; documented as before the threads start',
    'symgpu_shutdown': 'destroys the contexts; documented as after the threads end',
    'symgpu_set_device': "sets the calling thread's selection only (plus init of a new context)",
    'symgpu_current_device': "reads the calling thread's selection",
    'symgpu_device_count': 'asks the runtime; touches no context',
    'symgpu_n_initialised': 'counts ready contexts; touches none of their state',
    'symgpu_degraded': 'has its own mutex',
    'symgpu_last_error': "returns the calling thread's own error text",
    'symgpu_debug_counter': 'reads atomic counters',
    'symgpu_debug_counter_name': 'returns a string literal of the counter table; touches no context',
    'symgpu_op_info': "reads the handle's own fields (a handle has one owner)",
    'symgpu_dev_free': "allocator only: files the block under its owning device, under the allocator's mutex; needs no context",
}


def _strip_c_comments_and_strings(src):
    """`src` with comments, string and character literals blanked (same length), so that braces in them do not count."""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if src.startswith('//', i):
            j = src.find('\n', i)
            j = n if j < 0 else j
            out.append(' ' * (j - i)); i = j
        elif src.startswith('/*', i):
            j = src.find('*/', i + 2)
            j = n if j < 0 else j + 2
            out.append(re.sub(r'[^\n]', ' ', src[i:j])); i = j
        elif c in '"\'':
            j = i + 1
            while j < n and src[j] != c:
                j += 2 if src[j] == '\\' else 1
            out.append(c + ' ' * (j - i - 1) + c); i = j + 1
        else:
            out.append(c); i += 1
    return ''.join(out)


def _entry_point_bodies(src):
    """{name: body} of every `int symgpu_*(...) {...}` / `const char *symgpu_*(...) {...}` definition in one translation unit
    (declarations are skipped)."""
    clean = _strip_c_comments_and_strings(src)
    bodies = {}
    for m in re.finditer(r'^(?:int\s+|const char \*)(symgpu_\w+)\s*\(', clean, re.M):
        depth, i = 0, m.end() - 1
        while True:                                    # the parameter list
            depth += {'(': 1, ')': -1}.get(clean[i], 0)
            if depth == 0:
                break
            i += 1
        j = i + 1
        while clean[j].isspace():
            j += 1
        if clean[j] != '{':
            continue
        depth, k = 0, j
        while True:
            depth += {'{': 1, '}': -1}.get(clean[k], 0)
            if depth == 0:
                break
            k += 1
        assert m.group(1) not in bodies, f'{m.group(1)} defined twice'
        bodies[m.group(1)] = clean[j:k + 1]
    return bodies


def _lock_violations(sources, allow):
    """Problems with the lock discipline of `sources` ({file name: text}) under the allowlist `allow`."""
    bodies = {}
    for fname, src in sources.items():
        for name, body in _entry_point_bodies(src).items():
            assert name not in bodies, f'{name} defined in two files'
            bodies[name] = (fname, body)
    problems = [f'{name} ({fname}) takes no context lock: begin it with SG_ENTER(...) or list it in UNLOCKED_ENTRY_POINTS with a reason'
                for name, (fname, body) in sorted(bodies.items()) if name not in allow and 'SG_ENTER(' not in body]
    problems += [f'{name} is in UNLOCKED_ENTRY_POINTS but no longer defined' for name in sorted(allow) if name not in bodies]
    problems += [f'{name} is in UNLOCKED_ENTRY_POINTS but takes the lock all the same' for name in sorted(allow)
                 if name in bodies and 'SG_ENTER(' in bodies[name][1]]
    return problems, bodies


def _hip_sources():
    csrc = os.path.join(ROOT, 'symmer_amd', 'csrc')
    return {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}


def test_every_entry_point_takes_its_context_lock():
    problems, bodies = _lock_violations(_hip_sources(), UNLOCKED_ENTRY_POINTS)
    assert not problems, '\n'.join(problems)
    assert len(bodies) >= 80, f'the scan found only {len(bodies)} entry points: has the definition style changed?'
    assert all(reason.strip() for reason in UNLOCKED_ENTRY_POINTS.values())
    # every entry point the header declares is defined where the scan looks
    header = open(os.path.join(ROOT, 'include', 'symgpu.h')).read()
    declared = set(re.findall(r'^(?:int\s+|const char \*)(symgpu_\w+)\s*\(', _strip_c_comments_and_strings(header), re.M))
    assert declared <= set(bodies), f'declared but not found by the scan: {sorted(declared - set(bodies))}'


def test_lock_scan_names_an_entry_point_that_drops_its_lock_and_a_stale_allowlist():
    sources = _hip_sources()
    # SG_ENTER removed from one entry point: the scan names it
    fname = 'op_handles.hip'
    body = _entry_point_bodies(sources[fname])['symgpu_op_scale']
    assert body.count('SG_ENTER(op);') == 1
    start = sources[fname].index('int symgpu_op_scale(')
    broken = dict(sources)
    broken[fname] = sources[fname][:start] + sources[fname][start:].replace('SG_ENTER(op);', 'SG_TRY(require_ctx());', 1)
    problems, _ = _lock_violations(broken, UNLOCKED_ENTRY_POINTS)
    assert len(problems) == 1 and problems[0].startswith('symgpu_op_scale (op_handles.hip) takes no context lock'), problems
    # a name taken off the allowlist: the scan names it
    allow = dict(UNLOCKED_ENTRY_POINTS)
    del allow['symgpu_comm_barrier']
    problems, _ = _lock_violations(sources, allow)
    assert len(problems) == 1 and problems[0].startswith('symgpu_comm_barrier (comm.hip) takes no context lock'), problems
    # a name on the allowlist that no longer exists: the scan names it
    problems, _ = _lock_violations(sources, dict(UNLOCKED_ENTRY_POINTS, symgpu_gone='removed'))
    assert problems == ['symgpu_gone is in UNLOCKED_ENTRY_POINTS but no longer defined'], problems
    # braces and SG_ENTER inside comments and strings do not count
    fake = {'x.hip': 'int symgpu_fake(int a) {\n    // SG_ENTER(a); }\n    const char *s = "SG_ENTER( {";\n    return 0;\n}\n'}
    problems, bodies = _lock_violations(fake, {})
    assert list(bodies) == ['symgpu_fake'] and len(problems) == 1, problems


# ---- operator handles the library makes for itself have one owner (OwnedOp, common.h) ------------------------------------------------
# Raw symgpu_op_alloc / symgpu_op_free calls may stand where they are defined and in the owner, nowhere else.
RAW_HANDLE_CALLS_ALLOWED_IN = ('op_handles.hip', 'common.h')


def _raw_handle_calls(sources, allowed=RAW_HANDLE_CALLS_ALLOWED_IN):
    """'file:line: call' for every symgpu_op_alloc( / symgpu_op_free( in `sources` ({file name: text}) outside `allowed`."""
    found = []
    for fname, src in sorted(sources.items()):
        if fname in allowed:
            continue
        for n, line in enumerate(_strip_c_comments_and_strings(src).split('\n'), 1):
            found += [f'{fname}:{n}: {m.group(1)}(' for m in re.finditer(r'\b(symgpu_op_alloc|symgpu_op_free)\s*\(', line)]
    return found


def test_operator_handles_inside_the_library_go_through_their_owner():
    csrc = os.path.join(ROOT, 'symmer_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h'))}
    assert len(sources) >= 50 and set(RAW_HANDLE_CALLS_ALLOWED_IN) <= set(sources)
    found = _raw_handle_calls(sources)
    assert not found, 'raw operator handle calls (use OwnedOp, common.h):\n' + '\n'.join(found)
    # the owner is where the scan expects it, and the scan sees a call where there is one (comments and strings do not count)
    assert _raw_handle_calls({'common.h': sources['common.h']}, allowed=()) and 'struct OwnedOp' in sources['common.h']
    fake = {'x.hip': '// symgpu_op_free(a);\nconst char *s = "symgpu_op_alloc(";\nint f() {\n    return symgpu_op_free (res);\n}\n'}
    assert _raw_handle_calls(fake) == ['x.hip:4: symgpu_op_free(']
