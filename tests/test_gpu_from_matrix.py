"""PauliwordOp.from_matrix / haar_random on the device (csrc/pauli_decomp.hip) against the NumPy restatement of the contract
(tests/_pauli_decomp_oracle.py, which every device form must match bit for bit), the reference's answers (tests/golden/from_matrix.npz),
its own inverse to_sparse_matrix, and a molecular Hamiltonian."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse

import _csr_families as fam
import _pauli_decomp_oracle as po
from symmer_amd import PauliwordOp, kernels, packing, _lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def dyadic(rng, shape, zeros=0.3):
    m = (rng.integers(-8, 9, shape) + 1j * rng.integers(-8, 9, shape)) / 8.0
    m[rng.random(shape) < zeros] = 0
    return m


def gaussian(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def assert_is_restatement(op, n, expect):
    """Rows (packed, padding bits zero), ascending order and coefficient bits of a device result against (x, z, coeff)."""
    x, z, c = expect
    assert op.n_qubits == n and op.n_terms == len(c)
    assert op._dev is not None and op._packed_cache is None and op._coeff is None, 'the result did not stay on the device'
    symp = po.symp_of(x, z, n)
    packed = op.packed
    assert packed.shape == (len(c), 2) and np.array_equal(packed, packing.pack_rows(symp).reshape(len(c), 2))
    assert np.array_equal(op.symp_matrix, symp)
    assert po.bits_equal(op.coeff_vec, c), 'coefficients not bit-equal to the restatement'


def assert_same_operator(a, b):
    assert a.n_qubits == b.n_qubits and a.n_terms == b.n_terms
    assert np.array_equal(a.packed, b.packed)
    assert po.bits_equal(a.coeff_vec, b.coeff_vec)


def term_dict(op):
    x, z = po.xz_of(op.symp_matrix)
    return {(int(a), int(b)): c for a, b, c in zip(x, z, op.coeff_vec)}


# ---- dense input against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', range(1, 9))
def test_dense_dyadic_is_the_restatement_and_inverts_to_sparse_matrix(n):
    rng = np.random.default_rng(100 + n)
    M = dyadic(rng, (1 << n, 1 << n))
    op = PauliwordOp.from_matrix(M)
    assert_is_restatement(op, n, po.decompose(M, n))
    assert np.array_equal(op.to_sparse_matrix.toarray(), M)
    assert_same_operator(PauliwordOp.from_matrix(M, strategy='full_basis'), op)


@pytest.mark.parametrize('n', [1, 2, 6, 7])
def test_dense_gaussian_is_bit_equal_to_the_restatement(n):
    M = gaussian(np.random.default_rng(200 + n), (1 << n, 1 << n))
    assert_is_restatement(PauliwordOp.from_matrix(M), n, po.decompose(M, n))


@pytest.mark.parametrize('case', range(14))
def test_reference_answers(case):
    tag, layout, kind, n, dense, csr, ref_symp, ref_coeff = po.golden_cases()[case]
    matrix = dense if layout == 'dense' else scipy.sparse.csr_matrix(csr, shape=dense.shape)
    op = PauliwordOp.from_matrix(matrix)
    x, z = po.xz_of(op.symp_matrix)
    assert np.all(np.diff(x * (1 << n) + z) > 0)
    po.assert_matches_reference(x, z, op.coeff_vec, ref_symp, ref_coeff, kind, n, dense)


# ---- sparse input: bit-equal to the dense call on .toarray() ---------------------------------------------------------------------------
def _csr_inputs():
    rng = np.random.default_rng(300)
    n, side = 6, 64
    b = np.arange(side)
    out = {}
    rows, cols = np.concatenate([b, b, b]), np.concatenate([b ^ 0, b ^ 5, b ^ 63])
    out['three diagonals'] = scipy.sparse.csr_matrix((gaussian(rng, 3 * side), (rows, cols)), shape=(side, side))
    m = gaussian(rng, (side, side))
    m[rng.random((side, side)) >= 0.3] = 0
    out['density 0.3'] = scipy.sparse.csr_matrix(m)
    # three stored values per row, two of them in the same column, the columns descending: neither canonical nor sorted
    c0, c1 = rng.integers(1, side, side), rng.integers(0, side, side)
    hi, lo = np.maximum(c0, c1), np.minimum(c0, c1)
    lo = np.where(lo == hi, hi - 1, lo)
    indices = np.stack([hi, hi, lo], axis=1).reshape(-1)
    raw = scipy.sparse.csr_matrix((dyadic(rng, 3 * side, 0.0), indices, np.arange(0, 3 * side + 1, 3)), shape=(side, side))
    assert not raw.has_sorted_indices or not raw.has_canonical_format
    out['duplicates, unsorted'] = raw
    r, c = rng.integers(0, side, 400), rng.integers(0, side, 400)
    out['coo with duplicates'] = scipy.sparse.coo_matrix((dyadic(rng, 400, 0.0), (r, c)), shape=(side, side))
    out['csc'] = scipy.sparse.csc_matrix(m)
    z = scipy.sparse.csr_matrix(m)
    z.data[::3] = 0                                                  # stored zeros
    assert np.count_nonzero(z.data == 0) > 100
    out['stored zeros'] = z
    return n, out


@pytest.mark.parametrize('which', ['three diagonals', 'density 0.3', 'duplicates, unsorted', 'coo with duplicates', 'csc', 'stored zeros'])
def test_sparse_input_equals_dense_input(which):
    n, inputs = _csr_inputs()
    sp = inputs[which]
    parts = ('data', 'row', 'col') if which.startswith('coo') else ('data', 'indices', 'indptr')
    before = [getattr(sp, a).copy() for a in parts]
    op = PauliwordOp.from_matrix(sp)
    assert all(np.array_equal(getattr(sp, a), b) for a, b in zip(parts, before)), 'the input was changed'
    dense = sp.toarray()
    assert_same_operator(op, PauliwordOp.from_matrix(dense))
    if which == 'three diagonals':
        x, _ = po.xz_of(op.symp_matrix)
        assert set(x.tolist()) == {0, 5, 63} and op.n_terms == 3 * 64
    assert_is_restatement(PauliwordOp.from_matrix(sp), n, po.decompose(dense, n))


# ---- the two transform forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, tile_bits', [(7, 3), (10, 4)])
def test_two_pass_form_is_bit_equal_to_one_pass(monkeypatch, n, tile_bits):
    M = gaussian(np.random.default_rng(400 + n), (1 << n, 1 << n))
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS', raising=False)
    one, t_one, form_one = kernels.pauli_decompose_dense(M, n)
    monkeypatch.setenv('SYMGPU_PAULI_TILE_BITS', str(tile_bits))
    two, t_two, form_two = kernels.pauli_decompose_dense(M, n)
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS')
    assert form_one == kernels.PAULI_ONE_PASS and form_two == kernels.PAULI_TWO_PASS
    (r1, c1), (r2, c2) = one.download(), two.download()
    assert t_one == t_two == 4 ** n and np.array_equal(r1, r2) and po.bits_equal(c1, c2)
    x, z, c = po.decompose(M, n)
    assert po.bits_equal(c2, c)
    one.free(); two.free()


def test_two_pass_form_with_a_basis_and_csr_input(monkeypatch):
    n = 7
    rng = np.random.default_rng(410)
    m = gaussian(rng, (1 << n, 1 << n))
    m[rng.random(m.shape) >= 0.2] = 0
    sp = scipy.sparse.csr_matrix(m)
    bx, bz = rng.integers(0, 1 << n, 50).astype('<u8'), rng.integers(0, 1 << n, 50).astype('<u8')
    c_one, form_one = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n, bx, bz)
    monkeypatch.setenv('SYMGPU_PAULI_TILE_BITS', '3')
    c_two, form_two = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n, bx, bz)
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS')
    assert (form_one, form_two) == (kernels.PAULI_ONE_PASS, kernels.PAULI_TWO_PASS)
    full = po.coefficients_of_diagonals(po.diagonals(m, np.arange(1 << n)), np.arange(1 << n), n)
    assert po.bits_equal(c_one, full[bx.astype(np.int64), bz.astype(np.int64)]) and po.bits_equal(c_two, c_one)


def test_two_pass_form_at_its_natural_size(monkeypatch):
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS', raising=False)
    n, side = 14, 1 << 14
    rng = np.random.default_rng(420)
    xs = np.array([0, 0x2A5B], dtype=np.int64)
    diag = gaussian(rng, (2, side))
    b = np.arange(side, dtype=np.int64)
    sp = scipy.sparse.coo_matrix((diag.reshape(-1), (np.tile(b, 2), np.concatenate([b ^ xs[0], b ^ xs[1]]))), shape=(side, side)).tocsr()
    dev, t, form = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n)
    assert form == kernels.PAULI_TWO_PASS
    op = PauliwordOp._from_device(dev, n, t)
    assert_is_restatement(op, n, po.decompose_diagonals(diag, xs, n))
    # tiles of 8: the 11 bits above them take two strided launches (10 + 1)
    monkeypatch.setenv('SYMGPU_PAULI_TILE_BITS', '3')
    dev3, t3, form3 = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n)
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS')
    assert form3 == kernels.PAULI_TWO_PASS
    assert_same_operator(PauliwordOp._from_device(dev3, n, t3), op)


# ---- operator_basis --------------------------------------------------------------------------------------------------------------------
def _with_basis(matrix, basis):
    with pytest.warns(UserWarning, match='MAY not be sufficiently expressive'):
        return PauliwordOp.from_matrix(matrix, operator_basis=basis)


def _assert_projection(res, basis, full):
    """res = the cleaned basis's terms in its order with the full decomposition's coefficients (bits), zeros dropped."""
    cleaned = basis.copy().cleanup()
    x, z = po.xz_of(cleaned.symp_matrix)
    want = [(row, full[(int(a), int(b))]) for row, a, b in zip(cleaned.symp_matrix, x, z) if (int(a), int(b)) in full]
    assert res.n_terms == len(want)
    if want:
        assert np.array_equal(res.symp_matrix, np.array([w[0] for w in want]))
        assert po.bits_equal(res.coeff_vec, np.array([w[1] for w in want]))


@pytest.mark.parametrize('sparse', [False, True])
def test_basis_with_duplicates_and_non_unit_coefficients(sparse):
    n = 3
    rng = np.random.default_rng(500)
    M = gaussian(rng, (8, 8))
    M[rng.random((8, 8)) < 0.4] = 0
    basis = PauliwordOp.from_list(['XYZ', 'IIZ', 'XYZ', 'YYI', 'ZIX', 'IIZ', 'III', 'XXX'], [2, -0.5, 3j, 1, 7, 0.25, -1, 1e-3])
    full = term_dict(PauliwordOp.from_matrix(M))
    res = _with_basis(scipy.sparse.csr_matrix(M) if sparse else M, basis)
    assert basis.copy().cleanup().n_terms == 6
    _assert_projection(res, basis, full)
    assert res.n_terms == 6


@pytest.mark.parametrize('sparse', [False, True])
def test_basis_that_misses_diagonals_and_lists_absent_ones(sparse):
    n, side = 3, 8
    rng = np.random.default_rng(510)
    b = np.arange(side)
    M = np.zeros((side, side), dtype=complex)
    for x in (0, 3, 6):                                              # the matrix lives on the diagonals x = 0, 3, 6
        M[b, b ^ x] = dyadic(rng, side, 0.0)
    # the basis lists x = 0 (III, IIZ), x = 3 (IXY), x = 5 (XIX: no entry of the matrix) and not x = 6
    basis = PauliwordOp.from_list(['III', 'IIZ', 'IXY', 'XIX'], [1, 1, 1, 1])
    full = term_dict(PauliwordOp.from_matrix(M))
    res = _with_basis(scipy.sparse.csr_matrix(M) if sparse else M, basis)
    _assert_projection(res, basis, full)
    assert 'XIX' not in res.to_dictionary and res.n_terms <= 3


def _fixed():
    with open(os.path.join(GOLDEN, 'from_matrix_fixed.json')) as f:
        d = json.load(f)
    mat = lambda rows: np.array([[complex(*v) for v in row] for row in rows])
    return d, mat


def test_reference_examples_reproduce_their_input():
    d, mat = _fixed()
    one = d['defined_basis_dense']
    M = mat(one['matrix'])
    res = _with_basis(M, PauliwordOp.from_dictionary(one['basis']))
    assert np.array_equal(res.to_sparse_matrix.toarray(), M)
    two = d['defined_basis_sparse']
    M2 = mat(two['matrix'])
    res = _with_basis(scipy.sparse.csr_matrix(M2), PauliwordOp.from_dictionary(two['basis']))
    assert np.array_equal(res.to_sparse_matrix.toarray(), M2)
    # {'XX': 1}: the projection onto a basis that cannot express the matrix
    res = _with_basis(M, PauliwordOp.from_dictionary(d['incomplete_basis']['basis']))
    assert res.to_dictionary == {'XX': 1}
    _assert_projection(res, PauliwordOp.from_dictionary({'XX': 1}), term_dict(PauliwordOp.from_matrix(M)))


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
def test_one_by_one_and_all_zero():
    for m in (np.array([[2.5 - 1j]]), scipy.sparse.csr_matrix(np.array([[2.5 - 1j]]))):
        op = PauliwordOp.from_matrix(m)
        assert op.n_qubits == 0 and op.n_terms == 1 and op.coeff_vec[0] == 2.5 - 1j
    for m in (np.zeros((4, 4)), scipy.sparse.csr_matrix((4, 4)), scipy.sparse.csr_matrix(np.zeros((3, 4)))):
        op = PauliwordOp.from_matrix(m)
        assert op.n_terms == 0 and op.symp_matrix.shape == (0, 4) and op.coeff_vec.shape == (0,)


def test_rectangular_complex_input_is_padded_in_complex():
    M = gaussian(np.random.default_rng(600), (5, 3))
    padded = np.zeros((8, 8), dtype=complex)
    padded[:5, :3] = M
    expect = po.decompose(padded, 3)
    assert np.any(expect[2].imag != 0)
    for m in (M, scipy.sparse.csr_matrix(M), scipy.sparse.coo_matrix(M)):
        op = PauliwordOp.from_matrix(m)
        assert_is_restatement(op, 3, expect)
        assert np.allclose(op.to_sparse_matrix.toarray(), padded, rtol=0, atol=1e-14)


def test_np_matrix_input():
    M = dyadic(np.random.default_rng(610), (4, 4))
    assert_is_restatement(PauliwordOp.from_matrix(np.matrix(M)), 2, po.decompose(M, 2))


def test_nan_entry_keeps_its_whole_diagonal_and_nothing_else():
    n = 3
    M = dyadic(np.random.default_rng(620), (8, 8))
    clean = term_dict(PauliwordOp.from_matrix(M))
    M[2, 5] = np.nan                                                 # on the diagonal x = 7
    op = PauliwordOp.from_matrix(M)
    got = term_dict(op)
    x7 = [q for q in got if q[0] == 7]
    assert len(x7) == 8 and all(np.isnan(got[q].real) or np.isnan(got[q].imag) for q in x7)   # i^k moves the NaN between the components
    others = {q: c for q, c in got.items() if q[0] != 7}
    assert others.keys() == {q for q in clean if q[0] != 7}
    assert all(po.bits_equal(np.array([c]), np.array([clean[q]])) for q, c in others.items())
    ex, ez, ec = po.decompose(M, n)
    assert np.array_equal(op.symp_matrix, po.symp_of(ex, ez, n))
    assert np.array_equal(op.coeff_vec.real, ec.real, equal_nan=True) and np.array_equal(op.coeff_vec.imag, ec.imag, equal_nan=True)


def test_argument_errors():
    with pytest.raises(ValueError):
        PauliwordOp.from_matrix(np.eye(4), strategy='magic')
    with pytest.raises(ValueError):
        PauliwordOp.from_matrix([[1, 0], [0, 1]])
    with pytest.raises(ValueError):
        PauliwordOp.from_matrix(scipy.sparse.coo_matrix((2 ** 31 + 1, 1), dtype=complex))
    with pytest.raises(ValueError):
        PauliwordOp.from_matrix(np.eye(4), operator_basis=PauliwordOp.from_dictionary({'XXX': 1}))


# ---- residency ---------------------------------------------------------------------------------------------------------------------------
def test_result_stays_on_the_device_and_only_the_payload_moves():
    n, side = 5, 32
    rng = np.random.default_rng(700)
    M = dyadic(rng, (side, side))
    h2d, d2h, ups, downs = kernels.transfer_counters()
    op = PauliwordOp.from_matrix(M)
    after = kernels.transfer_counters()
    assert after[0] - h2d == 16 * side * side and after[1] == d2h and after[3] == downs
    assert op.n_terms > 0 and op._coeff is None and op._packed_cache is None and op._symp is None
    c = op.coeff_vec
    assert kernels.transfer_counters()[1] - d2h == 16 * op.n_terms and kernels.transfer_counters()[3] == downs + 1
    op.symp_matrix
    assert kernels.transfer_counters()[3] == downs + 2
    # CSR arrays, and the basis words with them
    sp = scipy.sparse.csr_matrix(M)
    payload = sp.data.nbytes + sp.indices.nbytes + sp.indptr.nbytes
    h2d, d2h, ups, downs = kernels.transfer_counters()
    op = PauliwordOp.from_matrix(sp)
    after = kernels.transfer_counters()
    assert after[0] - h2d == payload and after[1] == d2h and after[3] == downs
    bx, bz = np.arange(7, dtype='<u8'), np.arange(7, dtype='<u8')[::-1].copy()
    h2d, d2h, ups, downs = kernels.transfer_counters()
    coeff, _ = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n, bx, bz)
    after = kernels.transfer_counters()
    assert after[0] - h2d == payload + 2 * 8 * 7 and after[1] - d2h == 16 * 7 and after[3] == downs


# ---- a molecular Hamiltonian and a random unitary ----------------------------------------------------------------------------------------
def test_molecular_round_trip():
    with open(os.path.join(GOLDEN, 'B+_STO-3G_SINGLET_JW.json')) as f:
        d = json.load(f)
    H = PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()}).cleanup()
    n, T = H.n_qubits, H.n_terms
    back = PauliwordOp.from_matrix(H.to_sparse_matrix)
    atol = (T + n) * 2.0 ** -53 * float(np.sum(np.abs(H.coeff_vec)))
    got = term_dict(back)
    hx, hz = po.xz_of(H.symp_matrix)
    expected = {(int(a), int(b)): c for a, b, c in zip(hx, hz, H.coeff_vec)}
    assert len(expected) == T
    for q, c in expected.items():
        assert q in got or abs(c) <= atol, f'term {q} of the Hamiltonian is missing'
        assert abs(got.get(q, 0j) - c) <= atol, f'term {q}: {got.get(q)} vs {c}'
    for q, c in got.items():
        if q not in expected:
            assert abs(c) <= atol, f'spurious term {q}: {c}'


def test_haar_random():
    np.random.seed(11)
    op = PauliwordOp.haar_random(3)
    assert op.n_qubits == 3 and 0 < op.n_terms <= 64
    U = op.to_sparse_matrix.toarray()
    assert np.allclose(U @ U.conj().T, np.eye(8), rtol=0, atol=1e-12)
    assert PauliwordOp.haar_random(2, strategy='full_basis', disable_loading_bar=True).n_qubits == 2


# ---- the C ABI refuses bad arguments before it touches the device --------------------------------------------------------------------------
def _refusals():
    L = _lib.lib()
    m = np.eye(4, dtype=np.complex128)
    sp = scipy.sparse.identity(4, dtype=np.complex128, format='csr')
    bx = np.zeros(2, dtype='<u8')
    co = np.zeros(2, dtype=np.complex128)
    out, n_out, form = ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int(0)
    o, t, f = ctypes.byref(out), ctypes.addressof(n_out), ctypes.addressof(form)
    A = _lib.addr
    dense, csr = L.symgpu_from_matrix_dense, L.symgpu_from_matrix_csr
    good_csr = (A(sp.data), A(sp.indices), A(sp.indptr), 4, 4, 2)
    return out, [
        ('dense: null matrix', lambda: dense(None, 2, None, None, 0, o, t, None, f)),
        ('dense: n = 0', lambda: dense(A(m), 0, None, None, 0, o, t, None, f)),
        ('dense: n = 32', lambda: dense(A(m), 32, None, None, 0, o, t, None, f)),
        ('dense: null out', lambda: dense(A(m), 2, None, None, 0, None, t, None, f)),
        ('dense: null n_out', lambda: dense(A(m), 2, None, None, 0, o, None, None, f)),
        ('dense: K > 0, null basis_x', lambda: dense(A(m), 2, None, A(bx), 2, o, t, A(co), f)),
        ('dense: K > 0, null basis_z', lambda: dense(A(m), 2, A(bx), None, 2, o, t, A(co), f)),
        ('dense: K > 0, null coeff_out', lambda: dense(A(m), 2, A(bx), A(bx), 2, o, t, None, f)),
        ('dense: K < 0', lambda: dense(A(m), 2, None, None, -1, o, t, None, f)),
        ('dense: basis word out of range', lambda: dense(A(m), 2, A(np.array([4, 0], dtype='<u8')), A(bx), 2, o, t, A(co), f)),
        ('dense: all terms at n = 16', lambda: dense(A(m), 16, None, None, 0, o, t, None, f)),
        ('csr: null indptr', lambda: csr(A(sp.data), A(sp.indices), None, 4, 4, 2, None, None, 0, o, t, None, f)),
        ('csr: null data', lambda: csr(None, A(sp.indices), A(sp.indptr), 4, 4, 2, None, None, 0, o, t, None, f)),
        ('csr: negative nnz', lambda: csr(A(sp.data), A(sp.indices), A(sp.indptr), 4, -1, 2, None, None, 0, o, t, None, f)),
        ('csr: index_bytes 3', lambda: csr(A(sp.data), A(sp.indices), A(sp.indptr), 3, 4, 2, None, None, 0, o, t, None, f)),
        ('csr: n = 0', lambda: csr(A(sp.data), A(sp.indices), A(sp.indptr), 4, 4, 0, None, None, 0, o, t, None, f)),
        ('csr: n = 32', lambda: csr(A(sp.data), A(sp.indices), A(sp.indptr), 4, 4, 32, None, None, 0, o, t, None, f)),
        ('csr: null out', lambda: csr(*good_csr, None, None, 0, None, t, None, f)),
        ('csr: K > 0, null basis', lambda: csr(*good_csr, None, None, 2, o, t, A(co), f)),
        ('csr: K > 0, null coeff_out', lambda: csr(*good_csr, A(bx), A(bx), 2, o, t, None, f)),
    ], (m, sp, bx, co, n_out, form)


@pytest.mark.parametrize('k', range(20))
def test_c_abi_refusals(k):
    out, cases, keep = _refusals()
    assert len(cases) == 20
    name, call = cases[k]
    before = (kernels.transfer_counters(), kernels.counter('DEV_MALLOC_CALLS'))
    assert call() == _lib.E_INVALID, name
    assert 'invalid argument' in _lib.last_error()
    assert (kernels.transfer_counters(), kernels.counter('DEV_MALLOC_CALLS')) == before, f'{name}: the device was touched'
    assert not out.value


def test_c_abi_refuses_broken_csr_arrays():
    """Found on the device, before anything is scattered: a column outside the matrix, an indptr that does not ascend to nnz."""
    sp = scipy.sparse.identity(4, dtype=np.complex128, format='csr')
    out, n_out = ctypes.c_void_p(), ctypes.c_int64(0)
    bad_col = sp.indices.copy(); bad_col[2] = 4
    bad_ptr = sp.indptr.copy(); bad_ptr[2] = 0                      # 0, 1, 0, 3, 4
    short_ptr = sp.indptr.copy(); short_ptr[-1] = 3
    for what, indices, indptr in (('column 4', bad_col, sp.indptr), ('descending indptr', sp.indices, bad_ptr), ('indptr ends below nnz', sp.indices, short_ptr)):
        rc = _lib.lib().symgpu_from_matrix_csr(_lib.addr(sp.data), _lib.addr(indices), _lib.addr(indptr), 4, 4, 2, None, None, 0, ctypes.byref(out),
                                               ctypes.addressof(n_out), None, None)
        assert rc == _lib.E_INVALID and not out.value, what
    dev, t, form = kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, 2)
    assert t == 1 and form == kernels.PAULI_ONE_PASS                 # the same arrays, intact: the identity matrix is the term II
    dev.free()


# ---- the families of tests/_csr_families.py: index width, block bases of the dense gather, more than 16 qubits -------------------------
def _in_both_forms(monkeypatch, n, call):
    """call() in the one-pass form and with tiles of 8 slots (two-pass above 3 qubits); the forms are asserted."""
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS', raising=False)
    one = call()
    monkeypatch.setenv('SYMGPU_PAULI_TILE_BITS', '3')
    two = call()
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS')
    assert one[-1] == kernels.PAULI_ONE_PASS and two[-1] == (kernels.PAULI_TWO_PASS if n > 3 else kernels.PAULI_ONE_PASS)
    return one, two


def _terms_of(result):
    """(packed rows, coefficients, term count) of a (DeviceOp, n_terms, form) result; the handle is freed."""
    dev, t, _ = result
    rows, coeff = dev.download()
    dev.free()
    assert rows.shape[0] == t == coeff.shape[0]
    return rows, coeff, t


def _packed_of(x, z, n):
    """uint64[T, 2] of terms given as n-bit integers (qubit 0 the most significant bit): qubit q is bit q of the packed word."""
    x, z = np.asarray(x, dtype=np.uint64), np.asarray(z, dtype=np.uint64)
    out = np.zeros((len(x), 2), dtype='<u8')
    for q in range(n):
        s = np.uint64(n - 1 - q)
        out[:, 0] |= ((x >> s) & np.uint64(1)) << np.uint64(q)
        out[:, 1] |= ((z >> s) & np.uint64(1)) << np.uint64(q)
    return out


def test_packed_of_is_pack_rows():
    rng = np.random.default_rng(800)
    x, z = rng.integers(0, 1 << 20, 300), rng.integers(0, 1 << 20, 300)
    assert np.array_equal(_packed_of(x, z, 20), packing.pack_rows(po.symp_of(x, z, 20)).reshape(300, 2))


@pytest.mark.parametrize('which', ['three diagonals', 'density 0.3', 'duplicates, unsorted', 'coo with duplicates', 'csc', 'stored zeros'])
def test_int64_csr_indices_equal_int32(monkeypatch, which):
    n, inputs = _csr_inputs()
    m = scipy.sparse.csr_matrix(inputs[which], dtype=np.complex128, copy=True)
    m.sum_duplicates()
    m.sort_indices()
    if which == 'stored zeros':
        assert np.count_nonzero(m.data == 0) > 100               # kept: a stored zero is an entry like any other
    expect = po.decompose(m.toarray(), n)
    for width in (np.int32, np.int64):
        idx, ptr = m.indices.astype(width), m.indptr.astype(width)
        for res in _in_both_forms(monkeypatch, n, lambda: kernels.pauli_decompose_csr(m.data, idx, ptr, n)):
            rows, coeff, t = _terms_of(res)
            assert np.array_equal(rows, _packed_of(expect[0], expect[1], n)), width
            assert po.bits_equal(coeff, expect[2]), width


def test_int64_csr_indices_with_a_basis(monkeypatch):
    n = 7
    rng = np.random.default_rng(410)
    m = gaussian(rng, (1 << n, 1 << n))
    m[rng.random(m.shape) >= 0.2] = 0
    sp = scipy.sparse.csr_matrix(m)
    bx, bz = rng.integers(0, 1 << n, 50).astype('<u8'), rng.integers(0, 1 << n, 50).astype('<u8')
    full = po.coefficients_of_diagonals(po.diagonals(m, np.arange(1 << n)), np.arange(1 << n), n)
    want = full[bx.astype(np.int64), bz.astype(np.int64)]
    for width in (np.int32, np.int64):
        idx, ptr = sp.indices.astype(width), sp.indptr.astype(width)
        for c, _ in _in_both_forms(monkeypatch, n, lambda: kernels.pauli_decompose_csr(sp.data, idx, ptr, n, bx, bz)):
            assert po.bits_equal(c, want), width


@pytest.mark.parametrize('n, name', [(n, name) for n in sorted(fam.BLOCK_BASES) for name in fam.BLOCK_BASES[n]])
def test_dense_input_with_block_bases(monkeypatch, n, name):
    """The basis path of k_pd_gather_dense: blocks of 32 X-parts with bit 0 only, bit 31 only, all 32 bits, absent blocks, the last
    block of the range (tests/test_csr_families.py proves the masks).  The matrix is full, so a diagonal gathered into the wrong rank
    or from the wrong block brings other numbers."""
    bx, bz, facts = fam.block_basis(n, name)
    M = gaussian(np.random.default_rng(900 + n), (1 << n, 1 << n))
    full = po.coefficients_of_diagonals(po.diagonals(M, np.arange(1 << n)), np.arange(1 << n), n)
    want = full[bx.astype(np.int64), bz.astype(np.int64)]
    assert want.shape == (facts['K'],) and np.all(want != 0)
    for c, _ in _in_both_forms(monkeypatch, n, lambda: kernels.pauli_decompose_dense(M, n, bx, bz)):
        assert po.bits_equal(c, want), 'dense input'
    sp = scipy.sparse.csr_matrix(M)
    for c, _ in _in_both_forms(monkeypatch, n, lambda: kernels.pauli_decompose_csr(sp.data, sp.indices, sp.indptr, n, bx, bz)):
        assert po.bits_equal(c, want), 'CSR input'


_N20 = {}


def _n20():
    """Two diagonals of 2^20 Gaussian entries on the X-parts of the large-n family, as CSR arrays, and the restatement's coefficients of
    both diagonals (built once, shared, not written to)."""
    if not _N20:
        n, side = 20, 1 << 20
        symp, _, facts = fam.large_n(n)
        xs = np.array([x for x in facts['x_parts'] if x], dtype=np.int64)
        assert len(xs) == 2 and xs[0] == 1 << 19 and xs[1] & 1 and xs[1] > xs[0]
        diag = gaussian(np.random.default_rng(430), (2, side))
        b = np.arange(side, dtype=np.int64)
        sp = scipy.sparse.coo_matrix((diag.reshape(-1), (np.tile(b, 2), np.concatenate([b ^ xs[0], b ^ xs[1]]))), shape=(side, side)).tocsr()
        sp.sort_indices()
        _N20.update(n=n, xs=xs, sp=sp, coeff=po.coefficients_of_diagonals(diag, xs, n))
    return _N20


@pytest.mark.parametrize('width', [np.int32, np.int64])
def test_n20_natural_two_pass(monkeypatch, width):
    monkeypatch.delenv('SYMGPU_PAULI_TILE_BITS', raising=False)
    g = _n20()
    n, sp, xs, c = g['n'], g['sp'], g['xs'], g['coeff']
    idx, ptr = sp.indices.astype(width), sp.indptr.astype(width)
    res = kernels.pauli_decompose_csr(sp.data, idx, ptr, n)
    assert res[2] == kernels.PAULI_TWO_PASS                           # 13 bits in contiguous tiles, 7 in one strided launch
    rows, coeff, t = _terms_of(res)
    keep = ~((c.real == 0) & (c.imag == 0))
    j, z = np.nonzero(keep)
    assert t == len(j) and t > 2 * (1 << n) - 16
    assert np.array_equal(rows, _packed_of(xs[j], z, n))
    assert po.bits_equal(coeff, c[keep])
    # a basis of 50 picks: both diagonals and one X-part that the matrix does not have
    rng = np.random.default_rng(431)
    absent = 0x2A5B
    bx = rng.choice(np.array([xs[0], xs[1], absent]), 50).astype('<u8')
    bz = rng.integers(0, 1 << n, 50).astype('<u8')
    assert {int(v) for v in bx} == {int(xs[0]), int(xs[1]), absent}
    picked, form = kernels.pauli_decompose_csr(sp.data, idx, ptr, n, bx, bz)
    want = np.where(bx == absent, 0, c[np.searchsorted(xs, np.minimum(bx.astype(np.int64), xs[1])), bz.astype(np.int64)])
    assert form == kernels.PAULI_TWO_PASS and po.bits_equal(picked, want)


def test_round_trip_at_19_qubits():
    """P -> to_csr with int64 indices -> pauli_decompose_csr on those very arrays -> P's terms in (x, z) order, bit for bit (dyadic:
    the 2^19 entries of a diagonal sum exactly)."""
    n = 19
    symp, c, facts = fam.large_n(n)
    data, indices, indptr = kernels.to_csr(PauliwordOp(symp, c)._device(), n, index_dtype=np.int64)
    assert indices.dtype == np.int64 and indptr.dtype == np.int64 and len(data) == facts['nnz']
    rows, coeff, t = _terms_of(kernels.pauli_decompose_csr(data, indices, indptr, n))
    x, z = po.xz_of(symp)
    order = np.lexsort((z, x))
    assert t == 6 and np.array_equal(rows, _packed_of(x[order], z[order], n))
    assert np.array_equal(rows, packing.pack_rows(symp[order]).reshape(6, 2))
    assert po.bits_equal(coeff, c[order])


@pytest.mark.parametrize('width', [np.int32, np.int64])
def test_empty_and_one_entry_csr(width):
    n = 3
    none = np.zeros(0, dtype=np.complex128)
    idx, ptr = np.zeros(0, dtype=width), np.zeros((1 << n) + 1, dtype=width)
    rows, coeff, t = _terms_of(kernels.pauli_decompose_csr(none, idx, ptr, n))
    assert t == 0 and rows.shape[0] == 0 and coeff.shape == (0,)
    bx, bz = np.array([0, 7, 3, 0], dtype='<u8'), np.array([1, 7, 0, 0], dtype='<u8')
    picked, _ = kernels.pauli_decompose_csr(none, idx, ptr, n, bx, bz)
    assert po.bits_equal(picked, np.zeros(4, dtype=np.complex128))
    # one qubit, one stored entry: M = [[0, 2 - i], [0, 0]] = (1 - i/2) X + (1/2 + i) Y
    M = np.array([[0, 2 - 1j], [0, 0]])
    dev, t, form = kernels.pauli_decompose_csr(np.array([2 - 1j]), np.array([1], dtype=width), np.array([0, 1, 1], dtype=width), 1)
    assert form == kernels.PAULI_ONE_PASS
    expect = po.decompose(M, 1)
    assert expect[0].tolist() == [1, 1] and expect[1].tolist() == [0, 1] and expect[2].tolist() == [1 - 0.5j, 0.5 + 1j]
    assert_is_restatement(PauliwordOp._from_device(dev, 1, t), 1, expect)
