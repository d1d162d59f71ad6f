"""PauliwordOp.to_sparse_matrix on the device (csrc/sparse_matrix.hip) and QuantumState's sparse / dense vectors, against the definition
(an explicit Kronecker product), the NumPy restatement of the contract (tests/_sparse_oracle.py) and two molecular Hamiltonians."""
import json
import os

import numpy as np
import pytest
import scipy.sparse

import _sparse_oracle as so
from symmer_amd import PauliwordOp, QuantumState, kernels, packing

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 8.0


def random_symp(rng, n, t, p=0.4):
    return rng.random((t, 2 * n)) < p


def assert_canonical(A, n):
    side = 1 << n
    assert isinstance(A, scipy.sparse.csr_matrix)
    assert A.shape == (side, side) and A.dtype == np.complex128
    assert A.has_canonical_format
    assert np.all(np.diff(A.indptr) >= 0) and A.indptr[0] == 0 and A.indptr[-1] == A.nnz
    assert not np.any((A.data.real == 0) & (A.data.imag == 0)), 'a stored +-0 entry'
    for r in range(min(side, 256)):
        assert np.all(np.diff(A.indices[A.indptr[r]:A.indptr[r + 1]]) > 0)


def assert_csr_equal(got, want, exact=True):
    d, i, p = got
    wd, wi, wp = want
    assert np.array_equal(p, wp) and np.array_equal(i, wi)
    if exact:
        assert np.array_equal(d.view(np.float64), wd.view(np.float64)), 'data not bit-equal'
    else:
        assert np.allclose(d, wd, rtol=0, atol=1e-12)


BALANCE = ('DEV_BLOCKS_LIVE', 'DEV_FREE_UNKNOWN')


@pytest.fixture(scope='module', autouse=True)
def plans_and_buffers_are_balanced():
    """DEV_BLOCKS_LIVE is the same before and after the module's tests (after one warm-up call: the context keeps its sort state)."""
    rng = np.random.default_rng(0)
    kernels.to_csr(PauliwordOp(random_symp(rng, 5, 30), dyadic(rng, 30))._device(), 5)
    before = kernels.counters(BALANCE)
    yield
    assert np.array_equal(kernels.counters(BALANCE), before)


def test_a_plan_released_without_a_fill_leaves_nothing():
    """The routes on which to_csr gives a plan up: a fill call of null buffers, and a fill call that is refused."""
    import ctypes
    from symmer_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(9)
    n = 5
    Z0 = np.zeros((1, 2 * n), dtype=bool); Z0[0, n] = True
    for symp, c, nnz_want in ((np.vstack([Z0, Z0]), np.array([1.0, -1.0]), 0), (random_symp(rng, n, 30), dyadic(rng, 30), None)):
        with kernels.DeviceOp.upload(packing.pack_rows(symp), c) as op:
            before = kernels.counters(BALANCE)
            for refused in (False, True):
                nnz, scratch, plan = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_void_p()
                _lib.check(lib.symgpu_to_csr_count(op.handle, n, ctypes.addressof(nnz), ctypes.addressof(scratch), ctypes.byref(plan)))
                assert plan.value and (nnz.value == nnz_want if nnz_want is not None else nnz.value > 0)
                assert kernels.counters(BALANCE)[0] > before[0], 'the plan holds device blocks'
                if refused:                                    # an index width that is neither 4 nor 8: refused, the plan released all the same
                    indptr = np.empty((1 << n) + 1, dtype=np.int64)
                    assert lib.symgpu_to_csr_fill(plan, None, None, _lib.addr(indptr), 3) == _lib.E_INVALID
                else:
                    _lib.check(lib.symgpu_to_csr_fill(plan, None, None, None, 4))
                assert np.array_equal(kernels.counters(BALANCE), before)


# ---- the definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', range(1, 9))
def test_matches_kron_random(n):
    rng = np.random.default_rng(10 + n)
    symp, c = random_symp(rng, n, 4 * n + 3), dyadic(rng, 4 * n + 3)
    A = PauliwordOp(symp, c).to_sparse_matrix
    assert_canonical(A, n)
    assert np.array_equal(A.toarray(), so.kron_dense(symp, c))


@pytest.mark.parametrize('n', [1, 3, 6])
def test_single_terms_identity_and_all_y(n):
    rng = np.random.default_rng(n)
    I = np.zeros((1, 2 * n), dtype=bool)
    Y = np.ones((1, 2 * n), dtype=bool)
    for symp, c in ((I, [1.0]), (Y, [0.5 - 0.25j]), (random_symp(rng, n, 1), [-1j]), (np.vstack([Y, Y, I]), [1, 1j, -2])):
        A = PauliwordOp(symp, c).to_sparse_matrix
        assert_canonical(A, n)
        assert np.array_equal(A.toarray(), so.kron_dense(symp, c))
    assert PauliwordOp(I, [1.0]).to_sparse_matrix.nnz == 1 << n


def test_duplicates_zeros_and_exact_cancellation():
    rng = np.random.default_rng(5)
    n = 5
    symp = random_symp(rng, n, 12)
    symp = np.vstack([symp, symp[:6]])
    c = dyadic(rng, 18)
    c[3] = 0
    c[12:] = -c[:6]                                            # the first six terms cancel exactly
    A = PauliwordOp(symp, c).to_sparse_matrix
    assert_canonical(A, n)
    assert np.array_equal(A.toarray(), so.kron_dense(symp, c))
    # I + Z on qubit 0: the lower half of the diagonal cancels to an exact zero and is not stored
    I = np.zeros(2 * n, dtype=bool)
    Z0 = I.copy(); Z0[n] = True
    A = PauliwordOp(np.vstack([I, Z0]), [1.0, 1.0]).to_sparse_matrix
    assert A.nnz == 1 << (n - 1) and np.array_equal(A.indices, np.arange(1 << (n - 1)))
    assert PauliwordOp(np.vstack([Z0, Z0]), [1.0, -1.0]).to_sparse_matrix.nnz == 0


def test_nan_coefficient_is_stored():
    rng = np.random.default_rng(8)
    n = 4
    symp = random_symp(rng, n, 5)
    c = dyadic(rng, 5)
    c[2] = complex(np.nan, 0.0)
    A = PauliwordOp(symp, c).to_sparse_matrix
    x = so.bits_to_int(symp[2:3, :n])[0]
    for b in range(1 << n):
        row = A.indices[A.indptr[b]:A.indptr[b + 1]]
        assert b ^ x in row
        assert np.isnan(A.data[A.indptr[b] + np.searchsorted(row, b ^ x)].real)


# ---- against the NumPy restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, T', [(3, 40), (7, 200), (10, 600), (12, 1500), (14, 3000), (16, 10 ** 4)])
def test_to_csr_matches_oracle(n, T):
    rng = np.random.default_rng(1000 + n)
    # chemistry-like: many terms share their X-part (Z-only terms, a few hundred X-parts)
    x_parts = random_symp(rng, n, min(300, T // 4), 0.3)[:, :n]
    xs = x_parts[rng.integers(0, len(x_parts), T)]
    xs[: T // 3] = False
    symp = np.hstack([xs, rng.random((T, n)) < 0.4])
    cases = [(True, dyadic(rng, T))] + ([(False, rng.normal(size=T) + 1j * rng.normal(size=T))] if n < 16 else [])
    for exact, c in cases:
        want = so.to_csr(symp, c)
        assert want[0].nbytes + want[1].nbytes < 1 << 30
        op = PauliwordOp(symp, c)
        got = kernels.to_csr(op._device(), n)
        assert got[1].dtype == np.int32 and got[2].dtype == np.int32
        assert_csr_equal(got, want, exact)


LDS_MAX_D = 72 * 1024 // (20 * 32)       # the LDS fill needs 32 rows of D slots of 20 B in 72 KiB (csrc/sparse_matrix.hip): D <= 115


def _chemistry_like(rng, n, T, x_parts):
    xs = (rng.random((x_parts, n)) < 0.3)[rng.integers(0, x_parts, T)]
    xs[: T // 3] = False
    return np.hstack([xs, rng.random((T, n)) < 0.4])


def _fill_scratch_bytes(op, n):
    """The count call's report of the fill's scratch: 0 when the fill keeps its slots in LDS."""
    import ctypes
    from symmer_amd import _lib
    nnz, scratch, plan = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p()
    _lib.check(_lib.lib().symgpu_to_csr_count(op._device().handle, n, ctypes.addressof(nnz), ctypes.addressof(scratch), ctypes.byref(plan)))
    _lib.check(_lib.lib().symgpu_to_csr_fill(plan, None, None, None, 4))
    return scratch.value


def test_fill_lds_against_forced_scratch(monkeypatch):
    from symmer_amd import _lib
    rng = np.random.default_rng(78)
    n, T = 12, 2000
    symp = _chemistry_like(rng, n, T, 60)
    c = dyadic(rng, T)
    D = len(np.unique(so.bits_to_int(symp[:, :n])))
    assert 20 <= D <= LDS_MAX_D, D                             # the default fill runs in LDS, over 2^12 / (72 KiB / 20 D) workgroups
    op = PauliwordOp(symp, c)
    monkeypatch.delenv('SYMGPU_CSR_SCRATCH', raising=False)
    assert _fill_scratch_bytes(op, n) == 0, 'the default fill did not take the LDS form'
    default = kernels.to_csr(op._device(), n)
    monkeypatch.setenv('SYMGPU_CSR_SCRATCH', '1')
    assert _fill_scratch_bytes(op, n) > 0, 'SYMGPU_CSR_SCRATCH=1 did not force the scratch form'
    forced = kernels.to_csr(op._device(), n)
    want = so.to_csr(symp, c)
    assert_csr_equal(default, want)
    assert_csr_equal(forced, want)
    assert not any('k_csr_fill' in t for t in _lib.degraded())


def test_fill_above_lds_cap():
    rng = np.random.default_rng(77)
    n, T = 12, 12000
    symp, c = random_symp(rng, n, T, 0.5), dyadic(rng, T)
    D = len(np.unique(so.bits_to_int(symp[:, :n])))
    assert D > LDS_MAX_D and D * 20 > 72 * 1024, 'the case must exceed the LDS slot budget of one row'
    op = PauliwordOp(symp, c)
    assert _fill_scratch_bytes(op, n) > 0
    assert_csr_equal(kernels.to_csr(op._device(), n), so.to_csr(symp, c))


# ---- molecules -------------------------------------------------------------------------------------------------------------------
def _molecule(name):
    with open(os.path.join(GOLDEN, name)) as f:
        d = json.load(f)
    H = PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()})
    return H, d['data']


@pytest.mark.parametrize('name', ['B+_STO-3G_SINGLET_JW.json', 'BH_STO-3G_SINGLET_JW.json'])
def test_molecule_energies(name):
    H, data = _molecule(name)
    n = H.n_qubits
    A = H.to_sparse_matrix
    assert_canonical(A, n)
    assert abs(A - A.conj().T).max() < 1e-12, 'not Hermitian'
    hf = data['hf_array']
    hf_idx = int(''.join(str(b) for b in hf), 2)
    e_hf = A[hf_idx, hf_idx]
    assert abs(e_hf - data['calculated_properties']['HF']['energy']) < 1e-10
    sector = np.array([i for i in range(1 << n) if bin(i).count('1') == data['n_particles']])
    block = A[sector][:, sector].toarray()
    e_fci = np.linalg.eigvalsh(block)[0]
    assert abs(e_fci - data['calculated_properties']['FCI']['energy']) < 1e-9
    assert abs(H.expval(QuantumState(hf)) - e_hf.real) < 1e-10


# ---- QuantumState ----------------------------------------------------------------------------------------------------------------
def test_quantum_state_vectors_and_expval():
    H, _ = _molecule('B+_STO-3G_SINGLET_JW.json')
    n = H.n_qubits
    psi0 = QuantumState([[1, 0, 1] + [0] * (n - 3), [0, 1, 1] + [0] * (n - 3)], [0.6, 0.8j])
    ket, bra = psi0.to_sparse_matrix, psi0.dagger.to_sparse_matrix
    assert ket.shape == (1 << n, 1) and bra.shape == (1, 1 << n) and ket.dtype == np.complex128
    assert ket[int('101' + '0' * (n - 3), 2), 0] == 0.6 and bra[0, int('011' + '0' * (n - 3), 2)] == -0.8j
    assert np.array_equal(psi0.to_dense_matrix, ket.toarray())
    np.random.seed(3)
    A = H.to_sparse_matrix
    for terms in (5, 40):
        psi = QuantumState.random(n, terms)
        val = (psi.dagger.to_dense_matrix @ (A @ psi.to_dense_matrix))[0, 0]
        assert abs(val - H.expval(psi)) < 1e-12


# ---- edge cases ------------------------------------------------------------------------------------------------------------------
def test_edge_cases():
    z = PauliwordOp(np.zeros((3, 0), dtype=bool), [1, 2j, 3])
    A = z.to_sparse_matrix
    assert A.shape == (1, 3) and np.array_equal(A.toarray(), [[1, 2j, 3]])
    e = PauliwordOp(np.zeros((0, 16), dtype=bool), [])
    A = e.to_sparse_matrix
    assert A.shape == (256, 256) and A.nnz == 0
    with pytest.raises(ValueError):
        PauliwordOp(np.zeros((1, 64), dtype=bool), [1]).to_sparse_matrix
    with pytest.raises(ValueError):
        kernels.to_csr(PauliwordOp(np.zeros((1, 64), dtype=bool), [1])._device(), 32)


def test_device_product_and_coeff_change():
    rng = np.random.default_rng(21)
    n = 7
    P = PauliwordOp(random_symp(rng, n, 20), dyadic(rng, 20))
    Q = PauliwordOp(random_symp(rng, n, 15), dyadic(rng, 15))
    R = P * Q
    assert R._dev is not None and R._symp is None and R._packed_cache is None, 'the product is expected on the device only'
    A = R.to_sparse_matrix
    host = PauliwordOp(R.symp_matrix.copy(), R.coeff_vec.copy())
    assert_csr_equal((A.data, A.indices, A.indptr), (lambda B: (B.data, B.indices, B.indptr))(host.to_sparse_matrix))
    # a copy whose matrix was never formed, resident on the device, then negated through coeff_vec: the device coefficients are refreshed
    fresh = PauliwordOp(R.symp_matrix.copy(), R.coeff_vec.copy())
    fresh._device()
    fresh.coeff_vec *= -1
    B = fresh.to_sparse_matrix
    assert np.array_equal(B.toarray(), -A.toarray())
    # the cached matrix does not follow a later change of coeff_vec (as in the reference); copies carry the cached matrix with them
    fresh.coeff_vec *= -1
    assert fresh.to_sparse_matrix is B and fresh.copy().to_sparse_matrix.nnz == B.nnz
