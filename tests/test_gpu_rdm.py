"""GPU: symgpu_rdm (csrc/rdm.hip) — the reduced density matrix rho = M M^+ of a dense statevector in its two forms — and what stands on it:
kernels.rdm_dev, QuantumState.get_rdm / partial_trace_over_qubits, get_entanglement_entropy.  Expected matrices come from the NumPy
restatement (tests/_rdm_oracle.py, held against the reference's stored answers by tests/test_rdm_oracle.py); Gaussian amplitudes within
its entry tolerance 4 (m + 8) 2^-53 r_a r_a', dyadic amplitudes (integers in [-8, 8] over 8, both components: every product and sum is
exact) equal to it, the signs of zeros aside.  Every case also checks: rho is its own conjugate transpose byte for byte (the diagonal's
imaginary part +0.0), the trace within sum_a tol[a][a] of sum |psi|^2, a second call returns the same bytes, psi is unchanged."""
import ctypes
import json
import os
from itertools import combinations

import numpy as np
import pytest

import _rdm_oracle as ro
from symmer_amd import PauliwordOp, QuantumState, _lib, exact_gs_energy, get_entanglement_entropy, kernels

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
STREAM, TILED = kernels.RDM_STREAM, kernels.RDM_TILED
PATTERNS = ('low', 'high', 'interleaved')
KS, TILE_EDGE = 3, 64          # what include/symgpu.h (f9) documents for info[1] and info[3]: the one place a retune has to touch here


def gaussian(rng, n):
    return rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)


def dyadic(rng, n):
    return (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / 8.0


class forced:
    """``with forced('tiled'):`` — SYMGPU_RDM_FORM for the calls inside; None leaves the choice to the library."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.before = os.environ.pop('SYMGPU_RDM_FORM', None)
        if self.form is not None:
            os.environ['SYMGPU_RDM_FORM'] = self.form

    def __exit__(self, *exc):
        os.environ.pop('SYMGPU_RDM_FORM', None)
        if self.before is not None:
            os.environ['SYMGPU_RDM_FORM'] = self.before
        return False


def assert_hermitian_to_the_byte(rho):
    re, im = np.ascontiguousarray(rho.real), np.ascontiguousarray(rho.imag)
    diag = np.diag_indices(rho.shape[0])
    assert np.all(im[diag] == 0.0) and not np.any(np.signbit(im[diag])), 'the diagonal has an imaginary part (or -0.0)'
    assert re.tobytes() == np.ascontiguousarray(re.T).tobytes()
    mirrored = np.ascontiguousarray(-im.T)
    mirrored[diag] = 0.0
    assert im.tobytes() == mirrored.tobytes()


def check(psi, n, kept, form=None, exact=False, expect_form=None):
    """One case, every property of the module docstring; returns info."""
    psi = np.ascontiguousarray(psi, dtype=np.complex128)
    want, tol = ro.rdm_deposit(psi, n, kept), ro.entry_tolerance(psi, n, kept)
    with kernels.DeviceBuffer.upload(psi) as buf, forced(form):
        rho, info = kernels.rdm_dev(buf, n, kept, want_info=True)
        again = kernels.rdm_dev(buf, n, kept)
        after = buf.download(np.complex128, 1 << n)
    k = len(set(kept))
    assert rho.shape == (1 << k, 1 << k) and rho.dtype == np.complex128
    err = np.abs(rho - want)
    print(f'n = {n} kept = {list(kept)} form {info[0]} chunks {info[2]} workgroups {info[4]} scratch {info[5]}: '
          f'max error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3g}')
    if exact:
        assert np.array_equal(rho, want)
    assert np.all(err <= tol), (n, list(kept), float(err.max()))
    assert_hermitian_to_the_byte(rho)
    assert abs(np.trace(rho).real - np.sum(psi.real ** 2 + psi.imag ** 2)) <= np.trace(tol)
    assert rho.tobytes() == again.tobytes(), 'a second call gave other bytes'
    assert psi.tobytes() == after.tobytes(), 'psi was written'
    assert info[1] == KS and info[0] in (STREAM, TILED) and info[2] >= 1 and info[4] >= info[2] and info[5] > 0
    assert info[3] == (TILE_EDGE if info[0] == TILED else 0)
    if expect_form is not None:
        assert info[0] == expect_form
    return info


# ---- every small case ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', range(1, 7))
def test_every_single_qubit_and_pair_up_to_six_qubits(n):
    rng = np.random.default_rng(100 + n)
    g, d = gaussian(rng, n), dyadic(rng, n)
    kepts = [[]] + [[q] for q in range(n)] + [list(p) for p in combinations(range(n), 2)] + [list(range(n))]
    for kept in kepts:
        form = None if len(kept) <= KS else TILED
        check(g, n, kept, expect_form=form if form else STREAM)
        check(d, n, kept, exact=True)
        check(d, n, kept, form='tiled', exact=True, expect_form=TILED)
        check(g, n, kept, form='tiled', expect_form=TILED)


# ---- the boundary between the forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('extra', (0, 1, 9))
def test_form_boundary(extra, pattern):
    rng = np.random.default_rng(7)
    KS = int(check(gaussian(rng, 2), 2, [0])[1])
    for k in (KS, KS + 1):
        n = k + extra
        kept = ro.kept_patterns(n, k)[pattern]
        g, d = gaussian(rng, n), dyadic(rng, n)
        check(g, n, kept, expect_form=STREAM if k <= KS else TILED)
        check(d, n, kept, form='tiled', exact=True, expect_form=TILED)
        check(g, n, kept, form='tiled', expect_form=TILED)
        check(d, n, kept, form='stream', exact=True, expect_form=STREAM if k <= KS else TILED)      # beyond KS the switch is ignored


# ---- the first cut of the traced index -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,k,documented', [('stream', 2, 9), ('tiled', 4, 5), ('tiled', 2, 5)])
def test_chunk_boundary(form, k, documented):
    """n - k from 0 up to the first size at which the traced index is cut in two: every size below it is one chunk (and, below the
    staged block of 2^8 / 2^4 values, a partial block), and the first cut comes where the header says."""
    rng = np.random.default_rng(11)
    first = None
    for traced in range(0, documented + 2):
        n = k + traced
        info = check(gaussian(rng, n), n, ro.kept_patterns(n, k)['interleaved'], form=form, expect_form=STREAM if form == 'stream' else TILED)
        check(dyadic(rng, n), n, ro.kept_patterns(n, k)['low'], form=form, exact=True)
        if first is None and info[2] >= 2:
            first = traced
            assert info[2] == 2
        assert (info[2] == 1) == (first is None)
    assert first == documented


@pytest.mark.parametrize('form,k,pattern,per_workgroup', [('stream', 1, 'interleaved', 2), ('stream', 3, 'low', 1), ('stream', 0, 'low', 4),
                                                          ('tiled', 3, 'high', 8), ('tiled', 4, 'interleaved', 4), ('tiled', 8, 'low', 4),
                                                          ('tiled', 7, 'interleaved', 2)])
def test_several_tiles_or_blocks_per_workgroup(form, k, pattern, per_workgroup, psi20):
    """n = 20: a workgroup walks several STREAM tiles / TILED blocks, fetching the next while it works on the present one."""
    g, d = psi20
    kept = ro.kept_patterns(20, k)[pattern]
    info = check(g, 20, kept, form=form, expect_form=STREAM if form == 'stream' else TILED)
    units = (1 << (20 - k - min(8, 20 - k))) if form == 'stream' else (1 << (20 - k - 4))
    assert units // int(info[2]) == per_workgroup
    check(d, 20, kept, form=form, exact=True)


@pytest.fixture(scope='module')
def psi20():
    rng = np.random.default_rng(20)
    return gaussian(rng, 20), dyadic(rng, 20)


# ---- the tile edge -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', PATTERNS)
def test_tile_boundary(pattern):
    """k = t - 1 (a ragged tile), t (one tile), t + 1 (2 x 2 tiles, one pair off the diagonal) for the tile edge 2^t."""
    rng = np.random.default_rng(13)
    edge = int(check(gaussian(rng, 5), 5, [0, 1, 2, 3])[3])
    t = edge.bit_length() - 1
    assert edge == 1 << t
    for k, pairs in ((t - 1, 1), (t, 1), (t + 1, 3)):
        n = k + 5
        kept = ro.kept_patterns(n, k)[pattern]
        info = check(gaussian(rng, n), n, kept, expect_form=TILED)
        assert info[4] == pairs * info[2]
        check(dyadic(rng, n), n, kept, exact=True)


def test_single_kept_qubit_at_every_position_of_twelve():
    rng = np.random.default_rng(17)
    g, d = gaussian(rng, 12), dyadic(rng, 12)
    for q in range(12):
        check(g, 12, [q], expect_form=STREAM)
        check(d, 12, [q], exact=True)
        check(d, 12, [q], form='tiled', exact=True, expect_form=TILED)


@pytest.mark.parametrize('k', (10, 12))
def test_large_matrices_at_twelve_qubits(k):
    rng = np.random.default_rng(19)
    g, d = gaussian(rng, 12), dyadic(rng, 12)
    kept = ro.kept_patterns(12, k)['interleaved']
    info = check(g, 12, kept, expect_form=TILED)
    assert info[4] == (1 << (k - 6)) * ((1 << (k - 6)) + 1) // 2 * info[2] and info[5] == info[2] * 16 << (2 * k)
    if k == 12:
        with kernels.DeviceBuffer.upload(d) as buf:
            assert np.array_equal(kernels.rdm_dev(buf, 12, kept), np.outer(d, d.conj()))
    else:
        check(d, 12, kept, exact=True)


def test_thirteen_kept_qubits_are_refused():
    psi = np.ones(1 << 13, dtype=np.complex128)
    with pytest.raises(ValueError, match='12'):
        kernels.rdm_dev(psi, 13, range(13))
    kept = np.arange(13, dtype=np.int32)
    with kernels.DeviceBuffer.upload(psi) as buf, kernels.DeviceBuffer(1 << 20) as rho:
        assert _lib.lib().symgpu_rdm(buf.ptr, 13, kept.ctypes.data, 13, rho.ptr, None) == _lib.E_INVALID


# ---- refusals of the raw call ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_psi_and_rho_as_they_were():
    rng = np.random.default_rng(23)
    n = 5
    psi, sentinel = gaussian(rng, n), np.full(1 << (2 * n), -7.25 + 3.5j)
    lib = _lib.lib()
    arr = lambda *q: np.array(q, dtype=np.int32)
    with kernels.DeviceBuffer.upload(psi) as buf, kernels.DeviceBuffer.upload(sentinel) as rho:
        refused = [(buf.ptr, 0, arr(), 0, rho.ptr), (buf.ptr, 33, arr(0), 1, rho.ptr), (buf.ptr, -1, arr(0), 1, rho.ptr),
                   (buf.ptr, n, arr(0), -1, rho.ptr), (buf.ptr, n, arr(0, 1, 2, 3, 4, 5), 6, rho.ptr), (buf.ptr, 20, np.arange(13, dtype=np.int32), 13, rho.ptr),
                   (buf.ptr, n, arr(1, 1), 2, rho.ptr), (buf.ptr, n, arr(2, 1), 2, rho.ptr), (buf.ptr, n, arr(0, 5), 2, rho.ptr), (buf.ptr, n, arr(-1, 2), 2, rho.ptr),
                   (None, n, arr(0), 1, rho.ptr), (buf.ptr, n, arr(0), 1, None), (buf.ptr, n, None, 1, rho.ptr),
                   (buf.ptr, n, arr(0), 1, buf.ptr), (buf.ptr, n, arr(0), 1, ctypes.c_void_p(buf.ptr.value + 16 * 31)),
                   (ctypes.c_void_p(rho.ptr.value + 64), 3, arr(0, 1), 2, rho.ptr)]
        info = np.full(6, -1, dtype=np.int64)
        for psi_ptr, nq, kept, k, rho_ptr in refused:
            rc = lib.symgpu_rdm(psi_ptr, nq, None if kept is None else kept.ctypes.data, k, rho_ptr, info.ctypes.data)
            assert rc == _lib.E_INVALID, (nq, kept, k)
            assert 'invalid argument' in _lib.last_error()
        assert np.all(info == -1)
        assert buf.download(np.complex128, 1 << n).tobytes() == psi.tobytes() and rho.download(np.complex128, 1 << (2 * n)).tobytes() == sentinel.tobytes()
        # a null kept list is allowed for k = 0, and info may be NULL
        assert lib.symgpu_rdm(buf.ptr, n, None, 0, rho.ptr, None) == _lib.OK
        got = rho.download(np.complex128, 1 << (2 * n))
        assert abs(got[0] - np.sum(psi.real ** 2 + psi.imag ** 2)) <= ro.entry_tolerance(psi, n, [])[0, 0] and got[0].imag == 0.0
        assert got[1:].tobytes() == sentinel[1:].tobytes()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------------
GOLDEN_CASES = ro.golden_cases()


@pytest.mark.parametrize('tag,case', GOLDEN_CASES, ids=[tag for tag, _ in GOLDEN_CASES])
def test_quantum_state_methods_against_the_reference(tag, case):
    n = case['n']
    state = QuantumState(case['bits'].astype(int), case['amp'], vec_type=case['vec_type'])
    psi = ro.dense_amplitudes(n, case['bits'], case['amp'])
    for entry in case['lists']:
        tol = ro.entry_tolerance(psi, n, entry['qubits'])
        rdm, ptrace = state.get_rdm(entry['qubits']), state.partial_trace_over_qubits(entry['traced'])
        # tol carries a factor 2 over the textbook bound: the reference's sum and the device's each lie within half of it of the exact value
        assert np.all(np.abs(rdm - entry['rdm']) <= tol) and np.all(np.abs(ptrace - entry['ptrace']) <= tol), entry['qubits']
        assert rdm.tobytes() == ptrace.tobytes()
        assert_hermitian_to_the_byte(rdm)
        if case['kind'] == 'dyadic':
            assert np.array_equal(rdm, entry['rdm'])
        e_tol = ro.entropy_tolerance(tol)
        for given in (state, psi, psi.reshape(-1, 1)):
            got = get_entanglement_entropy(given, entry['qubits'])
            assert isinstance(got, float) and abs(got - entry['entropy']) <= e_tol, (entry['qubits'], got, entry['entropy'], e_tol)


def test_entropy_known_answers_and_refusals():
    n = 9
    ghz = QuantumState([[0] * n, [1] * n], np.array([1, 1]) / np.sqrt(2))
    psi = ghz.to_dense_matrix.reshape(-1)
    for qubits in ([0], [8], [1, 4, 7], list(range(5)), list(range(8))):
        tol = ro.entropy_tolerance(ro.entry_tolerance(psi, n, qubits if len(qubits) <= 4 else sorted(set(range(n)) - set(qubits))))
        assert abs(get_entanglement_entropy(ghz, qubits) - np.log(2)) <= tol
    assert np.array_equal(ghz.get_rdm([4]).real, np.eye(2) * ghz.get_rdm([4])[0, 0].real) and abs(ghz.get_rdm([4])[0, 0] - 0.5) <= 1e-15
    rng = np.random.default_rng(29)
    product = np.ones(1, dtype=complex)
    for _ in range(n):
        one = rng.standard_normal(2) + 1j * rng.standard_normal(2)
        product = np.kron(product, one / np.linalg.norm(one))
    for qubits in ([3], [0, 8], [1, 2, 3, 4], list(range(1, 9))):
        small = qubits if len(qubits) <= 4 else sorted(set(range(n)) - set(qubits))
        assert abs(get_entanglement_entropy(product, qubits)) <= ro.entropy_tolerance(ro.entry_tolerance(product, n, small))
    with pytest.raises(ValueError, match='repeated'):
        ghz.partial_trace_over_qubits([1, 1])
    with pytest.raises(ValueError, match='outside'):
        ghz.get_rdm([9])
    with pytest.raises(ValueError, match='outside'):
        get_entanglement_entropy(ghz, [9])
    with pytest.raises(ValueError, match='elements'):
        kernels.rdm_dev(np.ones(100, dtype=complex), 7, [0])
    s14 = QuantumState([[0] * 14, [1] * 14], [0.6, 0.8])
    with pytest.raises(ValueError, match='12'):
        s14.get_rdm(range(13))
    with pytest.raises(ValueError, match='12'):
        s14.partial_trace_over_qubits([])
    assert abs(get_entanglement_entropy(s14, range(13)) - (-0.36 * np.log(0.36) - 0.64 * np.log(0.64))) <= 1e-12      # the complement has one qubit
    assert s14.get_rdm(range(12)).shape == (4096, 4096)


def test_bh_ground_state_from_the_device_has_one_entropy_from_either_side():
    """12 qubits: rho over qubits 0 .. 4 (k = 5) and over 5 .. 11 (k = 7) of the state exact_gs_energy returns share their non-zero
    spectrum, so the two entropies agree within the sum of their tolerances."""
    with open(os.path.join(GOLDEN, 'BH_STO-3G_SINGLET_JW.json')) as f:
        H = PauliwordOp.from_dictionary({k: complex(*v) for k, v in json.load(f)['hamiltonian'].items()})
    assert H.n_qubits == 12
    _, psi = exact_gs_energy(H, return_array=True)
    left, right = list(range(5)), list(range(5, 12))
    with kernels.DeviceBuffer.upload(psi) as buf:
        rho_l, info_l = kernels.rdm_dev(buf, 12, left, want_info=True)
        rho_r, info_r = kernels.rdm_dev(buf, 12, right, want_info=True)
    assert info_l[0] == TILED and info_r[0] == TILED and rho_l.shape == (32, 32) and rho_r.shape == (128, 128)
    tol_l, tol_r = ro.entry_tolerance(psi, 12, left), ro.entry_tolerance(psi, 12, right)
    assert np.all(np.abs(rho_l - ro.rdm_deposit(psi, 12, left)) <= tol_l) and np.all(np.abs(rho_r - ro.rdm_deposit(psi, 12, right)) <= tol_r)
    s_l, s_r = ro.entropy(rho_l), ro.entropy(rho_r)
    bound = ro.entropy_tolerance(tol_l) + ro.entropy_tolerance(tol_r)
    print(f'S(0..4) = {s_l!r}, S(5..11) = {s_r!r}, bound {bound:.3g}')
    assert abs(s_l - s_r) <= bound and s_l > 1e-3
    assert get_entanglement_entropy(psi, left) == s_l == get_entanglement_entropy(psi, right)
