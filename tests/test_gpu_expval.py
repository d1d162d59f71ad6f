"""GPU: symgpu_expval_terms_dev (csrc/expval.hip) and what sits on it — kernels.expval_terms_dev, term_expvals, PauliwordOp.expval —
against tests/_expval_oracle.py (proved against the reference and a dense evaluator in tests/test_expval_oracle.py) and against the
reference's own answers (tests/golden/expval.npz).

Bars.  Goldens: 1e-12, the scope contract's tolerance (a sum of S <= 4096 products with sum |conj(psi[b ^ x]) psi[b]| <= 1 rounds below
4096 * 2^-53 = 4.5e-13).  Dyadic inputs (multiples of 1/8 in [-1, 1]): every product and sum is exact in any order, so terms and total
equal the oracle with ``==`` (the sign of a zero is not compared).  Gaussian inputs: the header pins the order of every addition, so
the two forms and two consecutive calls agree bit for bit, and so does the oracle run on the cleaned state in the device's row order.
Every case runs in the form the library picks and with SYMGPU_EXPVAL_FORM=global.  No bound here comes from the code under test."""
import os

import numpy as np
import pytest

from symmer_amd import PauliwordOp, QuantumState, kernels, packing, _lib
from symmer_amd._lib import SymgpuError
from symmer_amd.kernels import DeviceOp
from symmer_amd.operators import term_expvals, single_term_expval
import _expval_oracle as ora

pytestmark = pytest.mark.gpu
TOL = 1e-12
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expval.npz'))
N_CASES = int(GOLD['n_cases'])


@pytest.fixture(params=['auto', 'global'])
def form_env(request, monkeypatch):
    """The form the library picks by its rule, then the global form forced on the same input."""
    if request.param == 'global':
        monkeypatch.setenv('SYMGPU_EXPVAL_FORM', 'global')
    else:
        monkeypatch.delenv('SYMGPU_EXPVAL_FORM', raising=False)
    return request.param


def device_state(bits, amp):
    """A cleaned device state, as term_expvals makes it."""
    raw = DeviceOp.upload(packing.pack_rows(ora.state_symp(bits)), amp)
    try:
        return kernels.cleanup_dev(raw)
    finally:
        raw.free()


def run(symp, coeff, phi, psi=None):
    """(terms, total, form, S_phi after the cleanup) of one call; psi None: the expectation value, one handle for both sides."""
    op = DeviceOp.upload(packing.pack_rows(np.asarray(symp, dtype=bool)), coeff)
    hphi = device_state(*phi)
    hpsi = hphi if psi is None else device_state(*psi)
    try:
        terms, total, form = kernels.expval_terms_dev(op, hphi, hpsi)
        only_total = kernels.expval_terms_dev(op, hphi, hpsi, want_terms=False)
        assert only_total[0] is None and only_total[1:] == (total, form), 'the call without out_terms gives another total'
        return terms, total, form, hphi.n_terms
    finally:
        for h in {id(h): h for h in (op, hphi, hpsi)}.values():
            h.free()


def check_exact(symp, coeff, phi, psi, form_env, tag=''):
    """Dyadic inputs: terms and total equal the oracle with ==; the form is the one the header's rule gives."""
    n = np.asarray(symp).shape[1] // 2
    terms, total, form, S_phi = run(symp, coeff, phi, psi)
    a, b = ora.clean_state(*phi), ora.clean_state(*(phi if psi is None else psi))
    want = ora.term_elements(symp, a[0], a[1], b[0], b[1])
    assert S_phi == a[0].shape[0]
    assert form == (ora.GLOBAL if form_env == 'global' else ora.expected_form(S_phi, n)), f'{tag}: form {form} at S = {S_phi}, n = {n}'
    assert np.all(terms == want), f'{tag}: terms differ at {np.flatnonzero(terms != want)[:8]}'
    assert total == ora.total(coeff, want), f'{tag}: total {total} != {ora.total(coeff, want)}'
    return want, form


# ------------------------------------------------------------------------------------------------------------------------ goldens ----
@pytest.mark.parametrize('k', range(N_CASES))
def test_expval_and_term_expvals_match_the_reference(k, form_env):
    g = {name: GOLD[f'{k:02d}/{name}'] for name in ('n', 'symp', 'coeff', 'psi_bits', 'psi_coeff', 'expval', 'term_expvals')}
    H, psi = PauliwordOp(g['symp'], g['coeff']), QuantumState(g['psi_bits'].astype(int), g['psi_coeff'])
    per_term = term_expvals(H, psi)
    value = H.expval(psi)
    print(f'case {k}: largest per-term gap {np.max(np.abs(per_term - g["term_expvals"])):.3e}, expval gap {abs(value - float(g["expval"])):.3e}')
    assert per_term.dtype == np.float64 and per_term.shape == (H.n_terms,)
    assert np.max(np.abs(per_term - g['term_expvals'])) <= TOL
    assert np.ndim(value) == 0 and abs(value - float(g['expval'])) <= TOL
    # the kernel's own total also on the cases whose expval takes the bra x op x ket branch
    _, total, _, _ = run(g['symp'], g['coeff'], (g['psi_bits'], g['psi_coeff']))
    assert abs(total.real - float(g['expval'])) <= TOL


def test_single_term_operator_returns_a_scalar_and_agrees_with_the_per_term_loop(form_env):
    rng = np.random.default_rng(5)
    symp, coeff, bits, amp = ora.random_case(rng, 6, 12, 9, 'gaussian')
    H, psi = PauliwordOp(symp, coeff), QuantumState(bits.astype(int), amp)
    loop = np.array([single_term_expval(P, psi) for P in H])
    assert np.max(np.abs(term_expvals(H, psi) - loop)) <= TOL
    assert abs(H.expval(psi) - np.sum(loop * coeff).real) <= TOL
    one = H[3]
    value = one.expval(psi)
    assert np.ndim(value) == 0 and abs(value - (loop[3] * coeff[3]).real) <= TOL


# ------------------------------------------------------------------------------------------------------- exactness on dyadic inputs ----
@pytest.mark.parametrize('T', [1, 63, 64, 65, 257])
def test_term_tails(T, form_env):
    symp, coeff, bits, amp = ora.random_case(np.random.default_rng(T), 10, T, 70, 'dyadic')
    want, _ = check_exact(symp, coeff, (bits, amp), None, form_env, f'T={T}')
    assert T == 1 or np.count_nonzero(want) * 3 >= T


@pytest.mark.parametrize('S', [1, 2, 511, 512, 513, 1024, 1025])
def test_table_capacities(S, form_env):
    symp, coeff, bits, amp = ora.random_case(np.random.default_rng(S), 12, 65, S, 'dyadic')
    check_exact(symp, coeff, (bits, amp), None, form_env, f'S={S}')


@pytest.mark.parametrize('n,S,lds', [(13, 2047, True), (13, 2048, True), (13, 2049, False), (70, 1535, True), (70, 1536, True), (70, 1537, False),
                                     (130, 1228, True), (130, 1229, False)])
def test_form_flips_where_the_header_says(n, S, lds, form_env):
    """S_phi (16 + 8 Wq) + 4 cap <= 65536: the last S of the staged form and the first of the global one, Wq = 1, 2, 3."""
    symp, coeff, bits, amp = ora.random_case(np.random.default_rng(n + S), n, 33, S, 'dyadic')
    assert ora.expected_form(S, n) == (ora.LDS if lds else ora.GLOBAL)
    _, form = check_exact(symp, coeff, (bits, amp), None, form_env, f'n={n} S={S}')
    assert form == (ora.LDS if lds and form_env == 'auto' else ora.GLOBAL)


@pytest.mark.parametrize('S', [63, 64, 65, 4096, 4097])
def test_state_chunk_boundaries(S, form_env):
    """Chunks of 64 states up to S = 4096 (less than one chunk, exactly one, one state into the second; 64 full chunks), chunks of 128
    above (33 of them, the last with one state)."""
    symp, coeff, bits, amp = ora.random_case(np.random.default_rng(S), 14, 9 if S > 1000 else 65, S, 'dyadic')
    check_exact(symp, coeff, (bits, amp), None, form_env, f'S={S}')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 128, 130])
def test_word_boundaries(n, form_env):
    symp, coeff, bits, amp = ora.random_case(np.random.default_rng(n), n, 20, min(1 << n, 24), 'dyadic')
    want, _ = check_exact(symp, coeff, (bits, amp), None, form_env, f'n={n}')
    assert np.count_nonzero(want) * 3 >= 20


@pytest.mark.parametrize('n', [9, 70])
def test_phi_differs_from_psi_with_partial_overlap(n, form_env):
    rng = np.random.default_rng(n)
    symp, coeff, bits, amp = ora.random_case(rng, n, 65, 90, 'dyadic')
    phi = (bits[:60], ora.amplitudes(rng, 60, 'dyadic') + 0.125)
    psi = (bits[30:], amp[30:])
    want, _ = check_exact(symp, coeff, phi, psi, form_env, f'n={n}')
    assert np.count_nonzero(want.imag) > 0 and np.count_nonzero(want) * 3 >= 65
    back = ora.term_elements(symp, *ora.clean_state(*psi), *ora.clean_state(*phi))
    assert np.all(back == want.conj()), '<psi|P|phi> is the conjugate of <phi|P|psi>'


# ------------------------------------------------------------------------------------------------------------------ planted answers ----
def test_planted_answers(form_env):
    n = 5
    bits = np.array([[0, 0, 0, 0, 0], [1, 0, 1, 0, 0], [0, 1, 1, 0, 1], [1, 1, 1, 1, 1]])
    amp = np.array([0.5, -0.25 + 0.5j, 0.75j, 0.125 - 0.125j])
    psi = QuantumState(bits, amp)
    norm2 = float(np.sum(np.abs(amp) ** 2))
    paulis = ['IIIII',            # identity: sum |psi|^2
              'ZIZIZ',            # Z only: the signed sum
              'IIIXI',            # moves every state out of the support
              'XIXII',            # |00000> <-> |10100>, the others leave the support
              'YIXII', 'YIYII', 'YIYZY', 'YYYYY']
    H = PauliwordOp.from_list(paulis, [1, 2, 3, 0.5, 0.25, -1, 1j, 2])
    got = term_expvals(H, psi)
    signs = np.array([(-1) ** int(b[0] + b[2] + b[4]) for b in bits])
    assert got[0] == norm2 and got[1] == float(np.sum(signs * np.abs(amp) ** 2)) and got[2] == 0
    want = ora.expval(H.symp_matrix, H.coeff_vec, bits, amp)
    assert np.all(got == want[0]) and H.expval(psi) == want[1]
    # Y counts 0, 1, 2, 3 on a state that each of these terms maps onto itself: all 2^3 strings on qubits 0, 2, 4
    grid = np.array([[a, 0, b, 0, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    g_amp = np.array([0.5, 0.25 + 0.5j, -0.25, 0.125 + 0.25j, 1 - 0.5j, 0.75, 0.375j, -0.5 + 0.5j])
    terms = ['XIXIX', 'YIXIX', 'YZYIX', 'YIYZY', 'YYYIY']
    Hy = PauliwordOp.from_list(terms, np.ones(len(terms)))
    el, _, _, _ = run(Hy.symp_matrix, Hy.coeff_vec, (grid, g_amp))
    assert [int((Hy.symp_matrix[k, :n] & Hy.symp_matrix[k, n:]).sum()) for k in range(len(terms))] == [0, 1, 2, 3, 4]
    assert np.all(el == ora.term_elements(Hy.symp_matrix, grid, g_amp, grid, g_amp))
    assert np.all(el[:4] != 0) and el[4] == 0                          # YYYIY flips qubit 1: out of the support


def test_repeated_terms_and_complex_coefficients(form_env):
    bits = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 0]])
    amp = np.array([0.5, 0.5, -0.25])
    psi = QuantumState(bits, amp)
    H = PauliwordOp.from_list(['XII', 'ZZI', 'XII', 'YII', 'XII'], [0.5 + 1j, 0.25j, -2, 1 - 0.5j, 0.125])
    per_term = term_expvals(H, psi)
    assert per_term.shape == (5,) and per_term[0] == per_term[2] == per_term[4] != 0, 'a repeated term has its own entry'
    want_terms, want = ora.expval(H.symp_matrix, H.coeff_vec, bits, amp)
    assert np.all(per_term == want_terms)
    assert H.expval(psi) == want == np.sum(per_term * H.coeff_vec).real, 'expval is the real part of the total'
    assert np.sum(per_term * H.coeff_vec).imag != 0


def test_duplicate_and_cancelling_basis_strings(form_env):
    # |011> twice (merged: 0.5 + 0.25j), |110> twice with opposite amplitudes: it vanishes in the cleanup and must not be matched
    bits = np.array([[0, 1, 1], [1, 1, 0], [0, 0, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]])
    amp = np.array([0.5, 0.75, -0.5j, 0.25j, -0.75, 0.25])
    psi = QuantumState(bits, amp)
    # XIX and YIY map |011> to |110>, XXI maps |000> to |110>, and nothing else of theirs stays in the support
    H = PauliwordOp.from_list(['XIX', 'IIZ', 'XXI', 'YIY', 'IXX', 'III', 'XII'], [1, 0.5, 2, -1, 0.25j, 1, 0.125])
    clean_bits, clean_amp = ora.clean_state(bits, amp)
    assert clean_bits.tolist() == [[0, 1, 1], [0, 0, 0], [1, 1, 1]]
    want_terms, want = ora.expval(H.symp_matrix, H.coeff_vec, bits, amp)
    got = term_expvals(H, psi)
    assert np.all(got == want_terms) and H.expval(psi) == want
    assert got[0] == got[2] == got[3] == 0 and got[4] != 0 and got[6] != 0 and got[5] == float(np.sum(np.abs(clean_amp) ** 2))
    assert np.all(got == ora.dense_term_elements(H.symp_matrix, bits, amp, bits, amp).real)


def test_empty_operator_and_empty_state(form_env):
    rng = np.random.default_rng(3)
    symp, coeff, bits, amp = ora.random_case(rng, 7, 9, 12, 'dyadic')
    op, empty_op = DeviceOp.upload(packing.pack_rows(symp), coeff), DeviceOp.alloc(1, 1, True)
    state = device_state(bits, amp)
    nothing = device_state(bits[:2], np.zeros(2))                    # every amplitude below the threshold: a cleaned state without terms
    try:
        empty_op.set_rows(0)
        assert nothing.n_terms == 0
        terms, total, form = kernels.expval_terms_dev(empty_op, state, state)
        assert terms.shape == (0,) and total == 0 and form == 0
        for phi, psi in ((nothing, nothing), (nothing, state), (state, nothing)):
            terms, total, form = kernels.expval_terms_dev(op, phi, psi)
            assert np.all(terms == 0) and terms.shape == (9,) and total == 0 and form == 0
    finally:
        for h in (op, empty_op, state, nothing):
            h.free()


# ------------------------------------------------------------------------------------------------------------------------- forms ----
@pytest.mark.parametrize('n,T,S', [(12, 300, 700), (70, 130, 700), (14, 65, 3000)])
def test_gaussian_inputs_bit_for_bit(n, T, S, monkeypatch):
    """Two consecutive calls, the two forms, and the oracle on the cleaned state in the device's row order: the same bits."""
    rng = np.random.default_rng(n + T)
    symp, coeff, bits, amp = ora.random_case(rng, n, T, S, 'gaussian')
    op = DeviceOp.upload(packing.pack_rows(symp), coeff)
    state = device_state(bits, amp)
    try:
        monkeypatch.delenv('SYMGPU_EXPVAL_FORM', raising=False)
        first = kernels.expval_terms_dev(op, state, state)
        second = kernels.expval_terms_dev(op, state, state)
        monkeypatch.setenv('SYMGPU_EXPVAL_FORM', 'global')
        forced = kernels.expval_terms_dev(op, state, state)
        rows, c = state.download()
    finally:
        op.free(); state.free()
    assert first[2] == ora.expected_form(S, n) and second[2] == first[2] and forced[2] == ora.GLOBAL
    for other in (second, forced):
        assert first[0].tobytes() == other[0].tobytes() and first[1] == other[1]
    dev_bits = packing.unpack_rows(rows, n)[:, :n].astype(np.uint8)
    want = ora.term_elements(symp, dev_bits, c, dev_bits, c)
    assert np.all(first[0] == want), f'largest gap to the oracle in the same order: {np.max(np.abs(first[0] - want)):.3e}'
    assert first[1] == ora.total(coeff, want)
    loose = ora.expval(symp, coeff, bits, amp)
    assert np.max(np.abs(first[0].real - loose[0])) <= TOL and abs(first[1].real - loose[1]) <= TOL and np.max(np.abs(first[0].imag)) <= TOL


# --------------------------------------------------------------------------------------------------------------------- refusals ----
def test_refusals():
    rng = np.random.default_rng(9)
    symp, coeff, bits, amp = ora.random_case(rng, 7, 9, 12, 'dyadic')
    symp2, coeff2, bits2, amp2 = ora.random_case(rng, 70, 9, 12, 'dyadic')
    op, op2 = DeviceOp.upload(packing.pack_rows(symp), coeff), DeviceOp.upload(packing.pack_rows(symp2), coeff2)
    bare_op = DeviceOp.upload(packing.pack_rows(symp))
    state, state2 = device_state(bits, amp), device_state(bits2, amp2)
    raw = DeviceOp.upload(packing.pack_rows(ora.state_symp(bits)), amp)           # no cleanup has seen it
    bare = DeviceOp.upload(packing.pack_rows(ora.state_symp(bits)))              # no coefficients
    out, total = np.zeros(9, dtype=np.complex128), np.zeros(2)
    call = _lib.lib().symgpu_expval_terms_dev
    try:
        for args, what in (((op, raw, state), 'must come from a cleanup'), ((op, state, raw), 'must come from a cleanup'),
                           ((op, state2, state), 'Wq'), ((op2, state, state), 'Wq'), ((op, state, state2), 'Wq'),
                           ((op, bare, state), 'no coefficients'), ((op, state, bare), 'no coefficients'), ((bare_op, state, state), 'no coefficients')):
            with pytest.raises(SymgpuError) as err:
                kernels.expval_terms_dev(*args)
            assert err.value.code == _lib.E_INVALID and what in str(err.value), str(err.value)
        for a, b, c, t in ((None, state.handle, state.handle, total), (op.handle, None, state.handle, total), (op.handle, state.handle, None, total),
                           (op.handle, state.handle, state.handle, None)):
            assert call(a, b, c, _lib.addr(out), _lib.addr(t), None) == _lib.E_INVALID
        # out_terms and form may be null
        assert call(op.handle, state.handle, state.handle, None, _lib.addr(total), None) == _lib.OK
        assert complex(total[0], total[1]) == ora.total(coeff, ora.term_elements(symp, bits, amp, bits, amp))
    finally:
        for h in (op, op2, bare_op, state, state2, raw, bare):
            h.free()


# --------------------------------------------------------------------------------------------------------------------- weak hash ----
@pytest.mark.timeout(300)
def test_expval_on_a_weak_row_hash():
    """SYMGPU_HASH_WEAK_ODD=1 in a fresh process leaves the first seed's row hash four bits: every probe of the table walks DIFFERENT rows
    with EQUAL hashes, and the word-by-word comparison is all that keeps them apart (tests/_weak_hash_worker4.py)."""
    from test_gpu_multirank import _launch
    rc, o, e = _launch(['tests/_weak_hash_worker4.py'], 1, {'SYMGPU_HASH_WEAK_ODD': '1'}, timeout=240)[0]
    assert rc == 0 and 'WEAK_HASH4_OK' in o, f'rc={rc}\n{o}\n{e[-3000:]}'
