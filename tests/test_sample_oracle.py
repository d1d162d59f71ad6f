"""CPU: tests/_sample_oracle.py — the restatement of section f10 of include/symgpu.h that the GPU tests hold csrc/sample.hip and
csrc/basis.hip against — is held against things that do not share its text: NumPy's own Philox bit for bit, the exact inverse CDF over
rational prefixes, the Kronecker product of H, H S^+ and I, brute-force signed sums, and the reference's recorded answers
(tests/golden/measure_basis.json, tools/gen_golden_measure_basis.py).  Also: the header states what fixes bits, the entry points, their
bindings and the methods are in place, and the fixed seed of the finite-shot check passes on the restatement alone."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import _clique_oracle as co
import _sample_oracle as so
from _integration_doc import header_prototypes, header_text

SEEDS = (0, 1, (1 << 63) + 5)
OFFSETS = (0, 3, (1 << 40) + 1)
TREE_SIZES = (1, 15, 16, 17, 257, 4097)
GOLDEN = so.golden_cases()


# ---- uniforms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('first_draw', OFFSETS)
def test_philox_restatement_is_numpys_stream_bit_for_bit(seed, first_draw):
    got, want = so.philox_uniforms(seed, first_draw, 4099), so.numpy_uniforms(seed, first_draw, 4099)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if first_draw == 0:                                             # the plain generator, nothing set but the key
        plain = np.random.Generator(np.random.Philox(key=seed, counter=0)).random(4099)
        assert np.array_equal(got.view(np.uint64), plain.view(np.uint64))
    # the scalar block function against NumPy's raw words
    raw = np.random.Philox(key=seed, counter=first_draw // 4).random_raw(8)
    assert [int(w) for w in raw] == so.philox_block(seed, first_draw // 4 + 1) + so.philox_block(seed, first_draw // 4 + 2)


def test_numpy_advance_reaches_the_same_offset():
    """Philox.advance counts blocks of four draws: advancing by s div 4 and dropping s mod 4 numbers is draw s."""
    s = (1 << 40) + 1
    bit_gen = np.random.Philox(key=7, counter=0)
    bit_gen.advance(s // 4)
    want = np.random.Generator(bit_gen).random(64 + s % 4)[s % 4:]
    assert np.array_equal(so.philox_uniforms(7, s, 64).view(np.uint64), want.view(np.uint64))


# ---- the tree walk against the exact inverse CDF ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', TREE_SIZES)
def test_tree_walk_on_dyadic_weights_is_the_exact_inverse_cdf(m):
    rng = np.random.default_rng(1000 + m)
    amp = so.dyadic_amplitudes(rng, m)
    w = so.weights(amp)
    levels = so.tree_build(w)
    total = levels[-1][0]
    assert Fraction(total) == sum(Fraction(float(v)) for v in w), 'a dyadic sum must be exact'
    u = so.philox_uniforms(m, 0, 4099)
    _, prefix = so.exact_inverse_cdf(w, [])
    if m >= 3:
        assert total == 2.0 ** round(np.log2(total)), 'the total is a power of two, so that prefix / total is exact'
        # u exactly on boundaries (they belong to the upper interval), on 0 and just below 1
        on = np.array([float(p / Fraction(total)) for p in prefix[:-1]][:2000] + [0.0, 1.0 - 2.0 ** -53])
        assert all(Fraction(float(x)) * Fraction(total) in (set(prefix) | {0}) for x in on[:-1])
        u = np.concatenate([u, on])
    want, _ = so.exact_inverse_cdf(w, [Fraction(float(x)) * Fraction(total) for x in u])
    got = so.tree_walk(levels, u)
    assert np.array_equal(got, want)
    assert np.all(w[got] > 0)


@pytest.mark.parametrize('m', TREE_SIZES)
def test_tree_walk_on_gaussian_weights_differs_only_at_boundaries(m):
    rng = np.random.default_rng(2000 + m)
    amp = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    w = so.weights(amp)
    levels = so.tree_build(w)
    total = levels[-1][0]
    u = so.philox_uniforms(2000 + m, 0, 4099)
    r_exact = [Fraction(float(x)) * Fraction(total) for x in u]
    want, prefix = so.exact_inverse_cdf(w, r_exact)
    got = so.tree_walk(levels, u)
    # a draw may be left out only where u total lies within 2^-40 total of a boundary
    edges = np.array([float(p) for p in prefix])
    near = np.array([np.min(np.abs(edges - float(r))) <= 2.0 ** -40 * total for r in r_exact])
    print(f'm = {m}: {np.count_nonzero(got != want)} draws differ, {np.count_nonzero(near)} of {u.shape[0]} lie at a boundary')
    assert np.count_nonzero(near) <= u.shape[0] / 1000
    assert np.array_equal(got[~near], want[~near])
    assert np.all(w[got] > 0)
    assert abs(total - float(prefix[-1])) <= 2.0 ** -48 * total


def test_walk_never_returns_a_zero_weight_and_takes_the_edges():
    amp = np.zeros(300, dtype=np.complex128)
    amp[[17, 18, 255, 256]] = [0.5, 0.5j, 0.5, -0.5]
    u = np.array([0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -53, 0.2499999, 0.999])
    assert np.array_equal(so.draw(amp, u), [17, 18, 255, 256, 256, 17, 256])
    one_hot = np.zeros(4097, dtype=np.complex128)
    for at in (0, 4096):
        one_hot[:] = 0
        one_hot[at] = 1j
        assert np.all(so.draw(one_hot, np.array([0.0, 0.5, 1.0 - 2.0 ** -53])) == at)
    levels = so.tree_build(so.weights(np.ones(1)))
    assert len(levels) == 2 and levels[1][0] == 1.0, 'm = 1: one level above the weight'
    assert [lev.shape[0] for lev in so.tree_build(np.ones(4097))] == [4097, 257, 17, 2, 1]


# ---- the layer against the Kronecker product ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 2, 3, 5, 8))
def test_basis_change_restatement_is_the_kronecker_product(n):
    rng = np.random.default_rng(3000 + n)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    qubits = list(range(n))
    masks = [([], []), (qubits, []), ([], qubits), (qubits[::2], qubits[1::2]), (qubits[-1:], []), ([], qubits[:1])]
    for xs, ys in masks:
        h = len(xs) + len(ys)
        # the product is formed in extended precision, so that the bound is spent on the restatement alone
        got, want = so.basis_change(psi, n, xs, ys), so.layer_matrix(n, xs, ys, np.clongdouble) @ psi.astype(np.clongdouble)
        bound = 4 * h * 2.0 ** -53 * np.linalg.norm(psi)
        assert float(np.max(np.abs(got - want), initial=0.0)) <= bound, (xs, ys, float(np.max(np.abs(got - want))), bound)
        if h == 0:
            assert np.array_equal(got, psi)
    # the order is part of the contract: ascending index bit; and S^+ on a Y-qubit is exact
    v = so.basis_change(np.array([0, 1j], dtype=np.complex128), 1, [], [0])
    assert np.array_equal(v, [so.R_SQRT_HALF, -so.R_SQRT_HALF])
    assert so.R_SQRT_HALF.hex() == '0x1.6a09e667f3bcdp-1' and np.float64(so.R_SQRT_HALF).view(np.uint64) == 0x3FE6A09E667F3BCD


# ---- the reference's recorded answers ---------------------------------------------------------------------------------------------------------
def _as_dict(symp, coeff):
    return {tuple(int(v) for v in row): complex(c) for row, c in zip(symp, coeff)}


def test_golden_file_covers_what_it_should():
    assert {case['n'] for case in GOLDEN} == {3, 4, 5} and {case['kind'] for case in GOLDEN} == {'dense', 'dyadic', 'sparse'}
    assert any(np.any(case['Z_new_symp'][:, :case['n']]) for case in GOLDEN), 'no case whose Z_new keeps an X-part'
    assert any(len(case['U_coeff']) == 1 for case in GOLDEN), 'no case without a measured qubit'


@pytest.mark.parametrize('k', range(len(GOLDEN)))
def test_restatement_and_change_of_basis_reproduce_the_reference(k):
    from symmer_amd.operators import PauliwordOp, change_of_basis_XY_to_Z
    case = GOLDEN[k]
    n = case['n']
    psi = so.dense_amplitudes(n, case['bits'], case['amp'])
    x0, z0 = case['P_symp'][0, :n].astype(bool), case['P_symp'][0, n:].astype(bool)
    xs, ys = np.flatnonzero(x0 & ~z0), np.flatnonzero(x0 & z0)
    got = so.basis_change(psi, n, xs, ys)
    want = so.dense_amplitudes(n, case['psi_new_bits'], case['psi_new_amp'])
    assert np.max(np.abs(got - want)) <= 1e-14
    # change_of_basis_XY_to_Z, term by term
    U = change_of_basis_XY_to_Z(PauliwordOp(case['P_symp'].astype(bool), case['P_coeff']))
    mine, ref = _as_dict(U.symp_matrix, U.coeff_vec), _as_dict(case['U_symp'], case['U_coeff'])
    assert set(mine) == set(ref) and len(mine) == U.n_terms
    assert all(abs(mine[key] - ref[key]) <= 1e-14 for key in ref)
    # <psi|P|psi> = <psi'|Z_new|psi'>
    dense = lambda symp, coeff: sum(c * so.pauli_matrix(r[:n], r[n:]) for r, c in zip(symp, coeff))
    lhs = psi.conj() @ dense(case['P_symp'], case['P_coeff']) @ psi
    rhs = got.conj() @ dense(case['Z_new_symp'], case['Z_new_coeff']) @ got
    assert abs(lhs - rhs) <= 1e-13
    assert np.allclose(dense(case['U_symp'], case['U_coeff']), so.layer_matrix(n, xs, ys), rtol=0, atol=1e-14)


def test_change_of_basis_refuses_more_than_16_measured_qubits():
    from symmer_amd.operators import PauliwordOp, change_of_basis_XY_to_Z
    with pytest.raises(ValueError, match='16'):
        change_of_basis_XY_to_Z(PauliwordOp.from_list(['X' * 17 + 'Z']))
    assert change_of_basis_XY_to_Z(PauliwordOp.from_list(['XYZI'])).n_terms == 8


# ---- signed sums, header, bindings ------------------------------------------------------------------------------------------------------------
def test_signed_sums_restatement_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    for n in (1, 3, 7):
        z_rows = rng.random((9, n)) < 0.5
        idx = rng.choice(1 << n, size=min(1 << n, 20), replace=False)
        count = rng.integers(1, 1 << 40, idx.shape[0])
        want = []
        for z in z_rows:
            total = 0
            for b, c in zip(idx, count):
                bits = [(int(b) >> (n - 1 - q)) & 1 for q in range(n)]                  # qubit q is bit n-1-q of the index
                total += int(c) * (-1) ** sum(bits[q] for q in range(n) if z[q])
            want.append(total)
        assert np.array_equal(so.signed_sums(z_rows, n, idx, count), np.array(want, dtype=np.int64))


def test_header_states_what_fixes_bits():
    text = ' '.join(header_text().replace('\n *', ' ').split())          # a comment's line breaks and their stars do not count
    for needle in ('0xD2E7470EE14C6C93', '0xCA5A826395121157', '0x9E3779B97F4A7C15', '0xBB67AE8584CAA73B', 'Philox4x64-10',
                   'counter (s div 4 + 1, 0, 0, 0)', 'key (seed, 0)', '(word >> 11) * 2^-53', 'radix-16',
                   'added to 0 in ascending order', 'the first k with r < acc_k', 'FALLBACK', 'the last child with c_k > 0',
                   'r <- r - acc_{k-1}', '2^-53 relative per boundary', '0x3FE6A09E667F3BCD', 'descending qubit number',
                   'ascending index bit', 'a1 <- (a1.im, -a1.re)', 'SYMGPU_SAMPLE_COUNT=hist|sort', 'SYMGPU_BASIS_FORM=direct',
                   'first_draw + count >= 2^63', '#define SYMGPU_SAMPLE_HIST 1', '#define SYMGPU_SAMPLE_SORT 2',
                   '#define SYMGPU_BASIS_DIRECT 1', '#define SYMGPU_BASIS_TILED 2'):
        assert needle in text, f'include/symgpu.h (f10) does not state: {needle}'
    assert (so.M0, so.M1, so.W0, so.W1) == (0xD2E7470EE14C6C93, 0xCA5A826395121157, 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B) and so.RADIX == 16


def test_entry_points_bindings_and_methods_are_in_place():
    from symmer_amd import QuantumState, _lib, kernels, operators, utils
    protos = header_prototypes()
    for name, n_args in (('symgpu_philox_uniform', 4), ('symgpu_sample_plan', 3), ('symgpu_sample_free', 1), ('symgpu_sample_info', 3),
                         ('symgpu_sample_draw', 9), ('symgpu_basis_change', 5), ('symgpu_counts_signed_sums', 6)):
        assert len(protos[name]) == n_args and len(_lib.SIGNATURES[name]) == n_args, name
    for method in ('sample_state', 'sample_counts', 'measure_state_in_computational_basis'):
        assert callable(getattr(QuantumState, method))
    assert hasattr(QuantumState, 'normalize_counts') and callable(operators.change_of_basis_XY_to_Z) and callable(utils.sampled_expval)
    for name in ('SamplePlan', 'philox_uniforms', 'basis_change_dev', 'counts_signed_sums'):
        assert hasattr(kernels, name)
    assert (kernels.SAMPLE_HIST, kernels.SAMPLE_SORT, kernels.BASIS_DIRECT, kernels.BASIS_TILED) == (1, 2, 1, 2)
    if os.path.exists(_lib.LIB_PATH):                               # dlopen only: no GPU call
        lib = ctypes.CDLL(_lib.LIB_PATH, mode=os.RTLD_NOW | os.RTLD_LOCAL)
        assert all(hasattr(lib, name) for name in protos if name.startswith('symgpu_sample_'))


def test_normalize_counts_is_the_reference_formula():
    from symmer_amd import QuantumState
    counts = QuantumState([[0, 0], [0, 1], [1, 1]], [3, 0, 1])
    assert np.array_equal(counts.normalize_counts.state_op.coeff_vec, np.sqrt(np.array([3, 0, 1]) / 4 + 0j))
    assert np.array_equal(counts.normalize_counts.state_matrix, counts.state_matrix)


# ---- the fixed seed of the finite-shot check ------------------------------------------------------------------------------------------------
def test_finite_shot_case_passes_on_the_restatement_alone():
    symp, coeff, amp = so.expval_case()
    n = so.EXPVAL_QUBITS
    order = co.term_order(symp, coeff, 'QWC', 'largest_first')
    members = co.cliques_in_order(co.colouring(symp, order, 'QWC')[0], order)
    sums = so.sampled_sums(symp, n, amp, members, so.EXPVAL_SHOTS, so.EXPVAL_SEED)
    energy = float(coeff @ (sums / so.EXPVAL_SHOTS))
    exact, se = so.exact_energy(symp, coeff, n, amp), so.energy_standard_error(symp, coeff, n, amp, members, so.EXPVAL_SHOTS)
    print(f'{len(members)} cliques: sampled {energy:.6f}, exact {exact:.6f}, standard error {se:.6f}, off by {abs(energy - exact) / se:.2f} of them')
    assert se > 0 and abs(energy - exact) <= 6 * se
    assert np.all(np.abs(sums) <= so.EXPVAL_SHOTS) and np.all((sums - so.EXPVAL_SHOTS) % 2 == 0)
