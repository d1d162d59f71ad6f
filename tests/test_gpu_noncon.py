"""GPU: csrc/noncon.hip — symgpu_noncon_search, symgpu_noncon_signs_dev — and what sits on it (kernels.noncon_search / noncon_signs_dev,
NoncontextualOp, NoncontextualSolver) against tests/_noncon_oracle.py (held against the reference in tests/test_noncon_oracle.py) and the
reference's own answers (tests/golden/noncon_solve.npz).

The search blocks the assignment bits into L low bits (transformed in LDS) and the rest (strided over workgroups); L is read from the
call's info words, never written here, and the sizes sit on both sides of it.  Tolerance everywhere: 4 (T + 64) 2^-52 sum|c|, the
worst-case reordering error of a T-term double sum with a factor 4 for the squares and the square root."""
import ctypes

import numpy as np
import pytest

from symmer_amd import NoncontextualOp, NoncontextualSolver, PauliwordOp, kernels, packing, _lib
from symmer_amd.kernels import DeviceOp
import _noncon_oracle as no

pytestmark = pytest.mark.gpu
CASES = no.golden_cases()
_L = []


def low_bits():
    """L of the library, from the info words of an empty call"""
    if not _L:
        energy, best, info = kernels.noncon_search(np.zeros(0), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int32), 0, 0, want_info=True)
        assert (energy, best) == (0.0, 0) and list(info[1:]) == [1, 0, 1]
        assert 9 <= info[0] <= 12
        _L.append(int(info[0]))
    return _L[0]


def random_input(rng, T, f, Q, dyadic=False):
    coeff = rng.integers(-512, 513, T) / 64.0 if dyadic else rng.standard_normal(T)
    mask = rng.integers(0, 1 << f, T, dtype=np.uint64) if f else np.zeros(T, dtype=np.uint64)
    clique = rng.integers(-1, Q, T).astype(np.int32) if Q else np.full(T, -1, dtype=np.int32)
    return coeff, mask, clique


def check_search(coeff, mask, clique, f, Q, exact=False, want=None):
    """One device search against the restatement: the whole landscape, the returned minimum, the tie rule on the device's own values."""
    L = low_bits()
    energy, best, energies, info = kernels.noncon_search(coeff, mask, clique, f, Q, want_energies=True, want_info=True)
    want = no.landscape(coeff, mask, clique, f, Q) if want is None else want
    tol = no.tolerance(coeff)
    assert energies.shape == want.shape == (1 << f,)
    worst = float(np.max(np.abs(energies - want)))
    assert worst <= tol, f'f = {f} T = {len(coeff)} Q = {Q}: landscape off by {worst}, tolerance {tol}'
    if exact:
        assert np.array_equal(energies, want), 'exact sums must be bit-equal'
    assert energy == energies[best] and np.float64(energy).tobytes() == energies[best].tobytes()
    assert best == int(np.flatnonzero(energies == energies.min())[-1]), 'among equal energies the largest mask wins'
    assert want[best] <= want.min() + tol
    assert info[0] == L and info[1] == 1 << (f - min(f, L)) and info[2] == len(coeff) and 1 <= info[3] <= info[1], list(info)
    return energy, best, energies


# ---------------------------------------------------------------- the search kernel alone --------------------------------------------
@pytest.mark.parametrize('f_of_L', [lambda L: 0, lambda L: 1, lambda L: L - 1, lambda L: L, lambda L: L + 1, lambda L: L + 3],
                         ids=['0', '1', 'L-1', 'L', 'L+1', 'L+3'])
def test_search_random(f_of_L):
    f = f_of_L(low_bits())
    rng = np.random.default_rng(4100 + f)
    for T in (0, 1, 63, 64, 65, 300):
        for Q in (0, 1, 3, 17):
            check_search(*random_input(rng, T, f, Q), f, Q)


@pytest.mark.parametrize('f_of_L', [lambda L: 0, lambda L: 3, lambda L: L, lambda L: L + 2], ids=['0', '3', 'L', 'L+2'])
def test_search_dyadic_without_cliques_is_exact(f_of_L):
    f = f_of_L(low_bits())
    rng = np.random.default_rng(4200 + f)
    for T in (1, 65, 300):
        check_search(*random_input(rng, T, f, 0, dyadic=True), f, 0, exact=True)


def test_search_masks_in_the_high_bits_only():
    # every entry of a group folds onto slot 0: 300 and 40,000 entries on one slot (the second more than one round of item sums can hold
    # at the smallest chunk).  The energies depend on the high part alone: the restatement runs on the high bits and is repeated.
    L = low_bits()
    rng = np.random.default_rng(4301)
    for T, h, Q in ((300, 3, 3), (40000, 1, 0)):
        coeff, high, clique = random_input(rng, T, h, Q)
        want = np.repeat(no.landscape(coeff, high, clique, h, Q), 1 << L)
        check_search(coeff, high << np.uint64(L), clique, L + h, Q, want=want)


def test_search_masks_in_the_low_bits_only():
    L = low_bits()
    rng = np.random.default_rng(4302)
    coeff, low, clique = random_input(rng, 300, L, 3)
    energy, best, energies = check_search(coeff, low, clique, L + 2, 3)
    assert np.array_equal(energies.reshape(4, -1), np.tile(energies[:1 << L], (4, 1)))      # the high bits change nothing, bit for bit
    assert best >> L == 3


@pytest.mark.parametrize('where', ['low', 'boundary_low', 'boundary_high', 'top'])
def test_search_exact_two_fold_tie(where):
    # the terms of clique 0 all use one generator that nothing else uses: flipping it negates the clique's sum, the square is the same
    L = low_bits()
    f = L + 2
    bit = {'low': 0, 'boundary_low': L - 1, 'boundary_high': L, 'top': f - 1}[where]
    rng = np.random.default_rng(4400 + bit)
    coeff, mask, clique = random_input(rng, 120, f, 2)
    lone = np.uint64(1 << bit)
    mask = np.where(clique == 0, mask | lone, mask & ~lone)
    assert np.count_nonzero(clique == 0) > 5
    energy, best, energies = check_search(coeff, mask, clique, f, 2)
    flipped = np.arange(1 << f) ^ (1 << bit)
    assert np.array_equal(energies, energies[flipped]), 'the tie is exact'
    assert best & (1 << bit), 'the larger mask of the pair wins'


def test_search_zero_coefficients():
    L = low_bits()
    rng = np.random.default_rng(4500)
    coeff, mask, clique = random_input(rng, 200, L + 1, 3)
    coeff[rng.random(200) < 0.5] = 0.0
    coeff[3] = -0.0
    check_search(coeff, mask, clique, L + 1, 3)
    energy, best, energies = check_search(np.zeros(64), mask[:64], clique[:64], L + 1, 3)
    assert not energies.any() and energy == 0.0 and best == (1 << (L + 1)) - 1


def test_search_planted_minimum_across_the_boundary():
    # one term per generator: E(m) = sum_b c_b (-1)^{m_b}, minimal (and exactly -f) where m has a bit for c_b > 0 only: bits L-1 and L
    L = low_bits()
    f = L + 2
    planted = (1 << (L - 1)) | (1 << L)
    coeff = np.array([1.0 if (planted >> b) & 1 else -1.0 for b in range(f)])
    mask = np.array([1 << b for b in range(f)], dtype=np.uint64)
    energy, best, energies = check_search(coeff, mask, np.full(f, -1, dtype=np.int32), f, 0, exact=True)
    assert (energy, best) == (-float(f), planted) and np.count_nonzero(energies == energy) == 1


def test_search_is_deterministic():
    L = low_bits()
    rng = np.random.default_rng(4600)
    coeff, mask, clique = random_input(rng, 3000, L + 3, 5)
    mask[:600] &= np.uint64(~((1 << L) - 1) & ((1 << (L + 3)) - 1))          # long runs on slot 0 as well
    first = kernels.noncon_search(coeff, mask, clique, L + 3, 5, want_energies=True)
    second = kernels.noncon_search(coeff.copy(), mask.copy(), clique.copy(), L + 3, 5, want_energies=True)
    assert first[2].tobytes() == second[2].tobytes() and first[1] == second[1]
    assert np.float64(first[0]).tobytes() == np.float64(second[0]).tobytes()
    without = kernels.noncon_search(coeff, mask, clique, L + 3, 5)
    assert without == (first[0], first[1])


def test_search_refusals():
    lib = _lib.lib()
    coeff, mask, clique = np.array([1.0, -2.0]), np.array([1, 2], dtype=np.uint64), np.array([-1, 0], dtype=np.int32)
    energy, best = ctypes.c_double(7.0), ctypes.c_uint64(7)
    out = (ctypes.addressof(energy), ctypes.addressof(best))

    def refused(*args):
        rc = lib.symgpu_noncon_search(*args)
        assert rc == _lib.E_INVALID and 'noncon_search' in _lib.last_error()
        # the call after a refusal works
        assert kernels.noncon_search(coeff, mask, clique, 2, 1) == (-3.0, 3)

    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, 41, 1, *out, None, None)
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, -1, 1, *out, None, None)
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, 2, -1, *out, None, None)
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, -1, 2, 1, *out, None, None)
    for bad in (1, -2):
        wrong = np.array([-1, bad], dtype=np.int32)
        refused(coeff.ctypes.data, mask.ctypes.data, wrong.ctypes.data, 2, 2, 1, *out, None, None)
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, 1, 1, *out, None, None)          # mask bit 1 with one free generator
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, 2, 1, None, out[1], None, None)
    refused(coeff.ctypes.data, mask.ctypes.data, clique.ctypes.data, 2, 2, 1, out[0], None, None, None)
    refused(None, mask.ctypes.data, clique.ctypes.data, 2, 2, 1, *out, None, None)
    with pytest.raises(_lib.SymgpuError):
        kernels.noncon_search(np.array([np.inf, 1.0]), mask, clique, 2, 1)
    with pytest.raises(_lib.SymgpuError, match='1e154'):                # finite, but the squares of the sums would not be
        kernels.noncon_search(np.array([9e153, -9e153]), mask, clique, 2, 1)
    big = kernels.noncon_search(np.array([4e153, -5e153]), mask, clique, 2, 1, want_energies=True)
    assert np.all(np.isfinite(big[2])) and big[0] == big[2].min()
    assert (energy.value, best.value) == (7.0, 7), 'a refused call writes no result'


# ---------------------------------------------------------------- the signs kernel ----------------------------------------------------
def upload(symp):
    return DeviceOp.upload(packing.pack_rows(np.asarray(symp, dtype=bool)))


def device_signs(terms, gens, selection):
    with upload(terms) as t, upload(gens) as g:
        return kernels.noncon_signs_dev(t, g, selection)


@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_signs_match_reference(tag, case):
    gens = np.vstack([case['generators'], case['cliques']])
    selection = np.hstack([case['G_indices'], case['C_indices']]).astype(bool)
    got = device_signs(case['symp'], gens, selection)
    assert got.dtype == np.int8 and np.array_equal(got, case['pauli_mult_signs'])


@pytest.mark.parametrize('n', [1, 63, 64, 65, 130, 600])            # 600: ten words a half-row, more than the lanes that share a term
def test_signs_match_host_products(n):
    rng = np.random.default_rng(4700 + n)
    g, T = (3, 8) if n == 1 else (7, 14)
    gens = rng.random((g, 2 * n)) < (0.5 if n == 1 else min(0.5, 6.0 / n))
    selection = rng.random((T, g)) < 0.5
    selection[0] = False                                               # the empty product is the identity
    selection[1] = True
    terms, want = np.zeros((T, 2 * n), dtype=bool), np.zeros(T, dtype=np.int8)
    for k in range(T):
        product = PauliwordOp(np.zeros(2 * n, dtype=bool), [1])
        for j in np.flatnonzero(selection[k]):
            product = product * PauliwordOp(gens[j], [1])
        terms[k] = product.symp_matrix[0]
        c = complex(product.coeff_vec[0])
        assert abs(c) == 1 and (c.real == 0 or c.imag == 0)
        want[k] = int(c.real)
    got = device_signs(terms, gens, selection)
    assert np.array_equal(got, want), (n, got, want)
    assert want[0] == 1
    assert np.array_equal(no.product_signs(terms, gens, selection), want)
    # another row than the product: 0, whatever the phase
    other = terms.copy()
    other[:, 2 * n - 1] ^= True
    assert not device_signs(other, gens, selection).any()


def test_signs_known_answers():
    labels = lambda ls: PauliwordOp.from_list(ls).symp_matrix
    gens = labels(['XI', 'ZI', 'IZ', 'ZZ'])
    terms = labels(['YI', 'YI', 'ZZ', 'II', 'XZ', 'ZI'])
    selection = np.array([[1, 1, 0, 0],      # X Z = -iY: a phase -i
                          [0, 0, 1, 0],      # Z_1 is not Y_0
                          [0, 1, 1, 0],      # Z_0 Z_1 = +ZZ
                          [0, 1, 1, 1],      # Z_0 Z_1 ZZ = +II
                          [1, 0, 1, 0],      # X_0 Z_1 = +XZ
                          [1, 1, 0, 0]], dtype=bool)
    assert list(device_signs(terms, gens, selection)) == [0, 0, 1, 1, 1, 0]
    # YY is not II; (XZ)(ZX) = (-iY)(iY) = +YY; (YY)(XX) = (-iZ)(-iZ) = -ZZ — the expected signs also through the operator product
    gens = labels(['YY', 'XZ', 'ZX', 'XX'])
    terms = labels(['II', 'YY', 'ZZ'])
    selection = np.array([[1, 0, 0, 0], [0, 1, 1, 0], [1, 0, 0, 1]], dtype=bool)
    want = []
    for k in range(3):
        product = PauliwordOp.from_list(['II'])
        for j in np.flatnonzero(selection[k]):
            product = product * PauliwordOp(gens[j], [1])
        want.append(int(complex(product.coeff_vec[0]).real) if np.array_equal(product.symp_matrix[0], terms[k]) else 0)
    assert want == [0, 1, -1]
    assert list(device_signs(terms, gens, selection)) == want


# ---------------------------------------------------------------- the public API ------------------------------------------------------
@pytest.mark.parametrize('tag,case', CASES, ids=[tag for tag, _ in CASES])
def test_noncontextual_op_matches_reference(tag, case):
    import warnings
    H = NoncontextualOp(case['symp'], case['coeff'])
    tol = no.tolerance(case['coeff'].real)
    # the structure: every step is a port of a call that is pinned to the reference
    assert np.array_equal(H.symmetry_generators.symp_matrix, case['generators'])
    assert H.n_cliques == case['cliques'].shape[0] and np.array_equal(H.clique_operator.symp_matrix.reshape(H.n_cliques, 2 * H.n_qubits), case['cliques'])
    assert np.array_equal(H.G_indices, case['G_indices']) and np.array_equal(np.reshape(H.C_indices, case['C_indices'].shape), case['C_indices'])
    assert np.array_equal(H.pauli_mult_signs, case['pauli_mult_signs'])
    # two invariants that do not depend on the basis chosen
    if H.symmetry_generators.n_terms:
        assert np.all(H.symmetry_generators.commutes_termwise(H))
    gens = np.vstack([H.symmetry_generators.symp_matrix, H.clique_operator.symp_matrix.reshape(H.n_cliques, 2 * H.n_qubits)])
    selection = np.hstack([H.G_indices, np.reshape(H.C_indices, (H.n_terms, -1))]).astype(bool)
    for k in range(0, H.n_terms, max(1, H.n_terms // 12)):              # a dozen terms through the operator product itself
        product = PauliwordOp(np.zeros(2 * H.n_qubits, dtype=bool), [1])
        for j in np.flatnonzero(selection[k]):
            product = product * PauliwordOp(gens[j], [1])
        assert np.array_equal(product.symp_matrix[0], case['symp'][k])
        assert complex(product.coeff_vec[0]) * H.pauli_mult_signs[k] == 1
    assert np.array_equal(np.bitwise_xor.reduce(gens[None, :, :] & selection[:, :, None], axis=1), case['symp'])     # every term's row
    # ... and every term's sign, by the restated phase rule (held against the reference's signs in tests/test_noncon_oracle.py)
    assert np.array_equal(no.product_signs(case['symp'], gens, selection), H.pauli_mult_signs)

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                 # update_sector warns about the generators a state leaves free
        H.solve(strategy='brute_force', ref_state=case.get('ref_state'))
    assert abs(H.energy - float(case['energy'])) <= tol, (H.energy, float(case['energy']), tol)
    nu = np.asarray(H.symmetry_generators.coeff_vec)
    assert nu.shape == case['nu'].shape and set(np.unique(nu)) <= {-1, 1}
    assert abs(H.get_energy(nu) - H.energy) <= tol
    if case['unique']:
        assert np.array_equal(nu, case['nu'])
    if 'sector' in case:
        fixed = case['sector'] != 0
        assert np.array_equal(nu[fixed], case['sector'][fixed])
    if H.n_cliques:
        assert np.allclose(H.clique_operator.coeff_vec, H.get_symmetry_contributions(nu)[1], rtol=0, atol=tol)


def test_enough_golden_cases_pin_nu():
    n_unique = sum(bool(case['unique']) for _, case in CASES)
    assert 4 * n_unique >= 3 * len(CASES)


def test_solver_returns_energy_and_nu():
    case = dict(CASES)['10']
    H = NoncontextualOp.from_PauliwordOp(PauliwordOp(case['symp'], case['coeff']))
    energy, nu = NoncontextualSolver(H).energy_via_brute_force()
    assert abs(energy - float(case['energy'])) <= no.tolerance(case['coeff'].real) and np.array_equal(nu, case['nu'])
    # the search inputs are the restatement's
    for got, want in zip(NoncontextualSolver(H).search_inputs(), no.search_inputs(case['coeff'], H.G_indices, H.C_indices, H.pauli_mult_signs)):
        assert np.array_equal(got, want)
    # a fixed generator is folded into the signs: fixing the optimum's own values leaves the energy where it is
    fixed = np.zeros(len(nu), dtype=bool)
    fixed[::2] = True
    energy_fixed, nu_fixed = NoncontextualSolver(H, fixed, nu[fixed]).energy_via_brute_force()
    assert abs(energy_fixed - energy) <= no.tolerance(case['coeff'].real) and np.array_equal(nu_fixed, nu)
    with pytest.raises(ValueError):
        H.solve(strategy='no_such_strategy')


def test_binary_relaxation_runs_the_reference_optimiser():
    case = dict(CASES)['03']
    H = NoncontextualOp(case['symp'], case['coeff'])
    H.solve(strategy='binary_relaxation')
    # get_energy flips a sign only where nu is exactly -1, so the relaxed objective takes the values of the landscape and nothing else: the
    # optimiser's answer is one of them, no better than the minimum and no worse than the all-+1 assignment nearly every sample evaluates
    tol = no.tolerance(case['coeff'].real)
    energies = no.solve(case['coeff'], H.G_indices, H.C_indices, H.pauli_mult_signs)[2]
    assert np.min(np.abs(energies - H.energy)) <= tol
    assert float(case['energy']) - tol <= H.energy <= energies[0] + tol
    nu = np.asarray(H.symmetry_generators.coeff_vec)
    assert nu.shape == case['nu'].shape and set(np.unique(nu)) <= {-1, 1}


def test_from_hamiltonian():
    rng = np.random.default_rng(4800)
    symp = rng.random((60, 10)) < 0.4
    symp[:8, :5] = False                                                # some diagonal terms for certain
    H = PauliwordOp(symp, rng.standard_normal(60)).cleanup()
    diag = NoncontextualOp.from_hamiltonian(H, strategy='diag')
    keep = ~np.any(H.X_block, axis=1)
    assert np.array_equal(diag.symp_matrix, H.symp_matrix[keep]) and diag.n_cliques == 0
    case = dict(CASES)['05']
    full = PauliwordOp(case['symp'], case['coeff'])
    basis = PauliwordOp(np.vstack([case['generators'], case['cliques']]), np.ones(len(case['generators']) + len(case['cliques'])))
    again = NoncontextualOp.from_hamiltonian(full, strategy='generators', generators=basis, use_jordan_product=True)
    assert np.array_equal(again.symp_matrix, case['symp'])
    for strategy in ('stabilizers', 'DFS_magnitude', 'SingleSweep_random'):
        with pytest.raises(NotImplementedError):
            NoncontextualOp.from_hamiltonian(H, strategy=strategy)
    with pytest.raises(ValueError):
        NoncontextualOp.from_hamiltonian(H, strategy='nonsense')


def test_refusals_of_the_class(monkeypatch):
    with pytest.raises(AssertionError):
        NoncontextualOp.from_PauliwordOp(PauliwordOp.from_list(['XZ', 'ZX', 'ZI', 'IZ']))
    with pytest.raises(NotImplementedError, match='AntiCommutingOp'):
        NoncontextualOp.from_PauliwordOp(PauliwordOp.from_list(['XZ', 'ZX', 'XX', 'YY'])).noncon_state()
    # 41 independent commuting terms: 41 free generators, refused before the device is asked
    n = 41
    H = NoncontextualOp(np.hstack([np.zeros((n, n), dtype=bool), np.eye(n, dtype=bool)]), np.arange(1, n + 1, dtype=float))
    assert H.symmetry_generators.n_terms == n and H.n_cliques == 0

    def no_device_call(*args, **kwargs):
        raise AssertionError('the search was launched')
    monkeypatch.setattr(kernels, 'noncon_search', no_device_call)
    with pytest.raises(ValueError, match='41 free'):
        H.solve()
    monkeypatch.undo()
    H.solve(ref_state=np.ones(n, dtype=int))                            # every generator fixed: one evaluation
    assert H.energy == -float(n * (n + 1) // 2) and np.all(H.symmetry_generators.coeff_vec == -1)
