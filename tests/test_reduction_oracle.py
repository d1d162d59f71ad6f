"""The restatement of the reduction order (tests/_reduction_oracle.py) on the CPU: against a thread-by-thread loop written out from the
header's sentence, against the other means the suite already has (parameter shift, the dense commutator, NumPy's vdot and matrix
products), on dyadic inputs against integer arithmetic, and — for the very inputs the GPU tests feed at the sizes where a thread adds
more than one unit — against three orders the header does not state, which must give other values.  No GPU."""
import functools

import numpy as np
import pytest

import _ansatz_oracle as ao
import _matvec_oracle as mo
import _reduction_oracle as ro


# ---- the order itself ------------------------------------------------------------------------------------------------------------------
def by_threads(terms):
    """The header's sentence as loops: chunk by chunk, thread by thread, then the fold in a 256-entry array, then the chunk sums."""
    count = len(terms)
    chunk = max(256, count // 1024)
    chunk_sums = []
    for first in range(0, count, chunk):
        s = [0.0] * 256
        for t in range(256):
            for u in range(first + t, min(first + chunk, count), 256):
                s[t] = s[t] + terms[u]
        h = 128
        while h:
            for t in range(h):
                s[t] = s[t] + s[t + h]
            h //= 2
        chunk_sums.append(s[0])
    total = 0.0
    for c in chunk_sums:
        total = total + c
    return total


@pytest.mark.parametrize('count', [1, 2, 16, 255, 256, 257, 512, 700, 1 << 12, (1 << 18) + 3, 1 << 19, (1 << 19) + 1000])
def test_ordered_sum_against_the_loops(count):
    terms = np.random.default_rng(count).standard_normal(count)
    assert ro.ordered_sum(terms) == by_threads([float(v) for v in terms])
    assert ro.chunk_of(count) == (256 if count < (257 << 10) else count >> 10)


def test_ordered_sum_small_values():
    assert ro.ordered_sum(np.zeros(0)) == 0.0 and ro.ordered_sum([3.5]) == 3.5
    assert ro.ordered_sum_complex([1.0, 2.0], [0.5, -0.5]) == (3.0, 0.0)
    # 1 + 2^-53 + 2^-53: element 1 and element 129 meet in the fold before element 0 joins them only if the fold goes by halving
    t = np.zeros(256)
    t[0], t[1], t[129] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ro.ordered_sum(t) == 1.0 + 2.0 ** -52 and ro.two_level(t, 256, ro.fold_ascending) == 1.0
    assert ro.chunk_of(1 << 18) == 256 and ro.chunk_of(1 << 19) == 512 and ro.chunk_of(1 << 20) == 1024


def test_slots_cover_every_element_once():
    for n, x in ((1, 0), (1, 1), (5, 0), (5, 0b10000), (5, 0b00001), (5, 0b01101), (10, 0b1000000001)):
        b0, b1 = ro.slot_elements(x, n)
        assert np.array_equal(np.sort(np.concatenate([b0, b1])), np.arange(1 << n))
        assert np.all(np.diff(b0) > 0) and np.array_equal(b1, b0 ^ x if x else b0 + (1 << (n - 1)))
        assert not np.any(b0 & (1 << (x.bit_length() - 1 if x else n - 1)))


# ---- agreement with the other means ----------------------------------------------------------------------------------------------------
SMALL_GENS = {1: ['X', 'Z', 'Y', 'I'], 3: ['XYZ', 'ZIZ', 'YYX', 'YYY', 'IXI'],
              6: ['XIIIIY', 'ZZIIIZ', 'YYXYYI', 'IIIYXY', 'YIYIYI', 'IZIIII'],
              10: ['XIIIIIIIIY', 'ZIIIIIIIIZ', 'YYXXYYIIII', 'IIIIIIIYXY', 'YXYXYIIIIZ', 'IYIYIYIIII', 'ZZZZZZZZZZ']}


@pytest.mark.parametrize('n', [1, 3, 6, 10])
def test_gradients_and_energy_against_the_other_means(n):
    strings = SMALL_GENS[n]
    if n >= 6:
        assert {s.count('Y') for s in strings} >= {0, 1, 2, 3, 4}
    assert any(set(s) <= set('IZ') and 'Z' in s for s in strings)                    # an x = 0 string
    rng = np.random.default_rng(40 + n)
    T = 3 * n + 2
    h_symp, h_coeff = rng.random((T, 2 * n)) < 0.5, rng.standard_normal(T)
    gens = ro.symp_of(strings)
    K = len(strings)
    theta, ref = rng.uniform(-np.pi, np.pi, K), ro.unit(ro.gaussian(rng, 1 << n))
    R = ao.bound(n, K, T, h_coeff)
    psi = ao.state(gens, theta, ref)
    assert abs(ro.energy_ordered(h_symp, h_coeff, psi) - ao.energy(h_symp, h_coeff, psi)) <= R
    got, want = ro.sweep_grad_ordered(h_symp, h_coeff, gens, theta, ref), ao.grad_shift(h_symp, h_coeff, gens, theta, ref)
    print(f'n={n}: sweep max|g - g_shift| = {np.abs(got - want).max():.3e}, R = {R:.3e}')
    assert np.abs(got - want).max() <= R
    got, want = ro.pool_grad_ordered(h_symp, h_coeff, gens, psi), ao.pool_grad(ao.dense_operator(h_symp, h_coeff), gens, psi)
    print(f'n={n}: pool max|g - g_dense| = {np.abs(got - want).max():.3e}')
    assert np.abs(got - want).max() <= R


@pytest.mark.parametrize('n', [1, 3, 6, 10])
@pytest.mark.parametrize('use_mask', [False, True])
def test_lanczos_step_and_combine_against_plain_numpy(n, use_mask):
    rng = np.random.default_rng(50 + n)
    side, cap = 1 << n, min(3, 1 << n)
    T = 12
    symp = np.hstack([np.zeros((T, n), dtype=bool), rng.random((T, n)) < 0.5])      # Z strings and pairs XX + YY: the particle number is conserved
    c = rng.standard_normal(T)
    for q in range(n - 1):
        xx = np.zeros((2, 2 * n), dtype=bool)
        xx[:, [q, q + 1]] = True
        xx[1, [n + q, n + q + 1]] = True
        symp, c = np.vstack([symp, xx]), np.concatenate([c, [0.5 * (q + 1)] * 2])
    u = 2.0 ** -53
    tol = 64 * u * (len(c) + side) * np.abs(c).sum()
    mask = ro.particle_sector(n) if use_mask and n >= 6 else np.ones(side, dtype=bool)       # the small sectors have fewer than three states
    V = np.zeros((cap, side), dtype=complex)
    V[0] = ro.unit(ro.gaussian(rng, side) * mask)
    for j in range(cap - 1):
        alpha, beta, v_next = ro.lanczos_step_ordered(symp, c, mask if use_mask else None, V, j)
        w = mask * mo.matvec(symp, c, V[j])
        want_alpha = np.vdot(V[j], w).real
        for _ in range(2):
            w = w - V[:j + 1].T @ (V[:j + 1].conj() @ w)
        want_beta = np.linalg.norm(w)
        assert abs(alpha - want_alpha) <= tol and abs(beta - want_beta) <= tol
        assert np.abs(v_next - w / want_beta).max() <= tol / want_beta
        assert not v_next[~mask].any()
        V[j + 1] = v_next
    s = rng.standard_normal(cap)
    assert np.abs(ro.combine_ordered(V, s) - s @ V).max() <= 8 * u * cap * np.abs(s).max()
    got = ro.combine_ordered(V, s, normalise=True)
    assert np.abs(got - s @ V / np.linalg.norm(s @ V)).max() <= (16 * cap + side) * u
    assert np.array_equal(ro.combine_ordered(np.zeros((2, 4)), [1.0, 2.0], normalise=True), np.zeros(4))


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------
def test_the_shared_strings():
    for n in sorted(set(ro.SWEEP_SIZES + ro.ELEMENT_SIZES)):
        h, gens = ro.h_string(n), ro.generators(n)
        assert len(h) == n and h[0] != 'I' and h[-1] != 'I' and all(len(s) == n and ro.anticommute(s, h) for s in gens)
        assert len(gens) == (2 if n == 21 else 4)
        if n >= 3:
            assert set(h) == set('IXYZ')
            x, z, y = ao.gens_of(ro.symp_of(gens))
            assert x[0] == (1 << (n - 1)) | 1 and y[0] == 1 and x[-1] == 0 and z[-1] == (1 << (n - 1)) | 1
        if n >= 14 and n != 21:
            segs = ao.plan_runs(ro.symp_of(gens))
            assert [(k0, k1, tiled) for k0, k1, _, tiled in segs] == [(0, 2, True), (2, 3, False), (3, 4, True)]
            assert sum(ch in 'XY' for ch in gens[2]) >= 13
        assert set(ro.masked_h_string(n)) <= set('IZ')
    h_symp, h_coeff = ro.dyadic_operator(19)
    x = ao.gens_of(h_symp)[0]
    assert len(x) == 12 and x[2] == x[3] and np.array_equal(h_symp[10], h_symp[11]) and h_coeff[10] == -h_coeff[11]


@functools.lru_cache(maxsize=None)
def sweep_case(n):
    """[units of t_k] for k = K-1 .. 0 of the size's inputs."""
    return [units for _, units in ro.sweep_units(*ro.sweep_inputs(n))]


@functools.lru_cache(maxsize=None)
def pool_case(n):
    """[terms of row j] of the size's pool, then the terms of the energy."""
    h_symp, h_coeff, pool, psi = ro.pool_inputs(n)
    return list(ro.pool_terms(h_symp, h_coeff, pool, psi)) + [ro.energy_terms(h_symp, h_coeff, psi)]


@pytest.mark.parametrize('n', ro.SWEEP_SIZES)
def test_every_expected_sweep_gradient_is_large_enough(n):
    g = np.array([-2.0 * ro.ordered_sum(units) for units in sweep_case(n)])
    print(n, g)
    assert len(g) == (2 if n == 21 else 4) and np.abs(g).min() >= ro.MIN_GRADIENT
    assert all(len(units) == 1 << (n - 1) for units in sweep_case(n))


@pytest.mark.parametrize('n', ro.ELEMENT_SIZES)
def test_every_expected_pool_gradient_is_large_enough(n):
    g = np.array([-2.0 * ro.ordered_sum(terms) for terms in pool_case(n)[:-1]])
    print(n, g)
    assert len(g) == 4 and np.abs(g).min() >= ro.MIN_GRADIENT


def differs_from_the_other_orders(terms, what):
    want = ro.ordered_sum(terms)
    for name, other in ro.OTHER_ORDERS.items():
        assert other(terms) != want, f'{what}: "{name}" gives the same value; the input cannot tell the orders apart'


@pytest.mark.parametrize('n', ro.LARGE_SWEEP)
def test_the_large_sweep_inputs_tell_the_orders_apart(n):
    assert ro.chunk_of(1 << (n - 1)) > 256
    for i, units in enumerate(sweep_case(n)):
        differs_from_the_other_orders(units, f'n = {n}, sweep step {i}')


@pytest.mark.parametrize('n', ro.LARGE_ELEMENT)
def test_the_large_element_inputs_tell_the_orders_apart(n):
    assert ro.chunk_of(1 << n) > 256
    for j, terms in enumerate(pool_case(n)):
        differs_from_the_other_orders(terms, f'n = {n}, pool row {j} (4: the energy)')
    v0 = ro.lanczos_start(n)
    w = mo.matvec(ro.symp_of([ro.h_string(n)]), ro.H_COEFF, v0)
    re, im = ro.dot_terms(v0, w)
    differs_from_the_other_orders(re, f'n = {n}, Re <v_0, w>')
    differs_from_the_other_orders(im, f'n = {n}, Im <v_0, w>')
    differs_from_the_other_orders(w.real * w.real + w.imag * w.imag, f'n = {n}, <w, w>')
    keep = ro.particle_sector(n)
    v0 = ro.lanczos_start(n, keep)
    w = np.where(keep, mo.matvec(ro.symp_of([ro.masked_h_string(n)]), ro.H_COEFF, v0), 0.0)
    differs_from_the_other_orders(ro.dot_terms(v0, w)[0], f'n = {n}, masked Re <v_0, w>')
    differs_from_the_other_orders(w.real * w.real + w.imag * w.imag, f'n = {n}, masked <w, w>')


# ---- exactness -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ro.LARGE_ELEMENT)
def test_dyadic_inputs_give_the_integer_result_in_the_stated_order(n):
    (h_symp, h_coeff), pool, v = ro.dyadic_operator(n), ro.dyadic_pool(n), ro.dyadic_vector(n)
    energy, grad = ro.integer_results(h_symp, h_coeff, pool, v)
    assert energy != 0 and np.all(grad != 0)
    assert ro.energy_ordered(h_symp, h_coeff, v) == energy
    terms = list(ro.pool_terms(h_symp, h_coeff, pool, v))
    assert np.array_equal([-2.0 * ro.ordered_sum(t) for t in terms], grad)
    for name, other in ro.OTHER_ORDERS.items():                                       # exact: every order gives it
        assert np.array_equal([-2.0 * other(t) for t in terms], grad), name
    assert np.array_equal(ro.sweep_grad_ordered(h_symp, h_coeff, pool, np.zeros(len(pool)), v), grad)
    assert ro.lanczos_step_ordered(h_symp, h_coeff, None, v[None, :], 0)[0] == energy
