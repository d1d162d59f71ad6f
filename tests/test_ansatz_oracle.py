"""The NumPy oracle of the ansatz kernels (tests/_ansatz_oracle.py) against independent mathematics: Kronecker products of the 2 x 2 Pauli
matrices, scipy's matrix exponential, and central finite differences.  No GPU."""
import functools
import itertools

import numpy as np
import pytest
from scipy.linalg import expm

import _ansatz_oracle as ao

PAULI = {'I': np.eye(2, dtype=complex), 'X': np.array([[0, 1], [1, 0]], dtype=complex),
         'Y': np.array([[0, -1j], [1j, 0]]), 'Z': np.array([[1, 0], [0, -1]], dtype=complex)}


def symp_of(strings):
    n = len(strings[0])
    out = np.zeros((len(strings), 2 * n), dtype=bool)
    for r, s in enumerate(strings):
        for q, ch in enumerate(s):
            out[r, q], out[r, n + q] = ch in 'XY', ch in 'ZY'
    return out


def kron_of(s):
    return functools.reduce(np.kron, [PAULI[ch] for ch in s])


def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


STRINGS = ['Z', 'Y', 'XZ', 'YY', 'IY', 'XYZ', 'YYY', 'ZIX', 'YXYY', 'YYYY', 'IIII', 'ZZIZ', 'XIYZ', 'YYIY']


def test_strings_cover_every_y_count():
    assert {s.count('Y') for s in STRINGS} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize('s', STRINGS)
def test_apply_pauli_and_rotate_against_kron_and_expm(s):
    n = len(s)
    rng = np.random.default_rng(len(s) * 100 + s.count('Y'))
    v = gaussian(rng, 1 << n)
    (x,), (z,), (y,) = ao.gens_of(symp_of([s]))
    P = kron_of(s)
    assert np.array_equal(ao.apply_pauli(x, z, y, v), P @ v)
    assert np.array_equal(ao.dense_pauli(x, z, y, n), P)
    for theta in (0.0, 0.3, -2.1, np.pi / 4):
        want = expm(1j * theta * P) @ v
        got = ao.rotate(x, z, y, np.cos(theta), np.sin(theta), v)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(v).max() * 4
    assert np.array_equal(ao.rotate(x, z, y, 1.0, 0.0, v), v)


def test_all_strings_of_two_qubits():
    rng = np.random.default_rng(2)
    v = gaussian(rng, 4)
    for s in map(''.join, itertools.product('IXYZ', repeat=2)):
        (x,), (z,), (y,) = ao.gens_of(symp_of([s]))
        assert np.abs(ao.rotate(x, z, y, np.cos(0.7), np.sin(0.7), v) - expm(0.7j * kron_of(s)) @ v).max() <= 1e-14


def test_state_order_and_inverse():
    strings = ['XYZI', 'IZZY', 'YYXX', 'XYZI']
    rng = np.random.default_rng(3)
    theta, ref = rng.uniform(-np.pi, np.pi, 4), gaussian(rng, 16)
    want = ref
    for s, t in zip(strings, theta):                                   # rotation 0 first
        want = expm(1j * t * kron_of(s)) @ want
    got = ao.state(symp_of(strings), theta, ref)
    assert np.abs(got - want).max() <= 1e-13
    part = ao.state(symp_of(strings), theta, ref, 1, 3)
    assert np.abs(part - expm(1j * theta[2] * kron_of(strings[2])) @ expm(1j * theta[1] * kron_of(strings[1])) @ ref).max() <= 1e-13
    back = ao.state(symp_of(strings), theta, got, inverse=True)
    assert np.abs(back - ref).max() <= 1e-13


def test_energy_grad_shift_and_pool_grad():
    rng = np.random.default_rng(4)
    n = 4
    h_strings = ['ZIII', 'IZZI', 'XXYY', 'YXXY', 'IIIZ', 'XZXI', 'IIII']
    h_symp, h_coeff = symp_of(h_strings), rng.standard_normal(len(h_strings))
    Hd = sum(c * kron_of(s) for s, c in zip(h_strings, h_coeff))
    assert np.abs(ao.dense_operator(h_symp, h_coeff) - Hd).max() <= 1e-14
    gens = symp_of(['XYII', 'IXYI', 'YXXX', 'IIXY', 'ZZII'])
    theta, ref = rng.uniform(-np.pi, np.pi, 5), gaussian(rng, 16)
    ref /= np.linalg.norm(ref)
    psi = ao.state(gens, theta, ref)
    assert abs(ao.energy(h_symp, h_coeff, psi) - np.vdot(psi, Hd @ psi).real) <= 1e-13
    g = ao.grad_shift(h_symp, h_coeff, gens, theta, ref)
    eps = 1e-5
    for k in range(5):
        up, dn = theta.copy(), theta.copy()
        up[k] += eps
        dn[k] -= eps
        fd = (ao.energy_at(h_symp, h_coeff, gens, up, ref) - ao.energy_at(h_symp, h_coeff, gens, dn, ref)) / (2 * eps)
        assert abs(g[k] - fd) <= 1e-8
    # the pool gradient is the derivative of the energy in a NEW last parameter at 0
    pool = symp_of(['XYII', 'ZIII', 'YYYX', 'IXIY'])
    pg = ao.pool_grad(Hd, pool, psi)
    (x,), (z,), (y,) = ao.gens_of(pool[2:3])
    Pd = kron_of('YYYX')
    assert np.array_equal(ao.dense_pauli(x, z, y, 4), Pd) and abs(pg[2] - np.vdot(psi, 1j * (Hd @ Pd - Pd @ Hd) @ psi).real) <= 1e-13
    for j in range(4):
        grown = np.vstack([gens, pool[j:j + 1]])
        up, dn = np.append(theta, eps), np.append(theta, -eps)
        fd = (ao.energy_at(h_symp, h_coeff, grown, up, ref) - ao.energy_at(h_symp, h_coeff, grown, dn, ref)) / (2 * eps)
        assert abs(pg[j] - fd) <= 1e-8


def on_qubits(n, letters):
    return ''.join(letters.get(q, 'I') for q in range(n))


def test_run_planner_cut_rule():
    n = 14                                                              # index bit of qubit q: 13 - q; the low tile bits 0 .. 3 are qubits 10 .. 13
    bit = lambda *qs: sum(1 << (13 - q) for q in qs)
    low, pad10 = 0b1111, 0b1111111111                                  # a short run takes the lowest FREE bits until it has 10
    a, b = on_qubits(n, {0: 'X', 3: 'Y'}), on_qubits(n, {3: 'X', 5: 'X'})
    assert ao.plan_runs(symp_of([a])) == [(0, 1, bit(0, 3) | 0xFF, True)]
    assert ao.plan_runs(symp_of([a, b, 'Z' * n, a])) == [(0, 4, bit(0, 3, 5) | 0x7F, True)]          # x = 0 joins; a repeat adds nothing
    eight = on_qubits(n, {q: 'X' for q in range(8)})                    # 8 positions + 4 low bits: exactly the budget of 12
    assert ao.plan_runs(symp_of([eight])) == [(0, 1, low | bit(*range(8)), True)]
    assert ao.plan_runs(symp_of([eight, on_qubits(n, {11: 'Y'}), on_qubits(n, {8: 'X'}), eight])) == [
        (0, 2, low | bit(*range(8)), True), (2, 3, low | bit(8) | pad10, True), (3, 4, low | bit(*range(8)), True)]
    nine = on_qubits(n, {q: 'Y' for q in range(9)})                     # 13 bits with the low ones: a direct pass, adjacent ones merged
    assert ao.plan_runs(symp_of([a, nine, 'X' * n, b])) == [(0, 1, bit(0, 3) | 0xFF, True), (1, 3, 0, False), (3, 4, bit(3, 5) | 0xFF, True)]
    assert ao.plan_runs(symp_of([nine])) == [(0, 1, 0, False)]
    assert ao.plan_runs(symp_of(['Z' * n, 'I' * n])) == [(0, 2, pad10, True)]                               # only diagonal generators: the low bits
    assert ao.plan_runs(np.zeros((0, 2 * n), dtype=bool)) == []
    assert ao.plan_runs(symp_of(['XYZIXY', 'IIIIIZ'])) == [(0, 2, 0b111111, True)]                          # n = 6: the whole vector is one tile
    assert ao.plan_runs(symp_of(['X'])) == [(0, 1, 1, True)] and ao.plan_runs(symp_of(['XX' + 'I' * 30])) == [(0, 1, 3 << 30 | 0xFF, True)]


def test_bound_formula():
    assert ao.bound(10, 96, 156, [1.0, -2.0]) == (16 * 96 + 4 * 156 + 1024 + 64) * 2.0 ** -53 * 3.0
