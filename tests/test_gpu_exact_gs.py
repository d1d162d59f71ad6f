"""GPU: exact_gs_energy (symmer_amd/utils.py) — Lanczos with full reorthogonalisation on a resident basis (csrc/lanczos.hip) over the
matrix-free product (csrc/matvec.hip) — and its device calls taken alone.  Expected energies come from np.linalg.eigh of the NumPy
oracle's matrix (tests/_sparse_oracle.py), or from the molecule fixture's FCI entry; residuals from the oracle's product
(tests/_matvec_oracle.py).  With R = 2 tol sum|c|: |H psi - E psi|_2 <= R (the iteration stops at tol sum|c|; the factor 2 covers the
rounding of the estimate, of order 2^-53 |H| m) and |E - E_expected| <= R (an eigenvalue of a Hermitian matrix lies within the residual
of E, and E_expected is the lowest of the sector)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse

import _matvec_oracle as mo
import _sparse_oracle as so
from symmer_amd import PauliwordOp, QuantumState, exact_gs_energy, kernels, packing
from symmer_amd._lib import SymgpuError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
TOL = 1e-10


class Molecule:
    def __init__(self, name):
        with open(os.path.join(GOLDEN, name)) as f:
            d = json.load(f)
        self.H = PauliwordOp.from_dictionary({k: complex(*v) for k, v in d['hamiltonian'].items()})
        self.n = self.H.n_qubits
        self.symp, self.coeff = self.H.symp_matrix.copy(), np.array(self.H.coeff_vec)
        self.R = 2 * TOL * np.abs(self.coeff).sum()
        self.fci = d['data']['calculated_properties']['FCI']['energy']
        self.n_particles = d['data']['n_particles']
        self.hf = d['data']['hf_array']
        self.weight = np.array([bin(b).count('1') for b in range(1 << self.n)])
        self.csr = scipy.sparse.csr_matrix(so.to_csr(self.symp, self.coeff), shape=(1 << self.n, 1 << self.n))
        self._lowest = {}

    def lowest(self, n_particles=None):
        """The lowest eigenvalue of the (sector of the) oracle's matrix, by a dense eigh, computed once."""
        if n_particles not in self._lowest:
            idx = np.arange(1 << self.n) if n_particles is None else np.flatnonzero(self.weight == n_particles)
            self._lowest[n_particles] = np.linalg.eigvalsh(self.csr[idx][:, idx].toarray())[0]
        return self._lowest[n_particles]

    def check(self, E, psi, expected, n_particles=None):
        assert isinstance(E, float) and psi.shape == (1 << self.n,) and psi.dtype == np.complex128
        # |psi| = 1 up to the rounding of a sum of 2^n squares in any order, the root and the division
        assert abs(np.linalg.norm(psi) - 1) <= ((1 << self.n) + 4) * 2.0 ** -53
        residual = np.linalg.norm(mo.matvec(self.symp, self.coeff, psi) - E * psi)
        print(f'E = {E!r}, expected {expected!r}, residual {residual:.3e}, R {self.R:.3e}')
        assert residual <= self.R
        assert abs(E - expected) <= self.R
        if n_particles is not None:
            assert np.all(self.weight[np.flatnonzero(psi)] == n_particles)


def number_operator(n):
    """sum_q (1 - Z_q) / 2 of the Jordan-Wigner encoding."""
    symp = np.zeros((n + 1, 2 * n), dtype=bool)
    symp[1:, n:] = np.eye(n, dtype=bool)
    return PauliwordOp(symp, [n / 2] + [-0.5] * n)


@pytest.fixture(scope='module')
def bplus():
    return Molecule('B+_STO-3G_SINGLET_JW.json')


@pytest.fixture(scope='module')
def bh():
    return Molecule('BH_STO-3G_SINGLET_JW.json')


# ---- the molecules -----------------------------------------------------------------------------------------------------------------
def test_bplus_without_a_sector(bplus):
    E, psi = exact_gs_energy(bplus.H, return_array=True)
    bplus.check(E, psi, bplus.lowest())                      # a 6-fold level: some unit vector of its eigenspace


def test_bplus_four_particles(bplus):
    N = number_operator(bplus.n)
    E, state = exact_gs_energy(bplus.H, n_particles=4, number_operator=N)
    assert isinstance(state, QuantumState) and state.vec_type == 'ket' and state.n_qubits == bplus.n
    assert np.all(state.state_matrix.sum(axis=1) == 4)       # every kept amplitude belongs to the sector
    assert np.array_equal(mo.diagonal(N.symp_matrix, N.coeff_vec).real[so.bits_to_int(state.state_matrix)], np.full(state.n_terms, 4.0))
    psi = state.to_dense_matrix.reshape(-1)
    bplus.check(E, psi, bplus.lowest(4), 4)
    assert abs(bplus.lowest(4) - bplus.fci) <= 1e-9
    assert bplus.lowest(4) - bplus.lowest() > 0.1            # not the global ground state: the reference's n_eigs = 6 search misses it


def test_bplus_restarts_with_a_basis_of_eight(bplus):
    E, psi = exact_gs_energy(bplus.H, n_particles=4, number_operator=number_operator(bplus.n), max_basis=8, return_array=True)
    bplus.check(E, psi, bplus.lowest(4), 4)


def test_bplus_same_bits_on_a_second_run(bplus):
    N = number_operator(bplus.n)
    runs = [exact_gs_energy(bplus.H, n_particles=4, number_operator=N, return_array=True) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1].view(np.uint64), runs[1][1].view(np.uint64))


def test_bplus_initial_guesses(bplus):
    N = number_operator(bplus.n)
    E, psi = exact_gs_energy(bplus.H, initial_guess=QuantumState(bplus.hf), n_particles=4, number_operator=N, return_array=True)
    bplus.check(E, psi, bplus.lowest(4), 4)
    rng = np.random.default_rng(5)
    guess = rng.standard_normal(1 << bplus.n)
    E, psi = exact_gs_energy(bplus.H, initial_guess=guess, n_particles=4, number_operator=N, return_array=True)
    bplus.check(E, psi, bplus.lowest(4), 4)
    E, psi = exact_gs_energy(bplus.H, initial_guess=guess.reshape(-1, 1) * 3j, return_array=True)
    bplus.check(E, psi, bplus.lowest())


def test_a_quantum_state_guess_is_left_as_it_was(bplus):
    """An unnormalised guess with weight inside and outside the sector: masked and normalised in a copy, not in the state's cached vector."""
    n = bplus.n
    outside = [1] * 6 + [0] * (n - 6)
    guess = QuantumState([bplus.hf, outside], [3.0, 4.0j])
    before = guess.to_dense_matrix.copy()
    E, psi = exact_gs_energy(bplus.H, initial_guess=guess, n_particles=4, number_operator=number_operator(n), return_array=True)
    bplus.check(E, psi, bplus.lowest(4), 4)
    assert np.array_equal(guess.to_dense_matrix, before) and np.linalg.norm(before) == 5.0
    assert np.array_equal(guess.state_op.coeff_vec, [3.0, 4.0j])


def test_bh_without_a_sector(bh):
    E, psi = exact_gs_energy(bh.H, return_array=True)
    bh.check(E, psi, bh.fci)                                 # the fixture's FCI entry: the global ground state has 6 particles


@pytest.mark.parametrize('n_particles', [5, 7])
def test_bh_sectors(bh, n_particles):
    E, psi = exact_gs_energy(bh.H, n_particles=n_particles, number_operator=number_operator(bh.n), return_array=True)
    bh.check(E, psi, bh.lowest(n_particles), n_particles)    # eigh of the 792 x 792 sector block


# ---- small spaces: the basis is capped by the dimension ----------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3])
def test_small_operators_against_eigh(n):
    rng = np.random.default_rng(30 + n)
    T = 3 * n + 2
    symp, c = rng.random((T, 2 * n)) < 0.5, rng.standard_normal(T)       # real coefficients: Hermitian
    E, psi = exact_gs_energy(PauliwordOp(symp, c), return_array=True)
    R = 2 * TOL * np.abs(c).sum()
    dense = so.kron_dense(symp, c)
    assert abs(E - np.linalg.eigvalsh(dense)[0]) <= R and np.linalg.norm(dense @ psi - E * psi) <= R
    assert abs(np.linalg.norm(psi) - 1) <= ((1 << n) + 4) * 2.0 ** -53
    # a sector of one state: the basis has one vector
    N = number_operator(n)
    Hd = PauliwordOp(np.hstack([np.zeros((T, n), dtype=bool), symp[:, n:]]), c)
    E, state = exact_gs_energy(Hd, n_particles=n, number_operator=N)
    assert state.n_terms == 1 and np.all(state.state_matrix == 1)
    assert abs(E - so.kron_dense(Hd.symp_matrix, c)[-1, -1].real) <= R


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(bplus, bh):
    H, n = bplus.H, bplus.n
    N = number_operator(n)
    with pytest.raises(TypeError, match='PauliwordOp itself'):
        exact_gs_energy(bplus.csr)
    with pytest.raises(TypeError):
        exact_gs_energy(bplus.csr.toarray()[:4, :4])
    with pytest.raises(ValueError, match='Hermitian'):
        exact_gs_energy(PauliwordOp.from_list(['XZ', 'YI'], [1, 2j]))
    with pytest.raises(AssertionError):
        exact_gs_energy(H, n_particles=4)
    with pytest.raises(AssertionError):
        exact_gs_energy(H, n_particles=4, number_operator=N + PauliwordOp.from_list(['X' + 'I' * (n - 1)], [1]))
    z0 = PauliwordOp.from_list(['Z' + 'I' * (n - 1)], [1])
    with pytest.raises(ValueError, match='commute'):
        exact_gs_energy(H, n_particles=1, number_operator=z0)
    with pytest.raises(ValueError, match='empty'):
        exact_gs_energy(H, n_particles=11, number_operator=N)
    with pytest.raises(ValueError):
        exact_gs_energy(H, initial_guess=np.ones(8))
    with pytest.raises(RuntimeError, match='residual'):
        exact_gs_energy(bh.H, max_basis=4, max_restarts=1)


# ---- the device calls taken alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [3, 7])
def test_sector_mask_and_lanczos_step_against_numpy(n):
    rng = np.random.default_rng(70 + n)
    side, cap = 1 << n, 3                                    # n = 3: the 2-particle sector has three states
    # a Hermitian operator that conserves the particle number: Z strings and pairs XX + YY
    T = 12
    symp = np.hstack([np.zeros((T, n), dtype=bool), rng.random((T, n)) < 0.5])
    c = rng.standard_normal(T)
    for q in range(n - 1):
        xx = np.zeros((2, 2 * n), dtype=bool)
        xx[:, [q, q + 1]] = True
        xx[1, [n + q, n + q + 1]] = True
        symp, c = np.vstack([symp, xx]), np.concatenate([c, [0.5 * (q + 1)] * 2])
    Nop = number_operator(n)
    weight = np.array([bin(b).count('1') for b in range(side)])
    u = 2.0 ** -53
    tol = 64 * u * (len(c) + side) * np.abs(c).sum()          # a-priori: the product's bound plus a sum of 2^n terms, per scalar
    with kernels.DeviceOp.upload(packing.pack_rows(symp), c.astype(complex)) as op, kernels.MatvecPlan(op, n) as plan, \
            kernels.DeviceOp.upload(packing.pack_rows(Nop.symp_matrix), np.asarray(Nop.coeff_vec, dtype=complex)) as nop, \
            kernels.MatvecPlan(nop, n) as plan_n, kernels.DeviceBuffer(side) as keep, kernels.DeviceBuffer(cap * side * 16) as basis:
        for particles in range(n + 2):
            kept = plan_n.sector_mask(particles, keep)
            mask = keep.download(np.uint8, side)
            assert np.array_equal(mask, (weight == particles).astype(np.uint8)) and kept == int(mask.sum())
        with pytest.raises(SymgpuError):
            plan.sector_mask(1, keep)                        # terms with an X: not a number operator
        particles = n // 2 + 1
        plan_n.sector_mask(particles, keep)
        for use_mask in (False, True):
            mask = (weight == particles) if use_mask else np.ones(side, dtype=bool)
            v0 = (rng.standard_normal(side) + 1j * rng.standard_normal(side)) * mask
            V = np.zeros((cap, side), dtype=complex)
            V[0] = v0 / np.linalg.norm(v0)
            basis.write(V[0])
            for j in range(cap):
                alpha, beta = plan.lanczos_step(keep if use_mask else None, basis, cap, j)
                w = mask * mo.matvec(symp, c, V[j])
                want_alpha = np.vdot(V[j], w).real
                for _ in range(2):
                    w = w - V[:j + 1].T @ (V[:j + 1].conj() @ w)
                want_beta = np.linalg.norm(w)
                assert abs(alpha - want_alpha) <= tol and abs(beta - want_beta) <= tol, (j, alpha, want_alpha, beta, want_beta)
                if j + 1 < cap:
                    V[j + 1] = w / want_beta
                    got = basis.download(np.complex128, (j + 2) * side).reshape(j + 2, side)
                    assert np.abs(got.conj() @ got.T - np.eye(j + 2)).max() <= 64 * u * (j + 1)
                    assert np.abs(got[j + 1] - V[j + 1]).max() <= tol / want_beta
                    if use_mask:
                        assert not got[j + 1][~mask].any()
            # the Ritz combination, into a buffer and into slot 0
            s = rng.standard_normal(cap)
            got = basis.download(np.complex128, cap * side).reshape(cap, side)
            with kernels.DeviceBuffer(side * 16) as out:
                kernels.vec_combine(basis, cap, n, s, out=out)
                assert np.abs(out.download(np.complex128, side) - s @ got).max() <= 8 * u * cap * np.abs(s).max()
            kernels.vec_combine(basis, cap, n, s, normalise=True)
            unit = basis.download(np.complex128, side)
            assert abs(np.linalg.norm(unit) - 1) <= (side + 4) * u
            assert np.abs(unit - s @ got / np.linalg.norm(s @ got)).max() <= (16 * cap + side) * u     # the sum, and the norm's own rounding
