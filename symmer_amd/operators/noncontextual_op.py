"""``NoncontextualOp`` / ``NoncontextualSolver`` — drop-in for the reference classes (``symmer/operators/noncontextual_op.py``): a
noncontextual Hamiltonian split into universally commuting symmetry generators G and pairwise anticommuting clique representatives C_i,
its reconstruction over G u {C_i}, and the classical objective

    E(nu) = sum_{k in S0} c_k s_k(nu)  -  sqrt( sum_i ( sum_{k in C_i} c_k s_k(nu) )^2 ),    s_k(nu) = prod_{j in G_indices[k]} nu_j

minimised over nu in {+1, -1}^g.  Every step of the construction is a call that already runs on the device (``is_noncontextual``,
``symmetry_generators``, ``generators``, ``generator_reconstruction``, ``jordan_generator_reconstruction``, ``clique_cover``); the signs
of the generator products are one ``symgpu_noncon_signs_dev`` call and the brute-force search over all 2^f assignments of the free
generators is one ``symgpu_noncon_search`` call (blocked Walsh-Hadamard transforms in LDS, ``csrc/noncon.hip``) where
the reference evaluates ``get_energy`` once per assignment in a process pool.

Out of scope: ``AntiCommutingOp`` and ``unitary_partitioning`` do not exist here, so ``clique_operator`` is a plain ``PauliwordOp``
whose coefficients after ``solve`` are the clique sums s_i themselves (the reference normalises them and keeps ``mapped_clique_rep``,
``unitary_partitioning_rotations`` and ``clique_normalization``), and ``noncon_state`` raises ``NotImplementedError``.  Also not built:
``draw_graph_structure``, ``random``, and the ``stabilizers`` strategy of ``from_hamiltonian``.

The sweeping constructors — ``_single_sweep_noncontextual_operator``, ``_dfs_noncontextual_op``, ``_diag_first_noncontextual_op`` — are
built on one device call per constructor (``symgpu_noncon_sweep_dev``, ``csrc/noncon_sweep.hip``, DESIGN.md §3.20: one commutation table,
one workgroup per sweep, all rolls of the DFS form in one launch); their public door is ``NoncontextualOp.from_sweep``, which parses
``SingleSweep_*``, ``DFS_*`` and ``diag_first``.  ``from_hamiltonian`` itself still refuses ``DFS_*`` and ``SingleSweep_*``.
"""
import warnings
from typing import Tuple
import numpy as np
from .. import kernels
from .base import PauliwordOp
from .independent_op import IndependentOp


class NoncontextualOp(PauliwordOp):
    """A noncontextual Hamiltonian: its terms are reconstructed under the Jordan product from G u {C_1, ..., C_M} where {C_i, C_j} = 0
    and G commutes with everything (https://arxiv.org/abs/1904.02260).  Attributes as in the reference: ``symmetry_generators``
    (``IndependentOp``), ``clique_operator``, ``decomposed``, ``n_cliques``, ``G_indices``, ``C_indices``, ``mask_S0``, ``mask_Ci``,
    ``pauli_mult_signs``, and ``energy`` after ``solve``.  See the module docstring for what is out of scope."""
    up_method = 'seq_rot'

    def __init__(self, symp_matrix, coeff_vec):
        super().__init__(symp_matrix, coeff_vec)
        assert self.is_noncontextual, 'Specified operator is contextual.'
        self.noncontextual_generators()
        self.noncontextual_reconstruction()

    # ---- constructors ------------------------------------------------------------------------------------
    @classmethod
    def from_PauliwordOp(cls, H: PauliwordOp) -> "NoncontextualOp":
        return cls(H.symp_matrix, H.coeff_vec)

    @classmethod
    def from_hamiltonian(cls, H: PauliwordOp, strategy: str = 'diag', generators: PauliwordOp = None, stabilizers: IndependentOp = None,
                         DFS_runtime: int = 10, use_jordan_product=False, override_noncontextuality_check: bool = True
                         ) -> "NoncontextualOp":
        """noncontextual_op.py:63-106 with the strategies ``'diag'`` and ``'generators'``; the others raise ``NotImplementedError``."""
        if not override_noncontextuality_check:
            if H.is_noncontextual:
                warnings.warn('input H is already noncontextual ignoring strategy')
                return cls.from_PauliwordOp(H)
        if strategy == 'diag':
            return cls._diag_noncontextual_op(H)
        if strategy == 'generators':
            return cls._from_generators_noncontextual_op(H, generators, use_jordan_product=use_jordan_product)
        if strategy == 'stabilizers' or strategy.find('DFS') != -1 or strategy.find('SingleSweep') != -1:
            raise NotImplementedError(f'noncontextual operator strategy {strategy} is not built here: use diag or generators')
        raise ValueError(f'Unrecognised noncontextual operator strategy {strategy}')

    @classmethod
    def _diag_noncontextual_op(cls, H: PauliwordOp) -> "NoncontextualOp":
        """noncontextual_op.py:108-124: the diagonal terms, the simplest noncontextual operator."""
        mask_diag = np.where(~np.any(H.X_block, axis=1))
        return cls(H.symp_matrix[mask_diag], H.coeff_vec[mask_diag])

    # ---- constructors by sweeping (csrc/noncon_sweep.hip) ------------------------------------------------
    @classmethod
    def from_sweep(cls, H: PauliwordOp, strategy: str = 'SingleSweep_magnitude', max_rolls: int = None) -> "NoncontextualOp":
        """The sweeping strategies of the reference's ``from_hamiltonian`` (noncontextual_op.py:99-104) and its ``_diag_first``
        constructor: ``'SingleSweep_magnitude' | 'SingleSweep_random' | 'SingleSweep_CurrentOrder'``, ``'DFS_magnitude' | 'DFS_largest'``
        (``max_rolls``: the first rolls only) and ``'diag_first'``."""
        if strategy == 'diag_first':
            return cls._diag_first_noncontextual_op(H)
        if strategy.find('DFS') != -1:
            _, strategy = strategy.split('_')
            return cls._dfs_noncontextual_op(H, strategy=strategy, max_rolls=max_rolls)
        if strategy.find('SingleSweep') != -1:
            _, strategy = strategy.split('_')
            return cls._single_sweep_noncontextual_operator(H, strategy=strategy)
        raise ValueError(f'Unrecognised noncontextual operator strategy {strategy}')

    @classmethod
    def _swept(cls, H: PauliwordOp, order: np.ndarray, starts=None) -> np.ndarray:
        """bool[n_starts, T]: the positions of ``order`` that the sweeps from ``starts`` keep, all sweeps in one device call."""
        if H.n_terms == 0:
            return np.zeros((1 if starts is None else len(starts), 0), dtype=bool)
        return kernels.noncon_sweep(H._device(rows_only=True), order=order, starts=starts)

    @classmethod
    def _single_sweep_noncontextual_operator(cls, H: PauliwordOp, strategy: str = 'magnitude') -> "NoncontextualOp":
        """noncontextual_op.py:193-226: order the terms by ``'magnitude'``, at ``'random'`` (``np.random.shuffle`` on the host, as the
        reference: seeding ``np.random`` reproduces its order) or leave them in their ``'CurrentOrder'``, and sweep once."""
        if strategy == 'magnitude':
            order = PauliwordOp._ORDERINGS['magnitude'](H)
        elif strategy == 'random':
            order = np.arange(H.n_terms)
            np.random.shuffle(order)
        elif strategy == 'CurrentOrder':
            order = np.arange(H.n_terms)
        else:
            raise ValueError('Unrecognised strategy, must be one of magnitude, random or CurrentOrder')
        kept = cls._swept(H, order)[0]
        return cls.from_PauliwordOp(H[order[np.flatnonzero(kept)]])

    @classmethod
    def _dfs_noncontextual_op(cls, H: PauliwordOp, runtime=10, strategy: str = 'magnitude', max_rolls: int = None) -> "NoncontextualOp":
        """noncontextual_op.py:126-169: one sweep per cyclic roll of the magnitude order, the best one kept — by the sum of the kept
        magnitudes (``'magnitude'``) or by the number of kept terms (``'largest'``); the first roll among equal scores wins, as in the
        reference's stable sort.  Every roll 0 .. T-1 runs, all of them in ONE device call on one commutation table; ``max_rolls`` runs
        the first ``max_rolls`` rolls only.  ``runtime`` is unused: the reference stops after that many seconds of wall clock, which
        is not reproducible, and the whole pass is affordable here."""
        if strategy not in ('magnitude', 'largest'):
            raise ValueError('Unrecognised noncontextual operator strategy.')
        T = H.n_terms
        order = PauliwordOp._ORDERINGS['magnitude'](H)
        if T == 0:
            return cls.from_PauliwordOp(H)
        if max_rolls is not None and max_rolls < 1:
            raise ValueError('max_rolls must be at least 1')
        n_rolls = T if max_rolls is None else min(int(max_rolls), T)
        kept = cls._swept(H, order, starts=np.arange(n_rolls))
        magnitudes = abs(H._c()[order])
        best, best_score, best_visit = -1, None, None
        for n in range(n_rolls):
            visit = np.roll(np.arange(T), -n)
            visit = visit[kept[n, visit]]                               # the kept positions in the order this roll visited them
            score = -np.sum(magnitudes[visit]) if strategy == 'magnitude' else -len(visit)
            if best < 0 or score < best_score:
                best, best_score, best_visit = n, score, visit
        return cls.from_PauliwordOp(H[order[best_visit]])

    @classmethod
    def _diag_first_noncontextual_op(cls, H: PauliwordOp) -> "NoncontextualOp":
        """noncontextual_op.py:171-191: the diagonal terms (they commute with each other: all are kept), then the off-diagonal terms by
        decreasing magnitude, each kept if the operator stays noncontextual — one sweep over that order."""
        diagonal = ~np.any(H.X_block, axis=1)
        off = np.flatnonzero(~diagonal)
        order = np.concatenate([np.flatnonzero(diagonal), off[np.argsort(-abs(H._c()[off]))]]).astype(np.int64)
        kept = cls._swept(H, order)[0]
        return cls.from_PauliwordOp(H[order[np.flatnonzero(kept)]])

    @classmethod
    def _from_generators_noncontextual_op(cls, H: PauliwordOp, generators: PauliwordOp, use_jordan_product: bool = False
                                          ) -> "NoncontextualOp":
        """noncontextual_op.py:228-251: the terms of H that a noncontextual generating set reconstructs."""
        assert generators is not None, 'Must specify a noncontextual generating set.'
        assert generators.is_noncontextual, 'Generating set is contextual.'
        if use_jordan_product:
            _, noncontextual_terms_mask = H.jordan_generator_reconstruction(generators)
        else:
            _, noncontextual_terms_mask = H.generator_reconstruction(generators, override_independence_check=True)
        return cls.from_PauliwordOp(H[noncontextual_terms_mask])

    # ---- G and C(r) --------------------------------------------------------------------------------------
    def noncontextual_generators(self) -> None:
        """noncontextual_op.py:418-500, line by line: an independent generating set G u {C_i} of the operator."""
        # get Z2 symmetries (may anticommute among themselves)
        Z2_general = IndependentOp.symmetry_generators(self, commuting_override=True)
        _, Z2_mask = self.generator_reconstruction(Z2_general)
        Z2_symmerties = self[Z2_mask].generators

        if not np.all(Z2_symmerties.commutes_termwise(Z2_symmerties)):
            # need to account for Z2_symmerties not commuting with themselves
            sym_gens = self.generators
            z2_mask = np.sum(sym_gens.commutes_termwise(sym_gens), axis=1) == sym_gens.n_terms
            Z2_incomplete = sym_gens[z2_mask]
            _, missing_mask = sym_gens.generator_reconstruction(Z2_incomplete)
            Z2_missing = sym_gens[~missing_mask]
            cover = Z2_missing.clique_cover('C')
            clique_rep_list = [C.sort()[0] for C in cover.values()]
            sym_from_cliques = sum((cover[n] - C_rep) * C_rep for n, C_rep in enumerate(clique_rep_list) if cover[n].n_terms > 1)
            Z2_symmerties = (sym_from_cliques + Z2_incomplete).generators
            _, z2_mask = self.generator_reconstruction(Z2_symmerties)
        else:
            _, z2_mask = self.generator_reconstruction(Z2_symmerties)

        remaining = self[~z2_mask]
        if remaining.n_terms > 0:
            # remaining is a disjoint union of commuting cliques: the unique rows of its adjacency matrix ARE the cliques
            adjacency = remaining.adjacency_matrix
            adj_matrix_view = np.ascontiguousarray(adjacency).view(np.dtype((np.void, adjacency.dtype.itemsize * adjacency.shape[1])))
            re_order_indices = np.argsort(adj_matrix_view.ravel())
            sorted_terms = adjacency[re_order_indices]
            diff_adjacent = np.diff(sorted_terms, axis=0)
            mask_unique_terms = np.append(True, np.any(diff_adjacent, axis=1))
            clique_mask = sorted_terms[mask_unique_terms]
            self.decomposed = {ind: remaining[c_mask] for ind, c_mask in enumerate(clique_mask)}
            self.n_cliques = len(self.decomposed)
            if self.n_cliques > 0:
                # clique representatives with the greatest coefficient (equation 3 of https://arxiv.org/pdf/2002.05693.pdf)
                clique_rep_list = [C.sort()[0] for C in self.decomposed.values()]
                representatives = sum(clique_rep_list)
                self.clique_operator = PauliwordOp(representatives.symp_matrix, np.ones(representatives.n_terms, dtype=complex))
                # cliques can form new Z2 symmetries
                sym_from_cliques = sum((self.decomposed[n] - C_rep) * C_rep for n, C_rep in enumerate(clique_rep_list)
                                       if self.decomposed[n].n_terms > 1)
                if sym_from_cliques:
                    Z2_symmerties = (sym_from_cliques + Z2_symmerties).generators
        else:
            self.clique_operator = PauliwordOp(np.zeros((0, 2 * self.n_qubits), dtype=bool), [])      # no rows, as the reference's cleaned empty()
            self.decomposed = dict()
            self.n_cliques = 0

        self.symmetry_generators = IndependentOp.from_PauliwordOp(Z2_symmerties)
        _, Z2_mask = self.generator_reconstruction(Z2_symmerties)
        self.decomposed['symmetry'] = self[Z2_mask]

    def noncontextual_reconstruction(self) -> None:
        """noncontextual_op.py:502-531: every term over G u {C_i} under the Jordan product (anticommuting elements never meet in one
        term), and the sign its generator product carries — all terms in one device call where the reference multiplies term by term."""
        n_sym = self.symmetry_generators.n_terms
        noncon_generators = PauliwordOp(np.vstack([self.symmetry_generators.symp_matrix, self.clique_operator.symp_matrix]),
                                        np.ones(n_sym + self.n_cliques))
        if noncon_generators.n_terms == 0:
            jordan_recon_matrix, successful = np.zeros((self.n_terms, 0), dtype=int), ~np.any(self.symp_matrix, axis=1)
        else:
            jordan_recon_matrix, successful = self.jordan_generator_reconstruction(noncon_generators)
        assert np.all(successful), 'The generating set is not sufficient to reconstruct the noncontextual Hamiltonian'
        self.G_indices = jordan_recon_matrix[:, :n_sym]
        self.C_indices = jordan_recon_matrix[:, n_sym:]
        assert np.all(np.count_nonzero(self.C_indices, axis=1) <= 1), 'A term was reconstructed with more than one clique representative'
        self.mask_S0 = ~np.any(self.C_indices, axis=1)
        self.mask_Ci = self.C_indices.astype(bool).T
        # elements of C commute with all of G: a product over G with one element of C never carries a complex phase, but it may carry a sign
        if noncon_generators.n_terms == 0 or self.n_terms == 0:
            signs = np.ones(self.n_terms, dtype=np.int8)
        else:
            signs = kernels.noncon_signs_dev(self._device(rows_only=True), noncon_generators._device(rows_only=True),
                                             jordan_recon_matrix.astype(bool))
        assert np.all(signs != 0), 'The product of the reconstructing generators is not the term up to a sign'
        self.pauli_mult_signs = signs.astype(int)

    # ---- the classical objective (host, one assignment) ------------------------------------------------------
    def get_symmetry_contributions(self, nu: np.array) -> Tuple[float, np.array]:
        """noncontextual_op.py:533-547: (s0, s_i) of one assignment."""
        nu = np.asarray(nu)
        coeff_mod = (self._c() * self.pauli_mult_signs *
                     (-1) ** np.count_nonzero(np.logical_and(self.G_indices == 1, nu == -1), axis=1))
        s0 = np.sum(coeff_mod[self.mask_S0]).real
        si = np.array([np.sum(coeff_mod[mask]).real for mask in self.mask_Ci])
        return s0, si

    def get_energy(self, nu: np.array, AC_ev: int = -1) -> float:
        """noncontextual_op.py:549-554."""
        s0, si = self.get_symmetry_contributions(nu)
        return s0 + AC_ev * np.linalg.norm(si, ord=2)

    def update_clique_representative_operator(self, clique_index: int = None) -> None:
        """noncontextual_op.py:556-566 without the unitary partitioning: the clique sums of the current assignment become the
        coefficients of ``clique_operator``."""
        _, si = self.get_symmetry_contributions(self.symmetry_generators.coeff_vec)
        self.clique_operator.coeff_vec = si

    def solve(self, strategy: str = 'brute_force', ref_state: np.array = None) -> None:
        """noncontextual_op.py:568-603: minimise the objective; afterwards ``energy``, ``symmetry_generators.coeff_vec`` (nu) and
        ``clique_operator.coeff_vec`` (s_i) hold the optimum.  ``ref_state`` fixes the generators it determines
        (``IndependentOp.update_sector``); the rest are searched."""
        if ref_state is not None:
            self.symmetry_generators.update_sector(ref_state)
            ev_assignment = self.symmetry_generators.coeff_vec
            fixed_ev_mask = ev_assignment != 0
            fixed_eigvals = (ev_assignment[fixed_ev_mask]).astype(int)
            NC_solver = NoncontextualSolver(self, fixed_ev_mask, fixed_eigvals)
        else:
            NC_solver = NoncontextualSolver(self)

        if strategy == 'brute_force':
            self.energy, nu = NC_solver.energy_via_brute_force()
        elif strategy == 'binary_relaxation':
            self.energy, nu = NC_solver.energy_via_relaxation()
        else:
            raise ValueError(f'Unknown optimization strategy: {strategy}')

        self.symmetry_generators.coeff_vec = nu.astype(int)
        if self.n_cliques > 0:
            self.update_clique_representative_operator()

    def noncon_state(self, UP_method='LCU'):
        """noncontextual_op.py:605-654 rotates the clique operator onto one term first (``AntiCommutingOp.unitary_partitioning``)."""
        raise NotImplementedError('noncon_state needs AntiCommutingOp.unitary_partitioning, which is not built here')


class NoncontextualSolver:
    """noncontextual_op.py:660-730: the minimisation over the symmetry generators that ``fixed_ev_mask`` leaves free."""
    method: str = 'brute_force'
    _nu = None

    def __init__(self, NC_op: NoncontextualOp, fixed_ev_mask: np.array = None, fixed_eigvals: np.array = None) -> None:
        self.NC_op = NC_op
        if fixed_ev_mask is not None:
            assert fixed_eigvals is not None, 'Must specify the fixed eigenvalues'
            assert np.sum(fixed_ev_mask) == len(fixed_eigvals), 'Number of non-zero elements in mask does not match the number of fixed eigenvalues'
            self.fixed_ev_mask = np.asarray(fixed_ev_mask, dtype=bool)
            self.fixed_eigvals = np.asarray(fixed_eigvals)
        else:
            self.fixed_ev_mask = np.zeros(NC_op.symmetry_generators.n_terms, dtype=bool)
            self.fixed_eigvals = np.array([], dtype=int)

    def search_inputs(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """What the device search reads: c_k = Re(h_k) * pauli_mult_signs[k] with the fixed -1 generators folded into its sign, the
        term's generators among the FREE ones as a bit mask (bit b <=> free generator f-1-b in generator order), its clique number
        (-1 outside the cliques), and the indices of the free generators."""
        op = self.NC_op
        G = np.asarray(op.G_indices).astype(bool).reshape(op.n_terms, -1)
        nu_fixed = np.ones(G.shape[1], dtype=int)
        nu_fixed[self.fixed_ev_mask] = self.fixed_eigvals
        coeff = op._c().real * op.pauli_mult_signs * (1 - 2 * (np.count_nonzero(G[:, nu_fixed == -1], axis=1) & 1))
        free = np.flatnonzero(~self.fixed_ev_mask)
        masks = np.zeros(op.n_terms, dtype=np.uint64)
        for j, column in enumerate(free):
            masks |= G[:, column].astype(np.uint64) << np.uint64(free.size - 1 - j)
        C = np.asarray(op.C_indices).astype(bool).reshape(op.n_terms, -1)
        clique = np.full(op.n_terms, -1, dtype=np.int32)
        term, number = np.nonzero(C)
        clique[term] = number
        return coeff.astype(np.float64), masks, clique, free

    def energy_via_brute_force(self) -> Tuple[float, np.array]:
        """noncontextual_op.py:686-704: every assignment of the free generators, all of them in one device call.  Among assignments of
        equal energy the one the reference's ``min`` over ``itertools.product([-1, 1], ...)`` meets first wins."""
        n_free = int(np.sum(~self.fixed_ev_mask))
        if n_free > kernels.NONCON_MAX_FREE:
            raise ValueError(f'{n_free} free symmetry generators: the brute-force search takes at most {kernels.NONCON_MAX_FREE} '
                             f'(fix some with a reference state, or use binary_relaxation)')
        coeff, masks, clique, free = self.search_inputs()
        energy, best = kernels.noncon_search(coeff, masks, clique, n_free, self.NC_op.n_cliques)
        nu = np.ones(self.NC_op.symmetry_generators.n_terms, dtype=int)
        nu[self.fixed_ev_mask] = self.fixed_eigvals
        nu[free] = [-1 if (best >> (n_free - 1 - j)) & 1 else 1 for j in range(n_free)]
        return energy, nu

    def energy_via_relaxation(self) -> Tuple[float, np.array]:
        """noncontextual_op.py:710-730, unchanged: the binary assignment relaxed to angles, ``scipy.optimize.shgo`` over ``get_energy``."""
        from scipy.optimize import shgo
        nu_bounds = [(0, np.pi)] * (self.NC_op.symmetry_generators.n_terms - np.sum(self.fixed_ev_mask))

        def get_nu(angles):
            nu = np.ones(self.NC_op.symmetry_generators.n_terms)
            nu[self.fixed_ev_mask] = self.fixed_eigvals
            nu[~self.fixed_ev_mask] = np.cos(angles)
            return nu

        optimizer_output = shgo(func=lambda angles: self.NC_op.get_energy(get_nu(angles)), bounds=nu_bounds)
        # if the optimisation was successful the optimal angles consist of 0 and pi
        fix_nu = np.sign(np.array(get_nu(np.cos(optimizer_output['x'])))).astype(int)
        self.NC_op.symmetry_generators.coeff_vec = fix_nu
        return optimizer_output['fun'], fix_nu
