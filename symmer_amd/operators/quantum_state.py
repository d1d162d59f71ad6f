"""``QuantumState`` — SURVEY.md §8f row f3 (reference ``symmer/operators/base.py:1564-2272``, the algebraic core only).

A sparse statevector is carried as a ``PauliwordOp`` (``|0> -> Z``, ``|1> -> X``, base.py:1564-1580), so applying an operator
to a state is the SAME device path as operator x operator: the fused all-pairs product + cleanup kernel, followed by the
``i^{Y}`` post-factor (base.py:854-857).  Expectation values reuse it (base.py:796-819, 2438-2471).
Sparse and dense vectors (``to_sparse_matrix``, ``to_dense_matrix``, base.py:1994-2023) are host code.  Reduced density matrices
(``partial_trace_over_qubits``, ``get_rdm``, base.py:2025-2054) are one device call on the dense amplitudes, ``rho = M M^+`` of
``csrc/rdm.hip`` (up to 32 qubits, up to 12 kept).  Measurement (``sample_state``, ``sample_counts``, ``normalize_counts``,
``measure_state_in_computational_basis``, ``change_of_basis_XY_to_Z``, base.py:1964-1975, 2070-2096, 2188-2212, 2474 ff.) draws on the
device from a sum tree over the weights (``csrc/sample.hip``) and changes basis in place on the dense amplitudes (``csrc/basis.hip``).
Not provided (plotting): outside the accelerated path.
"""
from copy import deepcopy
from functools import cached_property
from numbers import Number
from typing import Dict, List, Union
import warnings
import numpy as np


class QuantumState:
    sigfig = 3

    def __init__(self, state_matrix, coeff_vector=None, vec_type: str = 'ket') -> None:
        from .base import PauliwordOp
        if isinstance(state_matrix, list):
            state_matrix = np.array(state_matrix)
        if isinstance(coeff_vector, list):
            coeff_vector = np.array(coeff_vector)
        state_matrix = np.asarray(state_matrix)
        if len(state_matrix.shape) == 1:
            state_matrix = state_matrix.reshape([1, -1])
        state_matrix = state_matrix.astype(int)
        assert set(np.unique(state_matrix)).issubset({0, 1})
        self.n_terms, self.n_qubits = state_matrix.shape
        self.state_matrix = state_matrix
        if coeff_vector is None:
            coeff_vector = np.ones(self.n_terms) / np.sqrt(self.n_terms)
        self.vec_type = vec_type
        self.state_op = PauliwordOp(np.hstack([state_matrix, 1 - state_matrix]), coeff_vector)

    def copy(self) -> "QuantumState":
        return deepcopy(self)

    @classmethod
    def random(cls, num_qubits: int, num_terms: int, vec_type: str = 'ket') -> "QuantumState":
        random_state = np.random.randint(0, 2, (num_terms, num_qubits))
        coeff_vec = np.random.rand(num_terms) + np.random.rand(num_terms) * 1j
        return QuantumState(random_state, coeff_vec, vec_type=vec_type).cleanup().normalize

    @classmethod
    def zero(cls, n_qubits: int, vec_type: str = 'ket') -> "QuantumState":
        return QuantumState(np.zeros(n_qubits).reshape(1, -1), coeff_vector=np.array([1]), vec_type=vec_type)

    @classmethod
    def from_dictionary(cls, state_dict: Dict[str, complex]) -> "QuantumState":
        bits, coeffs = zip(*state_dict.items())
        coeffs = np.array([complex(*c) if isinstance(c, (tuple, list)) else c for c in coeffs])
        return cls(np.array([[int(i) for i in b] for b in bits]), coeffs)

    @classmethod
    def from_array(cls, statevector, threshold: float = 1e-15) -> "QuantumState":
        """base.py:2139-2186: the state of a dense vector of ``2^n`` amplitudes, host NumPy like ``to_sparse_matrix``, whose inverse it
        is.  A column ``(2^n, 1)`` makes a ket, a row ``(1, 2^n)`` a bra; amplitude ``b`` belongs to the basis string of ``b`` with qubit 0
        the most significant bit.  The amplitudes with ``|a| >= threshold`` are kept, in ascending index order; a vector that is not
        normalised only warns."""
        statevector = np.asarray(statevector)
        assert len(statevector.shape) == 2 and 1 in statevector.shape, 'state must be a bra (row) or ket (column) vector'
        vec_type = 'bra' if statevector.shape[0] == 1 else 'ket'
        statevector = statevector.reshape([-1])
        n = int(statevector.shape[0]).bit_length() - 1
        assert statevector.shape[0] == 1 << n, 'the statevector dimension is not a power of 2'
        if not np.isclose(np.linalg.norm(statevector), 1):
            warnings.warn('statevector is not normalized')
        non_zero = np.where(abs(statevector) >= threshold)[0]
        shifts = np.arange(n - 1, -1, -1, dtype=np.int64)
        state_matrix = ((non_zero[:, None] >> shifts) & 1).astype(int).reshape(non_zero.shape[0], n)
        return cls(state_matrix, statevector[non_zero], vec_type=vec_type)

    @cached_property
    def to_dictionary(self) -> Dict[str, complex]:
        s = self.cleanup()
        return dict(zip([''.join(str(i) for i in row) for row in s.state_matrix], s.state_op.coeff_vec))

    def __str__(self) -> str:
        out = ''
        for basis_vec, coeff in zip(self.state_matrix, self.state_op.coeff_vec):
            b = ''.join(str(i) for i in basis_vec)
            out += f'{coeff: .{self.sigfig}f} |{b}> +\n' if self.vec_type == 'ket' else f'{coeff: .{self.sigfig}f} <{b}| +\n'
        return out[:-3]

    __repr__ = __str__

    def __eq__(self, Qstate: "QuantumState") -> bool:
        return self.state_op == Qstate.state_op

    def __hash__(self):
        return hash(tuple(self.to_dictionary.items()))

    def __add__(self, Qstate: "QuantumState") -> "QuantumState":
        new_state = self.state_op + Qstate.state_op
        return QuantumState(new_state.X_block, new_state.coeff_vec)

    def __radd__(self, add_obj):
        if isinstance(add_obj, Number) and add_obj == 0:
            return self
        return self + add_obj

    def __sub__(self, Qstate: "QuantumState") -> "QuantumState":
        new_state_op = self.state_op - Qstate.state_op
        return QuantumState(new_state_op.X_block, new_state_op.coeff_vec)

    def __mul__(self, mul_obj):
        """bra * ket -> inner product; bra * PauliwordOp -> bra (base.py:1781-1830)."""
        from .base import PauliwordOp
        if isinstance(mul_obj, Number):
            return QuantumState(self.state_matrix, self.state_op.coeff_vec * mul_obj)
        assert self.n_qubits == mul_obj.n_qubits, 'Multiplication object defined for different number of qubits'
        assert self.vec_type == 'bra', 'Cannot multiply a ket from the right'
        if isinstance(mul_obj, QuantumState):
            assert mul_obj.vec_type == 'ket', 'Cannot multiply a bra with another bra'
            # base.py:1808-1815: the state with fewer terms is the left one; both are cleaned (to_dictionary, :2104), then the coefficients
            # of the basis strings they share are multiplied and added in the left state's order — here a hash join of the packed
            # basis rows on the device (csrc/project.hip), the products added in that same order
            left, right = (self, mul_obj) if self.state_op.n_terms < mul_obj.n_terms else (mul_obj, self)
            from .. import kernels
            cleaned = [kernels.cleanup_dev(s.state_op._device()) for s in (left, right)]
            try:
                return kernels.state_inner_dev(cleaned[0], cleaned[1])
            finally:
                for h in cleaned:
                    h.free()
        if isinstance(mul_obj, PauliwordOp):
            new_state_op = self.state_op * mul_obj
            coeff = new_state_op.coeff_vec * ((-1j) ** new_state_op.Y_count)
            return QuantumState(new_state_op.X_block, coeff, vec_type='bra').cleanup()
        raise ValueError('Trying to multiply QuantumState by unrecognised object - must be another Quantum state or PauliwordOp')

    def __getitem__(self, key) -> "QuantumState":
        if isinstance(key, (int, np.integer)):
            key = int(key)
            if key < 0:
                key += self.n_terms
            assert key < self.n_terms, 'Index out of range'
            mask = [key]
        elif isinstance(key, slice):
            mask = np.arange(0 if key.start is None else key.start, self.n_terms if key.stop is None else key.stop, key.step)
        else:
            mask = np.asarray(key)
        return QuantumState(self.state_matrix[mask], self.state_op.coeff_vec[mask])

    def __iter__(self):
        return iter([self[i] for i in range(self.n_terms)])

    def cleanup(self, zero_threshold=1e-15) -> "QuantumState":
        clean = self.state_op.cleanup(zero_threshold=zero_threshold)
        return QuantumState(clean.X_block, clean.coeff_vec, vec_type=self.vec_type)

    def sort(self, by='decreasing', key='magnitude') -> "QuantumState":
        if key == 'magnitude':
            order = np.argsort(-abs(self.state_op.coeff_vec))
        elif key == 'support':
            order = np.argsort(-np.sum(self.state_matrix, axis=1))
        else:
            raise ValueError('Only permitted sort key values are magnitude or support')
        if by == 'increasing':
            order = order[::-1]
        elif by != 'decreasing':
            raise ValueError('Only permitted sort by values are increasing or decreasing')
        return QuantumState(self.state_matrix[order], self.state_op.coeff_vec[order])

    @cached_property
    def normalize(self) -> "QuantumState":
        return QuantumState(self.state_matrix, self.state_op.coeff_vec / np.linalg.norm(self.state_op.coeff_vec), vec_type=self.vec_type)

    @cached_property
    def dagger(self) -> "QuantumState":
        return QuantumState(self.state_matrix, self.state_op.coeff_vec.conjugate(), vec_type='bra' if self.vec_type == 'ket' else 'ket')

    @cached_property
    def to_sparse_matrix(self):
        """base.py:1994-2014: the state as a ``scipy.sparse.csr_matrix`` (complex128) — a ket is a ``(2^n, 1)`` column, a bra a
        ``(1, 2^n)`` row (its coefficients are already conjugated).  Basis string ``s`` sits at index ``int(s, 2)`` (qubit 0 the most
        significant bit, as in ``PauliwordOp.to_sparse_matrix``); repeated basis strings are summed.  Cached, like the reference's."""
        from scipy.sparse import csr_matrix
        n = self.n_qubits
        weights = np.array([1 << (n - 1 - q) for q in range(n)], dtype=object if n >= 63 else np.int64)
        index = self.state_matrix @ weights if n else np.zeros(self.n_terms, dtype=np.int64)
        zeros = np.zeros_like(index)
        coeff = np.asarray(self.state_op.coeff_vec, dtype=np.complex128)
        shape = (1 << n, 1) if self.vec_type != 'bra' else (1, 1 << n)
        rc = (index, zeros) if self.vec_type != 'bra' else (zeros, index)
        return csr_matrix((coeff, rc), shape=shape, dtype=np.complex128)

    @cached_property
    def to_dense_matrix(self) -> np.ndarray:
        """base.py:2016-2023: ``to_sparse_matrix`` as a dense ndarray of the same shape."""
        return self.to_sparse_matrix.toarray()

    def _rdm_over(self, kept, what: str) -> np.ndarray:
        from .. import kernels
        n = self.n_qubits
        if not 1 <= n <= kernels.RDM_MAX_QUBITS:
            raise ValueError(f'{what}: {n} qubits; 1 .. {kernels.RDM_MAX_QUBITS} are supported (a dense vector of 2^n amplitudes)')
        if len(kept) > kernels.RDM_MAX_KEPT:
            raise ValueError(f'{what}: {len(kept)} qubits remain; at most {kernels.RDM_MAX_KEPT} are supported '
                             f'(a {1 << kernels.RDM_MAX_KEPT} x {1 << kernels.RDM_MAX_KEPT} matrix)')
        return kernels.rdm_dev(np.asarray(self.to_dense_matrix).reshape(-1), n, kept)

    def partial_trace_over_qubits(self, qubits: List[int] = []) -> np.ndarray:
        """base.py:2025-2039: the reduced density matrix of the qubits that remain when ``qubits`` are traced out, complex128
        ``[2^k, 2^k]`` with the remaining qubit of the lowest number as the most significant bit of the row and column index (the
        reference's ``tensordot`` of the ``[2] * n`` amplitudes with their conjugate over ``qubits``), computed on the device
        (``csrc/rdm.hip``).  The amplitudes are those of ``to_dense_matrix``: a bra gives the conjugate matrix, repeated basis strings add,
        nothing is normalised.  ValueError for a repeated or out-of-range entry of ``qubits``, beyond 32 qubits, or when more than 12
        qubits remain."""
        qubits = [int(q) for q in qubits]
        if len(set(qubits)) != len(qubits):
            raise ValueError(f'partial_trace_over_qubits: repeated qubit in {qubits}')
        if any(q < 0 or q >= self.n_qubits for q in qubits):
            raise ValueError(f'partial_trace_over_qubits: qubits {qubits} outside 0 .. {self.n_qubits - 1}')
        return self._rdm_over(sorted(set(range(self.n_qubits)) - set(qubits)), 'partial_trace_over_qubits')

    def get_rdm(self, qubits: List[int] = []) -> np.ndarray:
        """base.py:2041-2054: the reduced density matrix over ``qubits`` (the others are traced out); order and repeats in ``qubits`` are
        ignored, as the reference's set does.  See ``partial_trace_over_qubits``; ValueError for a qubit outside ``0 .. n-1``, beyond 32
        qubits, or for more than 12 kept qubits."""
        kept = sorted({int(q) for q in qubits})
        if any(q < 0 or q >= self.n_qubits for q in kept):
            raise ValueError(f'get_rdm: qubits {list(qubits)} outside 0 .. {self.n_qubits - 1}')
        return self._rdm_over(kept, 'get_rdm')

    def _is_normalized(self) -> bool:
        return bool(np.isclose(np.linalg.norm(self.state_op.cleanup().coeff_vec), 1))

    # ---- measurement (csrc/sample.hip, csrc/basis.hip) -------------------------------------------------------------------
    @cached_property
    def normalize_counts(self) -> "QuantumState":
        """base.py:1964-1975: coefficients ``sqrt(c / sum c)`` — the state a table of counts stands for."""
        coeff = self.state_op.coeff_vec
        return QuantumState(self.state_matrix, np.sqrt(coeff / np.sum(coeff)), vec_type=self.vec_type)

    @staticmethod
    def _seed_of(seed) -> int:
        """``seed`` itself, or one integer of NumPy's global generator (so that ``np.random.seed`` makes a run repeatable)."""
        return int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64)) if seed is None else int(seed)

    def sample_state(self, n_samples: int, return_normalized: bool = False, seed=None) -> "QuantumState":
        """base.py:2070-2096: ``n_samples`` measurements in the computational basis, as a state on the same ``state_matrix`` (same
        rows, same order, same ``vec_type``) whose coefficients are the counts — ``sqrt(count / n_samples)`` with
        ``return_normalized``; a row never drawn keeps a 0.  The terms are sampled as they stand (no cleanup) with weights ``|c_i|^2``:
        one sum tree over the T coefficients on the device and ``n_samples`` walks down it (``kernels.SamplePlan``), draw ``i`` from
        uniform ``i`` of the Philox4x64-10 stream of ``seed`` — the numbers of ``np.random.Generator(np.random.Philox(key=seed))``.
        ``seed=None`` takes one integer from NumPy's global generator.  ValueError for a state that is not normalised."""
        from .. import kernels
        if not self._is_normalized():
            raise ValueError('should not sample state that is not normalized')
        n_samples = int(n_samples)
        counter = np.zeros(self.n_terms, dtype=np.int64)
        with kernels.SamplePlan(np.asarray(self.state_op.coeff_vec, dtype=np.complex128)) as plan:
            idx, count = plan.draw(n_samples, self._seed_of(seed))
        counter[idx] = count
        coeff = np.sqrt(counter / n_samples) if return_normalized else counter
        return QuantumState(self.state_matrix, coeff, vec_type=self.vec_type)

    def sample_counts(self, n_samples: int, seed=None):
        """``n_samples`` measurements of the dense amplitudes (1 .. 32 qubits; repeated basis strings add, as in
        ``to_dense_matrix``): ``(indices, counts)``, the distinct basis indices ascending (qubit 0 the most significant bit) and their
        counts, both int64.  Nothing of size ``2^n`` exists on the host beyond the vector that is uploaded.  Seeds as in
        ``sample_state``; ValueError for a state that is not normalised."""
        from .. import kernels
        if not 1 <= self.n_qubits <= 32:
            raise ValueError(f'sample_counts: {self.n_qubits} qubits; 1 .. 32 are supported (a dense vector of 2^n amplitudes)')
        if not self._is_normalized():
            raise ValueError('should not sample state that is not normalized')
        with kernels.SamplePlan(np.asarray(self.to_dense_matrix).reshape(-1)) as plan:
            return plan.draw(int(n_samples), self._seed_of(seed))

    def measure_state_in_computational_basis(self, P_op):
        """base.py:2188-2212: ``(psi_new, Z_new)`` with ``<self|P_op|self> = <psi_new|Z_new|psi_new>``: ``psi_new = U |self>`` and
        ``Z_new = U P_op U^+`` for the layer ``U`` of ``change_of_basis_XY_to_Z(P_op)`` — H on the qubits where the FIRST row of
        ``P_op`` has X, H S^+ where it has Y.  Kets only.  The state goes through the device (``kernels.basis_change_dev`` on the dense
        amplitudes, 1 .. 32 qubits) and ``from_array``; ``U`` itself is never built for it.  When the layer diagonalises every term —
        each term qubitwise compatible with the first row and with no X or Y outside that row's — ``Z_new`` is written directly
        (``z' = z | x``, ``x' = 0``, coefficients unchanged: H X H = Z, H S^+ Y S H = Z); otherwise it is the reference's
        ``U * P_op * U.dagger`` on the product kernels."""
        from .. import kernels
        from .base import PauliwordOp
        assert self.vec_type == 'ket', 'cannot perform change of basis on bra'
        assert P_op.n_qubits == self.n_qubits, 'operator and state defined for different number of qubits'
        n = self.n_qubits
        if not 1 <= n <= 32:
            raise ValueError(f'measure_state_in_computational_basis: {n} qubits; 1 .. 32 are supported (a dense vector of 2^n amplitudes)')
        X, Z = np.asarray(P_op.X_block, dtype=bool), np.asarray(P_op.Z_block, dtype=bool)
        x0, z0 = X[0], Z[0]
        with kernels.DeviceBuffer.upload(np.asarray(self.to_dense_matrix, dtype=np.complex128).reshape(-1)) as psi:
            kernels.basis_change_dev(psi, n, np.flatnonzero(x0 & ~z0), np.flatnonzero(x0 & z0))
            psi_new = QuantumState.from_array(psi.download(np.complex128, 1 << n).reshape(-1, 1))
        if not np.any(X & ~x0) and not np.any(X & (Z ^ z0)) and not np.any(~X & Z & x0):
            Z_new = PauliwordOp(np.hstack([np.zeros_like(X), Z | X]), P_op.coeff_vec)
        else:
            U = change_of_basis_XY_to_Z(P_op)
            Z_new = U * P_op * U.dagger
        return psi_new, Z_new


# one qubit of the layer in the Pauli basis (I, X, Y, Z), from H = (X + Z) / sqrt 2 and S^+ = ((1 - i) I + (1 + i) Z) / 2
_LAYER_H = {'X': 1 / np.sqrt(2), 'Z': 1 / np.sqrt(2)}
_LAYER_HSDG = {p: c / (2 * np.sqrt(2)) for p, c in (('I', 1 + 1j), ('X', 1 - 1j), ('Y', 1 - 1j), ('Z', 1 - 1j))}
MAX_LAYER_QUBITS = 16


def change_of_basis_XY_to_Z(P_op):
    """base.py:2474 ff.: the operator ``U`` of H gates (where the first row of ``P_op`` has X) and H S^+ gates (where it has Y), with
    ``U * P * U.dagger`` equal to that row with Z in place of every X and Y.  Host construction, term by term: a qubit with X gives the
    two terms of ``(X + Z) / sqrt 2``, a qubit with Y the four of ``H S^+ = ((1 + i) I + (1 - i)(X + Y + Z)) / (2 sqrt 2)``, so ``U`` has
    ``2^#X 4^#Y`` terms, in lexicographic order of the choices.  ValueError beyond 16 such qubits: the operator would have at least
    65,536 terms and every product with it that many times the other operand's — ``measure_state_in_computational_basis`` applies the
    layer to the state on the device without it."""
    from .base import PauliwordOp
    x0, z0 = np.asarray(P_op.X_block, dtype=bool)[0], np.asarray(P_op.Z_block, dtype=bool)[0]
    measured = np.flatnonzero(x0)
    if measured.size > MAX_LAYER_QUBITS:
        raise ValueError(f'change_of_basis_XY_to_Z: {measured.size} qubits carry X or Y; beyond {MAX_LAYER_QUBITS} the operator has more '
                         f'than 2^{MAX_LAYER_QUBITS} terms (measure_state_in_computational_basis applies the layer without building it)')
    n = P_op.n_qubits
    symp, coeff = np.zeros((1, 2 * n), dtype=bool), np.ones(1, dtype=np.complex128)
    for q in measured:
        table = _LAYER_HSDG if z0[q] else _LAYER_H
        rows, cs = [], []
        for pauli, c in table.items():
            part = symp.copy()
            part[:, q], part[:, n + q] = pauli in 'XY', pauli in 'YZ'
            rows.append(part)
            cs.append(coeff * c)
        symp, coeff = np.vstack(rows), np.concatenate(cs)
    return PauliwordOp(symp, coeff)


def single_term_expval(P_op, psi: QuantumState) -> float:
    """base.py:2438-2471: <psi|P|psi> for ONE Pauli term (its coefficient is ignored) as the difference of the squared
    norms of the projections onto the +1 / -1 eigenspaces, each obtained with one operator x state product on the device."""
    from .base import PauliwordOp
    assert P_op.n_terms == 1, 'Supplied multiple Pauli terms.'
    proj = np.vstack([np.zeros(P_op.n_qubits * 2, dtype=bool), P_op.symp_matrix])
    norm_ev = lambda ev: np.linalg.norm((PauliwordOp(proj, [.5, .5 * ev]) * psi).state_op.coeff_vec)
    return (norm_ev(+1) ** 2 - norm_ev(-1) ** 2).real


def _expval_call(P_op, psi: QuantumState, want_terms: bool):
    """One device call for all terms of ``P_op`` (csrc/expval.hip): psi is cleaned on the device, as bra * ket cleans its operands."""
    from .. import kernels
    assert P_op.n_qubits == psi.n_qubits, 'operator and state defined for different number of qubits'
    cleaned = kernels.cleanup_dev(psi.state_op._device())
    try:
        return kernels.expval_terms_dev(P_op._device(), cleaned, cleaned, want_terms)
    finally:
        cleaned.free()


def term_expvals(P_op, psi: QuantumState) -> np.ndarray:
    """``single_term_expval`` of every term of ``P_op`` at once (the terms' coefficients are ignored), float64[n_terms]:
    <psi|P_k|psi> = Re i^Y sum_b conj(psi[b ^ x_k]) psi[b] (-1)^|z_k & b|, one table look-up per (term, basis state) instead of
    two operator x state products per term."""
    return _expval_call(P_op, psi, True)[0].real.copy()
