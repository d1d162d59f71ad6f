"""variational_optimization.py (reference: symmer/evolution/variational_optimization.py) — ``VQE_Driver`` and ``ADAPT_VQE`` on
device-resident statevectors (``csrc/ansatz.hip``).

The state is ``|psi(x)> = prod_k exp(i x_k P_k) |ref>``, rotation 0 applied first — what the reference's circuit builder prepares with
``rz(-2 x_k)``.  There are no circuits here: the reference state is uploaded once as ``2^n`` amplitudes, ``f`` is one state preparation
and one matrix-free ``H v``, ``gradient`` one more reverse sweep over two vectors (for a Pauli generator it equals the reference's
parameter shift ``f(x + pi/4 e_k) - f(x - pi/4 e_k)``), and the ADAPT pool gradient ``<psi| i [H, P_j] |psi>`` of every pool element is
one ``H v`` and one batched reduction.
"""
from typing import List

import numpy as np

from .. import kernels
from ..operators import PauliwordOp, QuantumState
from ..operators.utils import symplectic_to_string

_EVALS = ('statevector', 'observable_rotation')


def serialize_opt_data(opt_data) -> dict:
    """The fields of a ``scipy.optimize.OptimizeResult`` the reference keeps, as plain Python containers."""
    out = {key: getattr(opt_data, key) for key in ('message', 'success', 'status', 'fun')}
    out.update({key: tuple(getattr(opt_data, key)) for key in ('x', 'jac')})
    out.update({key: getattr(opt_data, key) for key in ('nit', 'nfev', 'njev')})
    return out


def _state_to_dict(psi: QuantumState) -> dict:
    return {bits: (c.real, c.imag) for bits, c in psi.to_dictionary.items()}


class VQE_Driver:
    """``expectation_eval`` is one of

    - ``'statevector'`` (default): state, energy and gradient on the device (``kernels.AnsatzPlan``);
    - ``'observable_rotation'``: the rotations applied to the observable instead, ``<ref| R(H) |ref>``, gradient by parameter shift —
      a second route through calls that do not touch the statevector kernels.

    The reference's ``symbolic_direct``, ``symbolic_projector``, ``sparse_array`` and ``dense_array`` need its circuits and raise
    ``NotImplementedError``."""
    expectation_eval = 'statevector'
    verbose = True

    def __init__(self, observable: PauliwordOp, ansatz_circuit=None, excitation_ops: PauliwordOp = None, ref_state=None) -> None:
        if ansatz_circuit is not None:
            raise NotImplementedError('VQE_Driver: there are no circuits here; pass excitation_ops (the generators of the ansatz)')
        assert np.all(np.asarray(observable.coeff_vec).imag == 0), 'Observable not Hermitian'
        self.observable = observable
        self.ref_state = ref_state
        self.circuit = None
        self._ref_dev = self._plan_H = self._ansatz = None
        self.excitation_generators = None
        if excitation_ops is not None:
            self.prepare_for_evolution(excitation_ops)

    # ---- device state -------------------------------------------------------------------------------------------------------------
    def _check_eval(self) -> str:
        if self.expectation_eval not in _EVALS:
            known = ('symbolic_direct', 'symbolic_projector', 'sparse_array', 'dense_array')
            kind = NotImplementedError if self.expectation_eval in known else ValueError
            raise kind(f'expectation_eval = {self.expectation_eval!r}: \'statevector\' and \'observable_rotation\' are the two routes here')
        return self.expectation_eval

    def _ref_amplitudes(self) -> np.ndarray:
        side = 1 << self.observable.n_qubits
        if isinstance(self.ref_state, QuantumState):
            assert self.ref_state.n_qubits == self.observable.n_qubits, 'reference state and observable differ in qubit count'
            return np.asarray(self.ref_state.to_dense_matrix, dtype=np.complex128).reshape(-1)
        amp = np.asarray(self.ref_state, dtype=np.complex128).reshape(-1)
        if amp.shape[0] != side:
            raise ValueError(f'ref_state: {amp.shape[0]} amplitudes for {self.observable.n_qubits} qubits; {side} wanted')
        return amp

    def _ref_quantum_state(self) -> QuantumState:
        if isinstance(self.ref_state, QuantumState):
            return self.ref_state
        return QuantumState.from_array(self._ref_amplitudes().reshape(-1, 1))

    def _device_ready(self) -> None:
        """The reference state (uploaded once) and H's grouped terms, resident from the first evaluation on."""
        if self._ref_dev is None:
            assert self.ref_state is not None, 'no reference state'
            self._ref_dev = kernels.DeviceBuffer.upload(self._ref_amplitudes())
        if self._plan_H is None:
            self._plan_H = self.observable._matvec_plan()
        if self._ansatz is None:
            assert self.excitation_generators is not None, 'no excitation generators: call prepare_for_evolution first'
            self._ansatz = self._plan_of(self.excitation_generators)

    @staticmethod
    def _plan_of(generators: PauliwordOp) -> "kernels.AnsatzPlan":
        if generators.n_terms == 0:
            with kernels.DeviceOp.alloc(1, 1, True) as none:
                none.set_rows(0)
                return kernels.AnsatzPlan(none, generators.n_qubits)
        return kernels.AnsatzPlan(generators._device(), generators.n_qubits)

    def prepare_for_evolution(self, excitation_ops: PauliwordOp) -> None:
        """Keeps the generators (unit coefficients, their order and repeats kept, identity rows dropped as the reference's circuit
        builder drops them); their device plan is built at the first evaluation."""
        symp = np.asarray(excitation_ops.symp_matrix, dtype=bool).reshape(excitation_ops.n_terms, -1)
        symp = symp[np.any(symp, axis=1)]
        self.excitation_generators = PauliwordOp(symp, np.ones(symp.shape[0]))
        if self._ansatz is not None:
            self._ansatz.free()
            self._ansatz = None

    @property
    def n_parameters(self) -> int:
        return self.excitation_generators.n_terms

    def _angles(self, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        assert x.shape[0] == self.n_parameters, f'{x.shape[0]} parameters for {self.n_parameters} generators'
        return x

    # ---- the reference's interface ------------------------------------------------------------------------------------------------
    def get_state(self, generators: PauliwordOp, x, as_array: bool = False):
        """``prod_k exp(i x_k P_k) |ref>`` over the rows of ``generators`` (identity rows included: global phases), prepared on the
        device: a ``QuantumState``, or with ``as_array`` the ``2^n`` amplitudes.  Under ``'observable_rotation'`` the rotations
        ``(P_k, -2 x_k)`` instead, LAST generator first: ``perform_rotations`` conjugates the observable by its list in order, so the
        rotation that acts on the reference state first must wrap the observable last — both routes then mean the same state."""
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if self._check_eval() == 'observable_rotation' and not as_array:
            return list(zip(generators, -2 * x))[::-1]
        self._device_ready()
        own = generators is self.excitation_generators
        plan = self._ansatz if own else self._plan_of(generators)
        try:
            side = 1 << self.observable.n_qubits
            with kernels.DeviceBuffer.upload(self._ref_amplitudes()) as psi:
                plan.apply(x, psi)
                amp = psi.download(np.complex128, side)
        finally:
            if not own:
                plan.free()
        return amp if as_array else QuantumState.from_array(amp.reshape(-1, 1))

    def f(self, x) -> float:
        x = self._angles(x)
        if self._check_eval() == 'observable_rotation':
            ref = self._ref_quantum_state()
            rotated = self.observable.perform_rotations(self.get_state(self.excitation_generators, x)) if x.shape[0] else self.observable
            return float((ref.dagger * rotated * ref).real)
        self._device_ready()
        return float(self._ansatz.energy_grad(self._plan_H, x, self._ref_dev, want_grad=False)[0])

    def partial_derivative(self, x, param_index: int) -> float:
        """The parameter shift rule: two energies."""
        upper = np.array(x, dtype=np.float64)
        lower = upper.copy()
        upper[param_index] += np.pi / 4
        lower[param_index] -= np.pi / 4
        return self.f(upper) - self.f(lower)

    def gradient(self, x) -> np.ndarray:
        x = self._angles(x)
        if self._check_eval() == 'observable_rotation':
            return np.asarray([self.partial_derivative(x, i) for i in range(x.shape[0])], dtype=np.float64)
        self._device_ready()
        return self._ansatz.energy_grad(self._plan_H, x, self._ref_dev)[1]

    def run(self, x0=None, **kwargs):
        """``scipy.optimize.minimize`` over the parameters with ``jac=self.gradient``.  Returns the serialised result and the history
        ``{'params', 'energy', 'gradient'}``, each keyed by the count of energy evaluations so far (some optimisers ask for fewer
        gradients than energies)."""
        from scipy.optimize import minimize
        if x0 is None:
            x0 = np.random.random(self.n_parameters)
        vqe_history = {'params': {}, 'energy': {}, 'gradient': {}}
        step = [-1]

        def fun(x):
            step[0] += 1
            energy = self.f(x)
            vqe_history['params'][step[0]] = tuple(x)
            vqe_history['energy'][step[0]] = energy
            if self.verbose:
                print(f'VQE evaluation {step[0]}: energy {energy!r}')
            return energy

        def jac(x):
            grad = self.gradient(x)
            vqe_history['gradient'][step[0]] = tuple(grad)
            if self.verbose:
                print(f'VQE evaluation {step[0]}: gradient norm {np.linalg.norm(grad):.3e}')
            return grad

        opt_out = minimize(fun=fun, jac=jac, x0=np.asarray(x0, dtype=np.float64), **kwargs)
        return serialize_opt_data(opt_out), vqe_history


class ADAPT_VQE(VQE_Driver):
    """qubit-ADAPT-VQE (https://doi.org/10.1103/PRXQuantum.2.020310): the ansatz grows by the pool element of largest energy derivative,
    re-optimised after every addition; ``TETRIS`` (https://doi.org/10.48550/arXiv.2209.10562) adds several elements of disjoint support
    per cycle.  ``derivative_eval`` keeps the reference's two names, ``'param_shift'`` and ``'commutators'``; both are the same number,
    ``<psi| i [H, P_j] |psi>``, and both are one ``kernels.pool_gradient`` call."""
    derivative_eval = 'param_shift'
    TETRIS = False
    topology_aware = False
    topology_bias = 1
    topology = None

    def __init__(self, observable: PauliwordOp, excitation_pool: PauliwordOp = None, ref_state=None) -> None:
        super().__init__(observable=observable, excitation_ops=PauliwordOp.empty(observable.n_qubits), ref_state=ref_state)
        self.excitation_pool = PauliwordOp(np.asarray(excitation_pool.symp_matrix, dtype=bool).reshape(excitation_pool.n_terms, -1),
                                           np.ones(excitation_pool.n_terms))
        self.adapt_operator = PauliwordOp.empty(observable.n_qubits)
        self.opt_parameters = []
        self.current_state = None

    def pool_gradient(self) -> np.ndarray:
        if self.derivative_eval not in ('param_shift', 'commutators'):
            raise ValueError('Unrecognised derivative_eval method')
        self._check_eval()
        self._device_ready()
        side = 1 << self.observable.n_qubits
        with kernels.DeviceBuffer(side * 16) as psi:
            self._ansatz.energy_grad(self._plan_H, self.opt_parameters, self._ref_dev, psi_out=psi, want_grad=False)
            return kernels.pool_gradient(self._plan_H, self.excitation_pool._device(), psi)

    def pool_score(self) -> np.ndarray:
        if self.topology_aware:
            raise NotImplementedError('ADAPT_VQE: topology_aware scoring (subgraph matching against a device topology) is not part of this port')
        return abs(self.pool_gradient())

    def append_to_adapt_operator(self, excitations_to_append: List[PauliwordOp]) -> None:
        for excitation in excitations_to_append:
            if not np.any(self.adapt_operator.symp_matrix):          # still the empty operator: the first term replaces it
                self.adapt_operator = excitation.copy()
            else:
                self.adapt_operator = self.adapt_operator.append(excitation)

    def _select(self, scores: np.ndarray, gtol: float) -> List[PauliwordOp]:
        """The pool element of largest score; under ``TETRIS`` every further element, by falling score, whose qubits are still free,
        until all qubits are taken or the scores fall below ``gtol``."""
        ranked = [int(i) for i in np.argsort(scores)[::-1]]
        if not self.TETRIS:
            return [self.excitation_pool[ranked[0]]]
        chosen, taken = [], np.zeros(self.observable.n_qubits, dtype=bool)
        for i in ranked:
            term = self.excitation_pool[i]
            qubits = np.asarray(term.X_block | term.Z_block, dtype=bool).reshape(-1)
            if not (qubits & taken).any():
                chosen.append(term)
                taken |= qubits
            if taken.all() or scores[i] < gtol:
                break
        return chosen

    def optimize(self, max_cycles: int = 10, gtol: float = 1e-3, atol: float = 1e-10, target: float = 0, target_error: float = 1e-3):
        """The ADAPT loop: score the pool, append the selection, re-optimise all parameters with BFGS from the previous optimum (new
        parameters at 0).  A cycle starts only while the last largest score exceeds ``gtol``, fewer than ``max_cycles`` cycles have run,
        the last two energies differ by more than ``atol`` and the last energy is further than ``target_error`` from ``target``.
        Returns ``{'result', 'interim_data', 'ref_state', 'adapt_operator'}``; ``interim_data[c]`` holds cycle c (from 1) and
        ``interim_data['history']`` the energies."""
        interim_data = {'history': []}
        result, largest, energy, previous = None, 1.0, 1.0, 0.0                 # the reference's starting values: the first cycle always runs
        cycle = 1
        while largest > gtol and cycle <= max_cycles and abs(energy - previous) > atol and abs(energy - target) > target_error:
            scores = self.pool_score()
            largest = float(scores.max())
            selected = self._select(scores, gtol)
            names = [symplectic_to_string(term.symp_matrix[0]) for term in selected]
            self.append_to_adapt_operator(selected)
            if self.verbose:
                print(f'ADAPT cycle {cycle}: largest pool derivative {largest:.5f}, appending ' + ', '.join(names))
            self.prepare_for_evolution(self.adapt_operator)
            result, vqe_history = self.run(x0=np.append(self.opt_parameters, np.zeros(len(selected))), method='BFGS')
            interim_data[cycle] = {'output': result, 'history': vqe_history, 'gmax': largest, 'excitation': names}
            previous, energy = energy, result['fun']
            interim_data['history'].append(energy)
            if self.verbose:
                print(f'ADAPT cycle {cycle}: energy {energy:.8f}')
            self.opt_parameters = result['x']
            cycle += 1
        return {
            'result': result,
            'interim_data': interim_data,
            'ref_state': _state_to_dict(self._ref_quantum_state()),
            'adapt_operator': [symplectic_to_string(row) for row in self.adapt_operator.symp_matrix],
        }
