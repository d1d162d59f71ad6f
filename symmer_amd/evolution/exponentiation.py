"""Operator-level exponentials (reference ``symmer/evolution/exponentiation.py``): ``exp`` of a single Pauli term in closed form, and the
first-order Trotter product of a sum, as ``PauliwordOp`` — sums and products on the device kernels of ``+`` and ``*``.  The number of
terms of a Trotter product can grow with every factor; ``evolve_state`` (``time_evolution.py``) propagates a state instead and needs no
product of operators."""
import numpy as np

from ..operators import PauliwordOp


def exponentiate_single_Pop(P: PauliwordOp) -> PauliwordOp:
    """``exp(c P) = cosh(c) I + sinh(c) P`` for a one-term operator ``c P`` (``P^2 = I``).  For ``exp(i theta P)`` the coefficient must
    be ``i theta``: the imaginary unit is part of it."""
    assert P.n_terms == 1, 'Can only exponentiate single Pauli terms'
    c = complex(np.asarray(P.coeff_vec)[0])
    identity = np.zeros((1, 2 * P.n_qubits), dtype=bool)
    return PauliwordOp(identity, [np.cosh(c)]) + PauliwordOp(np.asarray(P.symp_matrix, dtype=bool).copy(), [np.sinh(c)])


def trotter(op: PauliwordOp, trotnum: int = 1) -> PauliwordOp:
    """``(prod_k exp(c_k P_k / trotnum))^trotnum`` with the factors in operator order, the first term leftmost: ``exp(op)`` exactly when
    the terms commute, otherwise its first-order Trotter approximation, which improves as ``trotnum`` grows."""
    trotnum = int(trotnum)
    assert trotnum >= 1, 'trotnum must be at least 1'
    scaled = op.multiply_by_constant(1 / trotnum)
    factors = [exponentiate_single_Pop(scaled[k]) for k in range(scaled.n_terms)] * trotnum
    assert factors, 'Cannot exponentiate an operator without terms'
    out = factors[0]
    for factor in factors[1:]:
        out = out * factor
    return out


def truncated_exponential(op: PauliwordOp, truncate_at: int = 10) -> PauliwordOp:
    raise NotImplementedError
