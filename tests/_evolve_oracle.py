"""NumPy restatement of the contract of symgpu_cheb_apply (include/symgpu.h f11): out = sum_{k=0..K} c_k T_k((H - centre) / half_width) psi
by the three-term recurrence, on the row sum of the matvec oracle (tests/_matvec_oracle.py).  Real and imaginary parts are separate
float64 arrays throughout, so that no complex multiplication is left to NumPy: every product and every sum below is one IEEE operation
per element, in the order the header states, and the device result is compared bit for bit.  Test infrastructure only."""
import numpy as np

import _matvec_oracle as mo


def cmul(cr, ci, vr, vi):
    """The plain complex product of f7 / f11, the coefficient (cr, ci) in the place of D."""
    return cr * vr - ci * vi, cr * vi + ci * vr


def cheb_apply(symp_matrix, coeff_vec, centre, half_width, coeffs, psi):
    """complex128[2^n]: the f11 result for the operator as given (not cleaned)."""
    coeffs = np.asarray(coeffs, dtype=np.complex128).reshape(-1)
    psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
    assert coeffs.shape[0] >= 1
    centre = np.float64(centre)
    inv = np.float64(1.0) / np.float64(half_width)
    v, u = (psi.real.copy(), psi.imag.copy()), None                     # T_{k-1}, T_{k-2}
    out_r, out_i = cmul(coeffs[0].real, coeffs[0].imag, v[0], v[1])
    for k in range(1, coeffs.shape[0]):
        h = mo.matvec(symp_matrix, coeff_vec, mo._complex(v[0], v[1]))
        t_r, t_i = h.real - centre * v[0], h.imag - centre * v[1]
        s = inv if k == 1 else np.float64(2.0) * inv
        w_r, w_i = s * t_r, s * t_i
        if u is not None:
            w_r, w_i = w_r - u[0], w_i - u[1]
        p_r, p_i = cmul(coeffs[k].real, coeffs[k].imag, w_r, w_i)
        out_r, out_i = out_r + p_r, out_i + p_i
        u, v = v, (w_r, w_i)
    return mo._complex(out_r, out_i)


def hermitian_case(seed, n, norm1=4.0):
    """(symp bool[T, 2n], real coeff float64[T]) of the statevector families' Hermitian draw `seed` on n qubits, at most 24 terms, as
    given (not cleaned: repeated and cancelling rows stay), scaled to sum|c| = norm1 so that half_width * t stays within 5 norm1."""
    import _statevector_families as sf
    op = sf.operator(seed, hermitian=True, n=n, t_max=24)
    coeff = np.asarray(op.coeff, dtype=np.float64)
    return op.symp, coeff * (norm1 / np.abs(coeff).sum())


def propagate(symp_matrix, coeff_vec, interval, coeffs, psi, dt=None):
    """cheb_apply with the phase exp(-i centre dt) of a real-time step folded into the coefficients as evolve_state folds it (dt None:
    an imaginary-time step, no phase)."""
    centre, half_width = interval
    coeffs = np.asarray(coeffs, dtype=np.complex128)
    if dt is not None:
        coeffs = coeffs * np.exp(-1j * centre * dt)
    return cheb_apply(symp_matrix, coeff_vec, centre, half_width, coeffs, psi)
