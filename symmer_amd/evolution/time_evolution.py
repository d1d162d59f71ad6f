"""``evolve_state``: ``exp(-i H t) |psi>`` and ``exp(-tau H) |psi>`` for a Hermitian ``PauliwordOp`` on a dense statevector, without the
matrix and without a Trotter product.  The propagator is expanded in Chebyshev polynomials of the operator scaled to
``[-1, 1]``,

    exp(-i z x) = sum_k (2 - delta_k0) (-i)^k J_k(z) T_k(x),        exp(-z x) = sum_k (2 - delta_k0) (-1)^k I_k(z) T_k(x),

with ``x = (H - centre) / half_width`` and ``z = half_width * t``.  The Bessel coefficients are formed here on the host
(``chebyshev_coefficients``); the sum ``sum_k c_k T_k(x) psi`` is one device call (``MatvecPlan.chebyshev``, ``csrc/evolve.hip``) of one
launch per order, which keeps four vectors whatever the order.  ``|T_k(x)| <= 1`` on the interval, so the coefficients that are dropped
bound the error of the propagator in the operator norm: the tolerance asked for is a bound — provided the spectrum of ``H`` lies in the
interval (``spectral_interval``)."""
import contextlib

import numpy as np
from scipy.special import ive, jv

from .. import kernels
from ..operators import PauliwordOp, QuantumState

LANCZOS_STEPS = 32           # steps of the 'lanczos' spectral estimate at most
LANCZOS_MARGIN = 0.01        # ... whose interval is widened by this share of its width on either side
_I_POW = np.array([1, -1j, -1, 1j], dtype=np.complex128)          # (-i)^k by k mod 4, exact


def chebyshev_coefficients(z, tol, imaginary=False):
    """``(coeffs, tail)``: the Chebyshev coefficients ``c_0 .. c_K`` of ``exp(-i z x)`` on ``[-1, 1]``
    (``c_k = (2 - delta_k0) (-i)^k J_k(z)``), or with ``imaginary`` of ``exp(-z (x + 1))`` (``c_k = (2 - delta_k0) (-1)^k e^-z I_k(z)``:
    the propagator scaled by ``e^-z``, at most 1 on the interval, so that it never overflows), for ``z >= 0``.  ``K`` is the smallest
    order whose dropped tail ``sum_{k > K} |c_k|`` is at most ``tol``; ``tail`` is that sum, which bounds the error of the truncated series
    everywhere on ``[-1, 1]``.  The tail is summed over the orders up to ``ceil(z) + 64 + 8 z^(1/3)``, beyond which the coefficients have
    fallen by more than thirty orders of magnitude from their largest; ValueError if no order before the end of that window reaches
    ``tol`` (a tolerance below what doubles resolve).  Host NumPy / SciPy only.  ``z = 0`` gives ``([1], 0.0)``."""
    z, tol = float(z), float(tol)
    if not (np.isfinite(z) and z >= 0):
        raise ValueError(f'chebyshev_coefficients: z = {z}; a finite z >= 0 wanted')
    if not tol > 0:
        raise ValueError(f'chebyshev_coefficients: tol = {tol}; a positive tolerance wanted')
    if z == 0:
        return np.ones(1, dtype=np.complex128), 0.0
    k = np.arange(int(np.ceil(z) + 64 + 8 * z ** (1.0 / 3.0)) + 1)
    weight = np.where(k == 0, 1.0, 2.0)
    if imaginary:
        c = (weight * np.where(k & 1, -1.0, 1.0) * ive(k, z)).astype(np.complex128)
    else:
        c = weight * jv(k, z) * _I_POW[k & 3]
    tails = np.concatenate([np.cumsum(np.abs(c)[::-1])[::-1][1:], [0.0]])        # tails[K] = sum_{k > K} |c_k| within the window
    reached = np.flatnonzero(tails[:-1] <= tol)
    if reached.shape[0] == 0:
        raise ValueError(f'chebyshev_coefficients: no order up to {k[-1]} has a tail within tol = {tol:.3g} at z = {z:.6g} '
                         f'(the smallest tail is {tails[-2]:.3g})')
    K = int(reached[0])
    return np.ascontiguousarray(c[:K + 1]), float(tails[K])


def _norm1_interval(H):
    coeff = np.asarray(H.coeff_vec)
    identity = ~np.any(np.asarray(H.symp_matrix, dtype=bool), axis=1)
    centre = float(np.sum(coeff[identity].real))
    half_width = float(np.sum(np.abs(coeff[~identity])))
    return centre, half_width if half_width > 0 else 1.0


def _lanczos_interval(H, plan):
    n = H.n_qubits
    side = 1 << n
    fit = (kernels.mem_info()[0] // 2 - 2 * side * 16) // (side * 16)
    m = int(min(LANCZOS_STEPS, side, fit))
    if m < min(2, side):
        raise MemoryError(f'spectral_interval: fewer than two vectors of 2^{n} amplitudes fit half of the free device memory')
    rng = np.random.default_rng(0)
    v0 = rng.standard_normal(side) + 1j * rng.standard_normal(side)
    v0 /= np.linalg.norm(v0)
    alphas, betas = [], []
    with kernels.DeviceBuffer(m * side * 16) as basis:
        basis.write(v0)
        for j in range(m):
            alpha, beta = plan.lanczos_step(None, basis, m, j)
            alphas.append(alpha)
            betas.append(beta)
            if not beta > 0:
                break
    t = np.diag(np.asarray(alphas, dtype=np.float64))
    if len(alphas) > 1:
        off = np.asarray(betas[:-1], dtype=np.float64)
        t += np.diag(off, 1) + np.diag(off, -1)
    theta, s = np.linalg.eigh(t)
    low = theta[0] - abs(betas[-1] * s[-1, 0])
    high = theta[-1] + abs(betas[-1] * s[-1, -1])
    margin = LANCZOS_MARGIN * (high - low)
    return float(low - margin), float(high + margin)


def spectral_interval(H, plan=None, method='norm1'):
    """``(centre, half_width)`` of an interval meant to hold the spectrum of the Hermitian ``PauliwordOp`` ``H``.

    ``'norm1'`` (rigorous): every Pauli string has norm 1, so the spectrum lies within ``sum_k |c_k|`` over the terms other than the
    identity, around the identity's (real) coefficient.  No device call.
    ``'lanczos'`` (an estimate, NOT a proof): ``min(32, 2^n)`` steps of the device Lanczos iteration (``MatvecPlan.lanczos_step``) from a
    fixed Gaussian start vector; the extreme Ritz values, each pushed outward by its residual bound ``|beta_m s_m|``, the interval
    widened by 1 % of its width on either side and intersected with the ``'norm1'`` interval.  ``sum |c|`` overestimates the width
    of a chemistry Hamiltonian severalfold and the number of Chebyshev orders grows with the width, which is what this buys; but a
    Krylov space of 32 vectors can miss an eigenvalue the start vector hardly overlaps with, and outside the interval the expansion
    diverges.  ``plan``: the ``MatvecPlan`` of ``H`` (one is made and freed when None); ``'norm1'`` does not use it.
    A ``(centre, half_width)`` pair is passed through.  An interval of no width (``H`` a multiple of the identity) gets half_width 1."""
    if not isinstance(method, str):
        centre, half_width = (float(q) for q in method)
        if not (np.isfinite(centre) and np.isfinite(half_width) and half_width > 0):
            raise ValueError(f'spectral_interval: ({centre}, {half_width}); a finite centre and a finite half_width > 0 wanted')
        return centre, half_width
    centre, half_width = _norm1_interval(H)
    if method == 'norm1':
        return centre, half_width
    if method != 'lanczos':
        raise ValueError(f"spectral_interval: method {method!r}; 'norm1', 'lanczos' or a (centre, half_width) pair wanted")
    if plan is None:
        with H._matvec_plan() as own:
            low, high = _lanczos_interval(H, own)
    else:
        low, high = _lanczos_interval(H, plan)
    low, high = max(low, centre - half_width), min(high, centre + half_width)
    if not high > low:
        return centre, half_width if high < low else 1.0
    return 0.5 * (low + high), 0.5 * (high - low)


class EvolutionResult:
    """What ``evolve_state`` returns for a time grid or with observables: ``times``; ``states`` (a ``QuantumState`` per time, None with
    ``return_states=False``); ``expvals`` (float ``[n_times][n_obs]``, None without observables); ``orders`` and ``tails`` (the Chebyshev
    order ``K`` and the dropped tail of every step, 0 for a step of no duration); ``norms`` (imaginary time only, else None: the norm of
    every step's result before it was normalised); ``interval`` (the ``(centre, half_width)`` used)."""

    def __init__(self, times, states, expvals, orders, tails, norms, interval):
        self.times, self.states, self.expvals, self.orders, self.tails, self.norms, self.interval = times, states, expvals, orders, tails, norms, interval

    def __repr__(self):
        return f'EvolutionResult(times={self.times!r}, orders={self.orders!r}, interval={self.interval!r})'


def _dense_amplitudes(psi, n_qubits):
    side = 1 << n_qubits
    if isinstance(psi, QuantumState):
        if psi.n_qubits != n_qubits:
            raise ValueError(f'evolve_state: the state has {psi.n_qubits} qubits, the operator {n_qubits}')
        return np.array(psi.to_dense_matrix, dtype=np.complex128).reshape(-1)
    v = np.array(psi, dtype=np.complex128).reshape(-1)
    if v.shape[0] != side:
        raise ValueError(f'evolve_state: the vector has {v.shape[0]} elements, 2^{n_qubits} wanted')
    return v


def evolve_state(H, psi, t, *, imaginary=False, tol=1e-10, spectral_bounds='norm1', observables=None, return_states=True):
    """``exp(-i H t) |psi>`` — with ``imaginary``, ``exp(-t H) |psi>`` normalised — for a ``PauliwordOp`` ``H`` of 1 .. 32 qubits whose
    coefficients are real after ``cleanup()`` (ValueError otherwise: the expansion assumes a real spectrum) and ``psi`` a
    ``QuantumState`` or ``2^n`` amplitudes (qubit 0 the most significant bit of the index).  The state stays on the device; the
    matrix of ``H`` is never built.

    ``t``: a time ``>= 0``, or a non-decreasing sequence of them; every state is propagated from the one before by the difference (two
    device buffers taking turns), and a repeated time returns the same state without a device call.  A step of duration ``dt`` is
    one call of ``MatvecPlan.chebyshev`` with the coefficients of ``chebyshev_coefficients(half_width * dt, tol, imaginary)``, in real
    time multiplied by the phase ``exp(-i centre dt)`` on the host.  ``spectral_bounds``: ``'norm1'`` (rigorous, the default),
    ``'lanczos'`` (usually several times narrower and as many times cheaper, but an estimate) or a ``(centre, half_width)`` pair; see
    ``spectral_interval``.

    Accuracy.  Real time: the dropped tail of a step (at most ``tol``) bounds the error of the propagator in the operator norm, so after
    several steps the error of a unit state is at most the sum of the tails, plus rounding.  Imaginary time: a step computes
    ``exp(-dt (H - E_low)) |psi>`` with ``E_low = centre - half_width`` (norm at most 1, no overflow) within its tail, reports the norm
    of that vector, and divides by it (``vec_combine`` with ``normalise``); the error of the normalised state is then at most
    ``tol / norm`` to first order, which grows as the overlap with the low-lying states shrinks — read ``norms`` before trusting it.

    ``observables``: a list of ``PauliwordOp``; ``<psi(t_i)| O_j |psi(t_i)>`` (the real part) is taken on the device with a plan of
    ``O_j`` on the state as it is, and only scalars return.  ``return_states=False`` skips the download of the states (4 GiB each at 28
    qubits).  A scalar ``t`` without observables returns the ``QuantumState``; everything else an ``EvolutionResult``.  Every plan and
    buffer is freed on return, also on an error."""
    if not isinstance(H, PauliwordOp):
        raise TypeError(f'evolve_state: H must be a PauliwordOp ({type(H).__name__})')
    n = H.n_qubits
    if not 1 <= n <= 32:
        raise ValueError(f'evolve_state: {n} qubits; 1 .. 32 are supported')
    scalar = np.ndim(t) == 0
    times = np.atleast_1d(np.asarray(t, dtype=np.float64)).reshape(-1)
    if times.shape[0] == 0 or not np.all(np.isfinite(times)) or np.any(times < 0):
        raise ValueError('evolve_state: the times must be finite and >= 0')
    if np.any(np.diff(times) < 0):
        raise ValueError('evolve_state: the times must not decrease')
    observables = list(observables) if observables is not None else []
    for O in observables:
        if not isinstance(O, PauliwordOp) or O.n_qubits != n:
            raise ValueError(f'evolve_state: every observable must be a PauliwordOp of {n} qubits')
    amplitudes = _dense_amplitudes(psi, n)
    side = 1 << n
    Hc = H.cleanup()
    if not np.allclose(np.asarray(Hc.coeff_vec).imag, 0):
        raise ValueError('evolve_state: the operator is not Hermitian (its cleaned coefficients have imaginary parts)')
    Hc = PauliwordOp(Hc.symp_matrix, np.asarray(Hc.coeff_vec).real.astype(np.float64))

    states = [] if return_states else None
    expvals = np.zeros((times.shape[0], len(observables)), dtype=np.float64) if observables else None
    orders, tails, norms = [], [], [] if imaginary else None
    one = np.ones(1, dtype=np.float64)
    with contextlib.ExitStack() as stack:
        plan = stack.enter_context(Hc._matvec_plan())
        centre, half_width = spectral_interval(Hc, plan, spectral_bounds)
        obs_plans = [stack.enter_context(O._matvec_plan()) for O in observables]
        unit = stack.enter_context(PauliwordOp.from_list(['I' * n], [1])._matvec_plan()) if imaginary else None
        bufs = [stack.enter_context(kernels.DeviceBuffer.upload(amplitudes)), stack.enter_context(kernels.DeviceBuffer(side * 16))]
        cur, previous = 0, 0.0
        for i, now in enumerate(times):
            dt = float(now - previous)
            previous = float(now)
            if dt == 0:                                                             # t = 0, or a repeated time: no propagation
                orders.append(0)
                tails.append(0.0)
                if imaginary:
                    norms.append(1.0)
                if i > 0:                                                           # the same state again, without a device call
                    if return_states:
                        states.append(states[-1])
                    if observables:
                        expvals[i] = expvals[i - 1]
                    continue
            else:
                coeffs, tail = chebyshev_coefficients(half_width * dt, tol, imaginary)
                if not imaginary:
                    coeffs = coeffs * np.exp(-1j * centre * dt)
                plan.chebyshev(centre, half_width, coeffs, bufs[cur], bufs[1 - cur])
                cur = 1 - cur
                orders.append(coeffs.shape[0] - 1)
                tails.append(tail)
                if imaginary:
                    norms.append(float(np.sqrt(unit.lanczos_step(None, bufs[cur], 1, 0)[0])))      # <v|1|v> on the vector as it is
                    kernels.vec_combine(bufs[cur], 1, n, one, out=bufs[cur], normalise=True)
            for j, obs_plan in enumerate(obs_plans):
                expvals[i, j] = obs_plan.lanczos_step(None, bufs[cur], 1, 0)[0]
            if return_states:
                # every non-zero amplitude is kept: the default threshold of from_array would add an error of its own to the bound above
                states.append(QuantumState.from_array(bufs[cur].download(np.complex128, side).reshape(-1, 1), threshold=np.finfo(np.float64).tiny))
    if scalar and not observables and return_states:
        return states[0]
    return EvolutionResult(times, states, expvals, orders, tails, norms, (centre, half_width))
