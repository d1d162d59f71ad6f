"""``exact_gs_energy`` (reference ``symmer/utils.py:14-76``) without the matrix: a Lanczos iteration with full reorthogonalisation whose
vectors stay on the device.  ``H v`` is the matrix-free product of ``csrc/matvec.hip``; a step (product, Gram-Schmidt done twice, norm,
next vector) is one call of ``csrc/lanczos.hip`` that returns two scalars; Python keeps the small tridiagonal matrix and takes its lowest
eigenpair with NumPy.

``get_entanglement_entropy`` (reference ``symmer/utils.py:78-94``): the reduced density matrix of the smaller side of the bipartition is
one device call on the dense amplitudes (``csrc/rdm.hip``); its small Hermitian eigenproblem is NumPy's.

``sampled_expval``: the finite-shot estimate of ``<psi|H|psi>`` from measurements of the QWC cliques of ``H`` (``csrc/basis.hip``,
``csrc/sample.hip``)."""
import numpy as np

from . import kernels
from .operators import PauliwordOp, QuantumState

MAX_BASIS = 256          # vectors of the resident basis at most
MIN_BASIS = 4            # fewer than this do not fit: MemoryError
RITZ_EVERY = 8           # steps between two looks at the Ritz pair: np.linalg.eigh after every step was three quarters of the BH run


def _start_vector(initial_guess, n_qubits):
    side = 1 << n_qubits
    if initial_guess is None:
        rng = np.random.default_rng(0)
        return rng.standard_normal(side) + 1j * rng.standard_normal(side)
    if isinstance(initial_guess, QuantumState):
        if initial_guess.n_qubits != n_qubits:
            raise ValueError(f'exact_gs_energy: initial_guess has {initial_guess.n_qubits} qubits, the operator {n_qubits}')
        return np.array(initial_guess.to_dense_matrix, dtype=np.complex128).reshape(-1)     # a copy: the state caches its dense vector
    v = np.asarray(initial_guess, dtype=np.complex128).reshape(-1)
    if v.shape[0] != side:
        raise ValueError(f'exact_gs_energy: initial_guess has {v.shape[0]} elements, 2^{n_qubits} wanted')
    return v.copy()


def _lowest_ritz_pair(alphas, betas):
    """(theta, s) of the tridiagonal matrix with diagonal ``alphas`` and off-diagonal ``betas[:len(alphas) - 1]``."""
    m = len(alphas)
    t = np.diag(np.asarray(alphas, dtype=np.float64))
    if m > 1:
        off = np.asarray(betas[:m - 1], dtype=np.float64)
        t += np.diag(off, 1) + np.diag(off, -1)
    w, s = np.linalg.eigh(t)
    return float(w[0]), np.ascontiguousarray(s[:, 0])


def exact_gs_energy(H, initial_guess=None, n_particles=None, number_operator=None, n_eigs=6, *, tol=1e-10, max_basis=None,
                    max_restarts=1000, return_array=False):
    """The lowest eigenvalue of the Hermitian ``PauliwordOp`` ``H`` (1 .. 32 qubits) and a unit eigenvector of it, as ``(float,
    QuantumState)``; with ``return_array=True`` the vector comes as the raw complex128 array of ``2^n`` amplitudes (qubit 0 the most
    significant bit of the index).  With ``n_particles`` the lowest eigenpair of that sector of the diagonal ``number_operator`` (which
    must commute with ``H``): the start vector and every product are multiplied by the sector's mask, so the Krylov space never leaves
    the sector.

    Unlike the reference, ``H`` is the operator itself, not its matrix: the matrix is never built (TypeError for anything else; there
    is no host eigensolver behind this function).  The iteration is Lanczos with full reorthogonalisation on a resident basis of at
    most ``max_basis`` vectors (default: up to 256, as many as fit half of the free device memory beside two work vectors and the plan,
    never more than the dimension of the (sector) space); when the basis is full it restarts from the current Ritz vector.  Every
    eighth step (and when the basis is full) it takes the lowest Ritz pair of the tridiagonal matrix and stops
    when the residual estimate ``|beta_m s_m|`` of the lowest Ritz pair is at most ``tol * sum_k |c_k|`` (the sum bounds ``||H||``);
    ``max_restarts`` restarts without that raise RuntimeError with the residual reached.  The start vector is ``initial_guess`` (an
    ndarray of ``2^n`` numbers or a ``QuantumState``) or a Gaussian vector of ``np.random.default_rng(0)``; every sum on the device
    runs in a fixed order, so the same input gives the same bits on every run.  For a degenerate level the result is SOME unit vector
    of the eigenspace (which one depends on the start vector).

    ``n_eigs`` is accepted for compatibility with the reference's signature and is not used.  The reference computes the lowest
    ``n_eigs`` eigenvectors and searches them for one of the right particle number; for the 10-qubit B+ Hamiltonian the 4-particle
    ground state is the 19th eigenvalue, behind a 6-fold and a 12-fold level, so its default ``n_eigs=6`` raises, whereas the projected
    iteration here finds it in about 25 steps."""
    if not isinstance(H, PauliwordOp):
        raise TypeError(f'exact_gs_energy: pass the PauliwordOp itself, not its matrix ({type(H).__name__}): the product H v runs on the '
                        f'device without the matrix, and there is no host eigensolver behind this function')
    n = H.n_qubits
    if not 1 <= n <= 32:
        raise ValueError(f'exact_gs_energy: {n} qubits; 1 .. 32 are supported')
    if not np.allclose(H.cleanup().coeff_vec.imag, 0):
        raise ValueError('exact_gs_energy: the operator is not Hermitian (its cleaned coefficients have imaginary parts)')
    if n_particles is not None:
        assert number_operator is not None, 'Must specify the number operator.'
        assert number_operator.n_qubits == n, 'number operator defined for a different number of qubits'
        assert not np.any(number_operator.X_block), 'Number operator not diagonal'
        if not H.commutes(number_operator):
            raise ValueError('exact_gs_energy: the number operator does not commute with H: its sectors are not invariant')
    side = 1 << n
    norm_bound = float(np.abs(np.asarray(H.coeff_vec)).sum())
    v0 = _start_vector(initial_guess, n)

    with H._matvec_plan() as plan:
        keep, dim = None, side
        try:
            if n_particles is not None:
                keep = kernels.DeviceBuffer(side)
                with number_operator._matvec_plan() as plan_n:
                    dim = plan_n.sector_mask(n_particles, keep)
                if dim == 0:
                    raise ValueError(f'exact_gs_energy: no basis state has {n_particles} particles: the sector is empty')
                v0 *= keep.download(np.uint8, side)
            norm0 = np.linalg.norm(v0)
            if not norm0 > 0:
                raise ValueError('exact_gs_energy: the start vector is zero' + (' in the sector' if keep is not None else ''))
            v0 /= norm0

            if max_basis is None:
                fit = (kernels.mem_info()[0] // 2 - plan.info()[3] - 2 * side * 16) // (side * 16)
                if fit < min(MIN_BASIS, dim):
                    raise MemoryError(f'exact_gs_energy: fewer than {MIN_BASIS} vectors of 2^{n} amplitudes fit half of the free device memory')
                m_max = int(min(MAX_BASIS, dim, fit))
            else:
                if int(max_basis) < 2 and dim > 1:
                    raise ValueError('exact_gs_energy: max_basis must be at least 2')
                m_max = int(min(int(max_basis), dim))

            with kernels.DeviceBuffer(m_max * side * 16) as basis:
                basis.write(v0)                                                    # slot 0
                residual = np.inf
                for _ in range(int(max_restarts) + 1):
                    alphas, betas = [], []
                    for j in range(m_max):
                        alpha, beta = plan.lanczos_step(keep, basis, m_max, j)
                        alphas.append(alpha)
                        betas.append(beta)
                        # the Ritz pair is looked at every few steps, when the basis is full, and when beta alone meets the bound
                        if (j + 1) % RITZ_EVERY and j + 1 < m_max and beta > tol * norm_bound:
                            continue
                        theta, s = _lowest_ritz_pair(alphas, betas)
                        residual = abs(beta * s[-1])
                        if residual <= tol * norm_bound:
                            with kernels.DeviceBuffer(side * 16) as out:
                                kernels.vec_combine(basis, j + 1, n, s, out=out, normalise=True)
                                psi = out.download(np.complex128, side)
                            return (theta, psi) if return_array else (theta, QuantumState.from_array(psi.reshape(-1, 1)))
                    kernels.vec_combine(basis, m_max, n, s, out=None, normalise=True)      # restart from the Ritz vector
                raise RuntimeError(f'exact_gs_energy: not converged after {int(max_restarts)} restarts of a basis of {m_max} vectors: '
                                   f'residual {residual:.3e}, wanted {tol * norm_bound:.3e}')
        finally:
            if keep is not None:
                keep.free()


def get_entanglement_entropy(psi, qubits):
    """symmer/utils.py:78-94: the von Neumann entropy ``-sum lambda ln lambda`` of the bipartition ``qubits`` | the rest, over the positive
    eigenvalues of the reduced density matrix.  ``psi`` is a ``QuantumState``, or ``2^n`` amplitudes (qubit 0 the most significant bit of
    the index) as ``exact_gs_energy`` returns with ``return_array=True``; it is not normalised, as in the reference.  The matrix comes from
    the device (``csrc/rdm.hip``) and is Hermitian to the bit, so the eigenvalues are ``numpy.linalg.eigvalsh``'s.  It is taken over
    whichever of ``qubits`` and its complement is smaller — the non-zero spectra of ``M M^+`` and ``M^+ M`` are equal, so the value is the
    same.  ValueError for a qubit outside ``0 .. n-1``, beyond 32 qubits, or when the smaller side has more than 12 qubits."""
    if isinstance(psi, QuantumState):
        n = psi.n_qubits
        if not 1 <= n <= kernels.RDM_MAX_QUBITS:
            raise ValueError(f'get_entanglement_entropy: {n} qubits; 1 .. {kernels.RDM_MAX_QUBITS} are supported')
    else:
        psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
        n = int(psi.shape[0]).bit_length() - 1
        if psi.shape[0] != 1 << n or not 1 <= n <= kernels.RDM_MAX_QUBITS:
            raise ValueError(f'get_entanglement_entropy: {psi.shape[0]} amplitudes; 2^n for n in 1 .. {kernels.RDM_MAX_QUBITS} wanted')
    kept = {int(q) for q in qubits}
    if any(q < 0 or q >= n for q in kept):
        raise ValueError(f'get_entanglement_entropy: qubits {sorted(kept)} outside 0 .. {n - 1}')
    if len(kept) > n - len(kept):
        kept = set(range(n)) - kept
    if len(kept) > kernels.RDM_MAX_KEPT:
        raise ValueError(f'get_entanglement_entropy: the smaller side of the bipartition has {len(kept)} qubits; at most '
                         f'{kernels.RDM_MAX_KEPT} are supported')
    amplitudes = np.asarray(psi.to_dense_matrix).reshape(-1) if isinstance(psi, QuantumState) else psi
    eigvals = np.linalg.eigvalsh(kernels.rdm_dev(amplitudes, n, kept))
    eigvals = eigvals[eigvals > 0]
    return float(-np.sum(eigvals * np.log(eigvals)))



def sampled_expval(H, psi, n_shots, seed=None, strategy='largest_first', return_terms=False):
    """The finite-shot estimate of ``<psi|H|psi>``: what ``n_shots`` measurements per group of jointly measurable terms give, beside the
    exact ``H.expval(psi)``.  ``H``: a ``PauliwordOp`` of 1 .. 32 qubits; ``psi``: a normalised ket ``QuantumState`` or its ``2^n``
    amplitudes (qubit 0 the most significant bit of the index).

    The terms are grouped into qubitwise-commuting cliques by the device colouring of ``clique_cover(edge_relation='QWC')``
    (``strategy``: 'largest_first' or 'sorted_insertion').  ``psi`` is uploaded once; per clique ``g``, in the cover's order: a device
    copy, one layer of H / H S^+ on the clique's merged X / Y positions (``csrc/basis.hip``), a sampling plan, ``n_shots`` draws from
    uniforms ``g * n_shots ...`` of the Philox stream of ``seed`` (``csrc/sample.hip``), and the signed sums
    ``sum_j count_j (-1)^{|z_k & b_j|}`` of the clique's terms read as Z strings; only those integers return.  The estimate of a term is
    its sum over ``n_shots`` (the identity: 1) and the result ``sum_k c_k est_k`` (the real part for a Hermitian ``H``; complex
    coefficients are kept).  ``seed=None`` takes one integer from NumPy's global generator.  With ``return_terms``:
    ``(value, estimates, clique_of_term)``, both in ``H``'s term order."""
    if not isinstance(H, PauliwordOp):
        raise TypeError(f'sampled_expval: H must be a PauliwordOp ({type(H).__name__})')
    n = H.n_qubits
    if not 1 <= n <= 32:
        raise ValueError(f'sampled_expval: {n} qubits; 1 .. 32 are supported')
    if strategy not in ('largest_first', 'sorted_insertion'):
        raise ValueError(f"sampled_expval: strategy {strategy!r}; 'largest_first' and 'sorted_insertion' run on the device")
    n_shots = int(n_shots)
    if n_shots < 1:
        raise ValueError('sampled_expval: n_shots must be at least 1')
    if isinstance(psi, QuantumState):
        assert psi.vec_type == 'ket', 'sampled_expval: the state must be a ket'
        if psi.n_qubits != n:
            raise ValueError(f'sampled_expval: the state has {psi.n_qubits} qubits, the operator {n}')
        amplitudes = np.asarray(psi.to_dense_matrix, dtype=np.complex128).reshape(-1)
    else:
        amplitudes = np.ascontiguousarray(psi, dtype=np.complex128).reshape(-1)
        if amplitudes.shape[0] != 1 << n:
            raise ValueError(f'sampled_expval: {amplitudes.shape[0]} amplitudes, 2^{n} wanted')
    if not np.isclose(np.linalg.norm(amplitudes), 1):
        raise ValueError('should not sample state that is not normalized')
    seed = QuantumState._seed_of(seed)
    T = H.n_terms
    estimates, clique_of = np.zeros(T, dtype=np.float64), np.zeros(T, dtype=np.int64)
    if T == 0:
        return (0.0, estimates, clique_of) if return_terms else 0.0
    from . import packing
    X, Z = np.asarray(H.X_block, dtype=bool), np.asarray(H.Z_block, dtype=bool)
    members = H._clique_members_device(kernels.RELATIONS['QWC'], strategy)
    one = np.ones(1, dtype=np.float64)
    with kernels.DeviceBuffer.upload(amplitudes) as psi_dev, kernels.DeviceBuffer(amplitudes.nbytes) as work:
        for g, terms in enumerate(members):
            kernels.vec_combine(psi_dev, 1, n, one, out=work)                              # work = 1.0 * psi: a copy to the bit
            xg, zg = X[terms], Z[terms]
            kernels.basis_change_dev(work, n, np.flatnonzero(np.any(xg & ~zg, axis=0)), np.flatnonzero(np.any(xg & zg, axis=0)))
            z_rows = packing.pack_rows(np.hstack([np.zeros_like(xg), xg | zg]))
            with kernels.SamplePlan(work, 1 << n) as plan, kernels.DeviceOp.upload(z_rows) as z_op:
                idx, count, n_distinct = plan.draw_dev(n_shots, seed, g * n_shots)
                with idx, count:
                    sums = kernels.counts_signed_sums(z_op, n, idx, count, n_distinct)
            estimates[terms] = sums / n_shots
            clique_of[terms] = g
    value = complex(np.sum(np.asarray(H.coeff_vec) * estimates))
    value = value.real if np.allclose(np.asarray(H.coeff_vec).imag, 0) else value
    return (value, estimates, clique_of) if return_terms else value
