"""Plain NumPy restatement of the noncontextual objective (reference: symmer/operators/noncontextual_op.py:533-554, 686-704) over ALL
eigenvalue assignments, in the form the device search takes its input (include/symgpu.h, symgpu_noncon_search):

    E(m) = sum_{k in S0} c_k s_k(m)  -  sqrt( sum_i ( sum_{k in C_i} c_k s_k(m) )^2 ),     s_k(m) = (-1)^popcount(mask_k & m)

Bit b of an assignment m set <=> free generator number f-1-b (in generator order) is -1, so that m counts DOWN the reference's
``itertools.product([-1, 1], repeat=f)``: its first minimum (``min`` keeps the first) is the LARGEST m among equal energies.
Nothing here touches the GPU or the library.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'noncon_solve.npz')


def golden_cases():
    """[(tag, case)] of tests/golden/noncon_solve.npz (tools/gen_golden_noncon_solve.py): the reference's NoncontextualOp on ~40 operators.
    case: n, symp, coeff, generators, cliques, G_indices, C_indices, pauli_mult_signs, energy, nu, unique, and for the reference-state
    cases ref_state and sector (the eigenvalues the state fixes, 0 = free)."""
    z = np.load(GOLDEN)
    cases = [dict() for _ in range(int(z['n_cases']))]
    for key in z.files:
        if '/' in key:
            idx, field = key.split('/', 1)
            cases[int(idx)][field] = z[key]
    return [(f'{k:02d}', case) for k, case in enumerate(cases)]


def tolerance(coeff):
    """4 (T + 64) 2^-52 sum|c|: the worst-case reordering error of a T-term double sum, times 4 for the squares and the square root."""
    coeff = np.asarray(coeff, dtype=np.float64)
    return 4.0 * (coeff.size + 64) * 2.0 ** -52 * float(np.sum(np.abs(coeff)))


def _parity(a):
    """popcount(a) & 1 of a uint64 array"""
    a = a.copy()
    for s in (32, 16, 8, 4, 2, 1):
        a ^= a >> np.uint64(s)
    return (a & np.uint64(1)).astype(np.int64)


def landscape(coeff, mask, clique, n_free, n_cliques, chunk=1 << 12):
    """float64[2^n_free]: E(m) for every m, each sum taken over the terms in term order by np.sum."""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1)
    mask = np.asarray(mask, dtype=np.uint64).reshape(-1)
    clique = np.asarray(clique, dtype=np.int64).reshape(-1)
    size = 1 << n_free
    out = np.empty(size, dtype=np.float64)
    groups = [np.flatnonzero(clique == q) for q in range(-1, n_cliques)]
    for m0 in range(0, size, chunk):
        m = np.arange(m0, min(size, m0 + chunk), dtype=np.uint64)
        signed = coeff[None, :] * (1 - 2 * _parity(mask[None, :] & m[:, None]))
        s0 = np.sum(signed[:, groups[0]], axis=1)
        acc = np.zeros(m.size, dtype=np.float64)
        for idx in groups[1:]:
            si = np.sum(signed[:, idx], axis=1)
            acc = acc + si * si
        out[m0:m0 + m.size] = s0 - np.sqrt(acc)
    return out


def best_mask(energies):
    """the tie rule: the largest m among the entries that equal the minimum"""
    energies = np.asarray(energies)
    return int(np.flatnonzero(energies == energies.min())[-1])


def nu_of_mask(m, n_free):
    """eigenvalues of the free generators in generator order"""
    return np.array([-1 if (m >> (n_free - 1 - j)) & 1 else 1 for j in range(n_free)], dtype=np.int64)


def search_inputs(coeff, G_indices, C_indices, pauli_mult_signs, sector=None):
    """(c, mask, clique, free) of a recorded reconstruction.  sector: eigenvalues in {0, +1, -1} per generator, 0 = free (None: all free);
    a fixed -1 is folded into the sign of every term that uses the generator."""
    G = np.asarray(G_indices).astype(bool).reshape(len(coeff), -1)
    C = np.asarray(C_indices).astype(bool).reshape(len(coeff), -1)
    assert np.all(C.sum(axis=1) <= 1), 'a term lies in more than one clique'
    g = G.shape[1]
    sector = np.zeros(g, dtype=np.int64) if sector is None else np.asarray(sector).astype(np.int64)
    free = np.flatnonzero(sector == 0)
    c = np.asarray(coeff).real.astype(np.float64) * np.asarray(pauli_mult_signs).astype(np.float64)
    c = c * (1 - 2 * (np.count_nonzero(G[:, sector == -1], axis=1) & 1))
    f = free.size
    mask = np.zeros(len(c), dtype=np.uint64)
    for j, col in enumerate(free):
        mask |= G[:, col].astype(np.uint64) << np.uint64(f - 1 - j)
    clique = np.where(C.any(axis=1), np.argmax(C, axis=1) if C.shape[1] else 0, -1).astype(np.int32)
    return c, mask, clique, free


def solve(coeff, G_indices, C_indices, pauli_mult_signs, sector=None):
    """(energy, nu, energies): the reference's brute-force answer from its own recorded reconstruction"""
    c, mask, clique, free = search_inputs(coeff, G_indices, C_indices, pauli_mult_signs, sector)
    n_cliques = np.asarray(C_indices).reshape(len(c), -1).shape[1]
    energies = landscape(c, mask, clique, free.size, n_cliques)
    m = best_mask(energies)
    g = np.asarray(G_indices).reshape(len(c), -1).shape[1]
    nu = np.ones(g, dtype=np.int64) if sector is None else np.asarray(sector).astype(np.int64).copy()
    nu[free] = nu_of_mask(m, free.size)
    return float(energies[m]), nu, energies


def unique_minimum(energies, coeff):
    """True iff the gap between the best and the second-best energy exceeds 1e-9 sum|c| (a single assignment: trivially unique)"""
    e = np.sort(np.asarray(energies))
    return e.size == 1 or bool(e[1] - e[0] > 1e-9 * float(np.sum(np.abs(np.asarray(coeff).real))))


def product_signs(terms, gens, selection):
    """int8[T]: the sign of the product, in generator order from the identity, of the rows of ``gens`` that row k of ``selection`` picks,
    +-1 where it is +- ``terms[k]`` and 0 where the row differs or the phase is +-i — the phase rule
    e = 3 (Y_a + Y_b) + Y_out + 2 |x_a & z_b| mod 4 of a product a * b, all terms at once, one generator after the other."""
    terms, gens, selection = np.asarray(terms, dtype=bool), np.asarray(gens, dtype=bool), np.asarray(selection, dtype=bool)
    T, n = terms.shape[0], terms.shape[1] // 2
    ax, az, e = np.zeros((T, n), dtype=bool), np.zeros((T, n), dtype=bool), np.zeros(T, dtype=np.int64)
    for j in range(gens.shape[0]):
        pick = selection[:, j]
        bx, bz = gens[j, :n][None, :], gens[j, n:][None, :]
        ox, oz = ax ^ bx, az ^ bz
        step = (3 * (np.count_nonzero(ax & az, axis=1) + np.count_nonzero(bx & bz)) + np.count_nonzero(ox & oz, axis=1)
                + 2 * np.count_nonzero(ax & bz, axis=1))
        e = np.where(pick, e + step, e)
        ax, az = np.where(pick[:, None], ox, ax), np.where(pick[:, None], oz, az)
    same = np.all(np.hstack([ax, az]) == terms, axis=1)
    return np.where(same & (e % 2 == 0), 1 - (e % 4), 0).astype(np.int8)
