"""Task builders of tests/test_gpu_threads_statevector.py: the dense-statevector features — batched expval, matvec / exact_gs_energy,
AnsatzPlan / pool_gradient / VQE_Driver, rdm_dev, the sampler and the basis layer, sampled_expval, from_matrix, the clique colouring, the
noncontextual search — each as one task a worker thread runs over and over beside the other workers.

Every task has two halves.  X_case(rng, w) is the oracle half: worker w's inputs, their shapes, the forms those shapes reach, and the
expected result from the feature's own oracle module (tests/_*_oracle.py); it touches neither the library nor a device, and
tests/test_thread_tasks.py runs it alone.  make_X(rng, w) is the device half, run on the main thread before any worker starts: it makes
the call once, serially, holds the result to the oracle exactly as the feature's single-thread test does (equality for dyadic inputs,
otherwise the a-priori bound of the oracle module; no tolerance is defined here), keeps the serial result's BYTES, and returns run().
run() repeats the call and asserts those bytes: the features are bit-reproducible by contract, so a concurrent call returns what the
serial call returned.  run() returns the labels of the forms it saw ('rdm:TILED', ...), read from the calls' own form / info words.

No task reads or writes os.environ.  Forms are reached by shape alone; the rules are restated below from include/symgpu.h (f7 - f10) and
DESIGN.md 3.14 - 3.17, not imported from the library, and the shapes of the workers sit on both sides of every rule a shape can cross.
At most 13 qubits, a few hundred terms, 20,000 shots; every seed is explicit.  Test infrastructure only."""
from types import SimpleNamespace

import numpy as np

import _ansatz_oracle as ao
import _clique_oracle as co
import _expval_oracle as eo
import _matvec_oracle as mo
import _noncon_oracle as no
import _pauli_decomp_oracle as pdo
import _rdm_oracle as ro
import _sample_oracle as so
import _sparse_oracle as spo
import _statevector_families as sf

GS_TOL = 1e-10                    # TOL of tests/test_gpu_exact_gs.py (the GPU module asserts that the two are one number)
MAX_QUBITS, MAX_TERMS, MAX_SHOTS = 13, 400, 20_000


# ---- the shape rules, restated ---------------------------------------------------------------------------------------------------------
def expval_form(S, n):
    """csrc/expval.hip: phi's coefficients (16 bytes), X halves (8 Wq bytes) and the look-up table (4 bytes a slot; a power of two of
    slots, at least 2 S and 64) are staged in LDS while they fit 64 KiB; otherwise they stay in memory."""
    cap = 64
    while cap < 2 * S:
        cap *= 2
    return 'LDS' if S * (16 + 8 * ((n + 63) // 64)) + 4 * cap <= 65536 else 'GLOBAL'


def rdm_form(k):
    """f9: up to 3 kept qubits stream the vector once (STREAM); from 4 on the matrix is built tile by tile (TILED)."""
    return 'STREAM' if k <= 3 else 'TILED'


def sort_passes(m):
    """f10: P, the bytes of m - 1: the 8-bit passes of a radix sort over sample indices below m."""
    bits = 1
    while (1 << bits) < m:
        bits += 1
    return (bits + 7) // 8


def sample_form(m, n_samples):
    """f10: the counting form compares bytes moved: HIST where 28 m + 8 n_samples <= 24 P n_samples."""
    return 'HIST' if 28 * m + 8 * n_samples <= 24 * sort_passes(m) * n_samples else 'SORT'


def basis_tile_groups(n, measured_qubits):
    """f10: the measured index bits (qubit q is bit n-1-q) go, ascending, into groups; a group's tile is the 4 lowest index bits and its
    measured bits while it holds at most 2^12 amplitudes.  Returns the number of groups (passes over the vector)."""
    bits = sorted(n - 1 - int(q) for q in measured_qubits)
    budget, low = min(n, 12), set(range(min(n, 4)))
    groups, at = 0, 0
    while at < len(bits):
        tile = set(low)
        groups += 1
        while at < len(bits) and len(tile | {bits[at]}) <= budget:
            tile.add(bits[at])
            at += 1
    return groups


def ansatz_forms(symp):
    """f8: the forms a full-range apply reports: DIRECT alone when no generator fits a tile, else one bit per kind of segment."""
    segs = ao.plan_runs(symp)
    if not segs:
        return set()
    if not any(s[3] for s in segs):
        return {'DIRECT'}
    return {'TILED' if s[3] else 'DIRECT' for s in segs}


def noncon_blocks(n_free, low_bits):
    """csrc/noncon.hip: the assignment bits above the L low ones are strided over 2^(n_free - L) blocks."""
    return 1 << (n_free - min(n_free, low_bits))


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------------
def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


def unit(v):
    return v / np.linalg.norm(v)


def dyadic_coeff(rng, t, real=False):
    """Integers in [-64, 64] over 8 (sf.COEFF_SCALE), both components."""
    re = rng.integers(-64, 65, t) / float(sf.COEFF_SCALE)
    return re if real else re + 1j * rng.integers(-64, 65, t) / float(sf.COEFF_SCALE)


def dyadic_vector(rng, count, nonzero=False):
    """Integers in [-8, 8] over 16 (sf.AMP_SCALE), both components; nonzero: the imaginary part is at least 1/16."""
    return (rng.integers(-8, 9, count) + 1j * rng.integers(1 if nonzero else -8, 9, count)) / float(sf.AMP_SCALE)


def bits_of_index(idx, n):
    return ((np.asarray(idx, dtype=np.int64)[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8)


def as_bits(a):
    return np.ascontiguousarray(a, dtype=np.complex128).view(np.uint64)


def float_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the oracle halves -----------------------------------------------------------------------------------------------------------------
def expval_case(rng, w):
    """A dyadic real-coefficient operator on a dyadic state of S distinct basis strings: even workers keep S (16 + 8) + 4 cap within 64 KiB
    (LDS), odd workers go past S = 2048, where the table alone takes 32 KiB (GLOBAL)."""
    n, S = (11, 700 + 97 * w) if w % 2 == 0 else (12, 2049 + 61 * w)
    T = 10 + w
    symp = rng.random((T, 2 * n)) < 0.3
    coeff = dyadic_coeff(rng, T, real=True)
    idx = np.sort(rng.choice(1 << n, S, replace=False))
    bits, amp = bits_of_index(idx, n), dyadic_vector(rng, S, nonzero=True)
    elements = eo.term_elements(symp, bits, amp, bits, amp)
    return SimpleNamespace(shape=(n, T, S), forms={'expval:' + expval_form(S, n)}, dyadic=(coeff, n, amp), n=n, symp=symp, coeff=coeff, bits=bits,
                           amp=amp, elements=elements, total=eo.total(coeff, elements))


def matvec_case(rng, w):
    """A dyadic operator whose terms share a dozen X-parts, on a dyadic vector."""
    n, T = 9 + w % 4, 40 + 7 * w
    x_parts = rng.random((12, n)) < 0.3
    symp = np.hstack([x_parts[rng.integers(0, 12, T)], rng.random((T, n)) < 0.4])
    coeff, v = dyadic_coeff(rng, T), dyadic_vector(rng, 1 << n)
    return SimpleNamespace(shape=(n, T), forms={'matvec:DIRECT'}, dyadic=(coeff, n, v), n=n, symp=symp, coeff=coeff, v=v, want=mo.matvec(symp, coeff, v))


def hopping_operator(rng, n, scale):
    """sum_q a_q Z_q + sum_q t_q (X_q X_q+1 + Y_q Y_q+1): Hermitian, and it commutes with the number operator sum_q (1 - Z_q) / 2."""
    symp = np.zeros((n, 2 * n), dtype=bool)
    symp[:, n:] = np.eye(n, dtype=bool)
    coeff = list(rng.standard_normal(n))
    for q in range(n - 1):
        pair = np.zeros((2, 2 * n), dtype=bool)
        pair[:, [q, q + 1]] = True
        pair[1, [n + q, n + q + 1]] = True
        symp, coeff = np.vstack([symp, pair]), coeff + [0.5 * (q + 1) * scale] * 2
    return symp, np.array(coeff)


def exact_gs_case(rng, w):
    """Odd workers: the two-particle sector of a hopping operator (sector_mask, masked Lanczos steps); even workers: the whole space.
    max_basis is explicit — the default reads the free device memory, which the other threads change — and small enough to restart."""
    n, sector = 5 + w % 3, 2 if w % 2 else None
    symp, coeff = hopping_operator(rng, n, 1.0 + 0.1 * w)
    dense = spo.to_dense(symp, coeff)
    weight = np.array([bin(b).count('1') for b in range(1 << n)])
    idx = np.arange(1 << n) if sector is None else np.flatnonzero(weight == sector)
    lowest = float(np.linalg.eigvalsh(dense[np.ix_(idx, idx)])[0])
    return SimpleNamespace(shape=(n, sector, 8 + w), forms=set(), n=n, symp=symp, coeff=coeff, sector=sector, max_basis=8 + w, lowest=lowest,
                           weight=weight, R=2 * GS_TOL * float(np.abs(coeff).sum()))


def excitation_rows(rng, n, K):
    """K strings of 2 or 4 X/Y positions with stray Z's elsewhere, as tests/_statevector_families.py draws its generators."""
    rows = []
    for _ in range(K):
        pos = rng.choice(n, int(rng.choice([2, 4])), replace=False)
        x, z = np.zeros(n, dtype=bool), rng.random(n) < 0.08
        x[pos], z[pos] = True, rng.random(len(pos)) < 0.5
        rows.append(np.concatenate([x, z]))
    return np.array(rows, dtype=bool)


def ansatz_case(rng, w):
    """Even workers: 13 qubits with one generator of 13 X/Y positions in the middle — 4 low tile bits and 13 X bits exceed the budget of 12,
    so it takes a direct pass between two tiled runs.  Odd workers: 10 .. 12 qubits, where the budget is n and every generator fits.
    The pool gradient has a small problem of its own: its oracle needs the dense H."""
    wide = w % 2 == 0
    n, K = (13, 5 + w) if wide else (10 + (w // 2) % 3, 5 + w)
    symp = excitation_rows(rng, n, K)
    if wide:
        symp[K // 2] = np.concatenate([np.ones(n, dtype=bool), rng.random(n) < 0.5])
    theta, ref = rng.uniform(-np.pi, np.pi, K), unit(gaussian(rng, 1 << n))
    T = 6 + w % 3
    h_symp, h_coeff = rng.random((T, 2 * n)) < 0.3, rng.standard_normal(T)
    state = ao.state(symp, theta, ref)
    n_p, J, T_p = 7 + w % 3, 3 + w, 8
    p_h_symp, p_h_coeff = rng.random((T_p, 2 * n_p)) < 0.4, rng.standard_normal(T_p)
    pool, p_psi = rng.random((J, 2 * n_p)) < 0.4, unit(gaussian(rng, 1 << n_p))
    return SimpleNamespace(shape=(n, K, n_p, J), forms={'ansatz:' + f for f in ansatz_forms(symp)}, n=n, symp=symp, theta=theta, ref=ref, h_symp=h_symp,
                           h_coeff=h_coeff, state=state, back=ao.state(symp, theta, state, inverse=True),
                           energy=ao.energy_at(h_symp, h_coeff, symp, theta, ref), grad=ao.grad_shift(h_symp, h_coeff, symp, theta, ref),
                           R=ao.bound(n, K, T, h_coeff), n_p=n_p, p_h_symp=p_h_symp, p_h_coeff=p_h_coeff, pool=pool, p_psi=p_psi,
                           pool_grad=ao.pool_grad(ao.dense_operator(p_h_symp, p_h_coeff), pool, p_psi), pool_energy=ao.energy(p_h_symp, p_h_coeff, p_psi),
                           R_p=ao.bound(n_p, J, T_p, p_h_coeff))


def vqe_case(rng, w):
    """A driver of the worker's own: one energy and one gradient at fixed angles."""
    n, K, T = 6 + w % 3, 4 + w, 10 + w
    h_symp, h_coeff = rng.random((T, 2 * n)) < 0.4, rng.standard_normal(T)
    gens = rng.random((K, 2 * n)) < 0.5
    gens[:, 0] = True                                               # no identity row: the driver would drop it
    ref, x = unit(gaussian(rng, 1 << n)), rng.uniform(-np.pi, np.pi, K)
    return SimpleNamespace(shape=(n, K, T), forms=set(), n=n, h_symp=h_symp, h_coeff=h_coeff, gens=gens, ref=ref, x=x,
                           energy=ao.energy_at(h_symp, h_coeff, gens, x, ref), grad=ao.grad_shift(h_symp, h_coeff, gens, x, ref), R=ao.bound(n, K, T, h_coeff))


def rdm_case(rng, w):
    """k = 1 .. 6 kept qubits by worker: STREAM up to 3, TILED beyond.  Dyadic amplitudes (integers over 8, as tests/test_gpu_rdm.py
    draws them): every product and sum is exact."""
    n, k = 9 + w % 4, 1 + w % 6
    kept = sorted(int(q) for q in rng.choice(n, k, replace=False))
    psi = (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / 8.0
    small = kept if k <= n - k else sorted(set(range(n)) - set(kept))           # get_entanglement_entropy takes the smaller side
    tol_small = ro.entry_tolerance(psi, n, small)
    return SimpleNamespace(shape=(n, tuple(kept)), forms={'rdm:' + rdm_form(k), 'rdm:' + rdm_form(len(small))}, n=n, kept=kept, psi=psi,
                           rho=ro.rdm_deposit(psi, n, kept), tol=ro.entry_tolerance(psi, n, kept), small=small,
                           entropy=ro.entropy(ro.rdm_deposit(psi, n, small)), entropy_tol=ro.entropy_tolerance(tol_small))


def sample_case(rng, w):
    """Two plans a worker, one per counting form: many draws from few amplitudes (HIST) and few draws from 13 qubits' worth (SORT), the
    second from beyond draw 2^40 of its stream.  so.dyadic_amplitudes: the total is a power of two, every partial sum exact."""
    seed = 1000 + w
    pairs = []
    for m, S, first in ((64 + 3 * w, 5000 + 11 * w, 3 + w), (8192 - 5 * w, 100 + w, (1 << 40) + 1 + w)):
        amp = so.dyadic_amplitudes(rng, m)
        levels = so.tree_build(so.weights(amp))
        order = so.tree_walk(levels, so.philox_uniforms(seed, first, S))
        pairs.append(SimpleNamespace(m=m, S=S, first=first, amp=amp, total=levels[-1][0], depth=len(levels) - 1, order=order, counts=so.counts_of(order),
                                     form=sample_form(m, S)))
    u_first, u_count = (1 << 40) + 5 + w, 4099 + w
    return SimpleNamespace(shape=tuple((p.m, p.S) for p in pairs), forms={'sample:' + p.form for p in pairs}, seed=seed, pairs=pairs, u_first=u_first,
                           u_count=u_count, uniforms=so.numpy_uniforms(seed, u_first, u_count))


def basis_case(rng, w):
    """Even workers: 13 qubits, every one measured — nine measured index bits above bit 3, one more than a tile takes beside the four low
    bits: two groups.  Odd workers: six measured qubits of 9 .. 12: one group.  Gaussian amplitudes with zeros (their signs are bytes)."""
    if w % 2 == 0:
        n = 13
        measured = np.arange(n)
    else:
        n = 9 + w // 2
        measured = np.sort(rng.choice(n, 6, replace=False))
    is_y = rng.random(len(measured)) < 0.5
    xs, ys = [int(q) for q in measured[~is_y]], [int(q) for q in measured[is_y]]
    psi = gaussian(rng, 1 << n)
    psi[rng.integers(0, 1 << n, (1 << n) // 8)] = 0
    return SimpleNamespace(shape=(n, tuple(xs), tuple(ys)), forms={'basis:TILED'}, groups=basis_tile_groups(n, measured), n=n, xs=xs, ys=ys, psi=psi,
                           want=so.basis_change(psi, n, xs, ys))


def sampled_expval_case(rng, w):
    """Even workers: 6 qubits and thousands of shots (every clique's draw counts by HIST); odd workers: 12 qubits and a hundred shots (SORT).
    Also a small normalised state for QuantumState.sample_state / sample_counts."""
    n, shots = (6, 5000 + 13 * w) if w % 2 == 0 else (12, 100 + w)
    T, seed = 12 + w, 2000 + w
    codes = rng.permutation(np.unique(rng.integers(1, 1 << (2 * n), 4 * T)))[:T]       # distinct rows, none the identity
    assert len(codes) == T
    symp = ((codes[:, None] >> np.arange(2 * n)) & 1).astype(bool)
    coeff, amp = rng.standard_normal(T), unit(gaussian(rng, 1 << n))
    order = co.term_order(symp, coeff, 'QWC', 'largest_first')
    colours = co.colouring(symp, order, 'QWC')[0]
    members = co.cliques_in_order(colours, order)
    sums = so.sampled_sums(symp, n, amp, members, shots, seed)
    # the small state: distinct rows in ascending index order
    n_s, rows_s, draws = 6, 16 + w, 3000 + 7 * w
    idx = np.sort(rng.choice(1 << n_s, rows_s, replace=False))
    amp_s = unit(gaussian(rng, rows_s))
    uniforms = so.philox_uniforms(seed, 0, draws)
    dense = np.zeros(1 << n_s, dtype=np.complex128)
    dense[idx] = amp_s
    return SimpleNamespace(shape=(n, T, shots, rows_s), forms=set(), count_form=sample_form(1 << n, shots), n=n, shots=shots, seed=seed, symp=symp,
                           coeff=coeff, amp=amp, colours=colours, sums=sums, value=complex(np.sum(coeff.astype(complex) * (sums / shots))).real,
                           n_s=n_s, bits_s=bits_of_index(idx, n_s), amp_s=amp_s, draws=draws,
                           state_counts=np.bincount(so.draw(amp_s, uniforms), minlength=rows_s), dense_counts=so.counts_of(so.draw(dense, uniforms)))


def from_matrix_case(rng, w):
    """A dyadic matrix of 2 + w XOR-diagonals (entries integers over 8, three in ten zero), dense and as canonical CSR arrays."""
    n, d = 3 + w % 4, 2 + w
    side = 1 << n
    xs = rng.choice(side, d, replace=False)
    b = np.arange(side)
    matrix = np.zeros((side, side), dtype=np.complex128)
    for x in xs:
        entries = (rng.integers(-8, 9, side) + 1j * rng.integers(-8, 9, side)) / 8.0
        entries[rng.random(side) < 0.3] = 0
        matrix[b, b ^ x] = entries
    rows, cols = np.nonzero(matrix)                                  # row-major: the columns of a row ascend
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=side))]).astype(np.int32)
    return SimpleNamespace(shape=(n, d), forms={'pauli:ONE_PASS'}, n=n, matrix=matrix, data=matrix[rows, cols], indices=cols.astype(np.int32), indptr=indptr,
                           want=pdo.decompose(matrix, n))


def clique_case(rng, w):
    """230 + 12 w terms: up to worker 2 one block of 256 positions of the order, from worker 3 on two.  QWC (colour unions) and one of C / AC
    (pairs), a random order each; the QWC degrees, and the QWC table of the first 40 terms against all."""
    T, n = 230 + 12 * w, 6 + w % 3
    symp = rng.random((T, 2 * n)) < 0.4
    other = 'C' if w % 2 else 'AC'
    orders = {'QWC': rng.permutation(T), other: rng.permutation(T)}
    return SimpleNamespace(shape=(T, n), forms={'clique:UNIONS', 'clique:PAIRS'}, T=T, n=n, symp=symp, other=other, orders=orders,
                           colourings={rel: co.colouring(symp, order, rel) for rel, order in orders.items()}, degrees=co.degrees(symp, 'QWC'),
                           qwc_head=co.relation_table(symp[:40], symp, 'QWC'))


def noncon_case(rng, w):
    """The signs and the search of the smallest recorded case (the fewest terms; the first of those), and a search of the worker's own
    size: 3 .. 6 free generators, two cliques."""
    tag, case = min(no.golden_cases(), key=lambda tc: tc[1]['symp'].shape[0])
    gens = np.vstack([case['generators'], case['cliques']])
    selection = np.hstack([case['G_indices'], case['C_indices']]).astype(bool)
    c, mask, clique, free = no.search_inputs(case['coeff'], case['G_indices'], case['C_indices'], case['pauli_mult_signs'])
    n_cliques = np.asarray(case['C_indices']).reshape(len(c), -1).shape[1]
    T, f, Q = 40 + 3 * w, 3 + w % 4, 2
    own = (rng.standard_normal(T), rng.integers(0, 1 << f, T, dtype=np.uint64), rng.integers(-1, Q, T).astype(np.int32))
    return SimpleNamespace(shape=(T, f), forms=set(), tag=tag, terms=np.asarray(case['symp'], dtype=bool), gens=np.asarray(gens, dtype=bool),
                           selection=selection, signs=np.asarray(case['pauli_mult_signs']), search=(c, mask, clique, free.size, n_cliques),
                           landscape=no.landscape(c, mask, clique, free.size, n_cliques), energy=float(case['energy']), tol=no.tolerance(c),
                           own=own, own_f=f, own_Q=Q, own_landscape=no.landscape(*own, f, Q), own_tol=no.tolerance(own[0]))


def plan_churn_case(rng, w):
    """What four rounds of building and dropping a MatvecPlan, an AnsatzPlan, a SamplePlan and a DeviceBuffer each compute once."""
    n, T, K, m, S = 8 + w % 3, 30 + w, 4, 100 + w, 500 + w
    symp, coeff, v = rng.random((T, 2 * n)) < 0.3, dyadic_coeff(rng, T), dyadic_vector(rng, 1 << n)
    gens, theta = excitation_rows(rng, n, K), rng.uniform(-np.pi, np.pi, K)
    amp = so.dyadic_amplitudes(rng, m)
    order = so.tree_walk(so.tree_build(so.weights(amp)), so.philox_uniforms(w, 0, S))
    return SimpleNamespace(shape=(n, T, m), forms=set(), dyadic=(coeff, n, v), n=n, symp=symp, coeff=coeff, v=v, hv=mo.matvec(symp, coeff, v), gens=gens,
                           theta=theta, state=ao.state(gens, theta, v), amp=amp, S=S, seed=w, counts=so.counts_of(order))


CASES = {'expval': expval_case, 'matvec': matvec_case, 'exact_gs': exact_gs_case, 'ansatz': ansatz_case, 'vqe': vqe_case, 'rdm': rdm_case,
         'sample': sample_case, 'basis': basis_case, 'sampled_expval': sampled_expval_case, 'from_matrix': from_matrix_case, 'clique': clique_case,
         'noncon': noncon_case, 'plan_churn': plan_churn_case}

# every form a shape of at most 13 qubits reaches; the module docstring of the GPU file lists the forms only the environment reaches
REQUIRED_FORMS = {'expval:LDS', 'expval:GLOBAL', 'matvec:DIRECT', 'ansatz:DIRECT', 'ansatz:TILED', 'rdm:STREAM', 'rdm:TILED', 'sample:HIST', 'sample:SORT',
                  'basis:TILED', 'pauli:ONE_PASS', 'clique:PAIRS', 'clique:UNIONS'}


def worker_rng(n_workers, w, name):
    """One generator per (run size, worker, task): a failing task is reproduced from those three alone."""
    return np.random.default_rng([9100, n_workers, w, sorted(CASES).index(name)])


# ---- the device halves -----------------------------------------------------------------------------------------------------------------
# (symmer_amd is imported inside the builders: the oracle halves above load neither the package nor the library)
def _upload_rows(symp):
    from symmer_amd import kernels, packing
    return kernels.DeviceOp.upload(packing.pack_rows(np.asarray(symp, dtype=bool)))


def make_expval(rng, w):
    from symmer_amd import PauliwordOp, QuantumState, kernels
    from symmer_amd.operators import term_expvals
    from symmer_amd.operators.quantum_state import _expval_call
    c = expval_case(rng, w)
    code = {kernels.EXPVAL_LDS: 'expval:LDS', kernels.EXPVAL_GLOBAL: 'expval:GLOBAL'}

    def call():
        H, psi = PauliwordOp(c.symp, c.coeff), QuantumState(c.bits, c.amp)
        terms, total, form = _expval_call(H, psi, True)
        return terms, total, form, H.expval(psi), term_expvals(H, psi)
    terms, total, form, value, per_term = call()
    assert np.all(terms == c.elements), f'terms differ at {np.flatnonzero(terms != c.elements)[:8]}'       # dyadic: exact in any row order
    assert total == c.total and value == c.total.real and np.array_equal(per_term, c.elements.real)
    assert {code[form]} == c.forms, (form, c.forms)
    keep = (terms.tobytes(), total, form, float_bits(value).tobytes(), per_term.tobytes())

    def run():
        t, tot, f, val, per = call()
        assert (t.tobytes(), tot, f, float_bits(val).tobytes(), per.tobytes()) == keep, 'expval: other bytes than the serial call'
        return {code[f]}
    return run


def make_matvec(rng, w):
    from symmer_amd import PauliwordOp, kernels
    c = matvec_case(rng, w)

    def call():
        H = PauliwordOp(c.symp, c.coeff)
        with H._matvec_plan() as plan:
            through_plan, form = plan.matvec(c.v)
        return H.matvec(c.v), through_plan, form
    got, through_plan, form = call()
    assert np.array_equal(as_bits(got), as_bits(c.want)), 'H.matvec(v) is not bit-equal to the oracle'
    assert np.array_equal(as_bits(through_plan), as_bits(c.want)) and form == kernels.MATVEC_DIRECT
    keep = got.tobytes()

    def run():
        g, p, f = call()
        assert g.tobytes() == keep and p.tobytes() == keep and f == kernels.MATVEC_DIRECT, 'matvec: other bytes than the serial call'
        return {'matvec:DIRECT'}
    return run


def make_exact_gs(rng, w):
    from symmer_amd import PauliwordOp, exact_gs_energy
    from test_gpu_exact_gs import number_operator
    c = exact_gs_case(rng, w)

    def call():
        H = PauliwordOp(c.symp, c.coeff)
        if c.sector is None:
            return exact_gs_energy(H, max_basis=c.max_basis, return_array=True)
        return exact_gs_energy(H, n_particles=c.sector, number_operator=number_operator(c.n), max_basis=c.max_basis, return_array=True)
    E, psi = call()
    assert isinstance(E, float) and psi.shape == (1 << c.n,) and psi.dtype == np.complex128
    assert abs(np.linalg.norm(psi) - 1) <= ((1 << c.n) + 4) * 2.0 ** -53
    residual = np.linalg.norm(mo.matvec(c.symp, c.coeff, psi) - E * psi)
    assert residual <= c.R and abs(E - c.lowest) <= c.R, (E, c.lowest, residual, c.R)
    if c.sector is not None:
        assert np.all(c.weight[np.flatnonzero(psi)] == c.sector), 'an amplitude outside the sector'
    keep = (float_bits(E).tobytes(), psi.tobytes())

    def run():
        e, v = call()
        assert (float_bits(e).tobytes(), v.tobytes()) == keep, 'exact_gs_energy: other bytes than the serial call'
        return set()
    return run


def make_ansatz(rng, w):
    from symmer_amd import PauliwordOp, kernels
    c = ansatz_case(rng, w)
    side = 1 << c.n
    labels = lambda form: {name for bit, name in ((kernels.ANSATZ_DIRECT, 'ansatz:DIRECT'), (kernels.ANSATZ_TILED, 'ansatz:TILED')) if form & bit}

    def call():
        with _upload_rows(c.symp) as gens, kernels.AnsatzPlan(gens, c.n) as plan, PauliwordOp(c.h_symp, c.h_coeff)._matvec_plan() as plan_h, \
                kernels.DeviceBuffer.upload(c.ref) as ref, kernels.DeviceBuffer.upload(c.ref) as psi, kernels.DeviceBuffer(16 * side) as out:
            forward = plan.apply(c.theta, psi)
            state = psi.download(np.complex128, side)
            backward = plan.apply(c.theta, psi, inverse=True)
            back = psi.download(np.complex128, side)
            e, g = plan.energy_grad(plan_h, c.theta, ref, psi_out=out)
            prepared, ref_after = out.download(np.complex128, side), ref.download(np.complex128, side)
        with _upload_rows(c.pool) as pool, PauliwordOp(c.p_h_symp, c.p_h_coeff)._matvec_plan() as plan_p, kernels.DeviceBuffer.upload(c.p_psi) as p_psi:
            pg, pe = kernels.pool_gradient(plan_p, pool, p_psi, want_energy=True)
        return forward, backward, state, back, e, g, prepared, ref_after, pg, pe
    forward, backward, state, back, e, g, prepared, ref_after, pg, pe = call()
    assert labels(forward) == c.forms and labels(backward) == c.forms, (forward, backward, c.forms)
    assert np.array_equal(as_bits(state), as_bits(c.state)), 'apply: not the oracle state'
    assert np.array_equal(as_bits(back), as_bits(c.back)), 'apply(inverse=True): not the oracle state'
    assert np.array_equal(as_bits(prepared), as_bits(c.state)), 'psi_out is not the state of apply'
    assert np.array_equal(as_bits(ref_after), as_bits(c.ref)), 'the reference state was changed'
    assert abs(e - c.energy) <= c.R and g.shape == c.grad.shape and np.abs(g - c.grad).max() <= 2 * c.R, (e, c.energy, np.abs(g - c.grad).max(), c.R)
    assert pg.shape == c.pool_grad.shape and np.abs(pg - c.pool_grad).max() <= 2 * c.R_p and abs(pe - c.pool_energy) <= c.R_p
    keep = (forward, backward, state.tobytes(), back.tobytes(), float_bits(e).tobytes(), g.tobytes(), pg.tobytes(), float_bits(pe).tobytes())

    def run():
        fw, bw, st, bk, e_, g_, prep, ref_, pg_, pe_ = call()
        assert (fw, bw, st.tobytes(), bk.tobytes(), float_bits(e_).tobytes(), g_.tobytes(), pg_.tobytes(), float_bits(pe_).tobytes()) == keep, \
            'ansatz: other bytes than the serial call'
        assert prep.tobytes() == keep[2] and ref_.tobytes() == c.ref.tobytes()
        return labels(fw) | labels(bw)
    return run


def make_vqe(rng, w):
    from symmer_amd import PauliwordOp
    from symmer_amd.evolution import VQE_Driver
    c = vqe_case(rng, w)

    def call():
        vqe = VQE_Driver(PauliwordOp(c.h_symp, c.h_coeff), excitation_ops=PauliwordOp(c.gens, np.ones(len(c.gens))), ref_state=c.ref)
        return vqe.f(c.x), vqe.gradient(c.x)
    e, g = call()
    assert isinstance(e, float) and abs(e - c.energy) <= c.R and g.shape == c.grad.shape and np.abs(g - c.grad).max() <= 2 * c.R
    keep = (float_bits(e).tobytes(), g.tobytes())

    def run():
        e_, g_ = call()
        assert (float_bits(e_).tobytes(), g_.tobytes()) == keep, 'VQE_Driver: other bytes than the serial call'
        return set()
    return run


def make_rdm(rng, w):
    from symmer_amd import get_entanglement_entropy, kernels
    c = rdm_case(rng, w)
    code = {kernels.RDM_STREAM: 'rdm:STREAM', kernels.RDM_TILED: 'rdm:TILED'}

    def call():
        with kernels.DeviceBuffer.upload(c.psi) as buf:
            rho, info = kernels.rdm_dev(buf, c.n, c.kept, want_info=True)
            after = buf.download(np.complex128, 1 << c.n)
            _, info_small = kernels.rdm_dev(buf, c.n, c.small, want_info=True)
        return rho, info, after, get_entanglement_entropy(c.psi, c.kept), info_small
    rho, info, after, entropy, info_small = call()
    assert np.array_equal(rho, c.rho) and np.all(np.abs(rho - c.rho) <= c.tol)
    assert after.tobytes() == c.psi.tobytes(), 'psi was written'
    assert {code[int(info[0])], code[int(info_small[0])]} == c.forms, (info, info_small, c.forms)
    assert isinstance(entropy, float) and abs(entropy - c.entropy) <= c.entropy_tol, (entropy, c.entropy, c.entropy_tol)
    keep = (rho.tobytes(), info.tobytes(), float_bits(entropy).tobytes())

    def run():
        r, i, a, s, i_small = call()
        assert (r.tobytes(), i.tobytes(), float_bits(s).tobytes()) == keep and a.tobytes() == c.psi.tobytes(), 'rdm: other bytes than the serial call'
        return {code[int(i[0])], code[int(i_small[0])]}
    return run


def make_sample(rng, w):
    from symmer_amd import kernels
    c = sample_case(rng, w)
    code = {kernels.SAMPLE_HIST: 'sample:HIST', kernels.SAMPLE_SORT: 'sample:SORT'}

    def call():
        out = [kernels.philox_uniforms(c.seed, c.u_first, c.u_count)]
        for p in c.pairs:
            with kernels.DeviceBuffer.upload(p.amp) as buf, kernels.SamplePlan(buf) as plan:
                idx, count, order = plan.draw(p.S, seed=c.seed, first_draw=p.first, want_order=True)
                out.append((idx, count, order, plan.total, plan.info(), buf.download(np.complex128, p.m)))
        return out
    got = call()
    assert np.array_equal(float_bits(got[0]), float_bits(c.uniforms)), 'the uniforms are not NumPy\'s'
    for p, (idx, count, order, total, info, amp_after) in zip(c.pairs, got[1:]):
        assert total == p.total and info[0] == p.m and info[1] == p.depth
        assert np.array_equal(order, p.order) and np.array_equal(idx, p.counts[0]) and np.array_equal(count, p.counts[1])
        assert code[int(info[4])] == 'sample:' + p.form, (p.m, p.S, info)
        assert amp_after.tobytes() == p.amp.tobytes(), 'the amplitudes were written'
    keep = [got[0].tobytes()] + [(i.tobytes(), n.tobytes(), o.tobytes(), int(info[4])) for i, n, o, _, info, _ in got[1:]]

    def run():
        again = call()
        assert [again[0].tobytes()] + [(i.tobytes(), n.tobytes(), o.tobytes(), int(info[4])) for i, n, o, _, info, _ in again[1:]] == keep, \
            'sample: other bytes than the serial call'
        return {code[int(entry[4][4])] for entry in again[1:]}
    return run


def make_basis(rng, w):
    from symmer_amd import kernels
    c = basis_case(rng, w)

    def call():
        with kernels.DeviceBuffer.upload(c.psi) as buf:
            form = kernels.basis_change_dev(buf, c.n, c.xs, c.ys)
            return buf.download(np.complex128, 1 << c.n), form
    got, form = call()
    assert form == kernels.BASIS_TILED and got.tobytes() == c.want.tobytes(), np.flatnonzero(got != c.want)[:5]
    keep = got.tobytes()

    def run():
        g, f = call()
        assert g.tobytes() == keep and f == kernels.BASIS_TILED, 'basis_change: other bytes than the serial call'
        return {'basis:TILED'}
    return run


def make_sampled_expval(rng, w):
    from symmer_amd import PauliwordOp, QuantumState
    from symmer_amd.utils import sampled_expval
    c = sampled_expval_case(rng, w)

    def call():
        H, psi = PauliwordOp(c.symp, c.coeff), QuantumState.from_array(c.amp.reshape(-1, 1))
        value, terms, clique = sampled_expval(H, psi, c.shots, seed=c.seed, return_terms=True)
        small = QuantumState(c.bits_s, c.amp_s)
        sampled = small.sample_state(c.draws, seed=c.seed)
        return value, terms, clique, np.asarray(psi.to_dense_matrix).reshape(-1), sampled.state_op.coeff_vec, sampled.state_matrix, \
            small.sample_counts(c.draws, seed=c.seed)
    value, terms, clique, dense, counts, rows, (idx, count) = call()
    assert np.array_equal(dense, c.amp), 'from_array dropped an amplitude: the oracle ran on another vector'
    assert np.array_equal(clique, c.colours)
    assert np.array_equal(np.round(terms * c.shots).astype(np.int64), c.sums) and np.array_equal(terms, c.sums / c.shots)
    assert value == c.value
    assert np.array_equal(rows, c.bits_s) and np.all(counts.imag == 0) and np.array_equal(counts.real.astype(np.int64), c.state_counts)
    assert np.array_equal(idx, c.dense_counts[0]) and np.array_equal(count, c.dense_counts[1]) and idx.dtype == count.dtype == np.int64
    keep = (float_bits(value).tobytes(), terms.tobytes(), clique.tobytes(), counts.tobytes(), idx.tobytes(), count.tobytes())

    def run():
        v, t, q, _, n_, _, (i, k) = call()
        assert (float_bits(v).tobytes(), t.tobytes(), q.tobytes(), n_.tobytes(), i.tobytes(), k.tobytes()) == keep, \
            'sampled_expval / sample_state: other bytes than the serial call'
        assert np.array_equal(np.round(t * c.shots).astype(np.int64), c.sums)
        return set()
    return run


def make_from_matrix(rng, w):
    from symmer_amd import PauliwordOp, kernels
    c = from_matrix_case(rng, w)
    x, z, coeff = c.want
    want_symp = pdo.symp_of(x, z, c.n)

    def call():
        out = []
        for dev, t, form in (kernels.pauli_decompose_dense(c.matrix, c.n), kernels.pauli_decompose_csr(c.data, c.indices, c.indptr, c.n)):
            op = PauliwordOp._from_device(dev, c.n, t)
            out.append((np.array(op.symp_matrix), np.array(op.coeff_vec, dtype=np.complex128), form))
        return out
    got = call()
    for symp, cf, form in got:
        assert symp.shape == want_symp.shape and np.array_equal(symp, want_symp) and pdo.bits_equal(cf, coeff), 'not the restated decomposition'
        assert form == kernels.PAULI_ONE_PASS
    keep = [(s.tobytes(), cf.tobytes(), f) for s, cf, f in got]

    def run():
        assert [(s.tobytes(), cf.tobytes(), f) for s, cf, f in call()] == keep, 'from_matrix: other bytes than the serial call'
        return {'pauli:ONE_PASS'}
    return run


def make_clique(rng, w):
    from symmer_amd import kernels
    c = clique_case(rng, w)
    code = {kernels.CLIQUE_PAIRS: 'clique:PAIRS', kernels.CLIQUE_UNIONS: 'clique:UNIONS'}

    def call():
        with _upload_rows(c.symp) as op, _upload_rows(c.symp[:40]) as head:
            out = {rel: kernels.clique_colouring_dev(op, kernels.RELATIONS[rel], order, want_info=True) for rel, order in c.orders.items()}
            return out, kernels.relation_degrees_dev(op, kernels.REL_QWC), kernels.qwc_handles(head, op)
    got, degrees, table = call()
    for rel, (colours, n_colours, info) in got.items():
        want, want_n = c.colourings[rel]
        assert n_colours == want_n and np.array_equal(colours, want), f'{rel}: colours differ at terms {np.flatnonzero(colours != want)[:8]}'
        assert code[int(info[0])] == ('clique:UNIONS' if rel == 'QWC' else 'clique:PAIRS') and info[1] == (c.T + info[2] - 1) // info[2]
    assert np.array_equal(degrees, c.degrees) and np.array_equal(table, c.qwc_head)
    keep = ([(rel, col.tobytes(), k, info.tobytes()) for rel, (col, k, info) in got.items()], degrees.tobytes(), table.tobytes())

    def run():
        g, d, t = call()
        assert ([(rel, col.tobytes(), k, info.tobytes()) for rel, (col, k, info) in g.items()], d.tobytes(), t.tobytes()) == keep, \
            'clique: other bytes than the serial call'
        return {code[int(info[0])] for _, _, info in g.values()}
    return run


def make_noncon(rng, w):
    from symmer_amd import kernels
    c = noncon_case(rng, w)

    def call():
        with _upload_rows(c.terms) as t, _upload_rows(c.gens) as g:
            signs = kernels.noncon_signs_dev(t, g, c.selection)
        return signs, kernels.noncon_search(*c.search, want_energies=True, want_info=True), \
            kernels.noncon_search(*c.own, c.own_f, c.own_Q, want_energies=True, want_info=True)
    signs, recorded, own = call()
    assert signs.dtype == np.int8 and np.array_equal(signs, c.signs), f'case {c.tag}: signs differ from the reference'
    for (energy, best, energies, info), want, tol, f in ((recorded, c.landscape, c.tol, c.search[3]), (own, c.own_landscape, c.own_tol, c.own_f)):
        assert energies.shape == want.shape and np.max(np.abs(energies - want)) <= tol
        assert energy == energies[best] and best == no.best_mask(energies) and want[best] <= want.min() + tol
        assert info[1] == noncon_blocks(f, int(info[0]))
    assert abs(recorded[0] - c.energy) <= c.tol, (recorded[0], c.energy, c.tol)
    keep = (signs.tobytes(),) + tuple((float_bits(r[0]).tobytes(), r[1], r[2].tobytes(), r[3].tobytes()) for r in (recorded, own))

    def run():
        s, a, b = call()
        assert (s.tobytes(),) + tuple((float_bits(r[0]).tobytes(), r[1], r[2].tobytes(), r[3].tobytes()) for r in (a, b)) == keep, \
            'noncon: other bytes than the serial call'
        return set()
    return run


def make_plan_churn(rng, w):
    """Plans and buffers built, used once and dropped inside a reference cycle: the garbage collector frees them, on whichever thread
    runs it, as tests/test_gpu_threads.py make_handle_churn does with operators."""
    from symmer_amd import kernels, packing
    c = plan_churn_case(rng, w)
    side = 1 << c.n
    rows, gen_rows = packing.pack_rows(c.symp), packing.pack_rows(c.gens)

    def one_round():
        with kernels.DeviceOp.upload(rows, c.coeff) as op, kernels.DeviceOp.upload(gen_rows) as gens:
            matvec, ansatz = kernels.MatvecPlan(op, c.n), kernels.AnsatzPlan(gens, c.n)        # the plans outlive their operators
        sample = kernels.SamplePlan(c.amp)                                                       # it owns the upload of its amplitudes
        x, y = kernels.DeviceBuffer.upload(c.v), kernels.DeviceBuffer(16 * side)
        matvec.apply(x, y)
        hv = y.download(np.complex128, side)
        ansatz.apply(c.theta, x)
        state = x.download(np.complex128, side)
        idx, count = sample.draw(c.S, seed=c.seed)
        junk = {'plans': (matvec, ansatz, sample), 'buffers': (x, y)}
        junk['self'] = junk                                          # a reference cycle: nothing here is freed by hand
        return junk, (hv, state, idx, count)
    _, (hv, state, idx, count) = one_round()
    assert np.array_equal(as_bits(hv), as_bits(c.hv)) and np.array_equal(as_bits(state), as_bits(c.state))
    assert np.array_equal(idx, c.counts[0]) and np.array_equal(count, c.counts[1])
    keep = tuple(a.tobytes() for a in (hv, state, idx, count))

    def run():
        held = []
        for _ in range(4):
            junk, results = one_round()
            assert tuple(a.tobytes() for a in results) == keep, 'plan churn: other bytes than the serial call'
            held.append(junk)
        assert held[-1]['buffers'][1].download(np.complex128, side).tobytes() == keep[0]
        held.clear()
        return set()
    return run


TASKS = {'expval': make_expval, 'matvec': make_matvec, 'exact_gs': make_exact_gs, 'ansatz': make_ansatz, 'vqe': make_vqe, 'rdm': make_rdm,
         'sample': make_sample, 'basis': make_basis, 'sampled_expval': make_sampled_expval, 'from_matrix': make_from_matrix, 'clique': make_clique,
         'noncon': make_noncon, 'plan_churn': make_plan_churn}
