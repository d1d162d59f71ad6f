"""Seeded inputs for the third sweep (tests/test_gpu_fuzz3.py) over the dense-statevector features — to_sparse_matrix / from_matrix, batched
expval, matvec / exact_gs_energy, AnsatzPlan / pool_gradient, rdm_dev — and the identities that tie those features to one another, written
once in NumPy on the oracles each feature already has (tests/_*_oracle.py).  tests/test_statevector_families.py holds the identities on
the oracles alone and asserts what the committed seed lists cover; the GPU file holds the device to the same identities.

Every draw comes from np.random.default_rng(BASE[family] + seed): a failing case is reproduced by its family and seed alone.

Exactness.  A dyadic case has coefficients that are integers over COEFF_SCALE = 8 (both components) and amplitudes that are integers in
[-8, 8] over AMP_SCALE = 16 (both components).  Every quantity the identities form is then a sum of integers over a power of two, and
with  sum_k (|Re c_k| + |Im c_k|) 8 . 8 . 8 . 2 . 2^n < 2^52  (`assert_dyadic_is_exact`) every partial sum, in any order, is an exact
double: the two sides of an identity are EQUAL, not close.  Gaussian cases hold within the sum of the two sides' a-priori bounds, each taken
from the oracle module of the feature; no tolerance is defined here.  Test infrastructure only."""
from types import SimpleNamespace

import numpy as np

import _ansatz_oracle as ao
import _expval_oracle as eo
import _matvec_oracle as mo
import _pauli_decomp_oracle as pdo
import _rdm_oracle as ro
import _sparse_oracle as so

BASE = {'operator': 310000, 'vector': 320000, 'ansatz': 330000, 'kept': 340000, 'strings': 350000}
AMP_SCALE, COEFF_SCALE = 16, 8
MAX_QUBITS = 16

# The seeds of the GPU sweep, one list per feature group; tests/test_statevector_families.py asserts what they cover.
MATVEC_SEEDS = list(range(32))
EXPVAL_SEEDS = list(range(28))
RDM_SEEDS = list(range(48))          # 40 seeds reach 39 position masks, 48 the 40 that are asked for
ANSATZ_SEEDS = list(range(36))
ROUNDTRIP_SEEDS = list(range(24))
# the ansatz sweep's register size by seed: every size from 11 on (cap = n below 12, pad = 10 at 13), three in four at 14 and above,
# where a run is cut by the budget of 12 tile bits and a string of 13 X/Y positions takes a direct pass
ANSATZ_SIZES = [11, 14, 12, 15, 13, 16, 14, 15, 16, 14, 15, 16]


# ---- operators -------------------------------------------------------------------------------------------------------------------------
def draw_size(rng, n_max=MAX_QUBITS):
    """1 .. n_max, the sizes from 11 on five times as likely as the ones below."""
    sizes = np.arange(1, n_max + 1)
    w = np.where(sizes >= 11, 5.0, 1.0)
    return int(rng.choice(sizes, p=w / w.sum()))


def operator(seed, hermitian=False, n=None, n_max=MAX_QUBITS, t_max=300):
    """One operator of the family, as given (NOT cleaned): SimpleNamespace(seed, n, symp bool[T, 2n], coeff, kind, shape, planted).
    T is log-uniform in 1 .. 300 (at most t_max); rows of one density from 0.05 .. 0.5; shape 'one_x' gives every term the same X-part,
    'distinct_x' as many X-parts as terms (T <= 2^n), 'mixed' plants — each with probability 0.6 where T leaves room — repeated rows,
    the identity, diagonal terms, an all-Y string, a block sharing one X-part; a pair that cancels exactly is planted last in 'mixed' and
    'one_x'.  kind 'dyadic': integers in [-64, 64] over 8; 'gaussian': standard normal; hermitian: real coefficients (float64)."""
    rng = np.random.default_rng(BASE['operator'] + seed)
    n = draw_size(rng, n_max) if n is None else int(n)
    T = int(min(t_max, np.ceil(np.exp(rng.uniform(0.0, np.log(300.0))))))
    kind = 'dyadic' if rng.random() < 0.5 else 'gaussian'
    shape = str(rng.choice(['mixed', 'mixed', 'one_x', 'distinct_x']))
    symp = rng.random((T, 2 * n)) < rng.uniform(0.05, 0.5)
    planted = []
    if shape == 'one_x':
        symp[:, :n] = symp[0, :n]
    elif shape == 'distinct_x':
        T = min(T, 1 << n)
        xs = rng.permutation(1 << n)[:T]
        symp = symp[:T]
        symp[:, :n] = ((xs[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(bool)
    else:
        plant = lambda room: T >= room and rng.random() < 0.6
        if plant(4):
            symp[T // 2:T // 2 + T // 4] = symp[:T // 4]
            planted.append('repeated')
        if plant(2):
            symp[rng.integers(T)] = False
            planted.append('identity')
        if plant(3):
            symp[rng.integers(T, size=max(1, T // 8)), :n] = False
            planted.append('diagonal')
        if plant(2):
            symp[rng.integers(T)] = True
            planted.append('all_y')
        if plant(4):
            at = int(rng.integers(T - 2))
            symp[at:at + max(2, T // 6), :n] = symp[at, :n]
            planted.append('shared_x')
    if kind == 'dyadic':
        coeff = (rng.integers(-64, 65, T) + 1j * rng.integers(-64, 65, T)) / float(COEFF_SCALE)
    else:
        coeff = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    if shape != 'distinct_x' and T >= 2 and rng.random() < 0.6:
        i, j = (int(q) for q in rng.choice(T, 2, replace=False))
        symp[j], coeff[j] = symp[i], -coeff[i]
        planted.append('cancelling')
    if hermitian:
        coeff = np.ascontiguousarray(coeff.real)
    return SimpleNamespace(seed=seed, n=n, symp=symp, coeff=coeff, kind=kind, shape=shape, planted=planted)


def expval_operator(seed):
    """A Hermitian operator on at most 12 qubits for the expval sweep, cut to its first max(4, 2^17 / 2^n) terms: the expval oracle
    walks every (term, basis state) pair in Python."""
    op = operator(seed, hermitian=True, n_max=12)
    keep = max(4, (1 << 17) >> op.n)
    op.symp, op.coeff = op.symp[:keep], op.coeff[:keep]
    return op


def vector(seed, n, kind):
    """complex128[2^n]: 'dyadic' — integers in [-8, 8] over 16, both components; 'gaussian' — standard normal, normalised."""
    rng = np.random.default_rng(BASE['vector'] + seed)
    if kind == 'dyadic':
        return (rng.integers(-8, 9, 1 << n) + 1j * rng.integers(-8, 9, 1 << n)) / float(AMP_SCALE)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return v / np.linalg.norm(v)


def assert_dyadic_is_exact(coeff, n):
    """The condition of the module docstring: with it, every partial sum of every identity below is an integer below 2^52 over a power of
    two — H v in units of 1/128, <v|H v> and a gradient in units of 1/2048, a density-matrix entry in units of 1/256."""
    c = np.asarray(coeff, dtype=np.complex128) * COEFF_SCALE
    assert np.array_equal(c.real, np.rint(c.real)) and np.array_equal(c.imag, np.rint(c.imag)), 'a coefficient is not an integer over 8'
    assert int(np.abs(c.real).sum() + np.abs(c.imag).sum()) * 8 * 8 * 8 * 2 * (1 << n) < 2 ** 52


def assert_dyadic_vector(v):
    a = np.asarray(v, dtype=np.complex128) * AMP_SCALE
    assert np.array_equal(a.real, np.rint(a.real)) and np.array_equal(a.imag, np.rint(a.imag)) and np.abs(a.real).max() <= 8 and np.abs(a.imag).max() <= 8


def cleaned(symp, coeff):
    """(x, z, coeff) of the operator with equal rows merged (their coefficients added in operator order, per component), coefficients
    whose two components are both zero dropped, in ascending (x, z) order: what from_matrix lists."""
    x, z = pdo.xz_of(symp)
    acc = {}
    for key, c in zip(zip(x.tolist(), z.tolist()), np.asarray(coeff, dtype=np.complex128).tolist()):
        acc[key] = acc[key] + c if key in acc else c
    keys = sorted(k for k, c in acc.items() if c != 0)
    return (np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64),
            np.array([acc[k] for k in keys], dtype=np.complex128))


def compare_terms(got, want, bound):
    """Two term lists (x, z, coeff).  bound 0: the same terms with equal coefficients (==: the sign of a zero component is not compared).
    Otherwise every component within `bound`; a term that only one side lists has both components within `bound` of zero.  Returns the
    largest component gap."""
    a = {(int(x), int(z)): complex(c) for x, z, c in zip(*got)}
    b = {(int(x), int(z)): complex(c) for x, z, c in zip(*want)}
    assert len(a) == len(got[2]) and len(b) == len(want[2]), 'a term listed twice'
    if bound == 0:
        assert sorted(a) == sorted(b), f'term sets differ: {sorted(set(a) ^ set(b))[:8]}'
    worst = 0.0
    for q in set(a) | set(b):
        p, r = a.get(q, 0j), b.get(q, 0j)
        worst = max(worst, abs(p.real - r.real), abs(p.imag - r.imag))
        assert abs(p.real - r.real) <= bound and abs(p.imag - r.imag) <= bound, f'term {q}: {p!r} vs {r!r}, bound {bound:.3g}'
    return worst


# ---- the identities, on the oracles ----------------------------------------------------------------------------------------------------
def csr_times(symp, coeff, v):
    """The sparse oracle's matrix (so.to_csr) times v, the products of a row added in column order, per component."""
    data, indices, indptr = so.to_csr(symp, coeff)
    side = len(indptr) - 1
    rows = np.repeat(np.arange(side), np.diff(indptr))
    w = np.asarray(v, dtype=np.complex128).reshape(-1)[indices]
    pr, pi = data.real * w.real - data.imag * w.imag, data.real * w.imag + data.imag * w.real
    return mo._complex(np.bincount(rows, weights=pr, minlength=side), np.bincount(rows, weights=pi, minlength=side))


def state_of(v, threshold=1e-15):
    """(bits uint8[S, n], amplitudes) of a dense vector as QuantumState.from_array lists it: |a| >= threshold, ascending index."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    n = v.shape[0].bit_length() - 1
    at = np.flatnonzero(np.abs(v) >= threshold)
    return ((at[:, None] >> np.arange(n - 1, -1, -1)) & 1).astype(np.uint8).reshape(len(at), n), v[at]


def energy_bound(n, T, coeff):
    """|Re <v|H|v> - exact| for a unit v by any of the routes: ao.bound without rotations."""
    return ao.bound(n, 0, T, coeff)


def energy_routes(symp, coeff, v):
    """Re <v|H|v> three ways: {'ansatz': ao.energy, 'expval': the expval oracle's total on the state of v, 'vdot': Re vdot(v, mo.matvec)}."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    bits, amp = state_of(v)
    return {'ansatz': ao.energy(symp, coeff, v),
            'expval': eo.total(coeff, eo.term_elements(symp, bits, amp, bits, amp)).real,
            'vdot': float(np.vdot(v, mo.matvec(symp, coeff, v)).real)}


def strings_on(seed, n, kept, count=3):
    """(sub bool[count, 2k], padded bool[count, 2n]): `count` Pauli strings on the kept qubits (not the identity where k >= 1; for k = 0
    there is only the identity) and the same strings on n qubits, I outside the kept set."""
    rng = np.random.default_rng(BASE['strings'] + seed)
    kept = ro.kept_of(n, kept)
    k = len(kept)
    sub = rng.random((count, 2 * k)) < 0.5
    for row in sub:
        if k and not row.any():
            row[rng.integers(2 * k)] = True
    padded = np.zeros((count, 2 * n), dtype=bool)
    padded[:, kept] = sub[:, :k]
    padded[:, [n + q for q in kept]] = sub[:, k:]
    return sub, padded


def trace_with(rho, sub_row):
    """Re Tr(rho_A P_A), P_A = so.kron_dense of one string on the kept qubits: sum_a rho[a, a'] P_A[a', a], one product per row."""
    k = len(sub_row) // 2
    P = so.kron_dense(np.asarray(sub_row, dtype=bool).reshape(1, 2 * k), [1.0])
    return float(np.sum(rho * P.T).real)


def rdm_route(v, n, kept, sub_row):
    """(Re Tr(rho_A P_A) with rho_A from ro.rdm_deposit, its a-priori bound trace(tol): |sum_a err[a, a']| <= sum_a tol[a][a'] and
    r_a r_a' <= (r_a^2 + r_a'^2) / 2)."""
    return trace_with(ro.rdm_deposit(v, n, kept), sub_row), float(np.trace(ro.entry_tolerance(v, n, kept)))


def gradient_pair(h_symp, h_coeff, gens, theta, ref):
    """(ao.grad_shift(...)[K-1], ao.pool_grad of generator K-1 at the prepared state): one number, dE/dtheta_{K-1} = <psi| i [H, P] |psi>."""
    K = np.asarray(gens).shape[0]
    psi = ao.state(gens, theta, ref)
    return (ao.grad_shift(h_symp, h_coeff, gens, theta, ref)[K - 1],
            ao.pool_grad(ao.dense_operator(h_symp, h_coeff), np.asarray(gens)[K - 1:K], psi)[0])


def decomp_bound(symp, coeff, dense):
    """Per component, a decomposition of the operator's matrix against its cleaned terms: pdo.reference_bound for the 2^n-term sum and
    the butterfly over the matrix, plus mo.error_bound at a unit amplitude for the T additions that formed the entries and merged the terms."""
    n = np.asarray(symp).shape[1] // 2
    return pdo.reference_bound(n, dense) + mo.error_bound(symp, coeff, [1.0])


def roundtrip(symp, coeff):
    """(decompose(to_dense(H)), cleaned H, the dense matrix)."""
    n = np.asarray(symp).shape[1] // 2
    dense = so.to_dense(symp, coeff)
    return pdo.decompose(dense, n), cleaned(symp, coeff), dense


# ---- generator sequences ---------------------------------------------------------------------------------------------------------------
def _excitation(rng, n, rows):
    """1 .. 4 strings sharing 1, 2 or 4 X/Y positions, X or Y drawn per position, stray Z's anywhere else."""
    pos = rng.choice(n, min(n, int(rng.choice([1, 2, 4]))), replace=False)
    for _ in range(int(rng.integers(1, 5))):
        x, z = np.zeros(n, dtype=bool), rng.random(n) < 0.08
        x[pos], z[pos] = True, rng.random(len(pos)) < 0.5
        rows.append(np.concatenate([x, z]))


def _wide(rng, n, rows):
    """13 or more X/Y positions: no tile holds it."""
    pos = rng.choice(n, int(rng.integers(13, n + 1)), replace=False)
    x, z = np.zeros(n, dtype=bool), rng.random(n) < 0.08
    x[pos], z[pos] = True, rng.random(len(pos)) < 0.5
    rows.append(np.concatenate([x, z]))


def _diagonal(rng, n, rows):
    rows.append(np.concatenate([np.zeros(n, dtype=bool), rng.random(n) < 0.3]))


def ansatz_case(seed):
    """SimpleNamespace(seed, n, symp bool[K, 2n], theta, ranges): K in 36 .. 44 'excitation-like' generators, a diagonal string one time
    in ten; from n = 14 on a wide string now and then, and in most sequences one planted place with one or two adjacent wide strings,
    followed half the time by a diagonal string (the run after the direct pass is then opened by a generator without X-part)."""
    rng = np.random.default_rng(BASE['ansatz'] + seed)
    n = ANSATZ_SIZES[seed % len(ANSATZ_SIZES)]
    K = int(rng.integers(36, 45))
    plant_at = int(rng.integers(2, K - 4)) if n >= 14 and rng.random() < 0.85 else None
    rows = []
    while len(rows) < K:
        if plant_at is not None and len(rows) >= plant_at:
            for _ in range(2 if rng.random() < 0.35 else 1):
                _wide(rng, n, rows)
            if rng.random() < 0.5:
                _diagonal(rng, n, rows)
            plant_at = None
            continue
        u = rng.random()
        if u < 0.1:
            _diagonal(rng, n, rows)
        elif n >= 14 and u < 0.12:
            _wide(rng, n, rows)
        else:
            _excitation(rng, n, rows)
    symp = np.array(rows[:K], dtype=bool)
    theta = rng.uniform(-np.pi, np.pi, K)
    return SimpleNamespace(seed=seed, n=n, symp=symp, theta=theta, ranges=ansatz_ranges(rng, symp))


def ansatz_ranges(rng, symp):
    """[(kind, k_begin, k_end, inverse)] for the segments ao.plan_runs gives the sequence: 'whole'; 'empty'; 'inside' — strictly inside one
    tiled run (it is clipped at both ends), forward and reverse; 'spanning' — from inside one tiled run to inside a later one, forward
    and reverse; 'direct' — one direct segment alone.  A kind the sequence has no room for is left out."""
    segs = ao.plan_runs(symp)
    K = symp.shape[0]
    flag = lambda: bool(rng.integers(2))
    at = int(rng.integers(0, K + 1))
    out = [('whole', 0, K, flag()), ('empty', at, at, flag())]
    tiled = [s for s in segs if s[3]]
    long = [s for s in tiled if s[1] - s[0] >= 3]
    if long:
        k0, k1 = long[int(rng.integers(len(long)))][:2]
        kb = int(rng.integers(k0 + 1, k1 - 1))
        ke = int(rng.integers(kb + 1, k1))
        out += [('inside', kb, ke, False), ('inside', kb, ke, True)]
    room = [i for i, s in enumerate(tiled) if s[1] - s[0] >= 2]
    if len(room) >= 2:
        i, j = sorted(int(q) for q in rng.choice(len(room), 2, replace=False))
        a, b = tiled[room[i]], tiled[room[j]]
        kb, ke = int(rng.integers(a[0] + 1, a[1])), int(rng.integers(b[0] + 1, b[1]))
        out += [('spanning', kb, ke, False), ('spanning', kb, ke, True)]
    direct = [s for s in segs if not s[3]]
    if direct:
        k0, k1 = direct[int(rng.integers(len(direct)))][:2]
        out.append(('direct', k0, k1, flag()))
    return out


# ---- kept sets -------------------------------------------------------------------------------------------------------------------------
def kept_case(seed):
    """SimpleNamespace(seed, n, kept, kind): a uniformly random subset of k qubits, k in 0 .. min(8, n); seeds 6 mod 8 have fewer than 8
    traced qubits (a partial STREAM tile), seeds 7 mod 8 fewer than 4 (a partial TILED block)."""
    rng = np.random.default_rng(BASE['kept'] + seed)
    if seed % 8 < 6:
        n = draw_size(rng)
        k = int(rng.integers(0, min(8, n) + 1))
    else:
        k = int(rng.integers(0, 9))
        n = min(MAX_QUBITS, max(1, k + int(rng.integers(0, 8 if seed % 8 == 6 else 4))))
    kept = sorted(int(q) for q in rng.choice(n, k, replace=False))
    return SimpleNamespace(seed=seed, n=n, kept=kept, kind='dyadic' if rng.random() < 0.5 else 'gaussian')


RDM_KS, RDM_ST_E, RDM_T, RDM_S = 3, 8, 6, 4      # csrc/rdm.hip: STREAM up to 3 kept qubits, 2^8 traced values a tile; TILED 2^6 x 2^4


def _lowest_bits(mask, count):
    return int(ro.deposit(np.array([(1 << count) - 1], dtype=np.uint64), mask)[0])


def _extract(v, mask):
    out, at = 0, 0
    for pos in range(64):
        if (mask >> pos) & 1:
            out |= ((v >> pos) & 1) << at
            at += 1
    return out


def rdm_position_mask(n, kept, form):
    """The mask LA that csrc/rdm.hip derives (rdm_shape, rdm_launch): where the kept bits sit among the bits of the staged tile.
    'stream': S = KM | the min(n - k, 8) lowest traced bits, LA = KM's bits within S.  'tiled': V = the min(k, 6) lowest kept bits | the
    min(n - k, 4) lowest traced bits, LA = those kept bits within V."""
    kept = ro.kept_of(n, kept)
    k = len(kept)
    KM = sum(1 << (n - 1 - q) for q in kept)
    TM = ((1 << n) - 1) & ~KM
    if form == 'stream':
        assert k <= RDM_KS
        return _extract(KM, KM | _lowest_bits(TM, min(n - k, RDM_ST_E)))
    low_kept = _lowest_bits(KM, min(k, RDM_T))
    return _extract(low_kept, low_kept | _lowest_bits(TM, min(n - k, RDM_S)))


def rdm_forms(k):
    """The forms the sweep runs a case in: (None, 'tiled') — the library's choice, STREAM, and TILED forced — up to 3 kept qubits,
    TILED alone beyond."""
    return (None, 'tiled') if k <= RDM_KS else ('tiled',)
