"""Seeded inputs with answers that hold BY CONSTRUCTION for the three entry points of csrc/project.hip (noncontextuality test, bra * ket,
stabiliser projection).  Plain NumPy generators; shared by tests/test_f3_f4_families.py (every claimed answer against oracle.oracle_np
alone, on the CPU), tests/test_gpu_f3_f4.py and tests/_weak_hash_worker3.py (the kernels against the oracle on the same inputs).

Noncontextuality (utils.py:567-589): an operator is noncontextual iff commutation is an equivalence relation on the terms that do not
commute with everything.  The operators here are built from HEADS — the seven pairwise anticommuting Paulis on qubits 0..2 (the six
Jordan-Wigner Majorana strings X0, Y0, Z0 X1, Z0 Y1, Z0 Z1 X2, Z0 Z1 Y2 and their product Z0 Z1 Z2) — times TAILS, Z strings on the qubits from
3 on.  Tails commute with everything here, so two terms commute iff their heads are equal or one of them has none: terms without a head are
universal, terms with head c form clique c, different cliques anticommute term by term.  That is noncontextual.  A near-miss is that operator
with ONE term added or changed so that three named terms a ~ b ~ c, a !~ c exist among the non-universal ones (~ = commutes); the triple is
written down at each builder.  Tail qubit Q = 3 is where the near-misses act: in every clique the first member (before the shuffle) has Z on
Q, the second has not.
"""
import numpy as np

N_HEAD = 3                      # head qubits 0..2
Q = 3                           # the tail qubit the near-misses put an X on
NEAR_MISSES = ('partial', 'bridge', 'flipped')


# ---------------------------------------------------------------------------------------------------------------- noncontextuality ----
def heads(n):
    """bool[7, 2n]: the pairwise anticommuting head Paulis on qubits 0..2 (every pair differs from commuting on exactly one qubit)."""
    h = np.zeros((2 * N_HEAD + 1, 2 * n), dtype=bool)
    for j in range(N_HEAD):
        for k in (0, 1):
            r = h[2 * j + k]
            r[n:n + j] = True                       # Z_0 .. Z_{j-1}
            r[j] = True                             # X_j
            r[n + j] = bool(k)                      # ... or Y_j
    h[2 * N_HEAD] = np.logical_xor.reduce(h[:2 * N_HEAD], axis=0)      # the product of the six, up to a phase: Z0 Z1 Z2
    return h


def split_sizes(T, n_cliques, n_univ, single=False):
    """Clique sizes that add up to T - n_univ: equal shares, the remainder to the first clique (which gets at least two members whenever
    there are enough terms), `single`: the last clique has one member."""
    rest = T - n_univ
    assert n_cliques >= 1 and rest >= n_cliques
    if n_cliques == 1:
        return (rest,)
    if single:
        return split_sizes(T - 1, n_cliques - 1, n_univ) + (1,)
    share = rest // n_cliques
    return (rest - share * (n_cliques - 1),) + (share,) * (n_cliques - 1)


def _cliques(T, n_univ, sizes, n_tail, rng):
    """(symp bool[T, 2n], clique of every row or -1, index of every row inside its clique or -1), rows shuffled; n = 3 + n_tail."""
    n = N_HEAD + n_tail
    assert n_univ + sum(sizes) == T and len(sizes) <= 2 * N_HEAD + 1 and n_tail >= 2 and all(s >= 1 for s in sizes)
    H = heads(n)
    symp = np.zeros((T, 2 * n), dtype=bool)
    symp[:, n + N_HEAD:] = rng.random((T, n_tail)) < 0.5
    clique = np.full(T, -1, dtype=np.int64)
    member = np.full(T, -1, dtype=np.int64)
    at = n_univ
    for c, size in enumerate(sizes):
        symp[at:at + size] ^= H[c]
        clique[at:at + size] = c
        member[at:at + size] = np.arange(size)
        symp[at, n + Q] = True                       # first member: Z on Q
        if size > 1:
            symp[at + 1, n + Q] = False              # second member: no Z on Q
        at += size
    perm = rng.permutation(T)
    return symp[perm], clique[perm], member[perm]


def cliques(T, n_univ, sizes, n_tail, rng):
    """n_univ universal terms and len(sizes) cliques of the given sizes on 3 + n_tail qubits -> (symp, True)."""
    return _cliques(T, n_univ, sizes, n_tail, rng)[0], True


def _tail(n, rng, first=N_HEAD):
    r = np.zeros(2 * n, dtype=bool)
    r[n + first:] = rng.random(n - first) < 0.5
    return r


def near_miss(kind, T, n_univ, sizes, n_tail, rng, p):
    """The operator of `cliques` with one term added at row p ('partial', 'bridge': built from T - 1 terms, n_univ + sum(sizes) == T - 1)
    or the term at row p changed ('flipped': n_univ + sum(sizes) == T) -> (symp bool[T, 2n], False).  Needs two cliques, the first with
    two members.  With K the first clique, K' the second, k0 / k1 the first / second member of K and k0' the first member of K':
      partial  X_Q times a Z string on the qubits beyond Q.  It commutes with k1 (no Z on Q), not with k0 (Z on Q), and k0 ~ k1:
               part of one clique only (the goldens' kind 2).
      bridge   head_0 head_1 head_6 (it commutes with each of the three heads and anticommutes with the other four) times a tail.  It
               commutes with all of K and all of K' (and all of the seventh clique where there is one), and k0 !~ k0'.  It needs a THIRD
               clique: with two, nothing anticommutes with it, it is one more universal term and the operator stays noncontextual.
      flipped  k0 gets an X on Q (its Z on Q stays: a Y).  It still commutes with k1 (same head, no Z on Q), now also with k0' (the heads
               anticommute and so do X_Q and Z_Q), and k1 !~ k0'.
    In each case the three terms are non-universal, so commutation is not transitive on the non-universal terms: contextual."""
    assert kind in NEAR_MISSES and len(sizes) >= (3 if kind == 'bridge' else 2) and sizes[0] >= 2 and 0 <= p < T
    n = N_HEAD + n_tail
    if kind == 'flipped':
        symp, clique, member = _cliques(T, n_univ, sizes, n_tail, rng)
        at = int(np.flatnonzero((clique == 0) & (member == 0))[0])
        symp[at, Q] = True
        symp[[at, p]] = symp[[p, at]]
        return symp, False
    symp, _, _ = _cliques(T - 1, n_univ, sizes, n_tail, rng)
    if kind == 'partial':
        term = _tail(n, rng, first=Q + 1)
        term[Q] = True
    else:
        H = heads(n)
        term = _tail(n, rng) ^ H[0] ^ H[1] ^ H[6]
    return np.insert(symp, p, term, axis=0), False


def still_true(kind, T, n_univ, sizes, n_tail, rng):
    """Operators of T terms that stay noncontextual -> (symp, True).  'duplicate': T - 1 terms of `cliques` and a copy of one clique member
    appended (equal adjacency rows beyond the clique structure); 'universal_last': T - 1 terms and a universal term as the last row;
    'commuting': T Z strings (nothing is non-universal)."""
    n = N_HEAD + n_tail
    if kind == 'commuting':
        symp = np.zeros((T, 2 * n), dtype=bool)
        symp[:, n:] = rng.random((T, n)) < 0.4
        return symp, True
    symp, clique, _ = _cliques(T - 1, n_univ, sizes, n_tail, rng)
    if kind == 'duplicate':
        src = np.flatnonzero(clique >= 0)
        extra = symp[int(src[0]) if src.size else 0]
    else:
        assert kind == 'universal_last'
        extra = _tail(n, rng)
    return np.vstack([symp, extra]), True


def positions(T):
    """Rows a near-miss term is put at: 0, 63, 64, the first index of the last adjacency word, T - 1 (those that exist)."""
    return sorted({p for p in (0, 63, 64, 64 * ((T - 1) // 64), T - 1) if p < T})


def noncontextual_cases(T, n_cliques, univ, n_tail, single=False, seed=0, near=None, still=('duplicate', 'universal_last', 'commuting')):
    """[(id, symp, answer)] for one T: the True operator, every near-miss at every position, the still-True variants.  `univ`: 0, 1 or
    'half' (T // 2 of the terms the operator is built from).  One clique: there is no near-miss (everything commutes); two: no 'bridge'."""
    def args(t):
        nu = t // 2 if univ == 'half' else int(univ)
        return t, nu, split_sizes(t, n_cliques, nu, single), n_tail
    rng = np.random.default_rng([seed, T])
    out = [('true', *cliques(*args(T), rng))]
    if near is None:
        near = [(kind, p) for kind in NEAR_MISSES if n_cliques >= (3 if kind == 'bridge' else 2) for p in positions(T)]
    for kind, p in near:
        _, nu, sizes, nt = args(T if kind == 'flipped' else T - 1)
        out.append((f'{kind}@{p}', *near_miss(kind, T, nu, sizes, nt, rng, p)))
    for kind in still:
        out.append((kind, *still_true(kind, T, *args(T - 1)[1:], rng)))
    return out


# --------------------------------------------------------------------------------------------------------------------- bra * ket ----
AMPLITUDES = ('dyadic', 'gauss', 'wide', 'nonfinite')
OVERLAPS = ('none', 'third', 'all')
SPECIALS = ((np.inf, 1.0), (-np.inf, 0.5), (1.0, np.inf), (np.nan, 1.0), (1.0, np.nan), (-0.0, 1.0), (1.0, -0.0), (np.inf, np.nan), (-0.0, -0.0))


def amplitudes(rng, N, kind):
    """complex128[N].  'dyadic': multiples of 1/16, never 0 (any order of additions, fused or not, gives the same bits); 'gauss': standard
    normal parts; 'wide': parts of either sign with magnitudes 10^u, u uniform in [-8, 8] (the order of the additions shows in the low
    bits); 'nonfinite': Gaussian here, `states` then plants SPECIALS."""
    if kind == 'dyadic':
        re, im = rng.integers(-8, 9, N), rng.integers(-8, 9, N)
        re[(re == 0) & (im == 0)] = 1
        return (re + 1j * im) / 16.0
    if kind == 'wide':
        part = lambda: rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-8, 8, N)
        return part() + 1j * part()
    assert kind in ('gauss', 'nonfinite')
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


def states(rng, Na, Nb, nq, overlap, kind):
    """Two clean states (distinct basis rows within each) that share a chosen subset of rows ->
    (a_bits uint8[Na, nq], a_c, b_bits uint8[Nb, nq], b_c, match int64[Na]: the row of b equal to row i of a, or -1).
    Distinct by construction: the low bits of row u of the pool spell a number that no other row has.  'none' shares nothing, 'all'
    min(Na, Nb) rows, 'third' about a third of that; the shared rows sit at random places of both states."""
    small = min(Na, Nb)
    shared = {'none': 0, 'all': small, 'third': max(1, small // 3)}[overlap]
    U = Na + Nb - shared
    kbits = max(1, (U - 1).bit_length())
    assert kbits <= nq, 'not that many distinct rows on so few qubits'
    ids = rng.permutation(1 << kbits)[:U]
    pool = rng.integers(0, 2, (U, nq), dtype=np.uint8)
    pool[:, :kbits] = (ids[:, None] >> np.arange(kbits)) & 1
    sa = np.sort(rng.choice(Na, shared, replace=False))                 # the rows of a that b has too
    order_b = rng.permutation(Nb)                                       # b = [a's shared rows, the rest of the pool], shuffled
    b_bits = np.vstack([pool[sa], pool[Na:]])[order_b]
    where = np.empty(Nb, dtype=np.int64)
    where[order_b] = np.arange(Nb)
    match = np.full(Na, -1, dtype=np.int64)
    match[sa] = where[:shared]
    a_c, b_c = amplitudes(rng, Na, kind), amplitudes(rng, Nb, kind)
    if kind == 'nonfinite':
        # enough shared rows: specials of a on its first shared rows, specials of b on partners shifted by three, so that special x special
        # and special x finite pairs both occur.  Fewer: on the first rows of either state, shared or not (an infinite amplitude on a row
        # the other state lacks must add 0, not inf * 0)
        k = len(SPECIALS)
        rows_a, rows_b = (sa[:k], match[sa[3:k + 3]]) if shared >= k + 3 else (np.arange(min(k, Na)), np.arange(min(k, Nb)))
        for rows, c in ((rows_a, a_c), (rows_b, b_c)):
            for r, (re, im) in zip(rows, SPECIALS):
                c[r] = complex(re, im)
    return pool[:Na], a_c, b_bits, b_c, match


def state_symp(bits):
    """The operator a QuantumState carries (base.py:1564-1580): X where the bit is 1, Z where it is 0."""
    bits = np.asarray(bits, dtype=bool)
    return np.hstack([bits, ~bits])


def inner_sequential(a_rows, a_c, b_rows, b_c):
    """The reference's loop (base.py:1808-1815) on cleaned states, in the order of a's rows: every product as separate IEEE operations
    on the parts (no complex multiplication: its treatment of infinities is not the same everywhere), 0 for a row b does not have,
    and `re += p_re; im += p_im`.  -> (re, im) as np.float64."""
    index = {r.tobytes(): j for j, r in enumerate(np.ascontiguousarray(b_rows))}
    a_rows = np.ascontiguousarray(a_rows)
    ar_, ai_ = np.asarray(a_c).real.astype(np.float64), np.asarray(a_c).imag.astype(np.float64)
    br_, bi_ = np.asarray(b_c).real.astype(np.float64), np.asarray(b_c).imag.astype(np.float64)
    re, im = np.float64(0.0), np.float64(0.0)
    with np.errstate(all='ignore'):
        for i in range(a_rows.shape[0]):
            j = index.get(a_rows[i].tobytes())
            if j is None:
                p_re, p_im = np.float64(0.0), np.float64(0.0)
            else:
                ar, ai, br, bi = ar_[i], ai_[i], br_[j], bi_[j]
                p_re = ar * br - ai * bi
                p_im = ar * bi + ai * br
            re = re + p_re
            im = im + p_im
    return re, im


def same_bits(x, y):
    """Bit-for-bit equality of two doubles; a NaN equals any NaN (the sign and payload of a generated NaN are the platform's)."""
    x, y = np.float64(x), np.float64(y)
    if np.isnan(x) or np.isnan(y):
        return bool(np.isnan(x) and np.isnan(y))
    return x.tobytes() == y.tobytes()


# -------------------------------------------------------------------------------------------------------------------- projection ----
def projection_case(rng, n, T, stabs, survivors='half', collapse=0, coeff='dyadic', density=0.3):
    """A random operator of T terms on n qubits and single-qubit stabilisers `stabs` = [(qubit, 'X' | 'Z', eigenvalue in {-1, 0, +1})] ->
    dict(symp, coeff, stab bool[k, 2n], eig int64[k], keep int64[n - k], n_survived).  A term survives iff it commutes with every stabiliser:
    no X (or Y) on the qubit of a Z stabiliser, no Z (or Y) on the qubit of an X stabiliser.  `survivors`: 'all' clears those bits in
    every term, 'none' then sets one of them in every term, 'half' in every odd row.  `collapse` = c > 0: on the kept qubits only c
    of them (the first, the middle one, the last) carry Paulis, so all terms fall onto at most 4^c projected rows."""
    k = len(stabs)
    stab = np.zeros((k, 2 * n), dtype=bool)
    kills = np.zeros(k, dtype=np.int64)                  # the column of a term that makes it anticommute with stabiliser s
    for s, (q, kind, _) in enumerate(stabs):
        assert kind in ('X', 'Z') and 0 <= q < n
        stab[s, q + (n if kind == 'Z' else 0)] = True
        kills[s] = q + (0 if kind == 'Z' else n)
    eig = np.array([e for _, _, e in stabs], dtype=np.int64)
    keep = np.setdiff1d(np.arange(n), [q for q, _, _ in stabs])
    assert keep.size == n - k, 'one stabiliser per qubit'
    symp = rng.random((T, 2 * n)) < density
    if collapse:
        carry = keep[np.unique(np.linspace(0, keep.size - 1, collapse).astype(int))]
        idle = np.setdiff1d(keep, carry)
        symp[:, idle] = False
        symp[:, idle + n] = False
    symp[:, kills] = False
    rows = np.arange(T)
    hit = {'all': rows[:0], 'none': rows, 'half': rows[1::2]}[survivors]
    if k:
        symp[hit, kills[rng.integers(0, k, hit.size)]] = True
    c = amplitudes(rng, T, coeff)
    return dict(symp=symp, coeff=c, stab=stab, eig=eig, keep=keep, n_survived=T - (hit.size if k else 0))


def projection_expected(symp, coeff, stab, eig, keep, zero_threshold=1e-15):
    """The reference's lines (projection/base.py:60-84) on bool matrices with the oracle's commutation table and cleanup ->
    (rows bool[R, 2 * len(keep)], coeff, n_survived); nothing survives: the cleanup of an operator without terms, 0 * I."""
    from oracle import oracle_np as onp
    n = symp.shape[1] // 2
    survive = np.all(onp.commutes_termwise(symp, stab), axis=1) if stab.shape[0] else np.ones(symp.shape[0], dtype=bool)
    cols = np.nonzero(stab)[1]
    ev = symp[survive][:, cols] * np.asarray(eig, dtype=np.int64)
    ev[ev == 0] = 1                                                      # an eigenvalue 0 counts as 1 (:70)
    w = np.asarray(coeff)[survive] * np.prod(ev, axis=1)
    rows, c = onp.cleanup_op(symp[survive][:, np.hstack([keep, keep + n])], w, zero_threshold)
    return rows, c, int(survive.sum())


# ------------------------------------------------------------------------------------------------------------- the tables of cases ----
# T -> (cliques, universal terms, tail qubits, one clique of size 1): clique counts 2, 3, 7, universal counts 0, 1, T // 2, 8 .. 70 qubits and
# one operator on 130.  T = 4 is the smallest operator that reaches the kernel, 4097 has an odd number of adjacency words (65) and a
# last word with one bit, 4160 fills its 65th word.
NONCONTEXTUAL = {
    4: (2, 0, 5, False), 63: (3, 1, 5, False), 64: (7, 'half', 17, False), 65: (2, 0, 61, False), 128: (3, 'half', 67, False),
    129: (7, 1, 30, True), 192: (2, 'half', 62, False), 193: (2, 0, 20, False), 256: (3, 0, 40, False), 257: (7, 'half', 47, False),
    1000: (3, 1, 27, True), 4097: (7, 'half', 127, False), 4160: (3, 1, 37, False),
}
ONE_CLIQUE = {65: (1, 0, 9, False), 193: (1, 'half', 20, False)}       # one clique: everything commutes, whatever is appended
# 129 adjacency words per row, characters padded to 130 > 128 words (the first T with more than 128 is 8193)
T_WIDE = 8200
WIDE = (3, 1, 27, False)


def noncontextual_family(T, table=None):
    if T == T_WIDE and table is None:
        k, univ, n_tail, single = WIDE
        return noncontextual_cases(T, k, univ, n_tail, single, seed=3, near=[('bridge', T - 1), ('partial', 0)], still=())
    k, univ, n_tail, single = (NONCONTEXTUAL if table is None else table)[T]
    return noncontextual_cases(T, k, univ, n_tail, single, seed=1 if table is None else 2)


# (Na, Nb, qubits): around the table capacity steps (1024 slots until 2 Nb exceeds them: Nb = 512 / 513, 1024 / 1025) and long tables
INNER_SHAPES = [(1, 1, 1), (64, 64, 64), (65, 512, 65), (65, 513, 1000), (300, 1024, 1000), (300, 1025, 64), (1000, 200000, 130), (100000, 100000, 130)]


def inner_cases():
    """[(Na, Nb, nq, overlap, kind)]: every overlap and amplitude kind up to a thousand rows; the two long shapes with every kind at a
    third overlap and Gaussian amplitudes at none / all."""
    out = []
    for Na, Nb, nq in INNER_SHAPES:
        for overlap in OVERLAPS:
            if overlap == 'third' and min(Na, Nb) < 3:
                continue
            for kind in AMPLITUDES:
                if max(Na, Nb) > 2000 and overlap != 'third' and kind != 'gauss':
                    continue
                out.append((Na, Nb, nq, overlap, kind))
    return out


def make_stabs(rng, qubits):
    """[(qubit, kind, eigenvalue)] with random kinds and eigenvalues; the first eigenvalues are -1, 0, +1 so that each occurs."""
    qubits = list(qubits)
    kinds = rng.choice(['X', 'Z'], len(qubits))
    eig = rng.choice([-1, 0, 1], len(qubits))
    eig[:3] = [-1, 0, 1][:len(qubits)]
    return [(int(q), str(k), int(e)) for q, k, e in zip(qubits, kinds, eig)]


def _r(*spans):
    return [q for lo, hi in spans for q in range(lo, hi)]


# id -> (n, stabilised qubits, T, survivors, collapse, coefficients): n_keep = 64 / 63 / 1 / 64 / 65 / 128 / 129 / 128 / 129 / 65 / 129 / 65 / 65 / 63;
# stabilisers in the first word, on qubit n - 1 and on qubits 63 and 64
PROJECTION = {
    'n65-keep64-T1': (65, [64], 1, 'all', 0, 'dyadic'),
    'n65-keep63-T255': (65, [63, 64], 255, 'half', 0, 'dyadic'),
    'n65-keep1-T256': (65, _r((0, 30), (31, 65)), 256, 'half', 0, 'gauss'),
    'n128-keep64-T257': (128, _r((0, 16), (48, 80), (112, 128)), 257, 'all', 0, 'dyadic'),
    'n128-keep65-T255-none': (128, _r((0, 15), (48, 80), (112, 128)), 255, 'none', 0, 'dyadic'),
    'n130-keep128-T257': (130, [63, 129], 257, 'half', 0, 'gauss'),
    'n130-keep129-T70000': (130, [64], 70000, 'half', 0, 'dyadic'),
    'n200-keep128-T256': (200, _r((0, 24), (52, 76), (176, 200)), 256, 'half', 0, 'dyadic'),
    'n200-keep129-T257': (200, _r((0, 23), (52, 76), (176, 200)), 257, 'all', 0, 'gauss'),
    'n1000-keep65-T255': (1000, sorted(set(range(1000)) - set(range(2, 2 + 15 * 65, 15))), 255, 'half', 0, 'dyadic'),
    'n1000-keep129-T257': (1000, sorted(set(range(1000)) - set(range(2, 2 + 7 * 129, 7))), 257, 'half', 0, 'dyadic'),
    'collapse3-dyadic': (130, _r((0, 32), (63, 65), (99, 130)), 70000, 'half', 3, 'dyadic'),
    'collapse3-gauss': (130, _r((0, 32), (63, 65), (99, 130)), 70000, 'half', 3, 'gauss'),
    'collapse2-all': (65, [63, 64], 70000, 'all', 2, 'dyadic'),
}


def projection_family(name):
    n, qubits, T, survivors, collapse, coeff = PROJECTION[name]
    rng = np.random.default_rng([5, len(name), n, T])
    return projection_case(rng, n, T, make_stabs(rng, qubits), survivors, collapse, coeff)


def threshold_case():
    """Merged rows whose sums sit at, below and above a threshold of 0.5: every coefficient is 0.25 and the stabiliser's eigenvalue is +1, so
    a projected row that 1, 2, 3, ... terms fall onto sums to 0.25, 0.5, 0.75, ...; the strict `>` drops the first two kinds."""
    rng = np.random.default_rng(77)
    n = 70
    case = projection_case(rng, n, 120, [(5, 'Z', 1), (64, 'X', 0)], 'all', 0, 'dyadic')
    symp = np.repeat(case['symp'], np.arange(120) % 4 + 1, axis=0)      # term i once, twice, three or four times ...
    symp[:, n + 5] = rng.random(symp.shape[0]) < 0.5                    # ... the copies differing on a stabilised position only
    symp = symp[rng.permutation(symp.shape[0])]
    case.update(symp=symp, coeff=np.full(symp.shape[0], 0.25 + 0j), n_survived=symp.shape[0], thr=0.5)
    return case
