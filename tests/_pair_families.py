"""Operands for the fused product + cleanup (csrc/cleanup_driver.hip, cleanup_keys.hip, pair_dups.hip) whose answers are known BY
CONSTRUCTION, and the plan of a call restated as size arithmetic (plain NumPy, seeded; neither the oracle nor the library is called here —
tests/test_pair_families.py proves the answers against oracle_c.mul on the CPU, tests/test_gpu_pair_flows.py runs them on the device).

Common setting.  Rows are random at density 0.5 (packed words straight from the generator), n = 100 qubits unless stated: 200 random bits.
Two of P pairs have the same product row by accident with probability 2^-200 each; among the at most 7.6e7 pairs of the largest shape
(12,288 terms squared) that is P^2 / 2 * 2^-200 < 2e-45 — every coincidence is a planted one.  (n = 40: 80 bits and at most 1.6e6 pairs,
1e-12.)  Coefficients are drawn from {1, -1, i, -i} and the threshold is thr = 2.5: a product row that only one pair forms has |c| = 1, in
P * P 0 or 2 (the sum of the twins (i, o) and (o, i)), and is dropped.  Every row that survives is therefore one the builder lists — a few
thousand rows however many pairs there are — and the builder hands over the pairs that form them, `cand`: every pair that shares its row
with another pair or survives alone.  `answer` forms rows, sums and first pair indices of exactly those pairs.

All sums are Gaussian integers: they are exact in any order, so the comparison is bit for bit and says nothing about the ORDER a kernel
sums in.  Order-sensitive sums (Gaussian coefficients, the identity sum of P * P in the reference's order) stay with the oracle tests
(tests/test_gpu_parity.py, test_gpu_fullsize.py, test_gpu_coeff_edges.py).  A sum starts from +0.0 as np.add.at into zeros does: no
component of an answer is a negative zero.

Pair index (product.hip): pair (i, o) of inner row i and outer row o is term o * Ni + i; its row is inner[i] ^ outer[o] and its coefficient
c_i c_o i^e with e = 3 (Y_i + Y_o) + Y_out + 2 |x_left & z_right| mod 4, left = inner if inner_is_left else outer.  The output is ordered by
the first pair index of each row; in P * P (both orientations of every pair present) that is the identity first, then
min(i, o) * N + max(i, o), as tests/_expected.py states."""
import zlib

import numpy as np

UNITS = np.array([complex(1, 0), complex(0, 1), complex(-1, 0), complex(0, -1)])       # i^e (no negative zeros)
THR = 2.5


def wq_of(n):
    return max(1, (n + 63) // 64)


def random_rows(rng, T, n):
    """uint64[T, 2 Wq] packed rows (X words, then Z words; symmer_amd/packing.py), every one of the 2n bits set with probability 1/2."""
    wq = wq_of(n)
    w = rng.integers(0, 1 << 64, size=(T, 2 * wq), dtype=np.uint64)
    last = n - 64 * (wq - 1)
    if last < 64:
        mask = np.uint64((1 << last) - 1)
        w[:, wq - 1] &= mask
        w[:, 2 * wq - 1] &= mask
    return w


def units(rng, T):
    return UNITS[rng.integers(0, 4, T)]


def popcount(words):
    if hasattr(np, 'bitwise_count'):
        return np.bitwise_count(words).sum(axis=1, dtype=np.int64)
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)


def phase_exponent(left, right):
    """e of the header of product.hip for the row pairs (left[k], right[k])."""
    wq = left.shape[1] // 2
    y = lambda r: popcount(r[:, :wq] & r[:, wq:])
    return (3 * (y(left) + y(right)) + y(left ^ right) + 2 * popcount(left[:, :wq] & right[:, wq:])) % 4


class Product:
    """inner / outer: packed rows, ci / co: coefficients (outer is inner and co is ci: P * P); cand_i, cand_o: the listed pairs (P * P: each
    unordered pair once, i >= o, the diagonal included); relations: [(i_idx, o_idx, p)] with outer[o_idx[j]] == inner[i_idx[j]] ^ p."""

    def __init__(self, n, inner, ci, outer, co, cand_i, cand_o, thr=THR, relations=(), distinct=(True, True), note=''):
        self.n, self.inner, self.ci, self.outer, self.co, self.thr = n, inner, ci, outer, co, thr
        self.squared = outer is inner
        self.Ni, self.No = inner.shape[0], outer.shape[0]
        pid = np.unique(np.asarray(cand_o, dtype=np.int64) * self.Ni + np.asarray(cand_i, dtype=np.int64))      # a pair listed twice counts once
        self.cand_i, self.cand_o = pid % self.Ni, pid // self.Ni
        if self.squared:
            assert (self.cand_i >= self.cand_o).all()
        self.relations, self.distinct, self.note = list(relations), distinct, note

    @property
    def n_pairs(self):
        return self.Ni * self.No

    def pair_coeff(self, i, o, inner_is_left=True):
        I, O = self.inner[i], self.outer[o]
        e = phase_exponent(I, O) if inner_is_left else phase_exponent(O, I)
        return self.ci[i] * self.co[o] * UNITS[e]

    def _groups(self, i, o):
        rows = np.ascontiguousarray(self.inner[i] ^ self.outer[o])
        key = rows.view(np.dtype((np.void, rows.shape[1] * 8))).ravel()
        return np.unique(key, return_inverse=True)[1].ravel()

    def answer(self, inner_is_left=True):
        """-> (rows, coeff, first_i, first_o) of the complete output, in output order."""
        i, o = self.cand_i, self.cand_o
        if self.squared:                                                # both orientations of every pair off the diagonal
            off = i != o
            i, o = np.concatenate([i, o[off]]), np.concatenate([o, i[off]])
        inv = self._groups(i, o)
        c = self.pair_coeff(i, o, inner_is_left)
        G = int(inv.max()) + 1
        re, im = np.zeros(G), np.zeros(G)
        np.add.at(re, inv, c.real); np.add.at(im, inv, c.imag)
        first = np.full(G, np.iinfo(np.int64).max)
        np.minimum.at(first, inv, o * self.Ni + i)
        keep = re * re + im * im > self.thr * self.thr                 # integers against thr^2: nothing to round
        order = np.argsort(first[keep])
        first = first[keep][order]
        fi, fo = first % self.Ni, first // self.Ni
        return self.inner[fi] ^ self.outer[fo], (re[keep] + 1j * im[keep])[order], fi, fo

    def max_multiplicity(self):
        """Most KEYED pairs that share one row: all listed pairs, in P * P the pairs i > o (the diagonal is flagged by a loop of its own,
        pair_dups.hip).  16 pairs on one key saturate a 4-bit counter of the hash-table flag pass whatever the hash seed."""
        i, o = self.cand_i, self.cand_o
        if self.squared:
            off = i != o
            i, o = i[off], o[off]
        return int(np.bincount(self._groups(i, o)).max()) if i.size else 0

    def brute_first(self, row):
        """first pair index of a product row over ALL pairs, whatever the builder lists: for every outer row o in turn, the first inner row
        equal to row ^ outer[o] (CPU check of the listed first indices)."""
        if not hasattr(self, '_inner_first'):
            self._inner_first = {}
            for i in range(self.Ni - 1, -1, -1):
                self._inner_first[self.inner[i].tobytes()] = i
        for o in range(self.No):
            i = self._inner_first.get((self.outer[o] ^ row).tobytes())
            if i is not None:
                return o * self.Ni + i
        return -1


# ---------------------------------------------------------------- families ------------------------------------------------------------------
MS_ALL = (2, 3, 8, 15, 16, 40)
MS_SMALL = (2, 3, 8)


def _pairs_all(a, b):
    return np.repeat(a, len(b)), np.tile(b, len(a))


def _tri(s):
    """every unordered pair of the index set s, larger index first"""
    s = np.asarray(s, dtype=np.int64)
    x, y = np.triu_indices(len(s), 1)
    return np.maximum(s[x], s[y]), np.minimum(s[x], s[y])


def planted(rng, Ni, No=None, n=100, ms=MS_ALL, n_extra=1000, heavy=0, zero_p=False):
    """General (No given): for each multiplicity m of `ms`, m disjoint index pairs (i_j, o_j) and a random row p with B[o_j] = A[i_j] ^ p:
    row p occurs m times, each cross row A[i_j] ^ A[i_k] ^ p twice — as the pairs (i_j, o_k) and (i_k, o_j).  Squared (No None):
    A[o_j] = A[i_j] ^ p; then {i_j, i_k} and {o_j, o_k} share a row as well.  The first group holds the corner pairs — general (0, 0) and
    (Ni-1, No-1), whose cross pairs are the corners (Ni-1, 0) and (0, No-1); squared (1, 0) and (N-1, N-2), cross pair (N-1, 0).
    `n_extra` further groups of m = 2 (as many as fit beside a tenth of ordinary rows).  heavy: that many terms outside every group with
    coefficient 4 — their pairs survive ALONE (|c| = 4; P * P: twin sums 8 or 0).  zero_p: p = 0, the operands SHARE rows and p is the
    identity, found through the zero-word rule of the flag pass.
    How many rows of two pairs the extra groups give: a group of m = 2 is two such rows in a general product and three in P * P.  The default
    of 1,000 groups ("about 2,000 rows") fits from about 2,350 outer terms and from 4,650 terms squared on; the smaller shapes get what
    fits — 519 groups at 1255 x 1254, 742 at 1800 x 1750, 355 at 1774 squared, 520 at 2508 squared —, about half.  Which product bucket a
    planted pair falls into depends on the row hash, which only the library computes: that some of them fall into product bucket 0 (the
    `inside` loop of P * P) rests on their number — 1,065 planted rows over the 256 buckets of 1774 squared leave bucket 0 empty with
    probability e^-4.2 — and is not checked on the CPU.
    General products: the planted outer terms o_j have coefficient 2 x a unit.  With units alone a row that two pairs form sums to at most
    2 and would be dropped like the single terms: a lost merge would not show.  Now a single pair of an o_j has |c| = 2 (dropped), a row of
    two pairs 0, 2.83 or 4 — three in four survive.  (P * P needs none of it: its rows of two pairs are two twin sums of 0 or 2 each.)"""
    squared = No is None
    A = random_rows(rng, Ni, n)
    B = A if squared else random_rows(rng, No, n)
    ca = units(rng, Ni)
    cb = ca if squared else units(rng, No)
    if squared:
        corner_i, corner_o = [1, Ni - 1], [0, Ni - 2]
        pool = rng.permutation(np.arange(2, Ni - 2))
    else:
        corner_i, corner_o = [0, Ni - 1], [0, No - 1]
        pool = rng.permutation(np.arange(1, Ni - 1))
        pool_o = rng.permutation(np.arange(1, No - 1))
    used = [0, 0]

    def pool_take(k, side=0):
        src = pool if side == 0 or squared else pool_o
        s = 0 if squared else side
        out = src[used[s]:used[s] + k]
        assert out.size == k, 'the operands are too short for what is planted'
        used[s] += k
        return out

    heavy_idx = pool_take(heavy)
    ca[heavy_idx] = 4.0
    per_group = 4 if squared else 2
    room = (len(pool) if squared else min(len(pool), len(pool_o))) * 9 // 10 - per_group // 2 * sum(ms) - heavy
    n_extra = max(0, min(n_extra, room // per_group))
    ci_, co_, relations = [], [], []
    for g, m in enumerate(list(ms) + [2] * n_extra):
        k = m - 2 if g == 0 else m
        ii = np.concatenate([corner_i if g == 0 else [], pool_take(k, 0)]).astype(np.int64)
        oo = np.concatenate([corner_o if g == 0 else [], pool_take(k, 1)]).astype(np.int64)
        p = np.zeros_like(A[0]) if zero_p else random_rows(rng, 1, n)[0]
        B[oo] = A[ii] ^ p
        if not squared:
            cb[oo] *= 2.0
        relations.append((ii, oo, p))
        x, y = _tri(np.concatenate([ii, oo])) if squared else _pairs_all(ii, oo)
        ci_.append(x); co_.append(y)
    if squared:
        d = np.arange(Ni)
        ci_.append(d); co_.append(d)                                    # the diagonal: the identity
        for h in heavy_idx:
            ci_.append(np.maximum(d, h)); co_.append(np.minimum(d, h))
    else:
        x, y = _pairs_all(heavy_idx, np.arange(No))
        ci_.append(x); co_.append(y)
    return Product(n, A, ca, B, cb, np.concatenate(ci_), np.concatenate(co_), relations=relations,
                   note=f'planted ms={tuple(ms)} + {n_extra} x 2, heavy={heavy}, zero_p={zero_p}')


def shared_rows(rng, Ni, No=None, n=100, m=3):
    """General: the operands share m rows (B[o_j] = A[i_j]): the identity occurs m times, found through the zero-word rule, and each
    A[i_j] ^ A[i_k] twice.  Squared: m rows of P are repeated — twice (odd j; the copy has the negated coefficient) or three times (even
    j: c, -c and a third unit) —, which gives identity pairs OFF the diagonal, inside one operand bucket, and every other term a row it
    shares between the copies (sums 0, or 2 for the triples: dropped; the SECOND repeated row keeps its sign, so its sums with the terms that
    commute with it are 4 and survive — about N / 2 rows that are lost if those merges are)."""
    if No is not None:
        return planted(rng, Ni, No, n, ms=(m,), n_extra=0, zero_p=True)
    A = random_rows(rng, Ni, n)
    ca = units(rng, Ni)
    pool = rng.permutation(Ni)
    used, ci_, co_, relations = 0, [np.arange(Ni)], [np.arange(Ni)], []
    everyone = np.arange(Ni)
    for j in range(m):
        k = 3 if j % 2 == 0 else 2
        s = pool[used:used + k]; used += k
        A[s[1:]] = A[s[0]]
        ca[s[1]] = ca[s[0]] if j == 1 else -ca[s[0]]
        relations.append((np.repeat(s[0], k - 1), s[1:], np.zeros_like(A[0])))
        for x in s:
            ci_.append(np.maximum(everyone, x)); co_.append(np.minimum(everyone, x))
    return Product(n, A, ca, A, ca, np.concatenate(ci_), np.concatenate(co_), relations=relations, distinct=(False, False),
                   note=f'shared rows m={m} (squared: doubles and triples)')


def every_row_twice(rng, Ni, No, n=100, corner=32):
    """A = {r, r ^ g}, B = {r', r' ^ g}: (a, b) and (a', b') of the partners form the same row, so EVERY product row occurs exactly
    twice and every pair is listed by the flag pass.  Only the first `corner` rows r, r' and their partners have a coefficient (a unit:
    sums 0, +-2, +-2i, thr = 1.5); all others have coefficient 0, whose pairs are exact zeros and dropped: the answer is at most
    2 * corner^2 rows.  (An odd operand gets one more random row with coefficient 0.)"""
    g = random_rows(rng, 1, n)[0]
    ops = []
    for T in (Ni, No):
        K = T // 2
        R = random_rows(rng, T, n)
        R[K:2 * K] = R[:K] ^ g
        c = np.zeros(T, dtype=complex)
        live = np.concatenate([np.arange(corner), K + np.arange(corner)])
        c[live] = units(rng, 2 * corner)
        ops.append((R, c, live, K))
    (A, ca, la, Ka), (B, cb, lb, Kb) = ops
    x, y = _pairs_all(la, lb)
    P = Product(n, A, ca, B, cb, x, y, thr=1.5, relations=(), note=f'every row twice, {corner} live rows a half')
    P.partner = (Ka, Kb, g)
    return P


def block(rng, Ni, No, n=100, r=200, s=100):
    """One row u of A appears r times and one row v of B s times (all copies with coefficient 1), every other row once: u ^ v occurs r s
    times (|c| = r s), a row u ^ B[b] r times (|c| = r) and a row A[a] ^ v s times (|c| = s)."""
    A, B = random_rows(rng, Ni, n), random_rows(rng, No, n)
    ca, cb = units(rng, Ni), units(rng, No)
    ra, sb = np.sort(rng.choice(Ni, r, replace=False)), np.sort(rng.choice(No, s, replace=False))
    A[ra] = A[ra[0]]; B[sb] = B[sb[0]]
    ca[ra] = 1.0; cb[sb] = 1.0
    x1, y1 = _pairs_all(ra, np.arange(No))
    x2, y2 = _pairs_all(np.arange(Ni), sb)
    P = Product(n, A, ca, B, cb, np.concatenate([x1, x2]), np.concatenate([y1, y2]), distinct=(False, False), note=f'block {r} x {s}')
    P.copies = (ra, sb)
    return P


FAMILIES = {
    'planted': lambda rng, Ni, No, n: planted(rng, Ni, No, n, ms=MS_ALL, heavy=4),
    'planted-small': lambda rng, Ni, No, n: planted(rng, Ni, No, n, ms=MS_SMALL, heavy=4),
    'shared-3': lambda rng, Ni, No, n: shared_rows(rng, Ni, No, n, m=3),
    'shared-15': lambda rng, Ni, No, n: shared_rows(rng, Ni, No, n, m=15),
    'shared-16': lambda rng, Ni, No, n: shared_rows(rng, Ni, No, n, m=16),
    'twice': lambda rng, Ni, No, n: every_row_twice(rng, Ni, No, n),
    'block-200x100': lambda rng, Ni, No, n: block(rng, Ni, No, n, 200, 100),
    'block-300x5': lambda rng, Ni, No, n: block(rng, Ni, No, n, 300, 5),
    'block-300x300': lambda rng, Ni, No, n: block(rng, Ni, No, n, 300, 300),
}


def make(family, Ni, No=None, n=100):
    """The operands of `family` at a shape (No None: P * P), the same ones wherever they are asked for."""
    rng = np.random.default_rng([Ni, No or 0, n, zlib.crc32(family.encode())])
    return FAMILIES[family](rng, Ni, No, n)


# ---------------------------------------------------------------- the plan, restated --------------------------------------------------------
# pair_dups.hip
PD_THREADS, PD_QUOTA, PD_TARGET, PD_SLOT_BITS, PD_CAND, PD_CHAIN, PD_MIN_B, PD_TARGET_16, PD_MAX_BUCKET = 1024, 16, 12288, 17, 1792, 1024, 8, 9216, 255
PD_LDS_MAX = 160 * 1024 - 512
SUS_RUN_BITS = 16


def pd_lds_bytes(n_tab, nb, squared, sb):
    cap = nb // 2 + 4 if squared else nb
    return ((n_tab + 3) & ~3) * 4 + (1 << (sb - 3)) * 4 + cap * 8 + PD_CAND * 12 + PD_CHAIN * 4 + PD_THREADS * 4 + (1 if squared else 2) * (nb + 4) * 2


def pair_dups_fits(Ni, No, squared, Tk, direct=True):
    """-> (B, sb) of the hash-table flag pass, or None where the product does not take it."""
    if not direct:
        return None
    nI, nO = Ni, 0 if squared else No
    if nI + nO > 65535 or nI < 2 or (not squared and nO < 1):
        return None
    B, sb = 2, PD_SLOT_BITS
    while B < 12 and (Tk >> B) > PD_TARGET:
        B += 1
    if (Tk >> B) > PD_TARGET:
        B, sb = 13, 16
        if (Tk >> B) > PD_TARGET_16:
            return None
    if B < PD_MIN_B:
        return None
    if pd_lds_bytes(nI + nO, 1 << B, squared, sb) > PD_LDS_MAX:
        return None
    return B, sb


def sorted_bits(n, cap):
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min((lg + 5 + 7) // 8 * 8, cap)


def plan_cleanup(Ni, No, same, thr=THR, unpacked=False, nosquare=False, lazy=-1, suspects=1, key_bytes=True, direct=True, full_sort=False):
    """plan_cleanup of cleanup_driver.hip for a product (pair mode, rows of fewer than 256 chunks and SYMGPU_WIDE unset: the wide pair kernel
    never competes).  The switches are the SYMGPU_CLEANUP_* variables of the same names."""
    bi = bo = 0
    while (1 << bi) < Ni: bi += 1
    while (1 << bo) < No: bo += 1
    pl = {'bi': bi, 'bo': bo}
    pl['packed'] = bi + bo <= 32 and bi < 32 and not unpacked and not full_sort
    pl['squared'] = pl['packed'] and same and thr is not None and thr > 0 and not nosquare
    pl['Tk'] = Tk = Ni * (Ni + 1) // 2 if pl['squared'] else Ni * No
    pl['nbits'] = 64 if full_sort else sorted_bits(Tk, 64 - (bi + bo + 2) if pl['packed'] else 64)
    pl['lazy'] = lazy == 1 or (lazy == -1 and Tk >= (1 << (20 if pl['squared'] else 18)))
    pl['sus_try'] = pl['packed'] and pl['lazy'] and suspects != 0 and pl['nbits'] == 32 and (Tk >> SUS_RUN_BITS) <= 2048 and not (same and not pl['squared'])
    fits = pair_dups_fits(Ni, No, pl['squared'], Tk, direct) if pl['sus_try'] else None
    pl['direct'] = fits
    pl['key_bytes'] = fits is not None and key_bytes
    return pl


def flow_name(pl):
    if not pl['packed']: return '64-bit keys + index sort'
    if not pl['sus_try']: return 'complete sort' + (', lazy' if pl['lazy'] else ', not lazy')
    if pl['direct'] is None: return 'sorted flag pass'
    return f"hash-table flag pass B = {pl['direct'][0]}" + (', 16-bit counters' if pl['direct'][1] == 16 else '') + (', bytes' if pl['key_bytes'] else ', keys')


# the counters of the product + cleanup flows, by name (SYMGPU_COUNTER_LIST of include/symgpu.h), in id order; C_* index this tuple
FLOW_COUNTERS = ('FLOW_COMPLETE_SORT', 'FLOW_FLAGS_HASH_TABLES', 'FLOW_FLAGS_PARTIAL_SORT', 'FLOW_FLAGS_GAVE_UP',
                 'GIVEUP_PRODUCT_BUCKET', 'GIVEUP_COUNTER_SATURATED', 'GIVEUP_LIST_OVERFLOW', 'GIVEUP_OPERAND_BUCKET',
                 'FLOW_SORTED_WHOLE', 'FLOW_SORTED_FLAGGED', 'FLOW_MARKED_FROM_BYTES', 'FLOW_FULL_SORT_REPEAT')
C_FULL, C_DIRECT, C_SORTED, C_GIVEUP, C_R_BUCKET, C_R_SAT, C_R_LIST, C_R_OPERAND, C_WHOLE, C_ALONE, C_BYTES, C_REPEAT = range(12)
# ProductPath of product_common.h, in the enum's order (its counters: PRODUCT_* of the same list)
PRODUCT_PATHS = ('rows only', 'phase stream', 'wide coefficients, then rows', 'word-major coefficients, then rows', 'word-major coefficients beside rows')


def expected_counters(pl, outcome='alone', reasons=()):
    """What ONE attempt of cleanup_run counts for the plan `pl`.  outcome matters where the plan launches a flag pass:
      'alone'    the pass completed and the flagged keys were sorted alone;
      'whole'    the whole array was sorted after it — most keys flagged or SYMGPU_CLEANUP_SUSPECTS=2 (no give-up), or, with `reasons`,
                 a give-up of the hash-table pass for exactly those reasons (C_R_*);
      'gave up'  the whole array was sorted after a give-up that names no reason: the pass behind the partial sort (k_find_suspects)."""
    v = [0] * 12
    if not pl['packed']:
        return v
    if not pl['sus_try']:
        v[C_FULL] = 1
        return v
    v[C_DIRECT if pl['direct'] else C_SORTED] = 1
    v[C_BYTES] = 1 if pl['key_bytes'] else 0
    if outcome == 'alone':
        v[C_ALONE] = 1
    else:
        v[C_WHOLE] = 1
        for r in reasons:
            v[r] = 1
        if reasons or outcome == 'gave up':
            v[C_GIVEUP] = 1
    return v
