"""Structured operators and bases for ``PauliwordOp.to_sparse_matrix`` (csrc/sparse_matrix.hip) and ``PauliwordOp.from_matrix``
(csrc/pauli_decomp.hip): every builder returns ``(symp, coeff, facts)`` (host only: NumPy, no GPU), where ``facts`` names what the
family was built to hit.  tests/test_csr_families.py proves the facts with the NumPy restatements; tests/test_gpu_csr_families.py and
tests/test_gpu_from_matrix.py run the device code on them.

An X-part or Z-part written as an integer has qubit 0 as its MOST significant bit, as everywhere in the contract; the device groups
the terms by the bit-REVERSED X word (``sort_key``), stably, so ``sorted_order`` is the order in which the row sums walk the terms.
"""
import numpy as np

# the fill's constants (csrc/sparse_matrix.hip): 72 KiB of slots per workgroup, 20 B per slot, at most 256 and at least 32 rows
SLOT_LDS, SLOT_BYTES, WG_ROWS, MIN_LDS_ROWS = 72 * 1024, 20, 256, 32
TILE = 256                                    # sorted terms staged per round of the row sums
SCAN_ITEMS = 4096                             # rows per workgroup of the 64-bit scan; its top level takes 256 of these per round


def bits_of(value, n):
    """bool[n] of an n-bit integer, qubit 0 the most significant bit."""
    return np.array([(int(value) >> (n - 1 - q)) & 1 for q in range(n)], dtype=bool)


def symp_of(xs, zs, n):
    return np.array([np.concatenate([bits_of(x, n), bits_of(z, n)]) for x, z in zip(xs, zs)], dtype=bool).reshape(len(xs), 2 * n)


def x_ints(symp):
    n = symp.shape[1] // 2
    return symp[:, :n].astype(np.int64) @ (np.int64(1) << np.arange(n - 1, -1, -1, dtype=np.int64))


def sort_key(symp):
    """The device's grouping key: the X word read with qubit 0 as the LEAST significant bit."""
    n = symp.shape[1] // 2
    return symp[:, :n].astype(np.int64) @ (np.int64(1) << np.arange(n, dtype=np.int64))


def sorted_order(symp):
    """Operator indices in the order of the row sums: ascending key, operator order within a key (the sort is stable)."""
    return np.argsort(sort_key(symp), kind='stable')


def dyadic(rng, t):
    """Multiples of 1/8 between 1/8 and 1 of either sign in both components: sums of a few hundred are exact in any order, and no
    component is a zero whose sign a swap or a sum could change (signed zeros are the business of the 'zeros' kind)."""
    part = lambda: rng.integers(1, 9, t) * rng.choice([-1, 1], t) / 8.0
    return part() + 1j * part()


def fill_form(D, rows):
    """The fill's form for D X-parts, restated from the constants: (rows per workgroup, workgroups, rows of the last workgroup), or
    None where fewer than MIN_LDS_ROWS rows of D slots fit SLOT_LDS (the scratch form)."""
    if D * SLOT_BYTES * MIN_LDS_ROWS > SLOT_LDS:
        return None
    rb = min(WG_ROWS, SLOT_LDS // (SLOT_BYTES * D))
    groups = -(-rows // rb)
    return rb, groups, rows - (groups - 1) * rb


def mandatory_x_parts(n):
    """Qubit 0 only and qubit n-1 only (a wrong bit reversal maps one to the other and cannot cancel), the empty and the all-ones
    X-part (the two ends of the key range).  A set of fewer than four X-parts takes them in this order."""
    return [1 << (n - 1), 1, 0, (1 << n) - 1]


# ---- X-part sets: the boundaries of the fill form -------------------------------------------------------------------------------
X_PART_COUNTS = (1, 14, 15, 20, 115, 116)


def x_part_set(D, n=9, seed=0):
    """Exactly D distinct X-parts (the mandatory four first), two or three terms each with random Z-parts, in shuffled operator
    order, dyadic coefficients."""
    rng = np.random.default_rng(9000 + 31 * D + seed)
    must = mandatory_x_parts(n)[:D]
    others = [int(v) for v in rng.permutation(1 << n) if int(v) not in must][:D - len(must)]
    parts = np.array(must + others, dtype=np.int64)
    assert len(set(parts.tolist())) == D
    xs = np.concatenate([parts, parts, parts[rng.random(D) < 0.5]])
    xs = xs[rng.permutation(len(xs))]
    zs = rng.integers(0, 1 << n, len(xs))
    form = fill_form(D, 1 << n)
    facts = {'n': n, 'D': D, 'x_parts': sorted(parts.tolist()), 'lds': form is not None,
             'rows_per_workgroup': form[0] if form else None, 'workgroups': form[1] if form else None,
             'last_workgroup_rows': form[2] if form else None, 'last_workgroup_short': bool(form and form[2] < form[0])}
    return symp_of(xs, zs, n), dyadic(rng, len(xs)), facts


# ---- term tiles: groups against the 256-term staging rounds -----------------------------------------------------------------------
# group sizes in SORTED order (keys 0, 1, 2^(n-1): the empty X-part, qubit 0 only, qubit n-1 only).  Slot 255 of a tile exists from
# T = 256 on and a pair of slots 255 / 256 from T = 257 on; both at once, on different groups, need two tile ends: T = 513.
TERM_TILE_SIZES = {255: (100, 100, 55), 256: (100, 100, 56), 257: (100, 100, 57), 512: (256, 100, 156), 513: (256, 100, 157)}


def term_tiles(T, n=8):
    """D = 3 and T terms whose groups meet the tile ends as `facts` says: 'ends_at_255' lists the groups (sorted order) whose last
    term sits in slot 255 of a tile, 'straddles' those that hold slot 255 of one tile and slot 0 of the next."""
    rng = np.random.default_rng(8000 + T)
    sizes = TERM_TILE_SIZES[T]
    by_key = [0, 1 << (n - 1), 1]                             # X-parts in ascending key order
    xs = np.concatenate([np.full(s, x, dtype=np.int64) for s, x in zip(sizes, by_key)])
    xs = xs[rng.permutation(T)]                               # operator order interleaves the groups: the sort has work to do
    zs = rng.integers(0, 1 << n, T)
    ends = np.cumsum(sizes) - 1
    starts = ends - np.array(sizes) + 1
    facts = {'n': n, 'D': 3, 'T': T, 'sizes': sizes,
             'ends_at_255': [g for g in range(3) if ends[g] % TILE == TILE - 1],
             'straddles': [g for g in range(3) if any(starts[g] <= p < ends[g] for p in range(TILE - 1, T, TILE))]}
    return symp_of(xs, zs, n), dyadic(rng, T), facts


# ---- more than 16 qubits ------------------------------------------------------------------------------------------------------------
LARGE_N = (17, 19, 21)


def large_n(n):
    """T = 6 over the X-parts {qubit 0}, {qubit 0, a middle qubit, qubit n-1} and, for the pair I + Z, the empty one.  The Z-parts touch
    qubit 0 and qubit n-1.  Every group is c P (1 + Z_w) with w the qubit of weight 2^12, so the rows with that bit set cancel to
    exact zeros in all three groups: every odd block of 4,096 rows is EMPTY (a zero in the scan's block sums), every other row holds
    three entries of value +-2c."""
    assert n > 13
    rng = np.random.default_rng(7000 + n)
    w = 1 << 12
    q0, qlast, qmid = 1 << (n - 1), 1, 1 << (n - 1 - n // 2)
    xa, xb = q0, q0 | qmid | qlast
    c = dyadic(rng, 3)
    xs = [xb, 0, xa, xb, 0, xa]
    zs = [qlast, 0, q0, qlast | w, w, q0 | w]
    coeff = np.array([c[0], c[1], c[2], c[0], c[1], c[2]])
    rows = 1 << n
    facts = {'n': n, 'D': 3, 'T': 6, 'x_parts': sorted([0, xa, xb]), 'nnz': 3 * (rows // 2), 'entries_per_full_row': 3,
             'scan_blocks': rows // SCAN_ITEMS, 'empty_scan_blocks': rows // SCAN_ITEMS // 2,
             'scan_top_rounds': -(-(rows // SCAN_ITEMS) // 256), 'sort_passes': -(-n // 8)}
    return symp_of(xs, zs, n), coeff, facts


# ---- coefficient kinds ----------------------------------------------------------------------------------------------------------------
COEFF_KINDS = ('dyadic', 'wide', 'nonfinite', 'zeros')


def _complex(re, im):
    out = np.empty(len(re), dtype=np.complex128)
    out.real, out.imag = re, im                               # component-wise: complex(-0.0, 0.0) arithmetic would lose the signs
    return out


def coeff_kind(kind, n=5):
    rng = np.random.default_rng(6000 + COEFF_KINDS.index(kind))
    parts = mandatory_x_parts(n)
    if kind == 'dyadic':
        xs = np.array(parts * 5, dtype=np.int64)[rng.permutation(20)]
        zs = rng.integers(0, 1 << n, 20)
        return symp_of(xs, zs, n), dyadic(rng, 20), {'n': n, 'D': 4, 'kind': kind}
    if kind == 'wide':
        # per group: five terms with ONE Z-part (the same sign in every row, so each row adds the same five numbers) and two others
        xs, zs = [], []
        for x in parts[:3]:
            shared = int(rng.integers(0, 1 << n))
            xs += [x] * 7
            zs += [shared] * 5 + [int(v) for v in rng.integers(0, 1 << n, 2)]
        order = rng.permutation(len(xs))
        xs, zs = np.array(xs)[order], np.array(zs)[order]
        t = len(xs)
        mag = lambda: 10.0 ** rng.uniform(-8, 8, t) * rng.choice([-1.0, 1.0], t)
        return symp_of(xs, zs, n), _complex(mag(), mag()), {'n': n, 'D': 3, 'kind': kind, 'min_shared_z': 5}
    inf, nan = np.inf, np.nan
    if kind == 'nonfinite':
        a, b, c, d = parts                                    # a: +inf alone; b: +inf and -inf with different Z-parts; c: NaN in the
        xs = [a, b, b, c, d]                                  # imaginary part only (x & z = 0: no swap); d: an ordinary term
        zs = [3, 2, 4, 0, 5]                                  # (x & z = 0 in a, b, c: no component swap moves the infinities apart)
        coeff = _complex([inf, inf, -inf, 1.0, 0.5], [0.0, 0.0, 0.0, nan, -0.25])
        return symp_of(xs, zs, n), coeff, {'n': n, 'D': 4, 'kind': kind, 'inf_alone': a, 'inf_meets': b, 'meet_z': (2, 4), 'nan_imag': c, 'plain': d}
    if kind == 'zeros':
        a, b, c, d = parts
        e = 5                                                 # a fifth X-part of ordinary terms
        xs = [a, b, c, c, d, d, e, e]
        zs = [1, 2, 7, 7, 9, 9, 4, 6]
        coeff = _complex([-0.0, 0.0, 0.75, -0.75, 1.0, -1.0, 0.5, 0.125], [0.0, -0.0, -1.5, 1.5, 2.0, 1.0, 0.25, -1.0])
        return symp_of(xs, zs, n), coeff, {'n': n, 'D': 5, 'kind': kind, 'never_stored': sorted([a, b, c]), 'stored': sorted([d, e]),
                                           'imag_only': d, 'imag_only_value': 3.0}
    raise KeyError(kind)


# ---- from_matrix: bases against the aligned blocks of 32 X-parts of the dense gather -------------------------------------------------
# per n, named bases; each lists what its aligned blocks of 32 X-parts hold: 'first' (bit 0 of the mask only), 'last' (bit 31 only),
# 'all' (all 32), 'mixed' (bits 0, 31 and a few between) or None (the block is absent from the launch)
BLOCK_BASES = {
    5: {'first': ['first'], 'last': ['last'], 'all': ['all']},
    6: {'first, last': ['first', 'last'], 'all, absent': ['all', None], 'absent, all': [None, 'all']},
    8: {'every kind': ['first', 'last', 'all', None, 'mixed', None, None, 'mixed']},
}


def block_basis(n, name):
    """(basis_x uint64[K], basis_z uint64[K], facts): one to three Z-parts per listed X-part, in shuffled order (not (x, z) order);
    facts['blocks'] = [(x0, rank of the block's first X-part, 32-bit mask)] of the present blocks in ascending order."""
    rng = np.random.default_rng(5000 + 97 * n + sum(map(ord, name)))
    layout = BLOCK_BASES[n][name]
    assert len(layout) == (1 << n) // 32
    xs = []
    for blk, what in enumerate(layout):
        if what == 'first':
            bits = [0]
        elif what == 'last':
            bits = [31]
        elif what == 'all':
            bits = list(range(32))
        elif what == 'mixed':
            bits = sorted({0, 31} | {int(v) for v in rng.integers(1, 31, 5)})
        else:
            bits = []
        xs += [32 * blk + j for j in bits]
    bx, bz = [], []
    for j, x in enumerate(xs):
        for z in rng.choice(1 << n, int(rng.integers(2 if j == 0 else 1, 4)), replace=False):
            bx.append(x)
            bz.append(int(z))
    order = rng.permutation(len(bx))
    if np.all(np.diff((np.array(bx) * (1 << n) + np.array(bz))[order]) > 0):
        order = order[::-1]                                   # a short list that the shuffle happened to leave in (x, z) order
    bx, bz = np.array(bx, dtype='<u8')[order], np.array(bz, dtype='<u8')[order]
    blocks, rank = [], 0
    for blk in range(len(layout)):
        inside = [x - 32 * blk for x in xs if x // 32 == blk]
        if inside:
            blocks.append((32 * blk, rank, sum(1 << j for j in inside)))
            rank += len(inside)
    return bx, bz, {'n': n, 'layout': layout, 'D': len(xs), 'K': len(bx), 'blocks': blocks}
