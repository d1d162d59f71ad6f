"""Operands for the commutation kernels whose tables hold BY CONSTRUCTION (plain NumPy, seeded; neither the oracle nor the library is
called here — tests/test_commute_families.py proves the claimed answers against oracle_np.commutes_termwise on the CPU, and
tests/test_gpu_commute_families.py runs them through every commutation kernel).

Notation.  A symplectic row is [x_0..x_{n-1} | z_0..z_{n-1}]; symplectic column p < n is X of qubit p, column p >= n is Z of qubit p - n.
Packed (symmer_amd/packing.py) with Wq = max(1, ceil(n / 64)) words a half, column p sits at packed bit p (X half) or 64 Wq + p - n
(Z half).  The Four-Russians kernel (csrc/commute_m4r7.hip) cuts the packed row of the LEFT operand into 7-bit groups: group g is packed
bits [7g, 7g + 7), ng7 = ceil(128 Wq / 7) of them; it runs one step per PAIR of groups in which the left operand has any non-zero value
(an odd count is padded with an all-zero group), so S = ceil(k / 2) steps a tile for k non-zero groups.  Contraction bit c of the left
operand meets bit c + 64 Wq (c in the X half) or c - 64 Wq (Z half) of the right operand: partner(p) = p + n for p < n, else p - n.

True = the two terms commute, as everywhere in this project."""
import numpy as np


def wq_of(n):
    return max(1, (n + 63) // 64)


def ng7_of(n):
    return (128 * wq_of(n) + 6) // 7


def packed_bit(n, p):
    """Packed bit of symplectic column p (scalar or array)."""
    p = np.asarray(p)
    return np.where(p < n, p, 64 * wq_of(n) + p - n)


def partner(n, p):
    """The symplectic column that column p is contracted with (X of a qubit <-> Z of the same qubit)."""
    p = np.asarray(p)
    return np.where(p < n, p + n, p - n)


def group_of(n, p):
    """7-bit group of the packed row that symplectic column p falls in."""
    return packed_bit(n, p) // 7


def describe_column(n, p):
    """Where symplectic column p of a LEFT operand lives in the kernels' terms: for failure messages."""
    c = int(packed_bit(n, p)); q = int(packed_bit(n, partner(n, p)))
    return (f'symplectic column {int(p)} ({"X" if p < n else "Z"} of qubit {int(p) % n if n else 0}): packed bit {c} = word {c // 64} bit {c % 64}, '
            f'7-bit group {c // 7} bit {c % 7}; pairs with packed bit {q} of the right operand')


def random_bits(rng, shape):
    """bool array at density 0.5 (one byte of generator output per 8 entries)."""
    n = int(np.prod(shape))
    return np.unpackbits(np.frombuffer(rng.bytes((n + 7) // 8), dtype=np.uint8), count=n).astype(bool).reshape(shape)


def pack_cols(mat):
    """bool[R, C] -> uint64[R, ceil(C / 64)], bit j of word w = column 64 w + j, padding bits zero (the layout of a bit-packed table)."""
    mat = np.asarray(mat, dtype=bool)
    R, C = mat.shape
    wc = max(1, (C + 63) // 64)
    by = np.packbits(mat, axis=1, bitorder='little')
    out = np.zeros((R, wc * 8), dtype=np.uint8)
    out[:, :by.shape[1]] = by
    return out.view('<u8')


def unpack_cols(words, n_cols):
    words = np.ascontiguousarray(words, dtype='<u8')
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')[:, :n_cols].astype(bool)


# ---------------------------------------------------------------- one contraction bit a row -----------------------------------------------
def one_hot(n, M, rng, cols=None):
    """(A, B, C): A = the one-hot rows of the symplectic columns `cols` (default: all 2n of them, i.e. the 2n x 2n identity — row p holds
    only column p), B = M rows at density 0.5 with B[0] all zero and B[1] all ones.  Row p of A contracts exactly one bit, so
    C[p, j] = not B[j, partner(p)]: a wrong pairing of ONE contraction bit is a wrong named row of C (left operand) or column of C.T
    (right operand: commutation is symmetric, C.T is the table of (B, A))."""
    assert M >= 2
    cols = np.arange(2 * n) if cols is None else np.asarray(cols, dtype=np.int64)
    A = np.zeros((cols.size, 2 * n), dtype=bool)
    A[np.arange(cols.size), cols] = True
    B = random_bits(rng, (M, 2 * n))
    B[0] = False
    B[1] = True
    C = ~B[:, partner(n, cols)].T
    return A, B, np.ascontiguousarray(C)


# ---------------------------------------------------------------- rows that are dense across every word -----------------------------------
def majorana_stack(n):
    """(A, C): the 2n Jordan-Wigner Majorana strings gamma_{2j+k} = Z_0 .. Z_{j-1} (X_j if k = 0 else Y_j), then the n + 1 prefixes
    P_k = Z_0 .. Z_{k-1} (P_0 = identity).  C is the (3n + 1)^2 table of A with itself: distinct Majoranas anticommute (gamma block = identity
    matrix), Z strings commute (P block all True), and P_k meets gamma_{2j+k'} in the one anticommuting position j iff j < k, so
    C[P_k, gamma_{2j+k'}] = (j >= k); symmetric.  The rows run through every word of both halves: a dropped word or half shows on a whole
    triangle."""
    T = 3 * n + 1
    A = np.zeros((T, 2 * n), dtype=bool)
    j = np.arange(n)
    for k in (0, 1):
        A[2 * j + k, j] = True                                        # X part of X_j / Y_j
        if k:
            A[2 * j + k, n + j] = True                                # Y = X and Z
    below = j[None, :] < j[:, None]                                   # [j, q]: q < j
    A[0:2 * n:2, n:] |= below
    A[1:2 * n:2, n:] |= below
    A[2 * n:, n:] = j[None, :] < np.arange(n + 1)[:, None]            # P_k: Z on qubits < k
    C = np.zeros((T, T), dtype=bool)
    C[:2 * n, :2 * n] = np.eye(2 * n, dtype=bool)
    C[2 * n:, 2 * n:] = True
    pg = np.repeat(j, 2)[None, :] >= np.arange(n + 1)[:, None]        # [k, 2j + k']: j >= k
    C[2 * n:, :2 * n] = pg
    C[:2 * n, 2 * n:] = pg.T
    return A, C


# ---------------------------------------------------------------- left operands that live in named 7-bit groups ---------------------------
def live_columns(n, groups):
    """The symplectic columns whose packed bit lies in one of the 7-bit groups (padding bits of a half belong to no column)."""
    p = np.arange(2 * n)
    return p[np.isin(group_of(n, p), np.asarray(sorted(groups)))]


def steps_of(groups):
    """Steps a tile of the Four-Russians kernel for a left operand with these non-zero groups: pairs of groups, at least one."""
    return max(1, (len(set(groups)) + 1) // 2)


def group_sets(n):
    """Named sets of 7-bit groups, derived from n (Wq >= 2).  At n = 100: first {0}, word_straddle {9}, half_straddle+last {18, 32},
    odd3 {0, 9, 18}, five {0, 9, 14, 18, 27}.  With more than 64 groups (n = 257: 92) also half_straddle alone {45} and `high`
    {64, 73, 82}: nothing below group 64, so the first ballot round of the group compaction finds nothing."""
    wq = wq_of(n)
    assert wq >= 2 and (64 * wq) % 7 != 0, 'the sets need a second word and a group across the X/Z boundary'
    half = 64 * wq
    word_x = 63 // 7                                                  # holds packed bits 63 and 64: words 0 / 1 of the X half
    assert word_x == 64 // 7
    half_straddle = (half - 1) // 7                                   # holds the last bit of the X half and the first of the Z half
    assert half_straddle == half // 7
    word_z = (half + 63) // 7                                         # words 0 / 1 of the Z half
    assert word_z == (half + 64) // 7
    last_x = int(group_of(n, n - 1))                                  # the last live X column
    last = int(group_of(n, 2 * n - 1))                                # the last live column of the row
    sets = {
        'first': {0},
        'word_straddle': {word_x},
        'half_straddle+last': {half_straddle, last},
        'odd3': {0, word_x, half_straddle},
        'five': {0, word_x, last_x, half_straddle, word_z},
    }
    if ng7_of(n) > 64:
        sets['half_straddle'] = {half_straddle}
        z_words = [g for g in range(64, last) if (7 * g) // 64 != (7 * g + 6) // 64]   # groups >= 64 across a word boundary
        sets['high'] = {64, z_words[len(z_words) // 2], last}
        assert min(sets['high']) >= 64 and len(sets['high']) == 3
    for name, s in sets.items():
        assert all(live_columns(n, {g}).size for g in s), f'{name}: a group without a live column'
    return {k: sorted(v) for k, v in sets.items()}


def nonzero_groups(packed, n):
    """The 7-bit groups in which any of the packed rows (uint64[T, 2 Wq]) has a set bit."""
    packed = np.ascontiguousarray(packed, dtype='<u8')
    bits = np.unpackbits(packed.view(np.uint8).reshape(packed.shape[0], -1), axis=1, bitorder='little').any(axis=0)
    ng7 = ng7_of(n)
    padded = np.zeros(7 * ng7, dtype=bool)
    padded[:bits.size] = bits
    return sorted(np.flatnonzero(padded.reshape(ng7, 7).any(axis=1)).tolist())


def sparse_groups(n, groups, N, M, rng):
    """(A, B, Cbits): A = N rows at density 0.5 inside the live bits of the listed groups, zero elsewhere, row 0 the identity; B = M rows
    at density 0.5.  Cbits = the table BIT-PACKED (uint64[N, ceil(M / 64)], padding bits zero): row i is the complement of the XOR, over
    the set columns p of A[i], of column partner(p) of B — accumulated column by column on packed words (at most 7 columns a group)."""
    cols = live_columns(n, groups)
    A = np.zeros((N, 2 * n), dtype=bool)
    A[:, cols] = random_bits(rng, (N, cols.size))
    A[0] = False
    for g in groups:                                                  # every listed group is non-zero whatever the draw
        A[1 + list(groups).index(g), live_columns(n, {g})[0]] = True
    B = random_bits(rng, (M, 2 * n))
    Bt = pack_cols(np.ascontiguousarray(B[:, partner(n, cols)].T))    # [live column, Mw]
    acc = np.zeros((N, Bt.shape[1]), dtype='<u8')
    for k in range(cols.size):
        rows = np.flatnonzero(A[:, cols[k]])
        acc[rows] ^= Bt[k]
    np.invert(acc, out=acc)
    if M % 64:
        acc[:, -1] &= np.uint64((1 << (M % 64)) - 1)
    return A, B, acc
