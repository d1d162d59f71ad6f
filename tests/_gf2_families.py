"""Seeded GF(2) matrix families, each built to steer one of the decisions that csrc/gf2.hip takes from the DATA (which panel a block
runs on, where its window starts, where a block ends).  Plain NumPy; shared by tests/test_gf2_families.py (the claimed structure, on
the CPU), tests/test_gpu_gf2_structure.py (the kernels against the C oracle) and tests/stress_gf2.py (long randomised runs).

Every family is ``f(rng, R, C, **kw) -> bool[R, C]``; column c is bit ``c % 64`` of word ``c // 64`` of a packed row (``pack``).  "Leads
at column c" = the row's leftmost set bit is c.  Geometry the docstrings refer to (gf2.hip): a block holds up to 64 consecutive rows; its
panel keeps a WINDOW of 2 ("narrow") or 4 words of every block row, starting at ``window_start``; rows of at most FULL_WC = 256 words
may instead be panelled on the full rows in LDS; matrices of at most 64 rows and 64 words take a one-workgroup path of their own."""
import numpy as np

WORD = 64
BLOCK = 64            # rows per block (WK)
WINDOW_WORDS = 4      # WN
FULL_WC = 256         # rows of more words never take the full-row panel


def pack(m):
    """bool[R, C] -> uint64[R, max(1, ceil(C / 64))], little-endian bit order, zero padding."""
    m = np.asarray(m, dtype=bool)
    R, C = m.shape
    wc = max(1, (C + WORD - 1) // WORD)
    bits = np.zeros((R, wc * WORD), dtype=bool)
    bits[:, :C] = m
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u8').reshape(R, wc)


def unpack(words, C):
    words = np.ascontiguousarray(words, dtype='<u8')
    R = words.shape[0]
    if R == 0:
        return np.zeros((0, C), dtype=bool)
    return np.unpackbits(words.view(np.uint8).reshape(R, -1), axis=1, bitorder='little')[:, :C].astype(bool)


def leads(m):
    """Leading column of every row, -1 for a zero row."""
    m = np.asarray(m, dtype=bool)
    if m.shape[1] == 0:
        return np.full(m.shape[0], -1, dtype=np.int64)
    first = np.argmax(m, axis=1).astype(np.int64)
    first[~m.any(axis=1)] = -1
    return first


def dense(rng, R, C, density=0.5):
    """Unstructured rows.  The pivots of a block are (nearly) consecutive columns, so every row of a block leads inside two words:
    the NARROW two-word window (panel_loop_narrow) on every block, about ceil(R / 64) blocks, never the full-row panel."""
    return rng.random((R, C)) < density


def staircase(rng, R, C, step=67, density=0.3):
    """Row r leads at column (r * step) mod C and carries noise to the right of it.  With step >= 64 consecutive rows lead in
    different words: the leads of a block are scattered far beyond a four-word window.  Rows of at most 256 words: a row among the
    first 32 leads outside the window -> the FULL-ROW panel.  Longer rows: the four-word window (panel_loop<4>), whose blocks END EARLY
    at the first row that leads outside it (a handful of rows per block)."""
    m = np.zeros((R, C), dtype=bool)
    for r in range(R):
        c0 = (r * step) % C
        m[r, c0] = True
        m[r, c0 + 1:] = rng.random(C - c0 - 1) < density
    return m


def reverse_staircase(rng, R, C, step=67, density=0.3):
    """Row r leads at column ((R - 1 - r) * step) mod C, noise to the right: LATER rows lead further LEFT.  The smallest leading word of
    a block lies far left of its first row, so window_start's clamp (never so far left that the first row falls out) decides every
    window; and the guess for the next window (w_next = the block's largest pivot word) is right of where the next block's first row
    leads: the speculatively loaded window is thrown away every time."""
    m = np.zeros((R, C), dtype=bool)
    for r in range(R):
        c0 = ((R - 1 - r) * step) % C
        m[r, c0] = True
        m[r, c0 + 1:] = rng.random(C - c0 - 1) < density
    return m


def window_twins(rng, R, C, w=128, density=0.5):
    """Row 2k+1 equals row 2k on its first w columns and differs beyond (column w is flipped, the rest is independent noise).  When
    row 2k becomes a pivot row, row 2k+1 cancels to ZERO on the columns it shares with it — inside a two-word window for w = 128, inside
    a four-word window for w = 256 or 300 — while being non-zero beyond: the block must END there and re-window at the twin's new
    leading word.  (Needs C > w for the twins to differ; with C <= w they are plain duplicates.)"""
    m = rng.random((R, C)) < density
    for k in range(R // 2):
        m[2 * k + 1, :w] = m[2 * k, :w]
        if w < C:
            m[2 * k + 1, w] = ~m[2 * k, w]
    return m


def low_rank(rng, R, C, k=20, density=0.3):
    """Every row is the XOR of a random subset of k basis rows: rank <= k.  From row k (or so) on, rows that are non-zero when their
    block is entered become GENUINELY zero in the middle of it (pivot -1 for a row that was not NOLEAD), and later blocks hold no pivot
    at all.  k = 63 / 64 / 65 puts the last pivot at the last row of the first block, or just beyond it."""
    basis = rng.random((k, C)) < density
    coef = rng.integers(0, 2, (R, k))
    return (coef @ basis.astype(np.int64)) % 2 == 1


def zero_and_duplicate(rng, R, C, density=0.5):
    """Dense rows with zero rows first (row 0), last (row R-1) and — from R = 130 on — 64 in a row (rows 64..127, the whole second block of
    an otherwise dense matrix), and copies of the first non-zero row (row 1) at every 37th row, so in every later block.  NOLEAD rows in
    every position of a block, a block of zero rows only (no window at all), `todo` skipping rows, copies that cancel to zero."""
    m = rng.random((R, C)) < density
    if R > 1:
        m[1, 0] = True                                            # row 1 is never zero
        for r in range(1 + 37, R, 37):
            m[r] = m[1]
    if R >= 130:
        m[64:128] = False
    elif R >= 8:
        m[R // 4:R // 2] = False
    m[0] = False
    m[R - 1] = False
    return m


def identity_plus_noise(rng, R, C, density=0.05, right=False):
    """The shape of the symmetry-generator matrices: an identity and noise to the right of it.  right=False: the identity on the first
    min(R, C) columns, noise on the columns behind it.  right=True: the identity on the LAST min(R, C) columns, noise to the right of the
    diagonal inside it, nothing to the left: every pivot lies in the last words of the rows.  Pivots at every bit position of a word,
    bit 0 and bit 63 included; sparse rows whose leads climb one column per row."""
    m = np.zeros((R, C), dtype=bool)
    n = min(R, C)
    off = C - n if right else 0
    m[np.arange(n), off + np.arange(n)] = True
    if right:
        m[:n, off:] |= np.triu(rng.random((n, n)) < density, 1)
        if R > n:
            m[n:, off:] = rng.random((R - n, n)) < density
    elif C > n:
        m[:, n:] = rng.random((R, C - n)) < density
    return m


def banded(rng, R, C, width=40, slope=None, fill=0.6):
    """Row r leads at column floor(r * slope) (default slope C / R: the band runs corner to corner) and is non-zero on `width` columns
    from there.  The 64 pivots of a block straddle about `slope` words: 2, 3, 4 or 5 words for slope 1.5 .. 4.5 — the two-word window, the
    four-word window that just holds a block, and the one that does not."""
    if slope is None:
        slope = C / max(1, R)
    m = np.zeros((R, C), dtype=bool)
    for r in range(R):
        c0 = min(C - 1, int(r * slope))
        w = min(C - c0, width)
        m[r, c0:c0 + w] = rng.random(w) < fill
        m[r, c0] = True
    return m


def single_column(rng, R, C, col=None):
    """Every row holds the same single column.  Row 0 pivots on it and every other row of its block holds it: mask_0 has the full
    height of the block (the first term of the XOR count, sum_j |mask_j|), every other row of the matrix becomes zero."""
    m = np.zeros((R, C), dtype=bool)
    m[:, (C // 2) if col is None else col] = True
    return m


def single_bit_rows(rng, R, C):
    """Row j holds one bit, at column (64 * j + 63) mod C: bit 63 of word j.  One-bit windows, a pivot in the top bit of a word, every
    row in a word of its own (and, once 64 * j + 63 wraps around C, rows that repeat an earlier row's column)."""
    m = np.zeros((R, C), dtype=bool)
    m[np.arange(R), (WORD * np.arange(R) + WORD - 1) % C] = True
    return m


# name -> (function, keyword sets to run it with): what the tests and the stress script iterate over
FAMILIES = {
    'dense': (dense, [dict(density=0.5), dict(density=0.2)]),
    'staircase': (staircase, [dict(step=67)]),
    'reverse_staircase': (reverse_staircase, [dict(step=67)]),
    'window_twins': (window_twins, [dict(w=w) for w in (64, 128, 192, 256, 300)]),
    'low_rank': (low_rank, [dict(k=k) for k in (1, 20, 63, 64, 65)]),
    'zero_and_duplicate': (zero_and_duplicate, [dict()]),
    'identity_plus_noise': (identity_plus_noise, [dict(right=False), dict(right=True)]),
    'banded': (banded, [dict(slope=s) for s in (1.5, 2.5, 3.5, 4.5)]),
    'single_column': (single_column, [dict()]),
    'single_bit_rows': (single_bit_rows, [dict()]),
}


def variants():
    """[(id, function, kwargs)] over FAMILIES, ids such as 'window_twins-w256'."""
    out = []
    for name, (fn, kws) in FAMILIES.items():
        for kw in kws:
            tag = '-'.join(f'{k}{v}' for k, v in kw.items())
            out.append((name + ('-' + tag if tag else ''), fn, kw))
    return out


def pivots_of(reduced):
    """Pivot column per row of a matrix reduced by the reference loop: the leading column of every non-zero row (-1 for a zero row)."""
    return leads(reduced)
