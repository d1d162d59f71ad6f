"""GPU: every commutation kernel (csrc/commute.hip, commute_m4r.hip, commute_m4r7.hip, the wide-row path of wide.hip; the path of a call is
planned in commute_driver.hip) on operands whose
tables hold BY CONSTRUCTION (tests/_commute_families.py; tests/test_commute_families.py proves the answers against the NumPy oracle on the
CPU), bit for bit, with the path each call took asserted through the debug counters (kernels.counters):

  COMMUTE_REGISTER_TILE  calls served by the register-tile kernel     COMMUTE_M4R_TILE     Four-Russians launches with one tile per workgroup
  COMMUTE_WIDE_ROWS      calls served by the wide-row kernel           COMMUTE_M4R_STREAMK  Four-Russians stream-K launches

What the families pin that dense random operands leave inside random sums:
  one_hot         one contraction bit a row — every pairing "bit c of the left operand with bit c +- 64 Wq of the right one", the 7-bit
                  groups across a word boundary, across the X/Z halves, the padding bits of the last group, more than 64 groups; a wrong
                  pairing is a wrong NAMED row (column) of the table, and the failure message says which group and word it is;
  majorana_stack  rows that run through every word of both halves, table = identity / triangles / ones;
  sparse_groups   left operands that are non-zero in named 7-bit groups only: the step count S of the Four-Russians kernel, and with it
                  the stream-K ranges, the hand-over of split tiles and k_m7_fixup, depend on the data — S = 1, 2, 3 instead of the maximum.
Every output buffer is pre-filled with junk and the bytes (words) around the table must stay untouched."""
import ctypes

import numpy as np
import pytest

from symmer_amd import kernels, packing, _lib, PauliwordOp
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
import _commute_families as fam

pytestmark = pytest.mark.gpu

ENV_NAMES = ('SYMGPU_COMMUTE_M4R', 'SYMGPU_M4R_R', 'SYMGPU_WIDE', 'SYMGPU_M4R_STREAM', 'SYMGPU_M4R_FIXUP', 'SYMGPU_M4R_UNFUSED')
PATHS = ('register tile', 'wide rows', 'Four-Russians, one tile per workgroup', 'Four-Russians, stream-K')
PATH_COUNTERS = ('COMMUTE_REGISTER_TILE', 'COMMUTE_WIDE_ROWS', 'COMMUTE_M4R_TILE', 'COMMUTE_M4R_STREAMK')    # the counter of each path
TILE, WIDE, M4R_ONE, M4R_STREAM = 0, 1, 2, 3
# forced kernel -> (switches, the path that must have served the call)
KERNELS = {
    'm4r-R16': ({'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': '16'}, M4R_ONE),
    'm4r-R24': ({'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': '24'}, M4R_ONE),
    'm4r-R48': ({'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': '48'}, M4R_ONE),
    'tile': ({'SYMGPU_COMMUTE_M4R': '0'}, TILE),
    'wide': ({'SYMGPU_COMMUTE_M4R': '0', 'SYMGPU_WIDE': '1'}, WIDE),
}


def set_switches(monkeypatch, env):
    for k in ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                      # read per call (commute_driver.hip read_commute_switches; SYMGPU_WIDE: wide.hip)


def counters():
    return kernels.counters(PATH_COUNTERS)


def counted(call, path, what):
    """Run one commutation call and assert that exactly the path `path` served it (a tuple: any one of them)."""
    paths = path if isinstance(path, tuple) else (path,)
    before = counters()
    out = call()
    delta = (counters() - before).tolist()
    took = [PATHS[k] for k in range(4) for _ in range(delta[k])]
    assert sum(delta) == 1 and any(delta[p] == 1 for p in paths), f'{what}: expected [{" | ".join(PATHS[p] for p in paths)}], the call took {took}'
    return out


# ---------------------------------------------------------------- calls into junk-filled buffers ------------------------------------------
def table_bytes(A, B, lo=None, hi=None, off=3):
    """uint8[hi - lo, M] written by symgpu_commutes_dev at `off` bytes into a device buffer of 0xEE; the other bytes must stay 0xEE."""
    lib = _lib.lib()
    lo = 0 if lo is None else lo
    hi = A.n_terms if hi is None else hi
    N, M = hi - lo, B.n_terms
    total = off + N * M + 64
    buf = ctypes.c_void_p()
    _lib.check(lib.symgpu_dev_alloc(total, ctypes.byref(buf)))
    try:
        got = np.full(total, 0xEE, dtype=np.uint8)
        _lib.check(lib.symgpu_dev_upload(buf, got.ctypes.data, total))
        _lib.check(lib.symgpu_commutes_dev(A.handle, lo, hi, B.handle, ctypes.c_void_p(buf.value + off)))
        _lib.check(lib.symgpu_dev_download(buf, got.ctypes.data, total))
    finally:
        lib.symgpu_dev_free(buf)
    assert np.all(got[:off] == 0xEE) and np.all(got[off + N * M:] == 0xEE), 'bytes outside the table were written'
    return got[off:off + N * M].reshape(N, M)


def table_bits(A, B, lo=None, hi=None, lead=1, tail=8):
    """uint64[hi - lo, ceil(M / 64)] written by symgpu_commutes_bits_dev `lead` words into a device buffer of all-ones words; the other
    words must stay all ones (and the kernel must overwrite every word of the table completely: its padding bits are zero)."""
    lib = _lib.lib()
    lo = 0 if lo is None else lo
    hi = A.n_terms if hi is None else hi
    N, M = hi - lo, B.n_terms
    words = (M + 63) // 64
    total = lead + N * words + tail
    buf = ctypes.c_void_p()
    _lib.check(lib.symgpu_dev_alloc(total * 8, ctypes.byref(buf)))
    try:
        got = np.full(total, 0xFFFFFFFFFFFFFFFF, dtype='<u8')
        _lib.check(lib.symgpu_dev_upload(buf, got.ctypes.data, total * 8))
        _lib.check(lib.symgpu_commutes_bits_dev(A.handle, lo, hi, B.handle, ctypes.c_void_p(buf.value + 8 * lead)))
        _lib.check(lib.symgpu_dev_download(buf, got.ctypes.data, total * 8))
    finally:
        lib.symgpu_dev_free(buf)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.all(got[:lead] == ones) and np.all(got[lead + N * words:] == ones), 'words outside the table were written'
    return got[lead:lead + N * words].reshape(N, words)


def first_difference(got_bits, want_bits):
    """(row, column) of the first differing bit of two bit-packed tables."""
    i, w = np.argwhere(got_bits != want_bits)[0]
    x = int(got_bits[i, w]) ^ int(want_bits[i, w])
    return int(i), 64 * int(w) + (x & -x).bit_length() - 1


def assert_bits(got, want_bits, what, where=None):
    assert got.shape == want_bits.shape, f'{what}: shape {got.shape}, expected {want_bits.shape}'
    if not np.array_equal(got, want_bits):
        i, j = first_difference(got, want_bits)
        n_bad = int(np.unpackbits((got ^ want_bits).view(np.uint8)).sum())
        raise AssertionError(f'{what} [bit-packed]: {n_bad} entries differ ({int((got != want_bits).any(axis=1).sum())} rows), first at ({i}, {j})'
                             + (': ' + where(i, j) if where else ''))


def assert_bytes(got, want_bits, what, where=None):
    """uint8 table against the bit-packed expectation: every byte 0 or 1, and the bits equal."""
    assert got.shape[0] == want_bits.shape[0], f'{what}: {got.shape[0]} rows, expected {want_bits.shape[0]}'
    assert got.max(initial=0) <= 1, f'{what} [bytes]: a byte that is neither 0 nor 1'
    packed = fam.pack_cols(got.view(np.bool_))
    if not np.array_equal(packed, want_bits):
        i, j = first_difference(packed, want_bits)
        raise AssertionError(f'{what} [bytes]: {int((packed != want_bits).any(axis=1).sum())} rows differ, first at ({i}, {j})'
                             + (': ' + where(i, j) if where else ''))


def both_outputs(A, B, want_bits, path, what, where=None, lo=None, hi=None):
    assert_bytes(counted(lambda: table_bytes(A, B, lo, hi), path, what), want_bits, what, where)
    assert_bits(counted(lambda: table_bits(A, B, lo, hi), path, what), want_bits, what, where)


_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ---------------------------------------------------------------- 1. every kernel on one_hot ----------------------------------------------
ONE_HOT_N = [1, 63, 64, 65, 100, 128, 257]      # 128 is beyond the issue's list: the only size whose half-straddling group is live on both sides
ONE_HOT_M = 2113                                 # two column tiles of the Four-Russians kernel, a partial last word


def one_hot_case(n, M=ONE_HOT_M):
    def build():
        A, B, C = fam.one_hot(n, M, np.random.default_rng(1000 + n))
        return packing.pack_rows(A), packing.pack_rows(B), fam.pack_cols(C), fam.pack_cols(np.ascontiguousarray(C.T))
    return cached(('one_hot', n, M), build)


def where_left(n, cols=None):
    return lambda i, j: f'left row {i} = ' + fam.describe_column(n, i if cols is None else cols[i]) + f'; right row {j}'


def where_right(n):
    return lambda i, j: (f'right row {j} = one-hot symplectic column {j} (packed bit {int(fam.packed_bit(n, j))} of the right operand), reached from the left '
                         f'operand\'s ' + fam.describe_column(n, int(fam.partner(n, j))) + f'; left row {i}')


@pytest.mark.parametrize('side', ['left', 'right'])
@pytest.mark.parametrize('n', ONE_HOT_N)
@pytest.mark.parametrize('kernel', list(KERNELS))
def test_one_hot_every_kernel(kernel, n, side, monkeypatch):
    """The 2n one-hot rows as the left operand (row p of the table = NOT column partner(p) of B) and as the right operand (the transposed
    table), 2113 rows on the other side, bytes and bit-packed — on every forced kernel, which must be the one that ran."""
    env, path = KERNELS[kernel]
    a, b, c_bits, ct_bits = one_hot_case(n)
    set_switches(monkeypatch, env)
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        if side == 'left':
            both_outputs(A, B, c_bits, path, f'one_hot n={n} as the left operand [{kernel}]', where_left(n))
        else:
            both_outputs(B, A, ct_bits, path, f'one_hot n={n} as the right operand [{kernel}]', where_right(n))
    finally:
        A.free(); B.free()


def test_unfused_byte_expansion_on_one_hot(monkeypatch):
    """SYMGPU_M4R_UNFUSED=1: the Four-Russians kernel writes bit-packed rows to scratch and k_bits_to_bytes_flat expands them."""
    n = 100
    a, b, c_bits, ct_bits = one_hot_case(n)
    set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_UNFUSED': '1'})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        for off in (3, 16):
            assert_bytes(counted(lambda: table_bytes(A, B, off=off), M4R_ONE, 'unfused'), c_bits, f'one_hot n={n}, unfused, offset {off}', where_left(n))
            assert_bytes(counted(lambda: table_bytes(B, A, off=off), M4R_ONE, 'unfused'), ct_bits, f'one_hot n={n} (right), unfused, offset {off}', where_right(n))
    finally:
        A.free(); B.free()


# ---------------------------------------------------------------- 2. majorana_stack -------------------------------------------------------
MAJORANA_N = [64, 65, 200, 700]


def majorana_case(n):
    def build():
        A, C = fam.majorana_stack(n)
        return A, packing.pack_rows(A), C, fam.pack_cols(C)
    return cached(('majorana', n), build)


@pytest.mark.parametrize('force', ['1', '0'])
@pytest.mark.parametrize('n', MAJORANA_N)
def test_majorana_self_adjacency(n, force, monkeypatch):
    """The (3n + 1)^2 table of the Majorana strings and Z prefixes with themselves: through one handle on both sides (the register-tile
    kernel then shares one word-major copy), through a handle and its clone, and through the host entry point; both kernels, bytes and
    bit-packed (padding bits zero)."""
    _, a, C, c_bits = majorana_case(n)
    path = M4R_ONE if force == '1' else TILE
    set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': force})
    A = DeviceOp.upload(a)
    A2 = A.clone()
    try:
        both_outputs(A, A, c_bits, path, f'majorana n={n}, A with A [M4R={force}]')
        both_outputs(A, A2, c_bits, path, f'majorana n={n}, A with clone(A) [M4R={force}]')
    finally:
        A.free(); A2.free()
    got = counted(lambda: kernels.commutes(a, a), path, 'host entry, same array')
    assert np.array_equal(got, C), f'majorana n={n}: symgpu_commutes(a, a) [M4R={force}]'
    got = counted(lambda: kernels.commutes(a, a.copy()), path, 'host entry, two arrays')
    assert np.array_equal(got, C), f'majorana n={n}: symgpu_commutes(a, copy) [M4R={force}]'


@pytest.mark.parametrize('force', ['1', '0', None])
@pytest.mark.parametrize('n', [65, 700])
def test_majorana_through_the_operator_class(n, force, monkeypatch):
    """PauliwordOp.adjacency_matrix and commutes_termwise on the same operands."""
    A, _, C, _ = majorana_case(n)
    set_switches(monkeypatch, {} if force is None else {'SYMGPU_COMMUTE_M4R': force})
    P = PauliwordOp(A, np.ones(A.shape[0]))
    Q = PauliwordOp(A.copy(), np.ones(A.shape[0]))
    path = TILE if force is None else (M4R_ONE if force == '1' else TILE)       # (2,101^2 pairs: too few tiles for the library to choose Four Russians)
    adj = counted(lambda: P.adjacency_matrix, path, 'adjacency_matrix')
    assert adj.dtype == np.bool_ and np.array_equal(adj, C), f'majorana n={n}: adjacency_matrix [M4R={force}]'
    got = counted(lambda: P.commutes_termwise(Q), path, 'commutes_termwise')
    assert np.array_equal(got, C), f'majorana n={n}: commutes_termwise [M4R={force}]'
    k = 2 * n + n // 2                                                 # a slice that starts inside the prefixes
    got = counted(lambda: Q[k:].commutes_termwise(P), path, 'commutes_termwise of a slice')
    assert np.array_equal(got, C[k:]), f'majorana n={n}: commutes_termwise of rows {k}.. [M4R={force}]'


# ---------------------------------------------------------------- 3. sparse_groups, one tile per workgroup --------------------------------
SPARSE_SETS = [(100, name) for name in ('first', 'word_straddle', 'half_straddle+last', 'odd3', 'five')] + [(257, 'half_straddle'), (257, 'high')]


def sparse_case(n, name, N, M):
    def build():
        groups = fam.group_sets(n)[name]
        A, B, Cb = fam.sparse_groups(n, groups, N, M, np.random.default_rng(7 * n + len(name)))
        a = packing.pack_rows(A)
        assert fam.nonzero_groups(a, n) == groups
        return a, packing.pack_rows(B), Cb, fam.steps_of(groups)
    return cached(('sparse', n, name, N, M), build)


def where_sparse(i, j):
    return f'left row {i}, right row {j}: column tile {j // 2048}, word {j // 64} of the table row'


@pytest.mark.parametrize('r', ['16', '24', '48'])
@pytest.mark.parametrize('n,name', SPARSE_SETS, ids=[f'{n}-{name}' for n, name in SPARSE_SETS])
def test_sparse_groups_one_tile_per_workgroup(n, name, r, monkeypatch):
    """600 x 2113 (two row tiles at R = 16, two column tiles) with the left operand non-zero in the named 7-bit groups only: one step (one
    group + the zero group, or one pair), two steps with a padded pair, three steps, groups across a word / across the halves, and at
    n = 257 nothing below group 64 (the second ballot round of the group compaction).  Row 0 is the identity."""
    a, b, c_bits, S = sparse_case(n, name, 600, 2113)
    set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': r})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        both_outputs(A, B, c_bits, M4R_ONE, f'sparse_groups n={n} {name} (S = {S}) R={r}', where_sparse)
    finally:
        A.free(); B.free()


# ---------------------------------------------------------------- 4. sparse_groups, stream-K ----------------------------------------------
STREAM_SETS = {1: 'half_straddle+last', 2: 'odd3', 3: 'five'}        # S -> group set at n = 100 (S = 1 from an even count: no padding group)
# (tile height, S, mode); R = 16 with S = 2 comes last: test_sparse_groups_stream_k_bytes, next in the file, shares its operands
STREAM_CASES = [(r, S, mode) for r, S in (('16', 1), ('16', 3), ('24', 2), ('48', 2), ('16', 2)) for mode in ('stream', 'fixup')]
STREAM_M = 32750
_stream = {}


def stream_case(r, S):
    """One expected table at a time (35 to 107 MB); the cases are ordered so that both modes of a shape share it."""
    key = (r, S)
    if key not in _stream:
        _stream.clear()
        n, N = 100, 32 * int(r) * 17 - 37
        groups = fam.group_sets(n)[STREAM_SETS[S]]
        assert fam.steps_of(groups) == S
        A, B, Cb = fam.sparse_groups(n, groups, N, STREAM_M, np.random.default_rng(90 + S))
        a = packing.pack_rows(A)
        assert fam.nonzero_groups(a, n) == groups
        _stream[key] = (a, packing.pack_rows(B), Cb)
    return _stream[key]


def where_stream(r, S):
    rows = 32 * int(r)

    def where(i, j):
        tile = (j // 2048) * 17 + i // rows
        return (f'left row {i} (row tile {i // rows}, row {i % rows} of it), right row {j} (column tile {j // 2048}): tile {tile} of 272 = steps '
                f'[{tile * S}, {tile * S + S}) of the {272 * S} of the launch')
    return where


def stream_switches(r, mode):
    env = {'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': r, 'SYMGPU_M4R_STREAM': '1'}
    if mode == 'fixup':
        env['SYMGPU_M4R_FIXUP'] = '1'
    return env


@pytest.mark.parametrize('r,S,mode', STREAM_CASES, ids=[f'R{r}-S{S}-{mode}' for r, S, mode in STREAM_CASES])
def test_sparse_groups_stream_k(r, S, mode, monkeypatch):
    """The stream-K launch with S = 1, 2, 3 steps a tile (dense operands only ever give the maximum, 19 at n = 100): 17 x 16 = 272 tiles of
    S steps over the persistent workgroups — S = 1 splits no tile, S = 2 and 3 split tiles after their first or second step; `stream`: the
    owner of a tile's first steps adds the neighbour's published part, `fixup` (SYMGPU_M4R_FIXUP=1): both parts go to scratch and
    k_m7_fixup writes the tile.  Bit-packed output, EVERY bit compared with the by-construction table.  The launch must have been a
    stream-K launch (COMMUTE_M4R_STREAMK): fewer tiles than compute units would silently run one tile per workgroup."""
    a, b, c_bits = stream_case(r, S)
    set_switches(monkeypatch, stream_switches(r, mode))
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        what = f'stream-K n=100 {STREAM_SETS[S]} (S = {S}) R={r} [{mode}]'
        assert_bits(counted(lambda: table_bits(A, B), M4R_STREAM, what), c_bits, what, where_stream(r, S))
    finally:
        A.free(); B.free()


def test_sparse_groups_stream_k_bytes(monkeypatch):
    """The same launch with byte output: rows of 32,750 bytes (unaligned row starts, a byte-wise row end) from the stream-K epilogue and,
    for the tiles left to it, from k_m7_fixup."""
    r, S = '16', 2
    a, b, c_bits = stream_case(r, S)
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        for mode in ('stream', 'fixup'):
            set_switches(monkeypatch, stream_switches(r, mode))
            what = f'stream-K bytes n=100 odd3 (S = 2) R=16 [{mode}]'
            assert_bytes(counted(lambda: table_bytes(A, B), M4R_STREAM, what), c_bits, what, where_stream(r, S))
    finally:
        A.free(); B.free()


# ---------------------------------------------------------------- 5. the library's own choice ---------------------------------------------
def test_own_choice_small_table_takes_the_register_tile(monkeypatch):
    """No switch set: 200 x 300 is served by the register-tile kernel."""
    n = 100
    a, b, c_bits, ct_bits = one_hot_case(n, 300)
    set_switches(monkeypatch, {})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        assert a.shape[0] == 200 and b.shape[0] == 300
        both_outputs(A, B, c_bits, TILE, 'own choice, 200 x 300', where_left(n))
        both_outputs(B, A, ct_bits, TILE, 'own choice, 300 x 200', where_right(n))
    finally:
        A.free(); B.free()


def test_own_choice_many_tiles_take_four_russians(monkeypatch):
    """No switch set: 514 one-hot rows (n = 257) x 212,992 rows = 2 x 104 tiles of the shortest height, which the plan's Four-Russians threshold accepts
    (at least 3/4 of the 256 compute units): a Four-Russians launch, either kind.  Bit-packed (13.7 MB)."""
    n, M = 257, 104 * 2048
    rng = np.random.default_rng(4)
    A_, B_, C = fam.one_hot(n, M, rng)
    a, b, c_bits = packing.pack_rows(A_), packing.pack_rows(B_), fam.pack_cols(C)
    del A_, B_, C
    set_switches(monkeypatch, {})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        what = 'own choice, 514 x 212992'
        assert_bits(counted(lambda: table_bits(A, B), (M4R_ONE, M4R_STREAM), what), c_bits, what, where_left(n))
    finally:
        A.free(); B.free()


def test_own_choice_few_long_rows_take_the_wide_kernel(monkeypatch):
    """No switch set: rows of 256 words a half (n = 16,384) and 32 x 2048 = 65,536 pairs are served by the wide-row kernel.  The 32 one-hot
    rows sit at the ends of the halves, around word boundaries and in the last word."""
    n, M = 16384, 2048
    cols = np.array([0, 1, 63, 64, 65, 127, 128, 4095, 4096, 8191, 8192, 16320, 16382, 16383, 12345, 7])
    cols = np.concatenate([cols, cols + n])
    A_, B_, C = fam.one_hot(n, M, np.random.default_rng(5), cols=cols)
    a, b, c_bits = packing.pack_rows(A_), packing.pack_rows(B_), fam.pack_cols(C)
    del A_, B_
    assert a.shape == (32, 512)
    set_switches(monkeypatch, {})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        both_outputs(A, B, c_bits, WIDE, 'own choice, 32 x 2048 at n = 16384', where_left(n, cols))
    finally:
        A.free(); B.free()


# ---------------------------------------------------------------- 6. the cached bit-major copy of the right operand -----------------------
def test_cached_bit_major_copy_follows_the_rows(monkeypatch):
    """The Four-Russians kernel caches the bit-major copy of a resident right operand on its handle (valid while the row count it was
    built for is the handle's).  symgpu_op_write, symgpu_op_copy_rows and symgpu_op_set_rows change rows without changing the count at the
    end: every table must be the one of the rows B holds at that moment.  B holds one-hot rows, so a stale copy is a table whose columns
    are those of the EARLIER rows; A is random and table[i, t] = NOT A[i, partner(column of B's row t)]."""
    lib = _lib.lib()
    n, N = 100, 700
    T = 2 * n
    rng = np.random.default_rng(61)
    A_bool = fam.random_bits(rng, (N, 2 * n))
    A_bool[3] = False
    a = packing.pack_rows(A_bool)
    eye = packing.pack_rows(np.eye(T, dtype=bool))

    def want(cols):                                                   # the table for B = one-hot rows of `cols`
        return fam.pack_cols(~A_bool[:, fam.partner(n, np.asarray(cols))])

    set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': '1'})
    A = DeviceOp.upload(a)
    cols = np.arange(T)
    B = DeviceOp.upload(np.ascontiguousarray(eye[cols]))
    src = DeviceOp.upload(np.ascontiguousarray(eye[(cols + 7) % T]))
    try:
        both_outputs(A, B, want(cols), M4R_ONE, 'fresh operand')
        both_outputs(A, B, want(cols), M4R_ONE, 'second call on the cached copy')

        cols = cols[::-1].copy()                                      # other rows over [0, T): same T
        rows = np.ascontiguousarray(eye[cols])
        _lib.check(lib.symgpu_op_write(B.handle, 0, rows.ctypes.data, None, T))
        assert B.n_terms == T
        both_outputs(A, B, want(cols), M4R_ONE, 'after symgpu_op_write over all rows')

        rows = np.ascontiguousarray(eye[[5, 105]])                    # two rows in the middle
        _lib.check(lib.symgpu_op_write(B.handle, 50, rows.ctypes.data, None, 2))
        cols[50:52] = [5, 105]
        both_outputs(A, B, want(cols), M4R_ONE, 'after symgpu_op_write of two rows')

        _lib.check(lib.symgpu_op_copy_rows(B.handle, 40, src.handle, 10, 120))
        cols[40:160] = (np.arange(10, 130) + 7) % T
        assert B.n_terms == T
        both_outputs(A, B, want(cols), M4R_ONE, 'after symgpu_op_copy_rows into the operand')

        B.set_rows(T - 70)
        both_outputs(A, B, want(cols[:T - 70]), M4R_ONE, 'after symgpu_op_set_rows down')
        B.set_rows(T)
        both_outputs(A, B, want(cols), M4R_ONE, 'after symgpu_op_set_rows back up')

        B.set_coeff(np.arange(T) + 1j)                                # rows unchanged: the same table
        both_outputs(A, B, want(cols), M4R_ONE, 'after symgpu_op_set_coeff')

        # two slabs of the left operand against the same resident B = the one-call table
        full = want(cols)
        both_outputs(A, B, full[:N // 3], M4R_ONE, 'slab [0, N/3)', lo=0, hi=N // 3)
        both_outputs(A, B, full[N // 3:], M4R_ONE, 'slab [N/3, N)', lo=N // 3, hi=N)
        assert np.array_equal(B.download(with_coeff=False), eye[cols]), 'the operand itself'
    finally:
        A.free(); B.free(); src.free()


# ---------------------------------------------------------------- 7. the plan: precedence of the switches, read on every call --------------
def test_forcing_four_russians_beats_the_wide_kernel(monkeypatch):
    """2 x 2 pairs of rows of 256 words a half (n = 16,384) take the wide-row kernel by themselves; SYMGPU_COMMUTE_M4R=1 comes first in the
    plan: a Four-Russians launch (COMMUTE_M4R_TILE) and no wide-row call (COMMUTE_WIDE_ROWS)."""
    n = 16384
    cols = np.array([64, n + 16383])
    A_, B_, _ = fam.one_hot(n, 2, np.random.default_rng(70), cols=cols)
    a, b = packing.pack_rows(A_), packing.pack_rows(B_)
    assert a.shape == (2, 512) and b.shape == (2, 512)
    want = fam.pack_cols(onp.commutes_termwise(A_, B_))
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        set_switches(monkeypatch, {})
        both_outputs(A, B, want, WIDE, '2 x 2 at n = 16384, no switch', where_left(n, cols))
        set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': '1'})
        both_outputs(A, B, want, M4R_ONE, '2 x 2 at n = 16384, SYMGPU_COMMUTE_M4R=1', where_left(n, cols))
    finally:
        A.free(); B.free()


PLAN_N, PLAN_M = 256, 1024                          # one tile of the shortest height at n = 100: fewer tiles than compute units


def plan_case():
    def build():
        n = 100
        A_, B_, _ = fam.sparse_groups(n, fam.group_sets(n)['five'], PLAN_N, PLAN_M, np.random.default_rng(71))
        return packing.pack_rows(A_), packing.pack_rows(B_), onp.commutes_termwise(A_, B_)
    return cached(('plan', PLAN_N, PLAN_M), build)


def test_stream_asked_for_but_not_possible(monkeypatch):
    """SYMGPU_M4R_STREAM=1 on 256 x 1024 terms at n = 100: one tile, fewer than compute units, so the launch is one tile per workgroup
    (COMMUTE_M4R_TILE, not COMMUTE_M4R_STREAMK) and the table is the oracle's."""
    a, b, C = plan_case()
    set_switches(monkeypatch, {'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_STREAM': '1'})
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        both_outputs(A, B, fam.pack_cols(C), M4R_ONE, '256 x 1024 at n = 100, stream-K asked for', where_sparse)
    finally:
        A.free(); B.free()


@pytest.mark.parametrize('M', [PLAN_M, PLAN_M - 24])
def test_bit_output_ignores_unfused(M, monkeypatch):
    """symgpu_commutes_bits_dev with and without SYMGPU_M4R_UNFUSED (which concerns byte output only): the same bits, the oracle's, zero
    padding up to the word end (M = 1000: 24 padding bits in the last word of every row)."""
    a, b, C = plan_case()
    want = fam.pack_cols(C[:, :M])
    A, B = DeviceOp.upload(a), DeviceOp.upload(np.ascontiguousarray(b[:M]))
    try:
        got = []
        for env in ({'SYMGPU_COMMUTE_M4R': '1'}, {'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_UNFUSED': '1'}):
            set_switches(monkeypatch, env)
            what = f'256 x {M} at n = 100, bit-packed, {env}'
            got.append(counted(lambda: table_bits(A, B), M4R_ONE, what))
            assert_bits(got[-1], want, what, where_sparse)
        assert np.array_equal(got[0], got[1])
    finally:
        A.free(); B.free()


def test_switches_are_read_on_every_call(monkeypatch):
    """One process, one pair of operators, four calls: SYMGPU_COMMUTE_M4R=0, =1 at SYMGPU_M4R_R=16, =1 at R=48, unset.  The register tile,
    Four Russians twice and then the library's own choice (256 x 1024: one tile, the register tile again) serve them in that order, and
    every table is the oracle's."""
    a, b, C = plan_case()
    want = fam.pack_cols(C)
    A, B = DeviceOp.upload(a), DeviceOp.upload(b)
    try:
        for env, path in (({'SYMGPU_COMMUTE_M4R': '0'}, TILE), ({'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': '16'}, M4R_ONE),
                          ({'SYMGPU_COMMUTE_M4R': '1', 'SYMGPU_M4R_R': '48'}, M4R_ONE), ({}, TILE)):
            set_switches(monkeypatch, env)
            what = f'256 x 1024 at n = 100, {env or "no switch"}'
            assert_bytes(counted(lambda: table_bytes(A, B), path, what), want, what, where_sparse)
    finally:
        A.free(); B.free()
