"""GPU: every path of the GF(2) elimination (csrc/gf2.hip) and of its callers (symmetry generators, csrc/genrec.hip) on STRUCTURED
matrices, against the C oracle, bit for bit: reduced matrix (padding bits included), reference-order XOR count, pivot column per row.

The elimination decides from the data which panel a block runs on (two-word window, four-word window, full rows in LDS), where a window
starts and where a block ends.  The families of tests/_gf2_families.py steer those decisions (tests/test_gf2_families.py checks on the
CPU that they have the structure they claim); the counters GF2_BLOCKS_PANELLED / GF2_PANEL_FULL_ROWS / GF2_PANEL_WINDOW — blocks panelled by the blocked path, of these on the
full rows, of these on the two-word window — tell which decision was taken.  The counter tests assert FACTS a family is built for
("the full-row panel ran", "blocks ended early"), never exact block counts: a better heuristic passes, a lost path does not.

Expected values: oracle_c.rref(packed, want_pivots=True) for the elimination, oracle_np.symmetry_generators_symp /
generator_reconstruction / generators on bool matrices for the callers."""
import ctypes

import numpy as np
import pytest

from symmer_amd import kernels, packing, _lib, PauliwordOp
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
from oracle import oracle_c as oc
import _gf2_families as fam

pytestmark = pytest.mark.gpu

ENV_NAMES = ('SYMGPU_GF2_FUSED_SELECT', 'SYMGPU_GF2_M4R', 'SYMGPU_GF2_SMALL')
SCHEDULES = {
    'default': {},
    'separate_select': {'SYMGPU_GF2_FUSED_SELECT': '0'},
    'flag_sweep': {'SYMGPU_GF2_M4R': '0'},
    'no_small': {'SYMGPU_GF2_SMALL': '0'},
    'separate_select_no_small': {'SYMGPU_GF2_FUSED_SELECT': '0', 'SYMGPU_GF2_SMALL': '0'},
}
MAX_BITS = 3e7


def set_schedule(monkeypatch, env):
    for k in ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)            # read per call by rref_dev


def counters():
    """(blocks panelled by the blocked path, of these on the full rows in LDS, of these on the two-word window), cumulative."""
    return kernels.counters(('GF2_BLOCKS_PANELLED', 'GF2_PANEL_FULL_ROWS', 'GF2_PANEL_WINDOW'))


_cache = {}


def case(name, R, C, seed=2024):
    """(packed matrix, oracle's (reduced, XOR count, pivots)) of a family variant, built once per session."""
    key = (name, R, C, seed)
    if key not in _cache:
        assert R * C <= MAX_BITS
        fn, kw = VARIANT[name]
        p = fam.pack(fn(np.random.default_rng(seed), R, C, **kw))
        _cache[key] = (p, oc.rref(p, want_pivots=True))
    return _cache[key]


def assert_rref(p, expect, what):
    red, n_xor, piv = kernels.rref(p, want_pivots=True)
    ered, e_xor, epiv = expect
    assert np.array_equal(red, ered), f'{what}: reduced matrix differs in {int((red != ered).any(axis=1).sum())} rows'
    assert n_xor == e_xor, f'{what}: XOR count {n_xor}, oracle {e_xor}'
    assert np.array_equal(piv, epiv), f'{what}: pivots differ at rows {np.flatnonzero(piv != epiv)[:8]}'


VARIANTS = fam.variants()
VARIANT = {name: (fn, kw) for name, fn, kw in VARIANTS}
ROWS = [63, 64, 65, 129, 700]
C_FULL = [16384, 9000, 4160, 16320]            # Wc = 256, 141, 65, 255: the full-row panel is allowed
C_WINDOW = [16385, 16448, 20000]               # Wc = 257, 257, 313: windows only


def family_sizes():
    """Every family variant at one size of either kind; the row counts 63 / 64 / 65 / 129 / 700 rotate over the variants."""
    out = []
    for i, (name, _, _) in enumerate(VARIANTS):
        out.append((name, ROWS[i % 5], C_FULL[i % len(C_FULL)]))
        out.append((name, ROWS[(i + 2) % 5], C_WINDOW[i % len(C_WINDOW)]))
    return out


FAMILY_SIZES = family_sizes()


# ---------------------------------------------------------------- 1. families x schedules ---------------------------------------
@pytest.mark.parametrize('schedule', list(SCHEDULES))
@pytest.mark.parametrize('name,R,C', FAMILY_SIZES, ids=[f'{n}-{R}x{C}' for n, R, C in FAMILY_SIZES])
def test_family_on_every_schedule(name, R, C, schedule, monkeypatch):
    p, expect = case(name, R, C)
    set_schedule(monkeypatch, SCHEDULES[schedule])
    assert_rref(p, expect, f'{name} {R}x{C} [{schedule}]')


def test_every_family_runs_at_both_widths_and_every_row_count():
    wide = {n for n, _, C in FAMILY_SIZES if (C + 63) // 64 >= 257}
    full = {n for n, _, C in FAMILY_SIZES if (C + 63) // 64 <= 256}
    assert wide == full == set(VARIANT)
    assert {R for _, R, _ in FAMILY_SIZES} == set(ROWS)


# ---------------------------------------------------------------- 2. counter facts ----------------------------------------------
def run_counted(name, R, C, monkeypatch, env=None):
    p, expect = case(name, R, C)
    set_schedule(monkeypatch, env or {})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C}')
    blocks, full, narrow = counters() - before
    print(f'{name} {R}x{C} (Wc = {p.shape[1]}): {blocks} blocks, {full} on the full rows, {narrow} on the two-word window, '
          f'ceil(R/64) = {-(-R // 64)}')
    return int(blocks), int(full), int(narrow)


@pytest.mark.parametrize('R', [129, 700])
def test_staircase_short_rows_take_the_full_row_panel(R, monkeypatch):
    blocks, full, narrow = run_counted('staircase-step67', R, 16384, monkeypatch)
    assert full > 0, f'Wc = 256, leads a word apart: no block ran on the full rows ({blocks} blocks, {narrow} narrow)'
    assert full <= blocks


@pytest.mark.parametrize('R', [129, 700])
def test_staircase_long_rows_take_the_four_word_window_and_end_early(R, monkeypatch):
    blocks, full, narrow = run_counted('staircase-step67', R, 16385, monkeypatch)
    assert full == 0, f'Wc = 257 > FULL_WC: {full} blocks on the full rows'
    assert blocks > -(-R // 64), f'{blocks} blocks for {R} rows: no block ended early'
    assert narrow < blocks, 'every block ran on the two-word window although consecutive rows lead in different words'


@pytest.mark.parametrize('density', [0.5, 0.2])
@pytest.mark.parametrize('R,C', [(700, 16384), (700, 16448), (129, 4160), (64, 20000)])
def test_dense_takes_windows_and_whole_blocks(R, C, density, monkeypatch):
    """Bound on the blocks of a dense matrix.  (a) A block that neither ends early nor is the last takes 64 rows, so with E early ends
    there are at most R // 64 + 1 + E blocks.  (b) window_start (gf2_panel.h) puts the window at the smallest leading word of the block's
    rows: in a dense matrix, the word of the pivot frontier (the first column that is no pivot yet).  The window holds at least 128
    columns from the start of that word and the 64 pivots of a block move the frontier by 64 columns and the few a random row skips, so
    a block can only run out of window when the frontier entered it in the upper part of its word — and the block after such an end
    starts its window at a later word.  At most one early end per word the frontier enters ("a one-row block every 64 columns" was
    the round-2 defect that comment describes: that rate is the ceiling, not the norm), and the frontier stops at the rank, at most
    min(R, C): E <= min(R, C) // 64 + 1.  A panel that lost its window logic ends a block every few rows and overshoots several times."""
    name = f'dense-density{density}'
    blocks, full, narrow = run_counted(name, R, C, monkeypatch)
    bound = (R // 64 + 1) + (min(R, C) // 64 + 1)
    assert full == 0, f'{full} blocks of a dense matrix on the full rows'
    assert -(-R // 64) <= blocks <= bound, f'{blocks} blocks, bound {bound}'
    if density == 0.5:
        assert narrow > 0, 'no block of a dense matrix ran on the two-word window'


@pytest.mark.parametrize('w', [128, 256])
@pytest.mark.parametrize('R,C', [(128, 16448), (640, 20000)])
def test_window_twins_end_blocks(R, C, w, monkeypatch):
    """R is a multiple of 64 on purpose: then R / 64 blocks are only possible if NO block ends early.  (With w = 128 only the first twin
    meets a two-word window — the block that it opens has a four-word window, in which the later twins of that width survive — so
    there is a single one-row block, and at R = 129 = 1 + 64 + 64 it would hide in the last block's slack.)"""
    blocks, full, narrow = run_counted(f'window_twins-w{w}', R, C, monkeypatch)
    assert full == 0
    assert blocks > -(-R // 64), f'{blocks} blocks for {R} rows: the twins that cancel inside the window did not end their blocks'


@pytest.mark.parametrize('name', ['dense-density0.5', 'staircase-step67', 'identity_plus_noise-rightTrue'])
@pytest.mark.parametrize('R,C', [(64, 4096), (33, 64), (1, 1)])
def test_small_matrices_take_the_one_workgroup_path(name, R, C, monkeypatch):
    blocks, full, narrow = run_counted(name, R, C, monkeypatch)
    assert (blocks, full, narrow) == (0, 0, 0), 'R <= 64 and Wc <= 64: the blocked path ran'
    blocks, full, narrow = run_counted(name, R, C, monkeypatch, {'SYMGPU_GF2_SMALL': '0'})
    assert blocks > 0, 'SYMGPU_GF2_SMALL=0: the blocked path did not run'


def test_flag_sweep_schedule_counts_its_blocks(monkeypatch):
    """SYMGPU_GF2_M4R=0 panels with k_wpanel: its blocks are counted too, and it never takes the full rows."""
    blocks, full, narrow = run_counted('staircase-step67', 129, 16384, monkeypatch, {'SYMGPU_GF2_M4R': '0'})
    assert blocks > 2 and full == 0


# ---------------------------------------------------------------- 3. shape edges ------------------------------------------------
EDGE_R = [1, 2, 63, 64, 65, 127, 128, 129]
EDGE_C = [1, 63, 64, 65, 4096, 4097, 8192 + 1, 16384, 16384 + 1, 64 * 16385]


def edge_cases():
    """Every C with every R up to 2e6 bits; the widest columns (Wc = 129 and more) with a rotating pair of the larger row counts, the
    widest of all (Wc = 16385: more than 256 column tiles, one chunk) with 1 and 2 rows."""
    out = []
    for ci, C in enumerate(EDGE_C):
        if C >= 64 * 16385:
            rows = [1, 2]
        elif C > 4097:
            big = EDGE_R[2:]
            rows = [1, 2, big[ci % 6], big[(ci + 3) % 6]]
        else:
            rows = EDGE_R
        out += [(R, C) for R in rows]
    return out


EDGES = edge_cases()


def test_edge_cases_cover_every_value():
    assert {C for _, C in EDGES} == set(EDGE_C)
    wide_rows = {R for R, C in EDGES if C > 4097}
    assert {R for R, C in EDGES if C <= 4097} == set(EDGE_R) and wide_rows >= {1, 2} and len(wide_rows) >= 6
    assert {R for R, _ in EDGES} == set(EDGE_R)


@pytest.mark.parametrize('name', ['dense-density0.5', 'staircase-step67'])
@pytest.mark.parametrize('R,C', EDGES)
def test_shape_edges(name, R, C, monkeypatch):
    p, expect = case(name, R, C, seed=77)
    assert p.shape == (R, max(1, (C + 63) // 64))
    set_schedule(monkeypatch, {})
    assert_rref(p, expect, f'{name} {R}x{C}')
    if R <= 64 and p.shape[1] <= 64:
        set_schedule(monkeypatch, SCHEDULES['no_small'])          # the same edge on the blocked path
        assert_rref(p, expect, f'{name} {R}x{C} [no_small]')


# ---------------------------------------------------------------- 4. injected time-out ------------------------------------------
@pytest.mark.parametrize('name,R,C', [('window_twins-w128', 129, 16448), ('window_twins-w256', 700, 9000), ('low_rank-k20', 700, 9000),
                                      ('low_rank-k64', 129, 16448)])
def test_injected_time_out_on_structured_matrices(name, R, C, monkeypatch):
    """SYMGPU_GF2_FUSED_SELECT=2 treats the first, fused attempt as timed out (nothing faults, nothing waits): the matrix is restored
    and reduced with separate launches.  The injection must not latch the fallback: nothing is reported as degraded, and the next call
    runs the fused schedule again."""
    p, expect = case(name, R, C)
    degraded = _lib.degraded()
    set_schedule(monkeypatch, {'SYMGPU_GF2_FUSED_SELECT': '2'})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C} [injected time-out]')
    twice = (counters() - before)[0]
    set_schedule(monkeypatch, {})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C} [after the injection]')
    once = (counters() - before)[0]
    assert once > 0 and twice == 2 * once, f'the injected run panelled {twice} blocks, a plain run {once}: it did not run twice'
    assert _lib.degraded() == degraded, 'the injected time-out was reported as a degraded fast path'
    assert not any('GF(2)' in d for d in _lib.degraded())


@pytest.mark.parametrize('name', ['dense-density0.5', 'staircase-step67'])
@pytest.mark.parametrize('R,C', [(64, 4096), (33, 64)])
def test_injected_time_out_on_a_small_matrix_sent_through_the_blocked_path(name, R, C, monkeypatch):
    """SYMGPU_GF2_SMALL=0 sends a matrix of <= 64 rows and <= 64 words through the fused blocked schedule: plan_rref decides path and
    schedule in one place, so the matrix gets its safety copy and SYMGPU_GF2_FUSED_SELECT=2 reaches it like any other (restore, second
    run with separate launches: GF2_BLOCKS_PANELLED rises by twice a plain blocked run's).  Nothing is latched or reported, and the next plain
    call takes the one-workgroup path again.  (Before the plan existed, the copy and the injection were decided from the size alone
    and the injection was ignored here: GF2_BLOCKS_PANELLED rose once.)"""
    p, expect = case(name, R, C)
    assert R <= 64 and p.shape[1] <= 64
    degraded = _lib.degraded()
    set_schedule(monkeypatch, {'SYMGPU_GF2_SMALL': '0'})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C} [no_small]')
    once = (counters() - before)[0]
    set_schedule(monkeypatch, {'SYMGPU_GF2_SMALL': '0', 'SYMGPU_GF2_FUSED_SELECT': '2'})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C} [no_small, injected time-out]')
    twice = (counters() - before)[0]
    print(f'{name} {R}x{C}: {once} blocks plain, {twice} with the injected time-out')
    assert once > 0 and twice == 2 * once, f'the injected run panelled {twice} blocks, a plain blocked run {once}: it did not run twice'
    assert _lib.degraded() == degraded, 'the injected time-out was reported as a degraded fast path'
    assert not any('GF(2)' in d for d in _lib.degraded())
    set_schedule(monkeypatch, {})
    before = counters()
    assert_rref(p, expect, f'{name} {R}x{C} [after the injection]')
    assert tuple(counters() - before) == (0, 0, 0), 'the next plain call did not take the one-workgroup path'


# ---------------------------------------------------------------- 5. symgpu_rref_dev --------------------------------------------
@pytest.mark.parametrize('name,R,C', [('staircase-step67', 129, 16384), ('window_twins-w256', 129, 16448), ('low_rank-k65', 700, 9000)])
def test_rref_dev_on_structured_matrices(name, R, C):
    """The device-pointer entry point: the matrix is reduced where it lies, the call uploads nothing."""
    p, (ered, e_xor, epiv) = case(name, R, C)
    L = _lib.lib()
    d = ctypes.c_void_p()
    _lib.check(L.symgpu_dev_alloc(p.nbytes, ctypes.byref(d)))
    try:
        _lib.check(L.symgpu_dev_upload(d, p.ctypes.data, p.nbytes))
        h2d = kernels.transfer_counters()[0]
        xor, piv = ctypes.c_int64(-1), np.full(R, -7, dtype=np.int64)
        _lib.check(L.symgpu_rref_dev(d, R, p.shape[1], ctypes.addressof(xor), piv.ctypes.data))
        assert kernels.transfer_counters()[0] == h2d, 'rref_dev uploaded payload'
        got = np.full_like(p, 0xA5A5A5A5A5A5A5A5)
        _lib.check(L.symgpu_dev_download(d, got.ctypes.data, got.nbytes))
    finally:
        _lib.check(L.symgpu_dev_free(d))
    assert np.array_equal(got, ered) and xor.value == e_xor and np.array_equal(piv, epiv)


# ---------------------------------------------------------------- 6. callers: symmetry generators -------------------------------
def stacked_symmetry_matrix(h):
    """The matrix symmetry_generators reduces, rows as the device builds them: the transpose of independent_op.py:124's
    vstack([hstack([Z, X]), eye(2n)]) — row c = [column c of [Z | X] over the terms | e_c]."""
    n = h.shape[1] // 2
    zx = np.hstack([h[:, n:], h[:, :n]])
    return np.hstack([zx.T, np.eye(2 * n, dtype=bool)])


def z_only(rng, M, n, k):
    """Terms whose X part vanishes on the first k qubits: Z_0 .. Z_{k-1} commute with every term."""
    h = rng.random((M, 2 * n)) < 0.3
    h[:, :k] = False
    return h


def symmetry_operators():
    rng = np.random.default_rng(31)
    ops = {}
    for n in (63, 64, 65, 130):
        h = np.zeros((300, 2 * n), dtype=bool)
        h[:, n:] = rng.random((300, n)) < 0.4
        ops[f'all_Z-n{n}'] = h                                   # every Z_i is a symmetry: n generators
    for k, n, M in ((0, 64, 1000), (1, 65, 1000), (63, 63, 65), (130, 130, 64), (0, 20, 1000), (1, 130, 63)):
        ops[f'Z_first{k}-n{n}-M{M}'] = z_only(rng, M, n, k)
    for M in (1, 63, 64, 65):
        ops[f'terms{M}-n64'] = z_only(rng, M, 64, 5)
    base = z_only(rng, 40, 65, 3)
    ops['duplicate_terms-n65'] = base[rng.integers(0, 40, 1000)]
    ops['one_term_repeated-n63'] = np.repeat(z_only(rng, 1, 63, 0), 64, axis=0)
    return ops


SYM_OPS = symmetry_operators()


@pytest.mark.parametrize('via', ['host_rows', 'handle'])
@pytest.mark.parametrize('name', list(SYM_OPS))
def test_symmetry_kernel_on_structured_operators(name, via):
    h = SYM_OPS[name]
    n = h.shape[1] // 2
    rows = packing.pack_rows(h)
    if via == 'host_rows':
        gens, n_xor = kernels.symmetry_kernel(rows, n)
    else:
        op = DeviceOp.upload(rows)
        try:
            gens, n_xor = kernels.symmetry_kernel_handle(op, n)
        finally:
            op.free()
    expect = onp.symmetry_generators_symp(h)
    assert np.array_equal(packing.unpack_rows(gens, n), expect), f'{name}: {gens.shape[0]} generators, oracle {expect.shape[0]}'
    assert np.array_equal(gens, packing.pack_rows(expect)), 'padding bits of the generators'
    _, e_xor = oc.rref(fam.pack(stacked_symmetry_matrix(h)))
    assert n_xor == e_xor, f'{name}: XOR count {n_xor}, oracle {e_xor} on the stacked matrix'
    if name.startswith('all_Z'):
        assert gens.shape[0] >= n
    if name.startswith('Z_first') and h.shape[0] >= 1000:
        assert gens.shape[0] == int(name.split('-')[0][len('Z_first'):])


def test_symmetry_kernel_without_symmetry_writes_nothing():
    """A Hamiltonian with no symmetry at all: *k == 0 and the output buffer is not touched."""
    h = SYM_OPS['Z_first0-n64-M1000']
    assert onp.symmetry_generators_symp(h).shape[0] == 0
    rows = packing.pack_rows(h)
    n, wq = 64, 1
    L = _lib.lib()
    for via in ('host_rows', 'handle'):
        out = np.full((2 * n, 2 * wq), 0xA5A5A5A5A5A5A5A5, dtype='<u8')
        k, count = ctypes.c_int64(-1), ctypes.c_int64(-1)
        if via == 'host_rows':
            _lib.check(L.symgpu_symmetry_kernel(rows.ctypes.data, rows.shape[0], n, wq, out.ctypes.data, 2 * n, ctypes.addressof(k),
                                                ctypes.addressof(count)))
        else:
            op = DeviceOp.upload(rows)
            try:
                _lib.check(L.symgpu_symmetry_kernel_dev(op.handle, n, out.ctypes.data, 2 * n, ctypes.addressof(k), ctypes.addressof(count)))
            finally:
                op.free()
        assert k.value == 0 and (out == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), via
        assert count.value == oc.rref(fam.pack(stacked_symmetry_matrix(h)))[1]


# ---------------------------------------------------------------- 7. callers: rank, generators, reconstruction ------------------
def structured_terms():
    """name -> bool[T, 2n] whose rows come from the low-rank and the zero-and-duplicate family."""
    rng = np.random.default_rng(47)
    return {
        'low_rank20-n40': fam.low_rank(rng, 300, 80, k=20),
        'low_rank65-n130': fam.low_rank(rng, 700, 260, k=65),
        'low_rank64-n64': fam.low_rank(rng, 129, 128, k=64),
        'zero_dup-n40': fam.zero_and_duplicate(rng, 300, 80),
        'zero_dup-n130': fam.zero_and_duplicate(rng, 700, 260),
        'zero_dup-n63': fam.zero_and_duplicate(rng, 65, 126),
    }


TERMS = structured_terms()


@pytest.mark.parametrize('name', list(TERMS))
def test_rank_and_generators_on_structured_terms(name):
    symp = TERMS[name]
    n = symp.shape[1] // 2
    rows = packing.pack_rows(symp)
    ered, _, epiv = oc.rref(rows, want_pivots=True)             # the packed rows ARE the matrix genrec.hip reduces
    op = DeviceOp.upload(rows)
    try:
        assert kernels.gf2_rank_dev(op) == int((epiv >= 0).sum())
        g = kernels.generators_dev(op)
        try:
            g_rows, g_coeff = g.download()
        finally:
            g.free()
        r_after = op.download(with_coeff=False)
    finally:
        op.free()
    assert np.array_equal(np.asarray(r_after), rows), 'the operator itself was reduced'
    keep = ered.any(axis=1)
    assert np.array_equal(keep, epiv >= 0)
    assert np.array_equal(g_rows, ered[keep]), 'generators: not the non-zero rows of the reduction, in row order'
    assert np.array_equal(g_coeff, np.ones(int(keep.sum()), dtype=complex))
    assert np.array_equal(packing.unpack_rows(g_rows, n), onp.generators(symp))


# (terms, generators taken from, number of generators): more than 64 generators, and exactly 2n
RECON = [('low_rank20-n40', 'zero_dup-n40', 80), ('zero_dup-n40', 'low_rank20-n40', 65), ('low_rank65-n130', 'zero_dup-n130', 260),
         ('zero_dup-n130', 'low_rank65-n130', 100), ('zero_dup-n63', 'zero_dup-n63', 65), ('low_rank64-n64', 'low_rank64-n64', 128)]


@pytest.mark.parametrize('terms,gens,g', RECON, ids=[f'{t}-in-{g}of-{s}' for t, s, g in RECON])
def test_generator_reconstruction_on_structured_terms(terms, gens, g):
    symp, gsymp = TERMS[terms], TERMS[gens][-g:]
    n = symp.shape[1] // 2
    assert gsymp.shape == (g, 2 * n) and 64 < g <= 2 * n
    e_recon, e_mask = onp.generator_reconstruction(symp, gsymp)
    op, gop = DeviceOp.upload(packing.pack_rows(symp)), DeviceOp.upload(packing.pack_rows(gsymp))
    try:
        recon, mask = kernels.generator_reconstruction_dev(gop, op, n)
    finally:
        op.free()
        gop.free()
    assert np.array_equal(recon, e_recon) and np.array_equal(mask, e_mask)
    # the drop-in method on the same operands (the rows are dependent: the independence check is the caller's to waive)
    P = PauliwordOp(symp, np.ones(symp.shape[0]))
    G = PauliwordOp(gsymp, np.ones(g))
    recon2, mask2 = P.generator_reconstruction(G, override_independence_check=True)
    assert np.array_equal(recon2, e_recon) and np.array_equal(mask2, e_mask)
