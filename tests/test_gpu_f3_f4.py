"""GPU: the three entry points of csrc/project.hip (symgpu_noncontextual_dev, symgpu_state_inner_dev, symgpu_project_dev) and the
self-adjacency path of the bit-packed commutation table, at the sizes where their code takes another branch, against oracle.oracle_np on
the same inputs.  The inputs are the families of tests/_f3_f4_families.py, whose answers hold by construction and are proved with the oracle
alone in tests/test_f3_f4_families.py.

Bars.  Noncontextuality: the oracle's yes / no.  bra * ket: BIT FOR BIT the sum formed in the left state's row order from products made of
separate IEEE multiplications and one subtraction / addition (include/symgpu.h; a NaN equals a NaN) — for dyadic, Gaussian, wide-range and
non-finite amplitudes alike.  Projection: rows and row order exact; coefficients exact for dyadic input, within 1e-12 for Gaussian input
with rows of |c| <= 1e-12 discarded on both sides (the bar of tests/test_gpu_parity.py).  No bound here comes from the code under test."""
import ctypes
import numpy as np
import pytest

from symmer_amd import PauliwordOp, IndependentOp, QuantumState, kernels, packing, _lib
from symmer_amd.kernels import DeviceOp
from oracle import oracle_np as onp
from _golden import assert_op_equal
import _f3_f4_families as fam

pytestmark = pytest.mark.gpu
TOL = 1e-12
SWITCH = ['1', '0', None]                         # SYMGPU_COMMUTE_M4R: Four-Russians kernel forced, register-tile kernel forced, the library's choice

_oracle_cache = {}


def oracle_cases(key, build):
    """[(id, symp, the oracle's answer)] of one family, computed once and shared by the parametrisations that walk it."""
    if key not in _oracle_cache:
        out = []
        for name, symp, claimed in build():
            answer = onp.check_adjmat_noncontextual(onp.commutes_termwise(symp, symp))
            assert answer is claimed, f'{key} {name}: the construction and the oracle disagree'
            symp.setflags(write=False)
            out.append((name, symp, answer))
        _oracle_cache[key] = out
    return _oracle_cache[key]


def set_switch(monkeypatch, switch):
    if switch is None:
        monkeypatch.delenv('SYMGPU_COMMUTE_M4R', raising=False)
    else:
        monkeypatch.setenv('SYMGPU_COMMUTE_M4R', switch)


def check_noncontextual(cases, tag):
    for name, symp, answer in cases:
        packed = packing.pack_rows(symp)
        op = PauliwordOp._from_packed(packed, symp.shape[1] // 2, np.ones(symp.shape[0]))
        assert op.is_noncontextual is answer, f'{tag} {name}: PauliwordOp.is_noncontextual'
        assert op._symp is None and 'adjacency_matrix' not in op.__dict__, 'the noncontextuality test built a host matrix'
        h = DeviceOp.upload(packed)
        try:
            assert kernels.noncontextual_dev(h) is answer, f'{tag} {name}: noncontextual_dev'
        finally:
            h.free()


# ---------------------------------------------------------------------------------------------------------------- noncontextuality ----
@pytest.mark.parametrize('switch', SWITCH)
@pytest.mark.parametrize('T', sorted(fam.NONCONTEXTUAL))
def test_noncontextual_families(T, switch, monkeypatch):
    """The True operator, every near-miss (one term added or changed) at rows 0, 63, 64, the first row of the last adjacency word and T - 1,
    and the variants that stay True, for every T of the table: one and two adjacency words, an odd word count (padding word of the
    characters), a partial and a full last word, more words than a wavefront has lanes (T = 4097, 4160).  A kernel that drops a row, a
    column or a word answers True on a near-miss."""
    set_switch(monkeypatch, switch)
    check_noncontextual(oracle_cases(('table', T), lambda: fam.noncontextual_family(T)), f'T={T} M4R={switch}')


@pytest.mark.parametrize('switch', SWITCH)
@pytest.mark.parametrize('T', sorted(fam.ONE_CLIQUE))
def test_noncontextual_one_clique(T, switch, monkeypatch):
    set_switch(monkeypatch, switch)
    check_noncontextual(oracle_cases(('one', T), lambda: fam.noncontextual_family(T, fam.ONE_CLIQUE)), f'one clique T={T} M4R={switch}')


def test_noncontextual_character_rows_wider_than_128_words(monkeypatch):
    """T = 8200: 129 adjacency words per row, character rows of 130 words — the smallest even width above 128, reached from T = 8193 on.  The
    True operator, a bridge as the last term, a partial term as the first.  The commutation kernel is the library's own choice."""
    set_switch(monkeypatch, None)
    check_noncontextual(oracle_cases(('wide', fam.T_WIDE), lambda: fam.noncontextual_family(fam.T_WIDE)), f'T={fam.T_WIDE}')


def pack_table(table):
    """bool[N, M] -> uint64[N, ceil(M / 64)]: bit j of row i (little-endian words), zero padding."""
    N, M = table.shape
    words = (M + 63) // 64
    bits = np.zeros((N, words * 64), dtype=np.uint8)
    bits[:, :M] = table
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u8').reshape(N, words)


def commutes_bits(A, B, T):
    words = (T + 63) // 64
    lib = _lib.lib()
    buf = ctypes.c_void_p()
    _lib.check(lib.symgpu_dev_alloc(T * words * 8, ctypes.byref(buf)))
    try:
        junk = np.full(T * words, 0xFFFFFFFFFFFFFFFF, dtype='<u8')        # every word has to be overwritten, padding bits included
        _lib.check(lib.symgpu_dev_upload(buf, junk.ctypes.data, junk.nbytes))
        _lib.check(lib.symgpu_commutes_bits_dev(A.handle, 0, T, B.handle, buf))
        out = np.empty((T, words), dtype='<u8')
        _lib.check(lib.symgpu_dev_download(buf, out.ctypes.data, out.nbytes))
    finally:
        _lib.check(lib.symgpu_dev_free(buf))
    return out


@pytest.mark.parametrize('force', ['1', '0'])
@pytest.mark.parametrize('T', [65, 1000, 4097])
def test_self_adjacency_bit_packed(T, force, monkeypatch):
    """symgpu_commutes_bits_dev(A, 0, T, A): one word-major copy serves both sides (`same`).  Against the oracle's table packed bit by bit,
    the pad bits of every row's last word zero (the noncontextuality test counts set bits and relies on that), and bit for bit against the
    same call with a clone of A as B, which takes the two-copy path."""
    monkeypatch.setenv('SYMGPU_COMMUTE_M4R', force)
    rng = np.random.default_rng(500 + T)
    n = 70
    symp = rng.random((T, 2 * n)) < 0.3
    symp[T // 2] = symp[0]                                               # equal rows, an identity row, a clique-structured corner
    symp[T - 1] = False
    symp[1:40] = fam.cliques(39, 5, (20, 14), n - 3, rng)[0]
    A = DeviceOp.upload(packing.pack_rows(symp))
    B = A.clone()
    try:
        same = commutes_bits(A, A, T)
        two = commutes_bits(A, B, T)
    finally:
        A.free(); B.free()
    expect = pack_table(onp.commutes_termwise(symp, symp))
    if T % 64:
        pad = np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(T % 64)
        assert not (same[:, -1] & pad).any(), 'pad bits of the last word are set'
        assert not (two[:, -1] & pad).any()
    assert np.array_equal(same, expect)
    assert np.array_equal(two, expect) and np.array_equal(same, two)


# --------------------------------------------------------------------------------------------------------------------- bra * ket ----
def expected_inner(a_bits, a_c, b_bits, b_c, thr):
    """The sequential reference on the oracle's cleanup of both states; (re, im) and the cleaned states."""
    ar, ac = onp.cleanup_op(fam.state_symp(a_bits), a_c, thr)
    br, bc = onp.cleanup_op(fam.state_symp(b_bits), b_c, thr)
    return fam.inner_sequential(np.packbits(ar, axis=1), ac, np.packbits(br, axis=1), bc), (ar, ac), (br, bc)


def assert_same_bits(got, want, what):
    got_re, got_im = (got.real, got.imag) if isinstance(got, complex) else got
    print(f'{what}: got ({float(got_re)!r}, {float(got_im)!r}) want ({float(want[0])!r}, {float(want[1])!r})')
    assert fam.same_bits(got_re, want[0]) and fam.same_bits(got_im, want[1]), \
        f'{what}: got ({float(got_re).hex()}, {float(got_im).hex()}), sequential reference ({float(want[0]).hex()}, {float(want[1]).hex()})'


@pytest.mark.parametrize('Na,Nb,nq,overlap,kind', fam.inner_cases())
def test_state_inner_dev_bit_for_bit(Na, Nb, nq, overlap, kind):
    """kernels.state_inner_dev on handles from kernels.cleanup_dev: table capacities 1024 (Nb <= 512), 2048 (513 .. 1024), 4096 and
    beyond, 1 / 2 / 4 / 32 row words, no / a third / all rows shared; the non-finite amplitudes go through a cleanup without threshold so
    that the NaN rows reach the join."""
    rng = np.random.default_rng([Na, Nb, nq, fam.OVERLAPS.index(overlap), fam.AMPLITUDES.index(kind)])
    a_bits, a_c, b_bits, b_c, _ = fam.states(rng, Na, Nb, nq, overlap, kind)
    thr = None if kind == 'nonfinite' else 1e-15
    want, (ar, ac), (br, bc) = expected_inner(a_bits, a_c, b_bits, b_c, thr)
    raw = [DeviceOp.upload(packing.pack_rows(fam.state_symp(bits)), c) for bits, c in ((a_bits, a_c), (b_bits, b_c))]
    clean = []
    try:
        clean = [kernels.cleanup_dev(h, thr) for h in raw]
        assert clean[0].n_terms == ar.shape[0] and clean[1].n_terms == br.shape[0]
        if Na <= 2000:
            rows, c = clean[0].download()
            assert np.array_equal(rows, packing.pack_rows(ar)) and np.array_equal(c, ac, equal_nan=True), 'the cleaned left state is not the oracle\'s'
        got = kernels.state_inner_dev(clean[0], clean[1])
        assert_same_bits(got, want, f'{Na}x{Nb} n={nq} {overlap} {kind}')
        if Na <= 2000:
            # and with the roles exchanged: the sum runs in b's order over a table of a
            want_t = fam.inner_sequential(np.packbits(br, axis=1), bc, np.packbits(ar, axis=1), ac)
            assert_same_bits(kernels.state_inner_dev(clean[1], clean[0]), want_t, f'{Nb}x{Na} n={nq} {overlap} {kind} (exchanged)')
    finally:
        for h in raw + clean:
            h.free()


def bra_ket_expected(bra, ket, a, b):
    """`a`, `b`: (bits, coefficients) of bra and ket.  The state with fewer terms BEFORE the cleanup is the left one (base.py:1808: `<`, so
    equal counts make the ket the left state)."""
    left, right = (a, b) if bra.state_op.n_terms < ket.n_terms else (b, a)
    return expected_inner(left[0], left[1], right[0], right[1], 1e-15)[0]


@pytest.mark.parametrize('kind', ['dyadic', 'gauss', 'wide'])
@pytest.mark.parametrize('shape', ['duplicates', 'equal-counts', 'bra-larger'])
def test_bra_times_ket(shape, kind):
    """QuantumState bra * ket: states with duplicated rows inside (cleaned first, as the reference's to_dictionary does: the duplicates'
    amplitudes are added in input order), equal term counts (the ket becomes the left state), a bra with more terms than the ket."""
    rng = np.random.default_rng([3, len(shape), fam.AMPLITUDES.index(kind)])
    Na, Nb = {'duplicates': (300, 700), 'equal-counts': (513, 513), 'bra-larger': (1025, 65)}[shape]
    a_bits, a_c, b_bits, b_c, _ = fam.states(rng, Na, Nb, 70, 'third', kind)
    if shape == 'duplicates':
        ia, ib = rng.integers(0, Na, 90), rng.integers(0, Nb, 40)
        a_bits, a_c = np.vstack([a_bits, a_bits[ia]]), np.hstack([a_c, fam.amplitudes(rng, 90, kind)])
        b_bits, b_c = np.vstack([b_bits[ib], b_bits]), np.hstack([fam.amplitudes(rng, 40, kind), b_c])
    bra, ket = QuantumState(a_bits, a_c, vec_type='bra'), QuantumState(b_bits, b_c)
    want = bra_ket_expected(bra, ket, (a_bits, a_c), (b_bits, b_c))
    got = bra * ket
    assert isinstance(got, complex)
    assert_same_bits(got, want, f'bra * ket {shape} {kind}')


def test_bra_times_ket_nonfinite_rows_dropped_by_the_cleanup():
    """Through bra * ket the cleanup's threshold comes first: a row whose amplitude has a NaN part (and no infinite one) is dropped from
    its state, as np.abs(c) > 1e-15 drops it in the reference, and the infinities meet in the sum."""
    rng = np.random.default_rng(41)
    a_bits, a_c, b_bits, b_c, _ = fam.states(rng, 300, 1025, 65, 'third', 'nonfinite')
    bra, ket = QuantumState(a_bits, a_c, vec_type='bra'), QuantumState(b_bits, b_c)
    want = bra_ket_expected(bra, ket, (a_bits, a_c), (b_bits, b_c))
    assert_same_bits(bra * ket, want, 'bra * ket nonfinite')


# ------------------------------------------------------------------------------------------------------------------- weak hash ----
@pytest.mark.timeout(300)
@pytest.mark.parametrize('mode', ['inner', 'noncontextual', 'project'])
def test_project_hip_entry_points_on_a_weak_row_hash(mode):
    """SYMGPU_HASH_WEAK_ODD=1 in a fresh process leaves the first seed's row hash four bits: the join of bra * ket walks long probe chains
    of DIFFERENT rows with EQUAL hashes (its word-by-word comparison is all that keeps them apart), and the cleanups inside the
    noncontextuality test and the projection meet bulk collisions and reseed.  tests/_weak_hash_worker3.py compares with the oracle."""
    from test_gpu_multirank import _launch
    rc, o, e = _launch(['tests/_weak_hash_worker3.py', mode], 1, {'SYMGPU_HASH_WEAK_ODD': '1'}, timeout=240)[0]
    assert rc == 0 and f'WEAK_HASH3_OK {mode}' in o, f'rc={rc}\n{o}\n{e[-3000:]}'


# -------------------------------------------------------------------------------------------------------------------- projection ----
def run_projection(case, eig, thr=1e-15):
    """(rows bool, coeff, n_survived) through kernels.project_dev; nothing survives: the handle has no terms."""
    n = case['symp'].shape[1] // 2
    op = DeviceOp.upload(packing.pack_rows(case['symp']), case['coeff'])
    try:
        res, n_s = kernels.project_dev(op, packing.pack_rows(case['stab']), eig, case['keep'], n, thr)
    finally:
        op.free()
    rows, c = res.download()
    res.free()
    return packing.unpack_rows(rows, case['keep'].size), c, n_s


@pytest.mark.parametrize('name', sorted(fam.PROJECTION))
def test_projection_families(name):
    """Output widths of 1, 2, 3 and 5 words (n_keep = 1, 63, 64 | 65, 128 | 129), stabilisers in the first word, on the last qubit and on
    qubits 63 / 64, X and Z kinds, eigenvalues -1, 0 (counts as 1) and +1, T = 1, 255 .. 257 and 70,000 (more than one scan block), none /
    half / all of the terms surviving, 70,000 terms collapsing onto at most 64 (16) rows that are summed in input order.  Through
    kernels.project_dev (int eigenvalues, and the same as a complex +-1+0j vector) and through S3Projection._perform_projection."""
    from symmer_amd.projection.base import S3Projection
    case = fam.projection_family(name)
    symp, coeff, stab, eig, keep = case['symp'], case['coeff'], case['stab'], case['eig'], case['keep']
    n = symp.shape[1] // 2
    exact = fam.PROJECTION[name][5] == 'dyadic'
    er, ec, n_survived = fam.projection_expected(symp, coeff, stab, eig, keep)
    assert n_survived == case['n_survived'] == int(np.all(onp.commutes_termwise(symp, stab), axis=1).sum())
    for ev in (eig, eig.astype(complex)):
        rows, c, n_s = run_projection(case, ev)
        assert n_s == n_survived
        if n_survived == 0:
            assert rows.shape[0] == 0
        else:
            assert_op_equal(rows, c, er, ec, exact=exact, tol=TOL)
    op = PauliwordOp._from_packed(packing.pack_rows(symp), n, coeff)
    proj = S3Projection(IndependentOp(stab, np.ones(stab.shape[0], dtype=int)))
    proj.rotated_stabilizers = PauliwordOp(stab, eig)
    proj.free_qubit_indices = keep
    proj.rotated_flag = True
    out = proj._perform_projection(op)
    assert op._symp is None, 'the projection expanded its operand'
    assert out.n_qubits == keep.size
    assert_op_equal(out.symp_matrix, out.coeff_vec, er, ec, exact=exact, tol=TOL)       # (nothing survives: 0 * I on both sides)


def test_projection_threshold_drops_merged_sums_at_the_threshold():
    """Merged rows summing to 0.25, 0.5, 0.75 and 1.0 under a threshold of 0.5: `>` is strict, a sum equal to the threshold goes."""
    case = fam.threshold_case()
    er, ec, n_survived = fam.projection_expected(case['symp'], case['coeff'], case['stab'], case['eig'], case['keep'], case['thr'])
    all_r, all_c, _ = fam.projection_expected(case['symp'], case['coeff'], case['stab'], case['eig'], case['keep'], None)
    assert (np.abs(all_c) == case['thr']).sum() >= 10 and er.shape[0] < all_r.shape[0]
    rows, c, n_s = run_projection(case, case['eig'], case['thr'])
    assert n_s == n_survived == case['symp'].shape[0]
    assert_op_equal(rows, c, er, ec)
    rows, c, _ = run_projection(case, case['eig'], None)                 # no threshold: every merged row, in first-occurrence order
    assert_op_equal(rows, c, all_r, all_c)
