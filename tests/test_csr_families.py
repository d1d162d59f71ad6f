"""The families of tests/_csr_families.py are what they claim to be (host only): every fact that the GPU tests rely on is proved here
with the NumPy restatements of the two contracts (tests/_sparse_oracle.py, tests/_pauli_decomp_oracle.py), and against the explicit
Kronecker product where the matrix is small."""
import numpy as np
import pytest

import _csr_families as fam
import _pauli_decomp_oracle as po
import _sparse_oracle as so


def data_bits(d):
    return np.ascontiguousarray(d, dtype=np.complex128).view(np.uint64)


def row_entries(csr, b):
    d, i, p = csr
    return dict(zip(i[p[b]:p[b + 1]].tolist(), d[p[b]:p[b + 1]]))


# ---- X-part sets ----------------------------------------------------------------------------------------------------------------
# D -> (rows per workgroup, workgroups, rows of the last workgroup) for 512 rows, restated below from 72 KiB, 20 B and 32 alone
EXPECTED_FORMS = {1: (256, 2, 256), 14: (256, 2, 256), 15: (245, 3, 22), 20: (184, 3, 144), 115: (32, 16, 32), 116: None}


def test_fill_form_arithmetic():
    assert fam.X_PART_COUNTS == tuple(EXPECTED_FORMS)
    for D, want in EXPECTED_FORMS.items():
        per_row = 20 * D
        fits = 72 * 1024 // per_row
        got = None if fits < 32 else (min(256, fits), -(-512 // min(256, fits)), 512 - (-(-512 // min(256, fits)) - 1) * min(256, fits))
        assert got == want == fam.fill_form(D, 512), D
    assert 72 * 1024 // (20 * 14) >= 256 > 72 * 1024 // (20 * 15)          # 14 is the last full-width D
    assert 72 * 1024 // (20 * 115) == 32 and 72 * 1024 // (20 * 116) == 31    # 115 is the last LDS form
    assert 72 * 1024 // (20 * 32) == 115                                      # LDS_MAX_D of test_gpu_sparse_matrix.py


@pytest.mark.parametrize('D', fam.X_PART_COUNTS)
def test_x_part_sets(D):
    symp, c, facts = fam.x_part_set(D)
    n = facts['n']
    assert n == 9 and symp.shape == (len(c), 18) and symp.dtype == bool
    xs = fam.x_ints(symp)
    assert len(np.unique(xs)) == D == facts['D'] and sorted(np.unique(xs).tolist()) == facts['x_parts']
    for must in fam.mandatory_x_parts(n)[:D]:
        assert must in xs
    if D >= 4:
        assert {0, 511, 256, 1} <= set(xs.tolist())
        assert symp[xs == 256][0, :n].tolist() == [True] + [False] * 8 and symp[xs == 1][0, :n].tolist() == [False] * 8 + [True]
    want = EXPECTED_FORMS[D]
    assert facts['lds'] == (want is not None)
    if want:
        assert (facts['rows_per_workgroup'], facts['workgroups'], facts['last_workgroup_rows']) == want
        assert facts['last_workgroup_short'] == (want[2] < want[0]) == (D in (15, 20))
    assert not np.any((c.real == 0) & (c.imag == 0)) and np.array_equal(c * 8, np.round(c * 8))
    d, i, p = so.to_csr(symp, c)
    assert np.all(np.diff(p) <= D) and np.max(np.diff(p)) == D
    for b in (0, 1, 255, 256, 511):
        assert set(row_entries((d, i, p), b)) <= {b ^ x for x in facts['x_parts']}


def test_x_part_set_matches_the_definition_at_8_qubits():
    symp, c, facts = fam.x_part_set(20, n=8)
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))


# ---- term tiles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', sorted(fam.TERM_TILE_SIZES))
def test_term_tiles(T):
    symp, c, facts = fam.term_tiles(T)
    assert facts['n'] == 8 and len(c) == T == symp.shape[0]
    key = fam.sort_key(symp)
    order = fam.sorted_order(symp)
    skey = key[order]
    assert len(np.unique(key)) == 3 and np.all(np.diff(skey) >= 0)
    assert not np.array_equal(order, np.arange(T)), 'the operator order is already sorted'
    for k in np.unique(key):
        assert np.all(np.diff(order[skey == k]) > 0)                         # operator order within a group
    group = np.searchsorted(np.unique(key), skey)                             # group of every sorted position
    last = np.r_[group[1:] != group[:-1], True]
    ends = sorted(int(group[p]) for p in range(255, T, 256) if last[p])
    straddles = sorted(int(group[p]) for p in range(255, T - 1, 256) if group[p] == group[p + 1])
    assert ends == facts['ends_at_255'] and straddles == facts['straddles']
    want = {255: ([], []), 256: ([2], []), 257: ([], [2]), 512: ([0, 2], []), 513: ([0], [2])}[T]
    assert (ends, straddles) == want
    if T == 513:                                                              # the shape that has both, on different groups
        assert ends and straddles and set(ends).isdisjoint(straddles)
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))


# ---- more than 16 qubits ----------------------------------------------------------------------------------------------------------
_LARGE = {}


def large_case(n):
    if n not in _LARGE:
        symp, c, facts = fam.large_n(n)
        _LARGE[n] = (symp, c, facts, so.to_csr(symp, c))
    return _LARGE[n]


@pytest.mark.parametrize('n', fam.LARGE_N)
def test_large_n(n):
    symp, c, facts, (d, i, p) = large_case(n)
    rows = 1 << n
    assert symp.shape == (6, 2 * n) and facts['T'] == 6
    xs = fam.x_ints(symp)
    zs = fam.x_ints(np.hstack([symp[:, n:], symp[:, :n]]))
    q0, qlast = 1 << (n - 1), 1
    assert sorted(set(xs.tolist())) == facts['x_parts'] == sorted([0, q0, q0 | qlast | (1 << (n - 1 - n // 2))])
    assert any(z & q0 for z in zs) and any(z & qlast for z in zs)
    assert symp[:, 0].any() and symp[:, n - 1].any() and symp[:, n].any() and symp[:, 2 * n - 1].any()
    assert {(0, 0), (0, 1 << 12)} <= set(zip(xs.tolist(), zs.tolist()))      # the pair I + Z on the qubit of weight 2^12
    counts = np.diff(p)
    b = np.arange(rows)
    assert np.array_equal(counts, np.where(b & (1 << 12), 0, 3)) and len(d) == facts['nnz'] == 3 * rows // 2
    per_block = counts.reshape(-1, fam.SCAN_ITEMS).sum(axis=1)
    assert len(per_block) == facts['scan_blocks'] and np.count_nonzero(per_block == 0) == facts['empty_scan_blocks'] == len(per_block) // 2
    assert facts['scan_top_rounds'] == {17: 1, 19: 1, 21: 2}[n] and facts['sort_passes'] == 3
    assert 64 - n < 48
    for r in (0, 1, 4095, rows // 2, rows - 4097):
        assert sorted(row_entries((d, i, p), r)) == sorted(r ^ x for x in facts['x_parts'])
    for r in (4096, rows // 2 - 1, rows - 1):
        assert not row_entries((d, i, p), r)
    assert np.all(np.abs(d.real) + np.abs(d.imag) > 0) and np.array_equal(d * 4, np.round(d * 4))


# ---- coefficient kinds ------------------------------------------------------------------------------------------------------------
def test_dyadic_kind():
    symp, c, facts = fam.coeff_kind('dyadic')
    assert np.array_equal(c * 8, np.round(c * 8))
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))
    a, b = so.to_csr(symp, c), so.to_csr(symp[::-1], c[::-1])
    assert all(np.array_equal(u, v) for u, v in zip(a, b)), 'dyadic sums are exact in any order'


def test_wide_kind_depends_on_the_order_of_additions():
    symp, c, facts = fam.coeff_kind('wide')
    n = facts['n']
    mags = np.abs(np.concatenate([c.real, c.imag]))
    assert mags.min() >= 1e-8 and mags.max() <= 1e8 and mags.max() / mags.min() > 1e10
    assert np.any(c.real < 0) and np.any(c.real > 0)
    xs, zs = fam.x_ints(symp), fam.x_ints(np.hstack([symp[:, n:], symp[:, :n]]))
    for x in np.unique(xs):
        _, shared = np.unique(zs[xs == x], return_counts=True)
        assert shared.max() >= 4, 'a group without four terms of one Z-part'
    forward = so.to_csr(symp, c)
    backward = so.to_csr(symp[::-1], c[::-1])                                 # every group's terms added in reversed order
    assert np.array_equal(forward[1], backward[1]) and np.array_equal(forward[2], backward[2])
    assert np.count_nonzero(data_bits(forward[0]) != data_bits(backward[0])) > 0, 'the case says nothing about the order of additions'
    assert np.allclose(so.to_dense(symp, c), so.kron_dense(symp, c), rtol=0, atol=16 * 2.0 ** -52 * 7e8)


def test_nonfinite_kind():
    symp, c, facts = fam.coeff_kind('nonfinite')
    n = facts['n']
    with np.errstate(invalid='ignore'):                                       # inf - inf is the point
        csr = so.to_csr(symp, c)
    z1, z2 = facts['meet_z']
    parity = lambda v: bin(v).count('1') & 1
    seen = {'nan': 0, 'inf': 0}
    for b in range(1 << n):
        row = row_entries(csr, b)
        assert len(row) == 4
        alone = row[b ^ facts['inf_alone']]
        assert np.isinf(alone.real) and alone.imag == 0
        meet = row[b ^ facts['inf_meets']]
        if parity(b & z1) == parity(b & z2):                                  # +inf and -inf with the same sign flip: inf - inf
            assert np.isnan(meet.real) and not np.isnan(meet.imag)
            seen['nan'] += 1
        else:
            assert np.isinf(meet.real) and meet.imag == 0
            seen['inf'] += 1
        only_imag = row[b ^ facts['nan_imag']]
        assert only_imag.real == 1.0 and np.isnan(only_imag.imag)
        assert np.isfinite(row[b ^ facts['plain']])
    assert seen == {'nan': 1 << (n - 1), 'inf': 1 << (n - 1)}
    assert {np.sign(row_entries(csr, b)[b ^ facts['inf_alone']].real) for b in range(1 << n)} == {-1.0, 1.0}


def test_zeros_kind():
    symp, c, facts = fam.coeff_kind('zeros')
    n = facts['n']
    assert np.signbit(c.real[0]) and not np.signbit(c.imag[0]) and c[0] == 0
    assert not np.signbit(c.real[1]) and np.signbit(c.imag[1]) and c[1] == 0
    assert c[2] == -c[3] and c[2] != 0 and np.array_equal(symp[2], symp[3])
    assert c[4].real == -c[5].real and c[4].imag != -c[5].imag and np.array_equal(symp[4], symp[5])
    d, i, p = csr = so.to_csr(symp, c)
    assert np.all(np.diff(p) == len(facts['stored'])) and not np.any((d.real == 0) & (d.imag == 0))
    for b in range(1 << n):
        row = row_entries(csr, b)
        assert sorted(row) == sorted(b ^ x for x in facts['stored'])
        v = row[b ^ facts['imag_only']]
        assert v.real == 0 and abs(v.imag) == facts['imag_only_value']
    assert np.array_equal(so.to_dense(symp, c), so.kron_dense(symp, c))


# ---- the forced index width is refused on the host ------------------------------------------------------------------------------------
def test_forced_index_dtype():
    from symmer_amd import kernels
    big = np.iinfo(np.int32).max
    assert kernels.csr_forced_index_dtype(10, 4, None) is np.int32 and kernels.csr_forced_index_dtype(big + 1, 30, None) is np.int64
    assert kernels.csr_forced_index_dtype(big, 30, np.int32) is np.int32
    assert kernels.csr_forced_index_dtype(0, 31, None) is np.int64            # 2^31 rows: indptr's length alone needs int64
    with pytest.raises(ValueError, match='do not fit int32'):
        kernels.csr_forced_index_dtype(0, 31, np.int32)
    assert kernels.csr_forced_index_dtype(10, 4, np.int64) is np.int64 and kernels.csr_forced_index_dtype(10, 4, 'int64') is np.int64
    assert kernels.csr_forced_index_dtype(big + 1, 31, np.int64) is np.int64
    with pytest.raises(ValueError, match='do not fit int32'):
        kernels.csr_forced_index_dtype(big + 1, 31, np.int32)
    for bad in (np.uint32, np.int16, float):
        with pytest.raises(ValueError, match='neither int32 nor int64'):
            kernels.csr_forced_index_dtype(10, 4, bad)


# ---- from_matrix: the block bases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, name', [(n, name) for n in sorted(fam.BLOCK_BASES) for name in fam.BLOCK_BASES[n]])
def test_block_bases(n, name):
    bx, bz, facts = fam.block_basis(n, name)
    assert bx.dtype == np.dtype('<u8') and bx.shape == bz.shape == (facts['K'],) and bx.max() < 1 << n and bz.max() < 1 << n
    xs = np.unique(bx).astype(np.int64)
    assert len(xs) == facts['D']
    blocks = []
    for x0 in sorted({int(x) // 32 * 32 for x in xs}):                        # what pd_dense builds from the sorted distinct X-parts
        inside = xs[(xs >= x0) & (xs < x0 + 32)]
        blocks.append((x0, int(np.searchsorted(xs, x0)), sum(1 << int(x - x0) for x in inside)))
    assert blocks == facts['blocks']
    masks = {x0 // 32: m for x0, _, m in blocks}
    for blk, what in enumerate(facts['layout']):
        if what is None:
            assert blk not in masks
        elif what == 'first':
            assert masks[blk] == 1
        elif what == 'last':
            assert masks[blk] == 1 << 31
        elif what == 'all':
            assert masks[blk] == 0xFFFFFFFF
        else:
            assert masks[blk] & 1 and masks[blk] >> 31 and 2 < bin(masks[blk]).count('1') < 32
    kinds = [w for names in fam.BLOCK_BASES[n].values() for w in names]
    assert {'first', 'last', 'all'} <= set(kinds)
    if n > 5:
        assert None in kinds
        assert any(names[-1] is not None for names in fam.BLOCK_BASES[n].values()), 'the last block of the range is never present'
    if n == 8:
        lay = facts['layout']
        assert any(lay[k] is None and lay[k - 1] is not None and lay[k + 1] is not None for k in range(1, 7)), 'no absent block between two present ones'
        assert lay[-1] is not None and any(r > 0 and m != 0xFFFFFFFF for _, r, m in blocks[1:])
    _, per_x = np.unique(bx, return_counts=True)
    assert per_x.max() > 1, 'no X-part with several Z-parts'
    assert len(set(zip(bx.tolist(), bz.tolist()))) == facts['K']
    pair = bx.astype(np.int64) * (1 << n) + bz.astype(np.int64)
    assert facts['K'] > 1 and np.any(np.diff(pair) < 0), 'the basis is in (x, z) order'


def test_block_basis_picks_against_the_definition():
    """coefficients_of_diagonals at the basis's (x, z) are the Pauli coefficients of the matrix: rebuilt from them, a matrix made of
    exactly those terms comes back."""
    n = 5
    bx, bz, _ = fam.block_basis(n, 'all')
    rng = np.random.default_rng(3)
    c = fam.dyadic(rng, len(bx))
    M = so.kron_dense(po.symp_of(bx.astype(np.int64), bz.astype(np.int64), n), c)
    full = po.coefficients_of_diagonals(po.diagonals(M, np.arange(1 << n)), np.arange(1 << n), n)
    assert np.array_equal(full[bx.astype(np.int64), bz.astype(np.int64)], c)
    assert np.count_nonzero(full) == len(bx)
