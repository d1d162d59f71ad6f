"""CPU: the operand families of tests/_commute_families.py have the tables they claim, and live in the 7-bit groups they name.

Every claimed table is compared, in full, with oracle_np.commutes_termwise (the NumPy restatement of the reference's matmul_GF2) at the
sizes the GPU tests use or smaller ones with the same structure; the group bookkeeping (which 7-bit groups of the packed left operand are
non-zero — what sets the step count S of the Four-Russians kernel) is checked on the rows packed by symmer_amd.packing.pack_rows, the very
words the kernels read.  An edit to a family that loses its property fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from symmer_amd import packing
import _commute_families as fam

ONE_HOT_N = [1, 63, 64, 65, 100, 128, 257]
MAJORANA_N = [64, 65, 200, 700]


def test_notation():
    assert [fam.wq_of(n) for n in (1, 64, 65, 128, 129, 257)] == [1, 1, 2, 2, 3, 5]
    assert [fam.ng7_of(n) for n in (1, 64, 65, 100, 257)] == [19, 19, 37, 37, 92]
    n = 100
    assert fam.packed_bit(n, 0) == 0 and fam.packed_bit(n, 99) == 99 and fam.packed_bit(n, 100) == 128 and fam.packed_bit(n, 199) == 227
    assert fam.partner(n, 3) == 103 and fam.partner(n, 103) == 3
    # packed_bit is the rule of packing.pack_rows
    for n in (1, 64, 65, 100, 257):
        eye = np.eye(2 * n, dtype=bool)
        p = packing.pack_rows(eye)
        bits = fam.unpack_cols(p, 128 * fam.wq_of(n))
        assert np.array_equal(np.argmax(bits, axis=1), fam.packed_bit(n, np.arange(2 * n))) and (bits.sum(axis=1) == 1).all()
    m = np.random.default_rng(0).random((5, 131)) < 0.5
    assert np.array_equal(fam.pack_cols(m), packing.pack_bits(m)) and np.array_equal(fam.unpack_cols(fam.pack_cols(m), 131), m)


@pytest.mark.parametrize('n', ONE_HOT_N)
def test_one_hot_answer(n):
    M = 70
    A, B, C = fam.one_hot(n, M, np.random.default_rng(n))
    assert A.shape == (2 * n, 2 * n) and np.array_equal(A, np.eye(2 * n, dtype=bool))
    assert not B[0].any() and B[1].all() and 0.4 < B[2:].mean() < 0.6
    assert C[:, 0].all() and not C[:, 1].any()
    assert np.array_equal(C, onp.commutes_termwise(A, B)), 'one-hot rows as the left operand'
    assert np.array_equal(C.T, onp.commutes_termwise(B, A)), 'one-hot rows as the right operand'
    # a subset of the rows is the same rows of the table
    cols = np.array([0, n - 1, n, 2 * n - 1])
    A2, B2, C2 = fam.one_hot(n, M, np.random.default_rng(n), cols=cols)
    assert np.array_equal(B2, B) and np.array_equal(A2, A[cols]) and np.array_equal(C2, C[cols])


def test_one_hot_sizes_reach_the_named_bits():
    """What the sizes of ONE_HOT_N are for, in the packed layout."""
    assert fam.wq_of(1) == 1 and fam.wq_of(64) == 1                                        # one word, a full word
    g65 = set(fam.group_of(65, np.arange(130)).tolist())                                   # Wq = 2 with 63 padding bits a half
    assert fam.wq_of(65) == 2 and set(range(10, 18)).isdisjoint(g65) and {9, 18, 27}.issubset(g65)   # whole groups of padding stay zero
    for n in (65, 100, 128):
        assert 9 in fam.group_of(n, [63, 64]) and (fam.group_of(n, [63, 64]) == 9).all()   # group 9 = packed bits 63..69: words 0 / 1
        assert fam.group_of(n, n) == 18                                                    # Z of qubit 0 = packed bit 128, group 18 = bits 126..132
    assert (fam.group_of(128, [126, 127, 128, 129]) == 18).all()                           # n = 128: the straddling group is live on both sides
    assert fam.ng7_of(257) == 92 and fam.group_of(257, 2 * 257 - 1) == 82 > 64             # a second ballot round
    assert fam.group_of(257, 257) == fam.group_of(257, 258) == 45                          # Z of qubits 0, 1 = packed bits 320, 321: the group across the halves at Wq = 5


@pytest.mark.parametrize('n', MAJORANA_N)
def test_majorana_stack_answer(n):
    A, C = fam.majorana_stack(n)
    T = 3 * n + 1
    assert A.shape == (T, 2 * n) and C.shape == (T, T)
    x, z = A[:, :n], A[:, n:]
    j = n // 2
    assert x[2 * j].sum() == 1 and x[2 * j, j] and z[2 * j].sum() == j and z[2 * j, :j].all()                 # Z..Z X
    assert x[2 * j + 1, j] and z[2 * j + 1].sum() == j + 1 and z[2 * j + 1, :j + 1].all()                     # Z..Z Y
    assert not A[2 * n].any() and not x[2 * n:].any() and z[-1].all()                                        # P_0 = identity, P_n = all Z
    assert np.array_equal(C, C.T)
    assert np.array_equal(C, onp.commutes_termwise(A, A))
    # dense across every word of both halves
    p = packing.pack_rows(A)
    assert (p != 0).any(axis=0).all()


def test_group_sets_at_the_sizes_used():
    assert fam.group_sets(100) == {'first': [0], 'word_straddle': [9], 'half_straddle+last': [18, 32], 'odd3': [0, 9, 18],
                                   'five': [0, 9, 14, 18, 27]}
    s = fam.group_sets(257)
    assert s['half_straddle'] == [45] and 7 * 45 <= 319 and 320 < 7 * 46                    # the group across packed bit 320
    assert s['high'] == [64, 73, 82] and 7 * 73 <= 511 and 512 < 7 * 74                     # 73: across words 7 / 8 of the packed row
    assert [fam.steps_of(v) for v in fam.group_sets(100).values()] == [1, 1, 1, 2, 3]
    assert fam.steps_of(s['high']) == 2 and fam.steps_of(s['half_straddle']) == 1 and fam.steps_of([]) == 1


SPARSE_CASES = [(100, name) for name in ('first', 'word_straddle', 'half_straddle+last', 'odd3', 'five')] + [(257, 'half_straddle'), (257, 'high')]


@pytest.mark.parametrize('n,name', SPARSE_CASES, ids=[f'{n}-{name}' for n, name in SPARSE_CASES])
def test_sparse_groups_answer_and_groups(n, name):
    groups = fam.group_sets(n)[name]
    N, M = 150, 333
    A, B, Cb = fam.sparse_groups(n, groups, N, M, np.random.default_rng(5))
    assert A.shape == (N, 2 * n) and B.shape == (M, 2 * n) and Cb.shape == (N, 6) and Cb.dtype == np.dtype('<u8')
    assert not A[0].any() and 0.4 < B.mean() < 0.6
    assert fam.nonzero_groups(packing.pack_rows(A), n) == groups, 'the packed left operand is non-zero in exactly the named groups'
    live = fam.live_columns(n, groups)
    assert 0.4 < A[len(groups) + 1:, live].mean() < 0.6 and not np.delete(A, live, axis=1).any()
    C = onp.commutes_termwise(A, B)
    assert np.array_equal(fam.unpack_cols(Cb, M), C)
    assert np.array_equal(Cb, packing.pack_bits(C, 6)), 'padding bits of the last word are zero'
    assert fam.unpack_cols(Cb, M)[0].all()                                                  # the identity commutes with everything


def test_sparse_groups_every_column_of_a_straddling_group_matters():
    """The straddling groups at n = 100 have live columns on the side the kernel reaches through its second word / the other half."""
    assert fam.live_columns(100, {9}).tolist() == list(range(63, 70))                       # X of qubits 63..69: bit 63 of word 0, bits 0..5 of word 1
    assert fam.live_columns(100, {18}).tolist() == list(range(100, 105))                    # Z of qubits 0..4 (X of qubits 126, 127 do not exist)
    assert fam.live_columns(128, {18}).tolist() == [126, 127, 128, 129, 130, 131, 132]      # n = 128: X of 126, 127 and Z of 0..4
    assert fam.live_columns(100, {32}).tolist() == [196, 197, 198, 199]                     # the last group: 4 live bits, 3 of padding
    assert fam.live_columns(100, {36}).size == 0                                            # the row's last group is padding only


def test_families_are_seeded():
    a = fam.sparse_groups(100, [0, 9], 40, 70, np.random.default_rng(3))
    b = fam.sparse_groups(100, [0, 9], 40, 70, np.random.default_rng(3))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a = fam.one_hot(65, 40, np.random.default_rng(3)); b = fam.one_hot(65, 40, np.random.default_rng(3))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_sparse_groups_at_the_stream_k_size_is_quick():
    """The expected table of the stream-K tests (8,667 x 32,750, bit-packed: 35 MB) is built on packed words."""
    import time
    t0 = time.perf_counter()
    A, B, Cb = fam.sparse_groups(100, fam.group_sets(100)['five'], 32 * 16 * 17 - 37, 32750, np.random.default_rng(1))
    dt = time.perf_counter() - t0
    print(f'sparse_groups at the stream-K size: {dt:.2f} s')
    assert Cb.shape == (8667, 512)
    rows = [0, 1, 4000, 8666]
    assert np.array_equal(fam.unpack_cols(Cb[rows], 32750), onp.commutes_termwise(A[rows], B))
