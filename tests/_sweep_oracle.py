"""Oracles and case families of the noncontextual sweep (csrc/noncon_sweep.hip; reference symmer/operators/utils.py:592-616
``perform_noncontextual_sweep`` on ``check_adjmat_noncontextual``, :567-589).

``ref_sweep``   the reference loop, literally: pad the kept terms' adjacency matrix by the candidate's row and column, keep the candidate
                if the unique rows among the terms that do not commute with everything are disjoint.
``rule_sweep``  the rule the kernel implements, in plain NumPy, with labels: -2 rejected, -1 SYM (commutes with every kept term),
                c >= 0 the clique in order of creation.  tests/test_sweep_oracle.py holds the two against each other and ``ref_sweep``
                against the reference's recorded answers (tests/golden/noncon_sweep.npz).

Both take the T x T commutation table (anything that gives row t as ``adj[t]``) and the sequence of term indices to visit, and answer
in term indices, whatever the visit order."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
REJECTED, SYM = -2, -1


# ---- operators -------------------------------------------------------------------------------------------------------------------------
def symp_of(strings):
    """bool[T, 2n] of Pauli strings over I/X/Y/Z (qubit 0 first)."""
    chars = np.array([list(s) for s in strings])
    return np.hstack([(chars == 'X') | (chars == 'Y'), (chars == 'Z') | (chars == 'Y')])


def adjacency(symp):
    """bool[T, T]: True where terms commute."""
    symp = np.asarray(symp, dtype=bool)
    n = symp.shape[1] // 2
    x, z = symp[:, :n].astype(np.int64), symp[:, n:].astype(np.int64)
    return (x @ z.T + z @ x.T) % 2 == 0


class LazyAdjacency:
    """``adj[t]`` = row t of ``adjacency(symp)`` without the T x T matrix (for the sizes at which that matrix is too much)."""

    def __init__(self, symp):
        symp = np.asarray(symp, dtype=bool)
        n = symp.shape[1] // 2
        assert n < (1 << 22)                                         # the counts below are exact in float32
        self.xz = np.hstack([symp[:, :n], symp[:, n:]]).astype(np.float32)
        self.zx = np.hstack([symp[:, n:], symp[:, :n]]).astype(np.float32)
        self.shape = (symp.shape[0], symp.shape[0])

    def __getitem__(self, t):
        return ((self.xz @ self.zx[t]).astype(np.int32) & 1) == 0


# ---- the reference loop ------------------------------------------------------------------------------------------------------------------
def adjmat_noncontextual(adjmat):
    """utils.py:567-589: among the terms that do not commute with everything, the unique rows must not overlap."""
    non_universal = np.where(~np.all(adjmat, axis=1))[0]
    characters = np.unique(adjmat[non_universal, :][:, non_universal], axis=0)
    return bool(np.all(np.count_nonzero(characters, axis=0) == 1))


def ref_sweep(adj, visit=None):
    """Kept term indices, ascending in visit position (i.e. in the order they were kept), of the reference loop over ``visit``."""
    adj = np.asarray(adj, dtype=bool)
    visit = np.arange(adj.shape[0]) if visit is None else np.asarray(visit, dtype=np.int64)
    if len(visit) == 0:
        return np.zeros(0, dtype=np.int64)
    adj = adj[np.ix_(visit, visit)]
    noncon_indices = np.array([0])
    adjmat = np.array([[True]], dtype=bool)
    for index in range(len(visit) - 1):
        adjmat_vector = np.append(adj[index + 1, noncon_indices], True)
        adjmat_padded = np.pad(adjmat, pad_width=((0, 1), (0, 1)), mode='constant')
        adjmat_padded[-1, :] = adjmat_vector
        adjmat_padded[:, -1] = adjmat_vector
        if adjmat_noncontextual(adjmat_padded):
            noncon_indices = np.append(noncon_indices, index + 1)
            adjmat = adjmat_padded
    return visit[noncon_indices]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------
def rule_sweep(adj, visit=None):
    """(kept term indices in the order they were kept, int32 labels[T] by term index) of the rule over ``visit``."""
    T = adj.shape[0]
    visit = np.arange(T) if visit is None else np.asarray(visit, dtype=np.int64)
    labels = np.full(T, REJECTED, dtype=np.int32)
    kept, sym, clq = np.zeros(T, dtype=bool), np.zeros(T, dtype=bool), np.zeros(T, dtype=bool)
    kept_list, m = [], 0
    for i, t in enumerate(visit):
        row = np.asarray(adj[t], dtype=bool)
        anti = ~row & kept
        if i == 0 or not anti.any():
            label = SYM                                              # 1
        elif m == 0:
            labels[anti] = 0                                         # 2: the demotion
            sym &= ~anti
            clq |= anti
            label, m = 1, 2
        elif (anti & sym).any():
            continue                                                 # 3
        else:
            commuting = row & clq
            if not commuting.any():
                label, m = m, m + 1                                  # 4
            else:
                j = labels[np.flatnonzero(commuting)[0]]
                if not np.array_equal(commuting, clq & (labels == j)):
                    continue                                         # 5, rejected
                label = j                                            # 5, joined
        kept[t], labels[t] = True, label
        sym[t], clq[t] = label == SYM, label >= 0
        kept_list.append(t)
    return np.array(kept_list, dtype=np.int64), labels


# ---- case families -----------------------------------------------------------------------------------------------------------------------
def random_symp(rng, n, T, half_diagonal=False, density=0.5):
    symp = rng.random((T, 2 * n)) < density
    if half_diagonal:
        symp[: T // 2, :n] = False
    return symp


def small_random_cases(seed, count):
    """``count`` operators of 2 .. 5 qubits and 1 .. 39 terms, every third one with half of its terms diagonal; rows may repeat."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n, T = int(rng.integers(2, 6)), int(rng.integers(1, 40))
        yield random_symp(rng, n, T, half_diagonal=k % 3 == 0, density=float(rng.choice([0.3, 0.5])))


def majoranas(n):
    """2n + 1 mutually anticommuting strings on n qubits: Z..Z X I..I, Z..Z Y I..I per qubit, and Z..Z."""
    out = []
    for q in range(n):
        out += ['Z' * q + 'X' + 'I' * (n - q - 1), 'Z' * q + 'Y' + 'I' * (n - q - 1)]
    return out + ['Z' * n]


def z_strings(n, count):
    """``count`` distinct diagonal strings on n qubits: the binary digits of 1, 2, ... as Z (qubit 0 = lowest digit)."""
    assert count < (1 << n)
    return [''.join('Z' if (k >> q) & 1 else 'I' for q in range(n)) for k in range(1, count + 1)]


def demotion_case(count, n=8):
    """``count`` commuting diagonal terms, then X on qubit 0 (the terms with Z there become clique 0, X clique 1), then Y on qubit 0
    (anticommutes with both cliques, commutes with SYM: clique 2), then X on qubit 1 (anticommutes with the SYM term Z on qubit 1:
    rejected), then the identity (SYM)."""
    diag = z_strings(n, count)
    strings = diag + ['X' + 'I' * (n - 1), 'Y' + 'I' * (n - 1), 'IX' + 'I' * (n - 2), 'I' * n]
    labels = [0 if s[0] == 'Z' else SYM for s in diag] + [1, 2, REJECTED, SYM]
    return strings, labels


# every branch of the rule with its answer worked out by hand: (name, strings in visit order, label of each)
BY_HAND = [
    ('accept as SYM', ['ZI', 'IZ', 'ZZ', 'II'], [SYM, SYM, SYM, SYM]),
    ('demotion after 70', *demotion_case(70)),
    ('demotion after 130', *demotion_case(130)),
    ('new cliques: 13 anticommuting terms on 6 qubits', majoranas(6), list(range(13))),
    # XI | ZI: two cliques; XZ commutes with XI alone: joins clique 0; ZZ commutes with ZI alone (XI: anti, XZ: X.Z anti, Z.Z: commutes -> anti): joins 1
    ('join', ['XI', 'ZI', 'XZ', 'ZZ'], [0, 1, 0, 1]),
    # IZ commutes with XI and ZI and stays SYM; IX commutes with both cliques but anticommutes with IZ
    ('reject: anticommutes with a SYM term', ['IZ', 'XI', 'ZI', 'IX'], [SYM, 0, 1, REJECTED]),
    # clique 0 = {XI, XZ}; XX commutes with XI, anticommutes with XZ (second qubit) and with ZI
    ('reject: commutes with part of a clique', ['XI', 'ZI', 'XZ', 'XX'], [0, 1, 0, REJECTED]),
    # cliques {XI}, {ZI}, {YZ}; IX commutes with XI and ZI, anticommutes with YZ
    ('reject: commutes fully with two cliques', ['XI', 'ZI', 'YZ', 'IX'], [0, 1, 2, REJECTED]),
    ('identity first', ['II', 'XI', 'ZI', 'YI'], [SYM, 0, 1, 2]),
    ('identity last', ['XI', 'ZI', 'YI', 'II'], [0, 1, 2, SYM]),
    ('duplicate rows', ['XI', 'ZI', 'XI', 'ZI', 'XI'], [0, 1, 0, 1, 0]),
]

# the 12 terms of the reference's noncontextuality test (tests/test_operators/test_base.py): the cliques {IZI, ZII, IIY, ZZY},
# {XXZ, YYZ, XYX, YXX} and {XYZ, YXZ, XXX, YYX}.  IIX, visited sixth, commutes with IZI and ZII but not with IIY and ZZY: rejected.
TWELVE = ['IZI', 'ZII', 'IIY', 'ZZY', 'XXZ', 'XYZ', 'YXZ', 'YYZ', 'XXX', 'XYX', 'YXX', 'YYX']
TWELVE_AND_ONE = TWELVE[:5] + ['IIX'] + TWELVE[5:]
TWELVE_AND_ONE_KEPT = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12]
TWELVE_AND_ONE_LABELS = [0, 0, 0, 0, 1, REJECTED, 2, 2, 1, 2, 1, 1, 2]


# ---- the reference's recorded answers ----------------------------------------------------------------------------------------------------
def golden():
    return np.load(os.path.join(GOLDEN, 'noncon_sweep.npz'))


def golden_cases(gold=None):
    """[(tag, kind, symp, coeff)] of tests/golden/noncon_sweep.npz; kind 'sweep' cases carry ``kept`` only, kind 'dfs' cases all of
    ``kept``, ``single_magnitude``, ``dfs_magnitude``, ``dfs_largest``, ``diag_first`` (each a symp / coeff pair)."""
    gold = golden() if gold is None else gold
    return [(f'{k:02d}', str(gold[f'{k:02d}/kind']), gold[f'{k:02d}/symp'].astype(bool), gold[f'{k:02d}/coeff'])
            for k in range(int(gold['n_cases']))]
