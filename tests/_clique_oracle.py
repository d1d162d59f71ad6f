"""NumPy / plain-loop restatement of what csrc/clique.hip computes (include/symgpu.h, section g): the three termwise relations on boolean
symplectic matrices, relation degrees, the two term orders of ``PauliwordOp.clique_cover`` and first-fit.  No networkx, no device.
tests/test_clique_oracle.py holds it against answers of the reference (tests/golden/clique_cover.npz); tests/test_gpu_clique.py holds
the kernels against it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clique_cover.npz')
RELATIONS = ('C', 'AC', 'QWC')
STRATEGIES = ('sorted_insertion', 'largest_first')


def relation_table(symp_a, symp_b, relation):
    """bool[N, M]: term i of a related to term j of b.  Row by row, so that no [N, M, n] temporary exists."""
    a, b = np.asarray(symp_a, dtype=bool), np.asarray(symp_b, dtype=bool)
    n = a.shape[1] // 2
    xa, za, xb, zb = a[:, :n], a[:, n:], b[:, :n], b[:, n:]
    out = np.empty((a.shape[0], b.shape[0]), dtype=bool)
    for i in range(a.shape[0]):
        if relation == 'QWC':
            both = (xa[i] | za[i]) & (xb | zb)
            out[i] = ~np.any(both & ((xa[i] ^ xb) | (za[i] ^ zb)), axis=1)
        else:
            odd = (np.count_nonzero(xa[i] & zb, axis=1) + np.count_nonzero(za[i] & xb, axis=1)) % 2 == 1
            out[i] = odd if relation == 'AC' else ~odd
    return out


def graph_table(symp, relation):
    """The relation among the terms of one operator with the diagonal cleared: a term is never related to itself (the same index)."""
    table = relation_table(symp, symp, relation)
    np.fill_diagonal(table, False)
    return table


def degrees(symp, relation):
    return graph_table(symp, relation).sum(axis=1, dtype=np.int64)


def term_order(symp, coeff, relation, strategy):
    """The order in which ``clique_cover`` colours the terms."""
    T = len(coeff)
    if strategy == 'sorted_insertion':
        return np.argsort(-abs(np.asarray(coeff)))
    assert strategy == 'largest_first'
    return np.argsort(-(T - 1 - degrees(symp, relation)), kind='stable')


def first_fit(related, order):
    """related: bool[T, T] (its diagonal is not read).  Walks ``order``; every term takes the lowest colour all of whose members it is
    related to.  Returns (int32 colours by term index, number of colours)."""
    T = related.shape[0]
    colours = np.full(T, -1, dtype=np.int32)
    members = []
    for t in order:
        for k, clique in enumerate(members):
            if all(related[t, u] for u in clique):
                break
        else:
            k = len(members)
            members.append([])
        members[k].append(int(t))
        colours[t] = k
    return colours, len(members)


def colouring(symp, order, relation):
    return first_fit(relation_table(symp, symp, relation), order)


def cliques_in_order(colours, order):
    """Per colour the term indices in colouring order."""
    out = [[] for _ in range(int(colours.max()) + 1 if len(colours) else 0)]
    for t in order:
        out[colours[t]].append(int(t))
    return out


def golden_cases():
    """[(tag, dict)] of tests/golden/clique_cover.npz: n, symp bool[T, 2n], coeff, qwc bool[T, T], and per (relation, strategy) the
    reference's clique index of every term (``colour``) and the term indices clique after clique in the clique's own order (``members``)."""
    z = np.load(GOLDEN)
    cases = []
    for k in range(int(z['n_cases'])):
        tag = f'{k:02d}'
        case = {'n': int(z[f'{tag}/n']), 'symp': z[f'{tag}/symp'].astype(bool), 'coeff': z[f'{tag}/coeff'], 'qwc': z[f'{tag}/qwc'].astype(bool)}
        for rel in RELATIONS:
            for strat in STRATEGIES:
                key = f'{tag}/{rel}/{strat}'
                if f'{key}/colour' in z.files:
                    case[(rel, strat)] = (z[f'{key}/colour'].astype(np.int32), z[f'{key}/members'].astype(np.int64))
        cases.append((tag, case))
    return cases
