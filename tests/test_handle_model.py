"""CPU: the host model of a device handle and its sequence generator (tests/_handle_model.py) against oracle.oracle_np, so that the GPU
test that replays the sequences (tests/test_gpu_handle_state.py) compares the library with something that has itself been checked, and
cannot silently degenerate: every sequence it runs holds every hazard, is deterministic, and stays within exact arithmetic."""
import numpy as np
import pytest

import _handle_model as hm
from oracle import oracle_np as onp
from _golden import assert_op_equal

CASES = [(seed, n) for n in hm.GPU_SIZES for seed in hm.GPU_SEEDS]
HAZARD_FLOOR = 1                 # each hazard at least once in every sequence: the scripted prologue holds one of each


@pytest.fixture(scope='module')
def sequences():
    return {case: hm.generate(*case) for case in CASES}


def test_packing_matches_the_oracle():
    rng = np.random.default_rng(3)
    for n in (1, 64, 70, 128, 130):
        symp = rng.random((9, 2 * n)) < 0.4
        assert np.array_equal(hm.pack(symp), onp.pack_rows(symp)) and np.array_equal(hm.unpack(hm.pack(symp), n), symp)


def test_the_generator_is_deterministic_and_holds_every_hazard(sequences):
    """The floor that the GPU test relies on, per hazard and per sequence; the same seed gives the same steps again."""
    assert len(CASES) == 40
    for (seed, n), seq in sequences.items():
        again = hm.generate(seed, n)
        assert len(again.steps) == len(seq.steps) >= 30 + seq.n_slots and again.hazards == seq.hazards
        for a, b in zip(seq.steps, again.steps):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        print(seed, n, seq.hazards)
        for name in hm.HAZARDS:
            assert seq.hazards[name] >= HAZARD_FLOOR, (seed, n, name, seq.hazards)
    kinds = {step[0] for seq in sequences.values() for step in seq.steps}
    assert kinds == {'fresh', 'write', 'copy_rows', 'set_rows', 'set_coeff', 'scale', 'mul_into', 'clone', 'gather', 'concat', 'slice', 'cleanup',
                     'mul_cleanup', 'rotate', 'chain'}
    rotations = [step for seq in sequences.values() for step in seq.steps if step[0] == 'rotate']
    assert {step[4] for step in rotations} == {-1, 0, 1, 2, 3}


def test_the_models_operations_agree_with_the_oracle_on_the_generated_operands(sequences):
    """Replays every sequence on the model; every product, cleanup, rotation, commutation table and Y count the model forms on the way is
    recomputed by oracle_np on the unpacked operands (dyadic coefficients: bit for bit), and the bookkeeping of every step is checked:
    sizes within their bounds, exact arithmetic, and distinct_known only where the rows are pairwise distinct."""
    checked = dict.fromkeys(('product', 'cleanup', 'rotate', 'chain'), 0)
    for (seed, n), seq in sequences.items():
        model = hm.Model(seq.n_slots)
        U = lambda rows: hm.unpack(rows, n)
        for step in seq.steps:
            kind = step[0]
            before = [None if s is None else (s.rows[:s.T].copy(), s.coeff[:s.T].copy()) for s in model.slots]
            touched = model.apply(step)
            dst = model.slots[step[1]]
            got = (U(dst.live()[0]), dst.live()[1])
            if kind == 'mul_into':
                _, _, inner, outer, o0, o1, left = step
                (ri, ci), (ro, co) = before[inner], before[outer]
                l, r = ((U(ri), ci), (U(ro[o0:o1]), co[o0:o1]))
                rows, coeff = onp.product_rows_and_coeffs(*l, *r) if left else onp.product_rows_and_coeffs(*r, *l)
                if not left:                                           # the oracle orders pairs by its RIGHT operand: back to o * Ni + i
                    ni, no = ri.shape[0], o1 - o0
                    order = (np.arange(ni)[None, :] * no + np.arange(no)[:, None]).reshape(-1)
                    rows, coeff = rows[order], coeff[order]
                assert_op_equal(*got, rows, coeff)
                checked['product'] += 1
            elif kind == 'cleanup':
                assert_op_equal(*got, *onp.symplectic_cleanup(U(before[step[2]][0]), before[step[2]][1], 1e-15))
                checked['cleanup'] += 1
            elif kind == 'mul_cleanup':
                _, _, a, b, left = step
                (ra, ca), (rb, cb) = before[a], before[b]
                rows, coeff = hm.product(ra, ca, rb, cb, left)         # (the product itself is checked under mul_into)
                assert_op_equal(*got, *onp.symplectic_cleanup(U(rows), coeff, 1e-15))
            elif kind == 'rotate' and step[4] >= 0 and hm.distinct(before[step[2]][0]):
                # Clifford angles on duplicate-free rows: the reference's own arithmetic, exact
                _, _, src, q, k, _, _ = step
                er, ec = onp.rotate_by_single_pword(U(before[src][0]), before[src][1], U(q[None, :])[0], k * np.pi / 2)
                if not hm.commutes(before[src][0], q[None, :]).all():
                    assert_op_equal(*got, er, ec)
                    checked['rotate'] += 1
            elif kind == 'chain':
                _, s, qs, ks = step
                er, ec = onp.perform_rotations(U(before[s][0]), before[s][1], [(U(q[None, :])[0], int(k) * np.pi / 2) for q, k in zip(qs, ks)])
                assert_op_equal(*got, er, ec)
                checked['chain'] += 1
            for s in touched:
                slot = model.slots[s]
                rows, coeff = slot.live()
                assert 2 <= slot.T <= hm.MAX_T and slot.T <= slot.cap and not np.any(coeff == 0), (seed, n, kind)
                assert hm.span(coeff) <= 2 * hm.SPAN_LIMIT + 12, (seed, n, kind, hm.span(coeff))     # a product of two slots and a sum of up to 2^12 terms
                assert not slot.distinct_known or slot.distinct(), (seed, n, kind)
                assert np.array_equal(hm.y_count(rows), onp.y_count(U(rows)))
            other = model.slots[(step[1] + 1) % seq.n_slots]
            if other is not None:
                assert np.array_equal(hm.commutes(other.live()[0], dst.live()[0]), onp.commutes_termwise(U(other.live()[0]), U(dst.live()[0])))
    print(checked)
    assert all(v >= 10 for v in checked.values()), checked


def test_the_models_rotation_is_the_reference_rotation_at_a_true_angle():
    """The model rotates with cos and sin as plain factors (the sequences pass dyadic ones through the C ABI, so that every later
    comparison stays exact).  Here, once: with cos(t), sin(t) of a true angle it is onp.rotate_by_single_pword within 1e-12, on clean
    operands with a planted P / P Q pair and on operands with duplicate rows."""
    t = 0.37
    for seed, n in ((0, 70), (1, 130), (2, 20)):
        rng = np.random.default_rng(seed)
        symp = rng.random((80, 2 * n)) < 0.3
        symp[0, 0] = True
        coeff = rng.standard_normal(80) + 1j * rng.standard_normal(80)
        rows = hm.pack(symp)
        a, b = next((a, b) for a in range(10, 40) for b in range(a + 1, 40) if not hm.commutes(rows[a:a + 1], rows[b:b + 1])[0, 0])
        q = rows[a] ^ rows[b]                                          # rows a and b are a P / P Q pair, kept by both operands below
        for dup in (False, True):
            if dup:
                symp[50:60] = symp[:10]
            else:
                symp, coeff = onp.cleanup_op(symp, coeff)
                assert symp.shape[0] == 80
            rows = hm.pack(symp)
            r, c, all_commute = hm.rotate(rows, coeff, q, -1, float(np.cos(t)), float(np.sin(t)))
            q_bool = hm.unpack(q[None, :], n)
            er, ec = onp.rotate_by_single_pword(symp, coeff, q_bool[0], t)
            n_anti = int((~onp.commutes_termwise(symp, q_bool)).sum())
            assert not all_commute and er.shape[0] < onp.cleanup_op(symp, coeff)[0].shape[0] + n_anti       # something merged
            assert_op_equal(hm.unpack(r, n), c, er, ec, exact=False, tol=1e-12)
