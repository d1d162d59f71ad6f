"""A host model of a device operator handle, and a seeded generator of call sequences on a few handles (no GPU import).

tests/test_handle_model.py checks the model against oracle.oracle_np and the generator's promises on the CPU; tests/test_gpu_handle_state.py
replays the sequences on real handles and compares every observation with the model.

The model of a handle (`Slot`): packed rows uint64[cap, 2 Wq], coefficients complex128[cap], the term count T, a LOWER BOUND `cap` of the
handle's capacity (a result's capacity depends on the path that made it; it is never below its term count), `written` (rows beyond it
were never written and hold nothing defined, so set_rows never uncovers them; rows in [T, written) keep what was written there and
come back when set_rows grows T again), and `distinct_known`: the
model's rule for when the library PROMISES to know that no two rows are equal (symgpu_op_s::dup_free).  The library is ALLOWED to claim
it whenever rows [0, T) really are pairwise distinct (`Slot.distinct()`, read off the mirror): a non-Clifford rotation marks its input as a
side effect, which the model does not predict.

  distinct_known is set by    cleanup, product + cleanup, a run of Clifford rotations, a non-Clifford rotation (its result)
  is copied by                clone, a Clifford rotation (its result)
  survives                    set_coeff, scale
  is dropped by               every writer of rows: write, copy_rows, set_rows to another T, an all-pairs product into the handle
  is not given to             fresh rows, gather, concat, slice

All coefficients are Gaussian dyadics of a bounded width (`span`), so every product and sum below is exact in double precision and the
device must agree bit for bit; the generator renews a slot's coefficients (a set_coeff step) before they could outgrow that.

The hazards the generator is biased towards, counted per sequence in `Sequence.hazards`:
  overwrite_same_T     a write or a row copy wholly inside [0, T): the row count cannot give a stale cache away
  duplicate_row        a write that leaves two equal rows in the slot
  partner_generator    a rotation by Q = the XOR of two present rows that anticommute (a P / P Q pair: the join must merge them)
  mutator_after_warm   a mutator on the slot that the previous step touched, i.e. whose caches the observers have just warmed
Every sequence opens with a scripted prologue that holds each of them once, whatever the seed draws afterwards."""
import numpy as np

THR = 1e-15
CAP = 320              # capacity of a fresh slot
MAX_T = 300            # no slot grows beyond this
SPAN_LIMIT = 16        # bits between the highest and the lowest set bit of a slot's coefficients: a product of two slots, the sums of a cleanup
                       # and one more factor of 4 bits (the product observer of the GPU test) stay within the 53 bits of a double
HAZARDS = ('overwrite_same_T', 'duplicate_row', 'partner_generator', 'mutator_after_warm')
ROW_MUTATORS = ('fresh', 'write', 'copy_rows', 'set_rows', 'mul_into')
COEFF_MUTATORS = ('set_coeff', 'scale')


# ---- packed rows ----------------------------------------------------------------------------------------------------------------------
def words(n):
    return max(1, (n + 63) // 64)


def pack(symp):
    """bool[T, 2n] -> uint64[T, 2 Wq]: X words then Z words, bit j of word w = qubit 64 w + j."""
    symp = np.asarray(symp, dtype=bool)
    t, n = symp.shape[0], symp.shape[1] // 2
    wq = words(n)
    bits = np.zeros((t, 2, wq * 64), dtype=np.uint8)
    bits[:, 0, :n], bits[:, 1, :n] = symp[:, :n], symp[:, n:]
    return np.ascontiguousarray(np.packbits(bits.reshape(t, -1), axis=1, bitorder='little')).view('<u8').reshape(t, 2 * wq)


def unpack(rows, n):
    rows = np.ascontiguousarray(rows, dtype='<u8')
    t, wq = rows.shape[0], rows.shape[1] // 2
    bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder='little').reshape(t, 2, wq * 64)
    return np.hstack([bits[:, 0, :n], bits[:, 1, :n]]).astype(bool)


def weight(a):
    """Set bits along the last axis of a uint64 array."""
    a = np.ascontiguousarray(a, dtype='<u8')
    return np.unpackbits(a.view(np.uint8), axis=-1).sum(axis=-1, dtype=np.int64)


def y_count(rows):
    wq = rows.shape[1] // 2
    return weight(rows[:, :wq] & rows[:, wq:])


def commutes(a, b):
    """bool[N, M]: row i of a commutes with row j of b."""
    wq = a.shape[1] // 2
    xa, za, xb, zb = a[:, None, :wq], a[:, None, wq:], b[None, :, :wq], b[None, :, wq:]
    return weight((xa & zb) ^ (za & xb)) % 2 == 0


def times_i_pow(c, e):
    """c * i^e as component swaps (exact, as the kernels apply it)."""
    c = np.asarray(c, dtype=np.complex128)
    e = np.broadcast_to(np.asarray(e, dtype=np.int64) & 3, c.shape)
    out = np.empty(c.shape, dtype=np.complex128)
    out.real = np.choose(e, [c.real, -c.imag, -c.real, c.imag])
    out.imag = np.choose(e, [c.imag, c.real, -c.imag, -c.real])
    return out


def phase_exponent(left, right):
    """e of left[i] * right[i] = i^e (left ^ right) for the Y-counting convention of the packed rows."""
    wq = left.shape[-1] // 2
    out = left ^ right
    return (3 * (weight(left[..., :wq] & left[..., wq:]) + weight(right[..., :wq] & right[..., wq:])) + weight(out[..., :wq] & out[..., wq:])
            + 2 * weight(left[..., :wq] & right[..., wq:])) % 4


def product(inner, ci, outer, co, inner_is_left=True):
    """symgpu_mul_allpairs_dev: row o * Ni + i = inner[i] ^ outer[o], no cleanup."""
    ni, no = inner.shape[0], outer.shape[0]
    a = np.broadcast_to(inner[None, :, :], (no, ni, inner.shape[1]))
    b = np.broadcast_to(outer[:, None, :], (no, ni, inner.shape[1]))
    e = phase_exponent(a, b) if inner_is_left else phase_exponent(b, a)
    coeff = times_i_pow(ci[None, :] * co[:, None], e)
    return (a ^ b).reshape(no * ni, -1), coeff.reshape(-1)


def cleanup(rows, coeff, thr=THR):
    """Equal rows merged at their first occurrence, coefficients added in input order, |c| > thr kept."""
    index, first, sums = {}, [], []
    for t in range(rows.shape[0]):
        key = rows[t].tobytes()
        k = index.setdefault(key, len(first))
        if k == len(first):
            first.append(t)
            sums.append(0j)
        sums[k] = sums[k] + coeff[t]
    sums = np.array(sums, dtype=np.complex128).reshape(-1)
    keep = np.abs(sums) > thr
    return rows[np.array(first, dtype=np.int64)[keep]].reshape(-1, rows.shape[1]), sums[keep]


def rotate(rows, coeff, q, k, cos_t=0.0, sin_t=0.0, thr=THR):
    """symgpu_rotate_single_dev -> (rows, coeff, all_commute).  k < 0: cleanup([commuting, cos P, -i sin P Q]); k = 0 .. 3: [rotated
    anticommuting rows, commuting rows], odd k: P Q (-i) with equal rows merged, k in {2, 3}: negated."""
    anti = ~commutes(rows, q[None, :])[:, 0]
    if not anti.any():
        return rows, coeff, True
    pq = rows[anti] ^ q
    pq_c = times_i_pow(coeff[anti], phase_exponent(rows[anti], np.broadcast_to(q, pq.shape)) + 3)      # P Q (-i)
    if k < 0:
        r, c = cleanup(np.vstack([rows[~anti], rows[anti], pq]), np.hstack([coeff[~anti], cos_t * coeff[anti], sin_t * pq_c]), thr)
        return r, c, False
    rot, rot_c = cleanup(pq, pq_c, thr) if k & 1 else (rows[anti], coeff[anti])
    return np.vstack([rot, rows[~anti]]), np.hstack([-rot_c if k in (2, 3) else rot_c, coeff[~anti]]), False


def span(coeff):
    """Bits from the highest to the lowest set bit over all components of `coeff` on one fixed-point scale (0 for all-zero)."""
    v = np.abs(np.concatenate([np.real(coeff), np.imag(coeff)]))
    v = v[v != 0]
    if v.size == 0:
        return 0
    m, e = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = e - 53 + (np.frexp((mi & -mi).astype(np.float64))[1] - 1)
    return int(e.max() - low.min())


def _in_budget(coeff):
    """The generator's rule for exact arithmetic: at most SPAN_LIMIT bits wide, every non-zero component in [2^-24, 2^24]."""
    v = np.abs(np.concatenate([np.real(coeff), np.imag(coeff)]))
    v = v[v != 0]
    return span(coeff) <= SPAN_LIMIT and (v.size == 0 or (v.min() >= 2.0 ** -24 and v.max() <= 2.0 ** 24))


def distinct(rows):
    return len({r.tobytes() for r in rows}) == rows.shape[0]


# ---- the model of a handle ------------------------------------------------------------------------------------------------------------
class Slot:
    def __init__(self, rows, coeff, cap=None, distinct_known=False):
        t = rows.shape[0]
        self.cap = max(1, t) if cap is None else cap
        self.rows = np.zeros((max(self.cap, t), rows.shape[1]), dtype='<u8')
        self.coeff = np.zeros(max(self.cap, t), dtype=np.complex128)
        self.rows[:t], self.coeff[:t] = rows, coeff
        self.T = t
        self.written = t                 # rows [0, written) hold defined data on the device: set_rows may go up to here, never further
        self.distinct_known = distinct_known

    def live(self):
        return self.rows[:self.T], self.coeff[:self.T]

    def distinct(self):
        return distinct(self.rows[:self.T])


class Model:
    """The slots of one sequence; `apply(step)` performs a step on the mirrors and returns the slots it touched (to be observed)."""

    def __init__(self, n_slots):
        self.slots = [None] * n_slots

    def apply(self, step):
        kind, S = step[0], self.slots
        if kind == 'fresh':
            _, s, rows, coeff = step
            S[s] = Slot(rows, coeff, cap=CAP)
            return [s]
        if kind == 'write':
            _, s, at, rows, coeff = step
            k = rows.shape[0]
            assert at + k <= S[s].cap
            S[s].rows[at:at + k], S[s].coeff[at:at + k] = rows, coeff
            S[s].T = max(S[s].T, at + k)
            S[s].written = max(S[s].written, S[s].T)
            S[s].distinct_known = False
            return [s]
        if kind == 'copy_rows':
            _, s, at, src, begin, k = step
            assert s != src and begin + k <= S[src].T and at + k <= S[s].cap
            S[s].rows[at:at + k], S[s].coeff[at:at + k] = S[src].rows[begin:begin + k], S[src].coeff[begin:begin + k]
            S[s].T = max(S[s].T, at + k)
            S[s].written = max(S[s].written, S[s].T)
            S[s].distinct_known = False
            return [s]
        if kind == 'set_rows':
            _, s, t = step
            assert t <= S[s].written and t != S[s].T
            S[s].T = t
            S[s].distinct_known = False
            return [s]
        if kind == 'set_coeff':
            _, s, coeff = step
            S[s].coeff[:S[s].T] = coeff
            return [s]
        if kind == 'scale':
            _, s, const, conj = step
            c = S[s].coeff[:S[s].T]
            S[s].coeff[:S[s].T] = (c.conj() if conj else c) * const
            return [s]
        if kind == 'mul_into':
            _, s, inner, outer, o0, o1, left = step
            assert s not in (inner, outer)
            (ri, ci), (ro, co) = S[inner].live(), S[outer].live()
            rows, coeff = product(ri, ci, ro[o0:o1], co[o0:o1], left)
            assert rows.shape[0] <= S[s].cap
            S[s].rows[:rows.shape[0]], S[s].coeff[:rows.shape[0]] = rows, coeff
            S[s].T = rows.shape[0]
            S[s].written = max(S[s].written, S[s].T)
            S[s].distinct_known = False
            return [s]
        if kind == 'clone':
            _, dst, src = step
            S[dst] = Slot(*S[src].live(), distinct_known=S[src].distinct_known)
            return [dst]
        if kind == 'gather':
            _, dst, src, idx = step
            r, c = S[src].live()
            S[dst] = Slot(r[idx], c[idx])
            return [dst]
        if kind == 'concat':
            _, dst, a, b = step
            (ra, ca), (rb, cb) = S[a].live(), S[b].live()
            S[dst] = Slot(np.vstack([ra, rb]), np.hstack([ca, cb]))
            return [dst]
        if kind == 'slice':
            _, dst, src, begin, end = step
            r, c = S[src].live()
            S[dst] = Slot(r[begin:end], c[begin:end])
            return [dst]
        if kind == 'cleanup':
            _, dst, src = step
            S[dst] = Slot(*cleanup(*S[src].live()), distinct_known=True)
            return [dst]
        if kind == 'mul_cleanup':
            _, dst, a, b, left = step
            (ra, ca), (rb, cb) = S[a].live(), S[b].live()
            S[dst] = Slot(*cleanup(*product(ra, ca, rb, cb, left)), distinct_known=True)
            return [dst]
        if kind == 'rotate':
            _, dst, src, q, k, cos_t, sin_t = step
            r, c, all_commute = rotate(*S[src].live(), q, k, cos_t, sin_t)
            if all_commute:
                return [src]
            known = True if k < 0 else S[src].distinct_known
            S[dst] = Slot(r, c, distinct_known=known)
            return [dst] if dst == src else [dst, src]
        if kind == 'chain':
            _, s, qs, ks = step
            assert S[s].distinct_known
            r, c = S[s].live()
            for q, k in zip(qs, ks):
                r, c, _ = rotate(r, c, q, int(k))
                r, c = cleanup(r, c)
            S[s] = Slot(r, c, distinct_known=True)
            return [s]
        raise KeyError(kind)

    def all_commute(self, step):
        """Does the model expect the rotation `step` to report that every row commutes (no result handle)?"""
        _, _, src, q, _, _, _ = step
        return bool(commutes(self.slots[src].live()[0], q[None, :]).all())


# ---- the generator --------------------------------------------------------------------------------------------------------------------
class Sequence:
    def __init__(self, seed, n, n_slots, steps, hazards, probe_rows, probe_coeff):
        self.seed, self.n, self.n_slots, self.steps, self.hazards = seed, n, n_slots, steps, hazards
        self.probe_rows, self.probe_coeff = probe_rows, probe_coeff          # the fixed outer operand of the product observer


def _dyadic(rng, t):
    """Gaussian dyadics k / 16, neither component zero (so no coefficient is zero and conjugation always shows)."""
    pick = lambda: rng.choice(np.concatenate([np.arange(-8, 0), np.arange(1, 9)]), t)
    return (pick() + 1j * pick()) / 16.0


def _random_rows(rng, t, n):
    rows = rng.random((t, 2 * n)) < 0.3
    rows[:, 0] |= ~rows.any(axis=1)                                          # never the identity
    return pack(rows)


def _partner_generator(rng, rows):
    """Q = rows[a] ^ rows[b] for an anticommuting pair a != b (then rows[a] anticommutes with Q and rows[a] ^ Q = rows[b] is present);
    None if no two rows anticommute."""
    t = rows.shape[0]
    for _ in range(40):
        a, b = rng.choice(t, 2, replace=False)
        if not commutes(rows[a:a + 1], rows[b:b + 1])[0, 0]:
            return rows[a] ^ rows[b]
    return None


def generate(seed, n, n_steps=30):
    """The sequence of `seed` on n qubits: the initial fresh slots, the scripted prologue, then `n_steps` drawn steps (a renewal of
    coefficients that the span rule forces counts as a step).  Deterministic in (seed, n, n_steps)."""
    rng = np.random.default_rng([seed, n])
    n_slots = 3 + seed % 2
    model, steps, hazards = Model(n_slots), [], dict.fromkeys(HAZARDS, 0)
    last = [None]                                                            # the slots the previous step touched

    def emit(step):
        kind = step[0]
        s = step[1]
        if kind in ROW_MUTATORS + COEFF_MUTATORS and last[0] is not None and s in last[0]:
            hazards['mutator_after_warm'] += 1
        if kind in ('write', 'copy_rows'):
            at, k = step[2], (step[3].shape[0] if kind == 'write' else step[5])
            if at + k <= model.slots[s].T:
                hazards['overwrite_same_T'] += 1
        if kind == 'rotate' and step[-1] == 'partner':
            hazards['partner_generator'] += 1
            step = step[:-1]
        elif kind == 'rotate':
            step = step[:-1]
        last[0] = model.apply(step)
        if kind == 'write':
            live = [r.tobytes() for r in model.slots[s].live()[0]]
            if any(live.count(live[t]) > 1 for t in range(step[2], step[2] + step[3].shape[0])):
                hazards['duplicate_row'] += 1
        steps.append(step)

    for s in range(n_slots):
        t = int(rng.integers(60, 76 if s == 0 else 151))                     # slot 0 is rotated twice in the prologue: at most 4 x 75 rows
        emit(('fresh', s, _random_rows(rng, t, n), _dyadic(rng, t)))
    # the prologue: a non-Clifford rotation of slot 0 by a partner generator into slot 1 (slot 0 is now marked duplicate free as a side
    # effect), a copy of row 0 over row 1 of slot 0, an odd Clifford rotation of it (which must merge), an overwrite of the result of the
    # first rotation (handed-on hashes) with T unchanged and a rotation of that
    q = _partner_generator(rng, model.slots[0].live()[0])
    assert q is not None
    emit(('rotate', 1, 0, q, -1, 0.5, 0.75, 'partner'))
    r0, c0 = model.slots[0].live()
    emit(('write', 0, 1, r0[0:1].copy(), _dyadic(rng, 1)))
    emit(('rotate', 0, 0, q, 1, 0.0, 0.0, 'plain'))
    t1 = model.slots[1].T
    emit(('write', 1, 0, _random_rows(rng, t1, n), _dyadic(rng, t1)))
    q1 = _partner_generator(rng, model.slots[1].live()[0])
    emit(('rotate', 1, 1, q1 if q1 is not None else q, -1, 0.75, 0.5, 'partner' if q1 is not None else 'plain'))

    def draw():
        """One candidate step (or None if this draw does not fit the state)."""
        S = model.slots
        s = int(rng.integers(n_slots))
        if last[0] is not None and rng.random() < 0.5:
            s = last[0][0]
        other = [o for o in range(n_slots) if o != s]
        o = int(rng.choice(other))
        T, cap = S[s].T, S[s].cap
        kind = rng.choice(['write_all', 'write_two', 'write_grow', 'write_dup', 'copy_rows', 'set_rows', 'set_coeff', 'scale', 'mul_into', 'fresh',
                           'clone', 'gather', 'concat', 'slice', 'cleanup', 'rotate', 'rotate', 'rotate', 'chain', 'chain', 'mul_cleanup', 'mul_cleanup', 'mul_into'])
        if kind == 'write_all':
            return ('write', s, 0, _random_rows(rng, T, n), _dyadic(rng, T))
        if kind == 'write_two' and T >= 4:
            return ('write', s, T // 2, _random_rows(rng, 2, n), _dyadic(rng, 2))
        if kind == 'write_grow' and cap >= T + 3 and T + 3 <= MAX_T:
            return ('write', s, T - 1, _random_rows(rng, 4, n), _dyadic(rng, 4))
        if kind == 'write_dup' and T >= 4:
            i, j = rng.choice(T, 2, replace=False)
            return ('write', s, int(i), S[s].rows[j:j + 1].copy(), _dyadic(rng, 1))
        if kind == 'copy_rows':
            k = int(rng.integers(1, min(S[o].T, T) + 1))
            return ('copy_rows', s, int(rng.integers(0, T - k + 1)), o, int(rng.integers(0, S[o].T - k + 1)), k)
        if kind == 'set_rows':
            t = int(rng.integers(2, min(S[s].written, MAX_T) + 1))
            return ('set_rows', s, t) if t != T else None
        if kind == 'set_coeff':
            return ('set_coeff', s, _dyadic(rng, T))
        if kind == 'scale':
            return ('scale', s, complex(rng.choice([2.0, -0.5, 0.5j, 1 + 1j, -1j])), bool(rng.integers(2)))
        if kind == 'mul_into':
            inner, outer = (o, other[-1] if other[-1] != o else other[0]) if len(other) > 1 else (o, o)
            ni, no = S[inner].T, S[outer].T
            if ni > min(cap, MAX_T) or span(S[inner].live()[1]) + span(S[outer].live()[1]) > 2 * SPAN_LIMIT:
                return None
            width = int(rng.integers(1, min(no, min(cap, MAX_T) // ni) + 1))
            o0 = int(rng.integers(0, no - width + 1))
            return ('mul_into', s, inner, outer, o0, o0 + width, bool(rng.integers(2)))
        if kind == 'fresh':
            t = int(rng.integers(60, 151))
            return ('fresh', s, _random_rows(rng, t, n), _dyadic(rng, t))
        if kind == 'clone':
            return ('clone', s, o)
        if kind == 'gather':
            k = int(rng.integers(5, 41))
            return ('gather', s, o, rng.integers(0, S[o].T, k).astype(np.int64))             # repeats allowed
        if kind == 'concat':
            a = int(rng.choice(other + [s]))
            return ('concat', s, a, o) if S[a].T + S[o].T <= MAX_T else None
        if kind == 'slice':
            length = int(rng.integers(2, min(S[o].T, 60) + 1))
            begin = int(rng.integers(0, S[o].T - length + 1))
            return ('slice', s, o, begin, begin + length)
        if kind == 'cleanup':
            return ('cleanup', s, int(rng.choice(other + [s])))
        if kind == 'rotate':
            src = int(rng.choice(other + [s, s]))
            k = int(rng.choice([-1, -1, -1, 0, 1, 1, 2, 3]))
            if k < 0 and S[src].T > MAX_T // 2:
                k = 1
            q = _partner_generator(rng, S[src].live()[0]) if rng.random() < 0.6 else None
            tag = 'partner' if q is not None else 'plain'
            if q is None:
                q = _random_rows(rng, 1, n)[0]
            cos_t, sin_t = ((0.5, 0.75) if rng.integers(2) else (0.75, -0.5)) if k < 0 else (0.0, 0.0)
            return ('rotate', s, src, q, k, cos_t, sin_t, tag)
        if kind == 'chain' and S[s].distinct_known:
            K = int(rng.integers(1, 4))
            return ('chain', s, _random_rows(rng, K, n), rng.integers(0, 4, K).astype(np.int32))
        if kind == 'mul_cleanup':
            a = int(rng.choice(other + [s]))
            if S[a].T * S[o].T > 4 * MAX_T or span(S[a].live()[1]) + span(S[o].live()[1]) > 2 * SPAN_LIMIT:
                return None
            return ('mul_cleanup', s, a, o, bool(rng.integers(2)))
        return None

    def fits(step):
        """Would the step leave its slot with 2 .. MAX_T rows?  (Tried on a copy of the slots it replaces.)"""
        trial = Model(n_slots)
        trial.slots = list(model.slots)
        kind = step[0]
        if kind in ('write', 'copy_rows', 'set_rows', 'set_coeff', 'scale', 'mul_into'):
            return True                                                      # sized when drawn
        trial.apply(step[:-1] if kind == 'rotate' else step)
        return 2 <= trial.slots[step[1]].T <= MAX_T

    drawn = 0
    while drawn < n_steps:
        wide = [s for s in range(n_slots) if not _in_budget(model.slots[s].live()[1])]
        if wide:
            emit(('set_coeff', wide[0], _dyadic(rng, model.slots[wide[0]].T)))
            drawn += 1
            continue
        step = draw()
        if step is None or not fits(step):
            continue
        emit(step)
        drawn += 1
    return Sequence(seed, n, n_slots, steps, hazards, _random_rows(rng, 3, n), _dyadic(rng, 3))


GPU_SEEDS = tuple(range(20))
GPU_SIZES = (70, 130)
