"""Operands for a run of Clifford rotations (symgpu_rotate_clifford_chain_dev) whose answers are known WITHOUT the popcount formula the
kernels use (plain NumPy, seeded; neither the oracle nor the library is called here — tests/test_rotation_families.py proves the expected
answers against oracle_np on the CPU, tests/test_gpu_rotation_families.py runs the families through every form of the run).

One Clifford rotation of a clean operator (no duplicate rows, every |c| above the threshold) by k pi/2 about the Pauli Q
(reference: PauliwordOp._rotate_by_single_Pword, base.py:1139-1154, followed by cleanup()):
    rows that anticommute with Q:  odd k: P -> P Q with coefficient c * i^e * (-i), where P Q = i^e (P xor Q);  k in {2, 3}: c -> -c
    then the stable partition  [anticommuting rows | commuting rows]; nothing at all if every row commutes.
`table_step` forms e and the anticommutation parity QUBIT BY QUBIT from the 4 x 4 multiplication table of the single-qubit Paulis, with
integer arithmetic on the exponent; `packed_step` does the same on uint64 words through bit masks of the six ordered pairs of different
Paulis (for the sizes at which a [T, n] array of Pauli codes is too slow) and is proven against `table_step` on the CPU.

Notation.  Pauli codes: I = 0, X = 1, Z = 2, Y = 3 (code = x + 2 z).  Packed rows as symmer_amd/packing.py: uint64[T, 2 Wq], X words then Z
words, qubit 64 w + j at bit j of word w, Wq = max(1, ceil(n / 64)).  The chain kernels hold a row as WQ 16-byte chunks, one per lane:
chunk c < WQ / 2 is the X half of qubits [128 c, 128 c + 128), chunk c + WQ / 2 their Z half — a "128-qubit block" below."""
import collections

import numpy as np

I_, X_, Z_, Y_ = 0, 1, 2, 3
# PROD[p][q] = the Pauli of P Q, EXP[p][q] = the power of i in front of it: X Y = i Z, Y Z = i X, Z X = i Y and the reverses -i
PROD = np.array([[I_, X_, Z_, Y_],
                 [X_, I_, Y_, Z_],
                 [Z_, Y_, I_, X_],
                 [Y_, Z_, X_, I_]], dtype=np.uint8)
EXP = np.array([[0, 0, 0, 0],
                [0, 0, 3, 1],      # X X, X Z = -i Y, X Y = i Z
                [0, 1, 0, 3],      # Z X = i Y, Z Y = -i X
                [0, 3, 1, 0]],     # Y X = -i Z, Y Z = i X
               dtype=np.int64)
ANTI = (EXP != 0)

Case = collections.namedtuple('Case', 'name n rows coeff qs ks exp_rows exp_coeff')


def wq_of(n):
    return max(1, (n + 63) // 64)


# ---------------------------------------------------------------- layouts -------------------------------------------------------------------
def codes_to_packed(codes):
    """uint8[T, n] Pauli codes -> uint64[T, 2 Wq]."""
    codes = np.asarray(codes, dtype=np.uint8)
    T, n = codes.shape
    wq = wq_of(n)
    out = np.zeros((T, 2 * wq), dtype='<u8')
    for half, bit in ((0, 1), (1, 2)):
        bits = np.zeros((T, 64 * wq), dtype=np.uint8)
        bits[:, :n] = (codes & bit) != 0
        out[:, half * wq:(half + 1) * wq] = np.packbits(bits, axis=1, bitorder='little').view('<u8')
    return out


def packed_to_codes(rows, n):
    rows = np.ascontiguousarray(rows, dtype='<u8')
    wq = rows.shape[1] // 2
    bits = [np.unpackbits(np.ascontiguousarray(rows[:, h * wq:(h + 1) * wq]).view(np.uint8), axis=1, bitorder='little')[:, :n] for h in (0, 1)]
    return (bits[0] + 2 * bits[1]).astype(np.uint8)


def packed_to_symp(rows, n):
    """uint64[T, 2 Wq] -> bool[T, 2n] (the reference's layout)."""
    c = packed_to_codes(rows, n)
    return np.hstack([(c & 1) != 0, (c & 2) != 0])


def mul_i(coeff, e):
    """coeff * i^e, exact: swaps and sign changes only (e: int array)."""
    coeff = np.asarray(coeff, dtype=complex)
    e = np.asarray(e) & 3
    re, im = coeff.real, coeff.imag
    ore = np.where(e == 0, re, np.where(e == 1, -im, np.where(e == 2, -re, im)))
    oim = np.where(e == 0, im, np.where(e == 1, re, np.where(e == 2, -im, -re)))
    return ore + 1j * oim


def _partition(anti):
    return np.concatenate([np.flatnonzero(anti), np.flatnonzero(~anti)])


# ---------------------------------------------------------------- one step, from the table ------------------------------------------------
def table_step(rows, coeff, q, k, n):
    """One rotation of packed rows from the multiplication table, qubit by qubit -> (rows, coeff, number of anticommuting rows)."""
    codes = packed_to_codes(rows, n)
    qc = packed_to_codes(np.asarray(q, dtype='<u8').reshape(1, -1), n)[0]
    anti = np.zeros(codes.shape[0], dtype=np.int64)
    e = np.zeros(codes.shape[0], dtype=np.int64)
    for j in np.flatnonzero(qc):                                  # I on the other qubits: product P, exponent 0, commutes
        anti += ANTI[codes[:, j], qc[j]]
        e += EXP[codes[:, j], qc[j]]
    anti = (anti & 1) == 1
    if not anti.any():
        return rows, coeff, 0
    coeff = np.asarray(coeff, dtype=complex).copy()
    if k & 1:
        codes[anti] = PROD[codes[anti], qc[None, :]]
        coeff[anti] = mul_i(coeff[anti], e[anti] + 3)                # i^e * (-i)
    if k in (2, 3):
        coeff[anti] = mul_i(coeff[anti], 2)
    order = _partition(anti)
    return codes_to_packed(codes)[order], coeff[order], int(anti.sum())


# ---------------------------------------------------------------- one step, on packed words -----------------------------------------------
if hasattr(np, 'bitwise_count'):
    def _popcount(words):
        return np.bitwise_count(words).astype(np.int64)
else:
    _POP8 = np.array([bin(i).count('1') for i in range(256)], dtype=np.uint8)

    def _popcount(words):
        return _POP8[np.ascontiguousarray(words).view(np.uint8).reshape(-1, 8)].sum(axis=1, dtype=np.int64)


_UNITS = np.array([1, 1j, -1, -1j])


def packed_step(rows, coeff, q, k, n=None):
    """The same step on uint64 words: masks of the qubits whose ordered pair (P_j, Q_j) multiplies to +i (X Y, Y Z, Z X) and to -i."""
    rows = np.ascontiguousarray(rows, dtype='<u8')
    q = np.asarray(q, dtype='<u8').reshape(-1)
    wq = rows.shape[1] // 2
    cols = np.flatnonzero(q[:wq] | q[wq:])                            # the words in which Q is not I: the others contribute nothing
    n_plus, n_minus = np.zeros(rows.shape[0], dtype=np.int64), np.zeros(rows.shape[0], dtype=np.int64)
    for c in cols:
        x, z = np.ascontiguousarray(rows[:, c]), np.ascontiguousarray(rows[:, wq + c])
        q_x, q_z, q_y = q[c] & ~q[wq + c], q[wq + c] & ~q[c], q[c] & q[wq + c]     # where Q is X, Z, Y
        p_x, p_z, p_y = x & ~z, z & ~x, x & z                                         # where the row is X, Z, Y
        n_plus += _popcount((p_x & q_y) | (p_y & q_z) | (p_z & q_x))
        n_minus += _popcount((p_y & q_x) | (p_z & q_y) | (p_x & q_z))
    anti = ((n_plus + n_minus) & 1) == 1
    if not anti.any():
        return rows, coeff, 0
    e = np.zeros(rows.shape[0], dtype=np.int64)
    if k & 1:
        rows = rows.copy()
        mask = np.where(anti, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0))
        for c in np.concatenate([cols, wq + cols]):
            rows[:, c] ^= mask & q[c]
        e = n_plus + 3 * n_minus + 3                                   # i^e * (-i)
    if k in (2, 3):
        e = e + 2
    coeff = np.asarray(coeff, dtype=complex) * _UNITS[np.where(anti, e & 3, 0)]     # exact: a factor 1, i, -1 or -i
    order = _partition(anti)
    return np.take(rows, order, axis=0), np.take(coeff, order), int(anti.sum())


def run(rows, coeff, qs, ks, n, step=table_step):
    """A whole run -> (rows, coeff, [anticommuting rows of every step])."""
    counts = []
    for q, k in zip(qs, ks):
        rows, coeff, a = step(rows, coeff, q, int(k), n)
        counts.append(a)
    return rows, coeff, counts


# ---------------------------------------------------------------- building blocks ---------------------------------------------------------
def dyadic(rng, t):
    """Coefficients (a + i b) / 16 with integers |a|, |b| <= 8, never 0: every product with a power of i and every sign change is exact."""
    re, im = rng.integers(-8, 9, t), rng.integers(-8, 9, t)
    re = np.where((re == 0) & (im == 0), 1, re)
    return (re + 1j * im) / 16.0


def _mask_words(n):
    """uint64[Wq]: the bits of the qubits that exist."""
    wq = wq_of(n)
    m = np.full(wq, 0xFFFFFFFFFFFFFFFF, dtype='<u8')
    if n % 64:
        m[-1] = np.uint64((1 << (n % 64)) - 1)
    return m


def _set_pauli(rows, idx, qubit, code):
    """Pauli `code` (scalar or one per row of idx) on `qubit` of the packed rows idx."""
    wq = rows.shape[1] // 2
    w, b = qubit // 64, np.uint64(qubit % 64)
    code = np.broadcast_to(np.asarray(code, dtype=np.uint64), np.shape(idx))
    one = np.uint64(1)
    for half, bit in ((0, 1), (1, 2)):
        col = rows[idx, half * wq + w]
        col = (col & ~(one << b)) | (((code >> np.uint64(bit >> 1)) & one) << b)
        rows[idx, half * wq + w] = col


def distinct_rows(n, T, rng, reserve=1, density_half=True, z_only=False):
    """uint64[T, 2 Wq]: random rows at density 0.5 on qubits [0, n - reserve) — X and Z, or Z alone — made distinct by the row index, which
    is written (multiplied by an odd constant: a bijection of m-bit numbers) over the Z bits of the first m = min(n - reserve, 32) qubits.
    The last `reserve` qubits are left I for the family."""
    wq = wq_of(n)
    m = min(n - reserve, 32)
    assert m >= 1 and T <= (1 << m), f'{T} distinct rows need more than the {m} index qubits of n = {n}'
    rows = np.frombuffer(rng.bytes(T * 2 * wq * 8), dtype='<u8').reshape(T, 2 * wq).copy()
    live = _mask_words(n - reserve)
    full = np.zeros(wq, dtype='<u8')
    full[:live.shape[0]] = live
    rows[:, :wq] &= full[None, :]
    rows[:, wq:] &= full[None, :]
    if z_only:
        rows[:, :wq] = 0
    idx = (np.arange(T, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << m) - 1)
    rows[:, wq] = (rows[:, wq] & ~np.uint64((1 << m) - 1)) | idx
    return rows


def single_qubit_q(n, qubit, code):
    q = np.zeros((1, 2 * wq_of(n)), dtype='<u8')
    _set_pauli(q, np.array([0]), qubit, code)
    return q[0]


def is_clean(rows, coeff, thr=1e-15):
    """No duplicate rows and every |c| well above the threshold."""
    rows = np.ascontiguousarray(rows)
    keys = rows.view(np.dtype((np.void, rows.dtype.itemsize * rows.shape[1]))).ravel()
    return np.unique(keys).shape[0] == rows.shape[0] and bool((np.abs(coeff) > 1e6 * thr).all())


def _case(name, n, rows, coeff, qs, ks, step):
    qs = np.ascontiguousarray(qs, dtype='<u8')
    ks = np.asarray(ks, dtype=np.int32)
    beyond = ~np.concatenate([_mask_words(n), _mask_words(n)])
    assert not (rows & beyond).any() and not (qs & beyond).any(), f'{name}: a Pauli on a qubit that does not exist'
    er, ec, _ = run(rows, coeff, qs, ks, n, step)
    return Case(name, n, rows, coeff, qs, ks, er, ec)


# ---------------------------------------------------------------- last-qubit --------------------------------------------------------------
A_SETS = ('none', 'all', 'first', 'last', '1023mod1024', '0mod1024', 'every_other')


def index_set(name, T):
    t = np.arange(T)
    return {'none': t[:0], 'all': t, 'first': t[:1], 'last': t[-1:], '1023mod1024': t[t % 1024 == 1023], '0mod1024': t[t % 1024 == 0],
            'every_other': t[::2]}[name]


ANTICOMMUTING = {X_: (Z_, Y_), Z_: (X_, Y_), Y_: (X_, Z_)}


def last_qubit(n, T, a_set, q_pauli, ks, rng, step=table_step, cycle_q=False):
    """Q acts on qubit n - 1 alone.  The rows of the index set A carry one of the two Paulis that anticommute with it there (alternating),
    the others I or Q's own Pauli (alternating); the rest of every row is random and only makes the rows distinct.  So exactly the rows of
    A anticommute with Q — at EVERY step when all the rotations share Q (an odd k turns one anticommuting Pauli into the other), at the
    first step when cycle_q lets the Pauli of Q run through X, Y, Z."""
    rows = distinct_rows(n, T, rng)
    A = index_set(a_set, T)
    rest = np.setdiff1d(np.arange(T), A)
    a1, a2 = ANTICOMMUTING[q_pauli]
    _set_pauli(rows, A, n - 1, np.where(np.arange(A.shape[0]) % 2 == 0, a1, a2))
    _set_pauli(rows, rest, n - 1, np.where(np.arange(rest.shape[0]) % 2 == 0, I_, q_pauli))
    order = (X_, Y_, Z_)
    start = order.index(q_pauli)
    qs = np.stack([single_qubit_q(n, n - 1, order[(start + r) % 3] if cycle_q else q_pauli) for r in range(len(ks))])
    return _case(f'last_qubit n={n} T={T} A={a_set} Q={"IXZY"[q_pauli]}', n, rows, dyadic(rng, T), qs, ks, step), A


# ---------------------------------------------------------------- Y-ladder ----------------------------------------------------------------
def ladder_blocks(n):
    """The 128-qubit blocks that hold a Y of the ladder: those with at least the 56 qubits it uses."""
    return (n - 56) // 128 + 1


def y_ladder(n, T, rng, top=False, ks=(1, 3, 1, 2, 3, 1, 0, 1), step=table_step):
    """Row t holds t mod 8 Ys, rotation r is about a Q of r mod 8 Ys.  Y number j sits in 128-qubit block j mod (number of blocks of at least 56 qubits) — one
    per 16-byte chunk of the kernels' row where the row has 8 blocks, so the Y count mod 4 is right only if the sum over the lanes is —
    or, with `top`, all in the last block.  The Ys of a row and those of Q never share a qubit.  Q also carries Z on qubit 0, where the
    rows t with t mod 3 != 0 carry X: those anticommute with the first Q, and X Z = -i Y there is the only factor that is not 1, so the first
    odd step multiplies their coefficients by i^3 (-i) = -1.  Index bits: Z of qubits 1 .. 24.  n >= 64."""
    assert n >= 64 and T <= (1 << 24)
    wq = wq_of(n)
    nb = ladder_blocks(n)
    rows = np.zeros((T, 2 * wq), dtype='<u8')
    rows[:, wq] = ((np.arange(T, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << 24) - 1)) << np.uint64(1)
    t = np.arange(T)

    def block(j):
        return 128 * ((nb - 1) if top else (j % nb))

    for j in range(7):
        _set_pauli(rows, t[t % 8 > j], block(j) + 32 + j, Y_)
    _set_pauli(rows, t[t % 3 != 0], 0, X_)
    qs = np.zeros((len(ks), 2 * wq), dtype='<u8')
    for r in range(len(ks)):
        for j in range(r % 8):
            _set_pauli(qs, np.array([r]), block(j) + 48 + j, Y_)
        _set_pauli(qs, np.array([r]), 0, Z_)
    return _case(f'y_ladder n={n} T={T}{" top" if top else ""}', n, rows, dyadic(rng, T), qs, ks, step)


# ---------------------------------------------------------------- identity and all-commute steps ------------------------------------------
def commuting_steps(n, T, rng, with_action=True, step=table_step):
    """Z-type rows.  The run mixes Q = I, Z strings (both commute with every row: the step is the identity and must not re-order anything)
    and — with_action — X on the last qubit, which turns the rows that carry Z there into Y rows; the Z strings leave that qubit alone, so
    they still commute with everything afterwards."""
    wq = wq_of(n)
    rows = distinct_rows(n, T, rng, z_only=True)
    t = np.arange(T)
    _set_pauli(rows, t[t % 3 == 1], n - 1, Z_)
    zs = distinct_rows(n, 4, rng, z_only=True)
    ident = np.zeros(2 * wq, dtype='<u8')
    xl = single_qubit_q(n, n - 1, X_)
    if with_action:
        qs, ks = [zs[0], ident, xl, ident, zs[1], xl, zs[2], ident, xl], [1, 1, 1, 2, 3, 2, 0, 3, 3]
    else:
        qs, ks = [zs[0], ident, zs[1], ident, zs[2]], [1, 1, 3, 2, 2]
    return _case(f'commuting_steps n={n} T={T} action={with_action}', n, rows, dyadic(rng, T), np.stack(qs), ks, step)


# ---------------------------------------------------------------- long runs ---------------------------------------------------------------
LONG_K = (1, 8, 9, 10, 11, 32, 33, 39, 40, 41, 80, 81)


def long_run(n, T, K, rng, fourfold=False, q_words=None, step=table_step):
    """K rotations of random rows about random Qs (density 0.5).  The partition bit of rotation r goes to bit 22 + r of the register
    chain's key: K = 10 fills its lower word, 32 the first word of the packed ks, 40 a segment.  k cycles through 0 .. 3; with `fourfold`
    every Q is used four times running with k = 1 — a rotation by 2 pi, the identity on every row and coefficient — so after every
    fourth step the operator is the input up to the order of its rows.  q_words: every Q is I outside that many words, picked at random
    and always with the last word among them (large operands: the packed step then reads those words only)."""
    wq = wq_of(n)
    rows = distinct_rows(n, T, rng, reserve=0)
    n_q = (K + 3) // 4 if fourfold else K
    q = np.frombuffer(rng.bytes(n_q * 2 * wq * 8), dtype='<u8').reshape(n_q, 2 * wq).copy()
    q &= np.concatenate([_mask_words(n), _mask_words(n)])[None, :]
    if q_words is not None and q_words < wq:
        for r in range(n_q):
            keep = np.zeros(wq, dtype=bool)
            keep[rng.choice(wq - 1, q_words - 1, replace=False)] = True
            keep[wq - 1] = True
            q[r, :wq][~keep] = 0
            q[r, wq:][~keep] = 0
    if fourfold:
        qs, ks = np.repeat(q, 4, axis=0)[:K], np.ones(K, dtype=np.int32)
    else:
        qs, ks = q, np.arange(K, dtype=np.int32) % 4
    return _case(f'long_run n={n} T={T} K={K}{" fourfold" if fourfold else ""}', n, rows, dyadic(rng, T), qs, ks, step)


# ---------------------------------------------------------------- the plan, restated ------------------------------------------------------
FORMS = ('Registers', 'Lds', 'SingleWorkgroup', 'TwoLaunch', 'FourLaunch')
FORM_COUNTERS = ('CHAIN_REGISTERS', 'CHAIN_LDS', 'CHAIN_SINGLE_WORKGROUP', 'CHAIN_TWO_LAUNCHES', 'CHAIN_FOUR_LAUNCHES')   # the counter of each form


def header_constants(text):
    """The limits of rotate_common.h (and the register chain's index width of rotate_chain.hip) from the source text."""
    import re
    out = {}
    for name in ('CHAIN_TMAX', 'CHAIN_LOCAL_T', 'CHAIN_TWO_T', 'CHAIN_LDS_T', 'CHAIN_IDX_BITS', 'CHAIN_SEG'):
        m = re.search(r'constexpr\s+(?:int|i64)\s+' + name + r'\s*=\s*(\d+)\s*;', text)
        if m:
            out[name] = int(m.group(1))
    return out


def plan_chain(T, wq, c, chain_reg=True, local_t=None):
    """rotate_driver.hip plan_chain in the default build (the tuning switches are compiled out): the form of a run of T > 0 rows of wq
    words a half.  chain_reg: SYMGPU_CHAIN_REG != 0; local_t: the value of SYMGPU_CHAIN_LOCAL_T, None if unset."""
    W = 2 * wq
    pow2 = (wq & (wq - 1)) == 0
    regs = chain_reg and 1 <= T <= (1 << c['CHAIN_IDX_BITS']) and wq <= 32 and pow2
    lt = c['CHAIN_LOCAL_T'] if local_t is None else min(local_t, c['CHAIN_TMAX'])
    if regs and local_t is None:
        return 'Registers'
    if T <= lt and T <= c['CHAIN_LDS_T'] and W <= 128 and 2 * T * W * 8 <= 128 * 1024:
        return 'Lds'
    if T <= lt:
        return 'SingleWorkgroup'
    if regs:
        return 'Registers'
    if wq <= 64 and pow2 and T <= c['CHAIN_TWO_T']:
        return 'TwoLaunch'
    return 'FourLaunch'


def register_chunks(T, wq):
    """Chunks per lane of k_cchain_reg (rotate_chain.hip clifford_chain_registers)."""
    return (4 if wq == 32 else 2) if T * wq // 128 >= 8192 else 1


# ---------------------------------------------------------------- the one-launch rotation's plan, restated --------------------------------
RES_FORMS = ('Lds', 'Registers', 'RowsInMemory')                      # ResidentForm of rotate_common.h
RES_FORM_COUNTERS = ('RESIDENT_LDS', 'RESIDENT_REGISTERS', 'RESIDENT_ROWS_IN_MEMORY')   # the counter of each form
RES_NAMES = ('RES_THREADS', 'RES_MAX_WG', 'RES_LDS_MAX', 'RES_MIN_ROWS', 'RES_MAX_R', 'RES_REG_ROUNDS', 'RES_REG_MAX_WQ', 'RES_MAX_W', 'JOIN_MAX_T')


def resident_constants(text):
    """The limits of rotate_resident.h and JOIN_MAX_T of rotate_common.h from the source text (values written as a number, as a product of
    two numbers, or as ((i64)1 << b) - 1)."""
    import re
    out = {}
    for name in RES_NAMES:
        m = re.search(r'constexpr\s+(?:int|i64|u32|size_t)\s+' + name + r'\s*=\s*([^;]+);', text)
        if not m:
            continue
        expr = m.group(1).strip()
        shift = re.fullmatch(r'\(\(i64\)1 << (\d+)\) - 1', expr)
        prod = re.fullmatch(r'(\d+) \* (\d+)', expr)
        if shift:
            out[name] = (1 << int(shift.group(1))) - 1
        elif prod:
            out[name] = int(prod.group(1)) * int(prod.group(2))
        elif expr.isdigit():
            out[name] = int(expr)
    return out


def res_layout_total(R, wq, nreg, hbm, c):
    """res_layout(...).total of rotate_resident.h: the LDS bytes of a workgroup that owns R rows of wq chunks."""
    chunks = 0 if hbm else max(R * wq - nreg * c['RES_THREADS'], 0)
    o = chunks * 16 + R * (16 + 4 + 4 + 1 + 1)                      # rows; coefficient, join state / rank, rank of the new row, info, class
    o = (o + 15) & ~15
    return o + c['RES_MAX_W'] * 8 + 256 * 8 + 32 * 4                  # Q, per-(pass, wavefront) counts, the block's words


def plan_resident(T, wq, c, dup_free=True, k=-1, num_cu=256, hbm=1):
    """plan_resident of rotate_resident.hip: None where the operator does not qualify, else (form, G, R).  k: clifford_k (-1: not a
    Clifford angle); hbm: the value of SYMGPU_ROT_HBM (1 if unset)."""
    if T < 1 or 2 * wq > c['RES_MAX_W'] or T >= c['JOIN_MAX_T']:
        return None
    if (k < 0 or (k & 1)) and not dup_free:
        return None
    G = min(-(-T // c['RES_MIN_ROWS']), num_cu, c['RES_MAX_WG'])
    R = -(-T // G)
    G = -(-T // R)
    if R > c['RES_MAX_R']:
        return None
    form, total = 'Lds', res_layout_total(R, wq, 0, 0, c)
    if total > c['RES_LDS_MAX'] and wq <= c['RES_REG_MAX_WQ'] and (wq & (wq - 1)) == 0:
        form, total = 'Registers', res_layout_total(R, wq, c['RES_REG_ROUNDS'], 0, c)
    if (total > c['RES_LDS_MAX'] and hbm != 0) or hbm == 2:
        form, total = 'RowsInMemory', res_layout_total(R, wq, 0, 1, c)
    if total > c['RES_LDS_MAX']:
        return None
    return form, G, R


def resident_header_text():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'symmer_amd', 'csrc')
    return open(os.path.join(csrc, 'rotate_resident.h')).read() + open(os.path.join(csrc, 'rotate_common.h')).read()


def device_cu_count():
    """Compute units of the current device (GPU tests): the count symgpu_device_name reports, which is the property Context::num_cu is read from."""
    import ctypes, re
    from symmer_amd import _lib
    buf = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().symgpu_device_name(ctypes.addressof(buf), 256))
    m = re.search(r'(\d+) CUs\)$', buf.value.decode())
    assert m and int(m.group(1)) >= 1, buf.value
    return int(m.group(1))


RESIDENT_COUNTERS = ('RESIDENT_DONE', 'RESIDENT_FAILED') + RES_FORM_COUNTERS


def resident_counters():
    """RESIDENT_COUNTERS: one-launch rotations completed, failed, and launched in the LDS / registers / rows-in-memory form."""
    from symmer_amd import kernels
    return kernels.counters(RESIDENT_COUNTERS)
