"""NumPy-facing wrappers of the C-ABI: packed ``uint64`` rows + ``complex128`` coefficients in, same out.

Every function here runs on the GPU through ``libsymgpu.so``; there is no CPU path (a missing library or
GPU raises :class:`symmer_amd._lib.SymgpuError`).  Reference seams replaced (file:line in /root/reference):
``symplectic_cleanup`` utils.py:230, ``matmul_GF2``/``commutes_termwise`` utils.py:9 / base.py:938,
``_multiply_by_operator`` base.py:764, ``_rotate_by_single_Pword`` base.py:1090, ``_rref_binary`` utils.py:292,
``IndependentOp.symmetry_generators`` independent_op.py:90.
"""
import ctypes
import numpy as np
from . import _lib
from ._lib import addr, check

c_i64, c_int = ctypes.c_int64, ctypes.c_int


def _rows(a):
    a = np.ascontiguousarray(a, dtype='<u8')
    assert a.ndim == 2 and a.shape[1] % 2 == 0 and a.shape[1] >= 2, 'packed rows must be uint64[T, 2*Wq]'
    return a


def _coeff(c):
    return np.ascontiguousarray(c, dtype=np.complex128)


class DeviceOp:
    """Owner of a device-resident operator handle (``symgpu_op_t``).  ``shared`` is set once a handle is attached to more than one
    Python object (``copy()``): the in-place primitives (``set_coeff``, ``scale``) then work on a clone."""

    def __init__(self, handle):
        self.handle = handle
        self.shared = False

    def __deepcopy__(self, memo):
        # a handle is never duplicated by value (two owners of one symgpu_op_t would free it twice): copies share the object
        self.shared = True
        return self

    def __reduce__(self):
        raise TypeError('a DeviceOp is a pointer into this process\'s GPU memory and cannot be pickled: pickle the PauliwordOp that owns it '
                        '(it is brought to the host), or download() the rows')

    @classmethod
    def upload(cls, rows, coeff=None):
        rows = _rows(rows)
        coeff = None if coeff is None else _coeff(coeff)
        if coeff is not None:
            assert coeff.shape[0] == rows.shape[0]
        h = ctypes.c_void_p()
        check(_lib.lib().symgpu_op_upload(addr(rows), addr(coeff), rows.shape[0], rows.shape[1] // 2, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def upload_bool(cls, symp_matrix, coeff=None):
        """The reference layout itself (bool[T, 2n]) -> packed rows, packed on the device (``symgpu_op_upload_bool``)."""
        symp = np.ascontiguousarray(symp_matrix, dtype=np.bool_)
        assert symp.ndim == 2 and symp.shape[1] % 2 == 0 and symp.shape[1] >= 2
        coeff = None if coeff is None else _coeff(coeff)
        h = ctypes.c_void_p()
        check(_lib.lib().symgpu_op_upload_bool(addr(symp), addr(coeff), symp.shape[0], symp.shape[1] // 2, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def alloc(cls, capacity, wq, with_coeff=True):
        h = ctypes.c_void_p()
        check(_lib.lib().symgpu_op_alloc(int(capacity), int(wq), 1 if with_coeff else 0, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def random(cls, n_terms, n_qubits, density=0.3, seed=1234):
        h = ctypes.c_void_p()
        check(_lib.lib().symgpu_op_random(int(n_terms), int(n_qubits), float(density), int(seed), ctypes.byref(h)))
        return cls(h)

    def info(self):
        t, wq, cap = c_i64(0), c_int(0), c_i64(0)
        check(_lib.lib().symgpu_op_info(self.handle, ctypes.addressof(t), ctypes.addressof(wq), ctypes.addressof(cap)))
        return t.value, wq.value, cap.value

    @property
    def n_terms(self):
        return self.info()[0]

    def set_rows(self, t):
        check(_lib.lib().symgpu_op_set_rows(self.handle, int(t)))

    def copy_rows_from(self, src, src_begin, n, at=0):
        """Rows [src_begin, src_begin + n) of ``src`` to rows [at, at + n) of this operator (a peer copy when the devices differ).  The
        row count stays as it is (``set_rows``)."""
        if n:
            check(_lib.lib().symgpu_op_copy_rows(self.handle, int(at), src.handle, int(src_begin), int(n)))

    def write(self, at, rows, coeff, n):
        """``n`` host rows (and their coefficients, or None) to rows [at, at + n); the row count stays as it is."""
        check(_lib.lib().symgpu_op_write(self.handle, int(at), addr(rows), addr(coeff), int(n)))

    def download(self, with_coeff=True):
        t, wq, _ = self.info()
        rows = np.empty((t, 2 * wq), dtype='<u8')
        coeff = np.empty(t, dtype=np.complex128) if with_coeff else None
        check(_lib.lib().symgpu_op_download(self.handle, addr(rows), addr(coeff), t))
        return (rows, coeff) if with_coeff else rows

    def download_coeff(self):
        t = self.info()[0]
        coeff = np.empty(t, dtype=np.complex128)
        check(_lib.lib().symgpu_op_download(self.handle, None, addr(coeff), t))
        return coeff

    def download_bool(self, n_qubits):
        """bool[T, 2n] in the reference layout, unpacked on the device (``symgpu_op_download_bool``)."""
        t = self.info()[0]
        out = np.empty((t, 2 * int(n_qubits)), dtype=np.bool_)
        check(_lib.lib().symgpu_op_download_bool(self.handle, int(n_qubits), addr(out), t))
        return out

    def clone(self):
        h = ctypes.c_void_p()
        check(_lib.lib().symgpu_op_clone(self.handle, ctypes.byref(h)))
        return DeviceOp(h)

    def set_coeff(self, coeff):
        coeff = _coeff(coeff)
        assert coeff.shape[0] == self.info()[0]
        check(_lib.lib().symgpu_op_set_coeff(self.handle, addr(coeff)))

    def scale(self, const, conjugate_first=False):
        const = complex(const)
        check(_lib.lib().symgpu_op_scale(self.handle, const.real, const.imag, 1 if conjugate_first else 0))

    def ycount(self):
        out = np.zeros(self.info()[0], dtype=np.int64)
        check(_lib.lib().symgpu_op_ycount(self.handle, addr(out)))
        return out

    def checksum(self, with_coeff=True):
        _, wq, _ = self.info()
        x = np.zeros(2 * wq, dtype='<u8')
        c = np.zeros(1, dtype=np.complex128)
        check(_lib.lib().symgpu_op_checksum(self.handle, addr(x), addr(c) if with_coeff else None))
        return x, complex(c[0])

    def free(self):
        if self.handle is not None and self.handle.value:
            _lib.load().symgpu_op_free(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def concat_dev(parts, with_coeff=True):
    """Device operators (on any devices) stacked in order into a new one on the current device (device-to-device copies)."""
    sizes = [p.info() for p in parts]
    wq = sizes[0][1]
    total = sum(t for t, _, _ in sizes)
    out = DeviceOp.alloc(max(1, total), wq, with_coeff)
    at = 0
    for p, (t, w, _) in zip(parts, sizes):
        assert w == wq, 'operands packed with different Wq'
        out.copy_rows_from(p, 0, t, at)
        at += t
    out.set_rows(total)
    return out


def slice_dev(op, begin, end, with_coeff=True):
    """Rows [begin, end) of a device operator as a new one."""
    out = DeviceOp.alloc(end - begin, op.info()[1], with_coeff)
    out.copy_rows_from(op, begin, end - begin)
    return out


def counter(name):
    """The library's debug counter `name` (as spelled in SYMGPU_COUNTER_LIST of include/symgpu.h, e.g. 'H2D_BYTES'); KeyError if there is none."""
    v = c_i64(0)
    check(_lib.load().symgpu_debug_counter(_lib.counter_ids()[name], ctypes.addressof(v)))   # (needs no device)
    return v.value


def counters(names):
    """The debug counters `names`, in that order, as an int64 array."""
    return np.array([counter(name) for name in names], dtype=np.int64)


def transfer_counters():
    """(bytes host -> device, bytes device -> host, operator uploads, operator downloads) since the library was loaded."""
    return tuple(int(v) for v in counters(('H2D_BYTES', 'D2H_BYTES', 'OP_UPLOADS', 'OP_DOWNLOADS')))


def sync():
    check(_lib.lib().symgpu_sync())


def ycount(rows):
    rows = _rows(rows)
    out = np.zeros(rows.shape[0], dtype=np.int64)
    check(_lib.lib().symgpu_ycount(addr(rows), rows.shape[0], rows.shape[1] // 2, addr(out)))
    return out


_device_memory = {}


def device_memory_bytes():
    """Total memory of the calling thread's current device (cached per device)."""
    d = _lib.current_device() if _lib._initialised_device is not None else -1
    if d not in _device_memory:
        free_b, total_b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(_lib.lib().symgpu_mem_info(ctypes.addressof(free_b), ctypes.addressof(total_b)))
        _device_memory[_lib.current_device()] = int(total_b.value)
        d = _lib.current_device()
    return _device_memory[d]


def commutes(a_rows, b_rows):
    """bool[N, M]: True where a_rows[i] commutes with b_rows[j]."""
    a_rows, b_rows = _rows(a_rows), _rows(b_rows)
    assert a_rows.shape[1] == b_rows.shape[1], 'operands packed with different Wq'
    n, m = a_rows.shape[0], b_rows.shape[0]
    out = np.empty((n, m), dtype=np.uint8)
    if n and m:
        same = a_rows is b_rows
        check(_lib.lib().symgpu_commutes(addr(a_rows), n, addr(a_rows if same else b_rows), m, a_rows.shape[1] // 2, addr(out)))
    return out.view(np.bool_)


def _pair_table_handles(fn, a, b):
    """uint8[N, M] of the device entry point ``fn(a, 0, N, b, table)``: the table is computed into device memory and read back once."""
    (n, wq, _), (m, wq_b, _) = a.info(), b.info()
    assert wq == wq_b, 'operands packed with different Wq'
    out = np.empty((n, m), dtype=np.uint8)
    if n and m:
        buf = ctypes.c_void_p()
        check(_lib.lib().symgpu_dev_alloc(n * m, ctypes.byref(buf)))
        try:
            check(fn(a.handle, 0, n, b.handle, buf))
            check(_lib.lib().symgpu_dev_download(buf, addr(out), n * m))
        finally:
            _lib.lib().symgpu_dev_free(buf)
    return out.view(np.bool_)


def commutes_handles(a, b):
    """bool[N, M] for two device operators (rows only are used): the table is computed into device memory and read back once."""
    return _pair_table_handles(_lib.lib().symgpu_commutes_dev, a, b)


# ---- measurement grouping (csrc/clique.hip) --------------------------------------------------------------------------------------
REL_C, REL_AC, REL_QWC = 0, 1, 2             # SYMGPU_REL_*: the termwise relations
RELATIONS = {'C': REL_C, 'AC': REL_AC, 'QWC': REL_QWC}
CLIQUE_PAIRS, CLIQUE_UNIONS = 1, 2           # SYMGPU_CLIQUE_*: the form of a colouring call


def qwc_handles(a, b):
    """bool[N, M] for two device operators: True where a's term i and b's term j commute qubit by qubit (``symgpu_qwc_dev``); the table is
    computed into device memory and read back once."""
    return _pair_table_handles(_lib.lib().symgpu_qwc_dev, a, b)


def relation_degrees_dev(op, relation):
    """int64[T]: for every term of the device operator the number of OTHER terms it is related to (``relation``: REL_C / REL_AC / REL_QWC)."""
    deg = np.zeros(op.n_terms, dtype=np.int64)
    check(_lib.lib().symgpu_relation_degrees_dev(op.handle, int(relation), addr(deg)))
    return deg


def clique_colouring_dev(op, relation, order, want_info=False):
    """First-fit colouring of the terms of a device operator in ``order`` (a permutation of its term indices): every term takes the lowest
    colour all of whose members it is related to (``symgpu_clique_colour_dev``).  Returns (int32 colours[T] by term index, n_colours), with
    ``want_info`` also the call's info words (form, blocks resolved, terms a block, bitmap words a term)."""
    order = np.ascontiguousarray(order, dtype=np.int64)
    t = op.n_terms
    assert order.shape == (t,), 'order must name every term once'
    colours = np.zeros(t, dtype=np.int32)
    n_colours = c_i64(0)
    info = np.zeros(4, dtype=np.int64)
    check(_lib.lib().symgpu_clique_colour_dev(op.handle, int(relation), addr(order), addr(colours), ctypes.addressof(n_colours), addr(info)))
    return (colours, n_colours.value, info) if want_info else (colours, n_colours.value)


# ---- noncontextual operators (csrc/noncon.hip) ---------------------------------------------------------------------------------------
NONCON_MAX_FREE = 40                         # symgpu_noncon_search refuses more free generators


def noncon_signs_dev(terms, gens, selection):
    """int8[T]: for every term of the device operator ``terms`` the sign of the product, in generator order, of the terms of ``gens`` that
    row k of ``selection`` (bool[T, g]) selects: +1 / -1 if the product is +/- the term, 0 if it is another Pauli string or carries a phase
    +-i (``symgpu_noncon_signs_dev``)."""
    selection = np.asarray(selection).astype(bool)
    t, g = terms.n_terms, gens.n_terms
    assert selection.shape == (t, g), 'selection must be [terms, generators]'
    words = max(1, (g + 63) // 64)
    bits = np.zeros((t, words * 64), dtype=np.uint8)
    bits[:, :g] = selection
    sel = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u8').reshape(t, words)
    signs = np.zeros(t, dtype=np.int8)
    check(_lib.lib().symgpu_noncon_signs_dev(terms.handle, gens.handle, addr(sel), words, addr(signs)))
    return signs


def noncon_search(coeff, masks, clique, n_free, n_cliques, want_energies=False, want_info=False):
    """Brute-force minimum of the noncontextual objective over all 2^n_free assignments (``symgpu_noncon_search``): ``coeff`` float64[T],
    ``masks`` uint64[T] (bit b <=> free generator n_free-1-b), ``clique`` int32[T] (-1 outside the cliques).  Returns (energy, mask), then the
    float64[2^n_free] energies if ``want_energies`` (n_free <= 24), then the call's info words (L, blocks, entries a block, workgroups) if
    ``want_info``; among equal energies the largest mask wins."""
    coeff = np.ascontiguousarray(coeff, dtype=np.float64)
    masks = np.ascontiguousarray(masks, dtype=np.uint64)
    clique = np.ascontiguousarray(clique, dtype=np.int32)
    assert coeff.ndim == 1 and masks.shape == coeff.shape and clique.shape == coeff.shape, 'coeff, masks and clique must be [T]'
    assert not want_energies or n_free <= 24, 'the full landscape is returned up to 24 free generators'
    energy, best = ctypes.c_double(0.0), ctypes.c_uint64(0)
    energies = np.empty(1 << n_free, dtype=np.float64) if want_energies else None
    info = np.zeros(4, dtype=np.int64)
    check(_lib.lib().symgpu_noncon_search(addr(coeff), addr(masks), addr(clique), coeff.shape[0], int(n_free), int(n_cliques),
                                          ctypes.addressof(energy), ctypes.addressof(best), addr(energies), addr(info)))
    out = (energy.value, best.value)
    if want_energies:
        out += (energies,)
    if want_info:
        out += (info,)
    return out


# ---- noncontextual sweeps (csrc/noncon_sweep.hip) -------------------------------------------------------------------------------------
NONCON_SWEEP_MAX_T = 131072                  # SYMGPU_NONCON_SWEEP_MAX_T: symgpu_noncon_sweep_dev refuses more terms (a 2 GiB table)
SWEEP_REJECTED, SWEEP_SYM = -2, -1           # labels of a sweep; >= 0: the clique, numbered in order of creation


def noncon_sweep(op, order=None, starts=None, want_labels=False, want_info=False):
    """Noncontextual sweeps over the terms of a device operator (``symgpu_noncon_sweep_dev``): sweep ``s`` visits the terms
    ``order[(starts[s] + i) % T]``, i = 0 .. T-1, and keeps a term whenever the kept terms stay noncontextual.  ``order``: a permutation
    of the term indices (default: as they stand); ``starts``: the roll offsets (default: one sweep from position 0).  Returns
    bool[n_starts, T], True where the term at POSITION p of ``order`` was kept; then, with ``want_labels``, int32[n_starts, T] by position
    (``SWEEP_REJECTED``, ``SWEEP_SYM``, or the clique); then, with ``want_info``, the call's info words (table bytes, workgroups, sweeps
    a workgroup, largest clique count).  All sweeps of a call share one commutation table and run as one launch."""
    t = op.n_terms
    if t > NONCON_SWEEP_MAX_T:
        raise ValueError(f'{t} terms: a sweep takes at most {NONCON_SWEEP_MAX_T} (the commutation table takes T^2 / 8 bytes)')
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.int64)
        if order.shape != (t,) or not np.array_equal(np.sort(order), np.arange(t)):
            raise ValueError('order must be a permutation of the term indices')
    starts = np.zeros(1, dtype=np.int64) if starts is None else np.ascontiguousarray(starts, dtype=np.int64).reshape(-1)
    if t > 0 and starts.size and (starts.min() < 0 or starts.max() >= t):
        raise ValueError(f'every start must lie in [0, {t})')
    n_starts, words = starts.shape[0], (t + 63) // 64
    bits = np.zeros((n_starts, words), dtype='<u8')
    labels = np.full((n_starts, t), SWEEP_REJECTED, dtype=np.int32) if want_labels else None
    info = np.zeros(4, dtype=np.int64)
    check(_lib.lib().symgpu_noncon_sweep_dev(op.handle, addr(order), n_starts, addr(starts), addr(bits), addr(labels), addr(info)))
    kept = np.unpackbits(bits.view(np.uint8).reshape(n_starts, words * 8), axis=1, bitorder='little')[:, :t].astype(bool)
    out = (kept,)
    if want_labels:
        out += (labels,)
    if want_info:
        out += (info,)
    return out if len(out) > 1 else kept


def mul_allpairs(inner, ci, outer, co, inner_is_left=True):
    """Uncleaned product: row ``o*Ni + i`` = ``inner[i] ^ outer[o]`` with its phase-corrected coefficient."""
    inner, outer, ci, co = _rows(inner), _rows(outer), _coeff(ci), _coeff(co)
    assert inner.shape[1] == outer.shape[1]
    ni, no = inner.shape[0], outer.shape[0]
    rows = np.empty((ni * no, inner.shape[1]), dtype='<u8')
    coeff = np.empty(ni * no, dtype=np.complex128)
    if ni and no:
        check(_lib.lib().symgpu_mul_allpairs(addr(inner), addr(ci), ni, addr(outer), addr(co), no, inner.shape[1] // 2,
                                             1 if inner_is_left else 0, addr(rows), addr(coeff)))
    return rows, coeff


def _thr_args(zero_threshold):
    return (0.0, 0) if zero_threshold is None else (float(zero_threshold), 1)


def cleanup(rows, coeff, zero_threshold=1e-15):
    """First-occurrence dedup + sequential coefficient sums + strict threshold (None keeps everything)."""
    rows, coeff = _rows(rows), _coeff(coeff)
    assert rows.shape[0] == coeff.shape[0]
    if rows.shape[0] == 0:
        return rows.copy(), coeff.copy()
    with DeviceOp.upload(rows, coeff) as op, cleanup_dev(op, zero_threshold) as res:
        return res.download()


MAX_PAIRS_PER_CALL = 1 << 31      # one device call sorts 32-bit pair indices; larger products are tiled over the outer operand


def mul_cleanup_handles(a, b, inner_is_left=True, zero_threshold=1e-15, max_pairs=None):
    """Fused product + cleanup of two device operators (``a`` inner, ``b`` outer; ``a is b`` squares) -> new DeviceOp; the product rows are
    never materialised.  Products with more than ``max_pairs`` pairs are tiled over the outer (slow) index: every slab is cleaned on the
    device, the concatenation of the cleaned slabs is cleaned once more (same first-occurrence order; coefficient sums associate per slab,
    i.e. within 1e-16 relative).  Nothing returns to the host."""
    ni, no = a.info()[0], b.info()[0]
    thr, use = _thr_args(zero_threshold)
    max_pairs = MAX_PAIRS_PER_CALL if max_pairs is None else int(max_pairs)
    out = ctypes.c_void_p()
    if ni * no <= max_pairs:
        check(_lib.lib().symgpu_mul_cleanup_dev(a.handle, b.handle, 1 if inner_is_left else 0, thr, use, ctypes.byref(out)))
        return DeviceOp(out)
    slab = max(1, max_pairs // ni)
    parts = []
    try:
        for o0 in range(0, no, slab):
            part = ctypes.c_void_p()
            with slice_dev(b, o0, min(no, o0 + slab)) as piece:
                # partial sums must not be thresholded: a term may only cancel across slabs
                check(_lib.lib().symgpu_mul_cleanup_dev(a.handle, piece.handle, 1 if inner_is_left else 0, 0.0, 0, ctypes.byref(part)))
            parts.append(DeviceOp(part))
        stacked = concat_dev(parts)
    finally:
        for p in parts:                                            # gone before the final cleanup takes its workspace
            p.free()
    with stacked:
        return cleanup_dev(stacked, zero_threshold)


def mul_cleanup(inner, ci, outer, co, inner_is_left=True, zero_threshold=1e-15, max_pairs=None):
    """Host arrays in, host arrays out around :func:`mul_cleanup_handles` (``outer is inner``: one device operand serves both factors,
    which lets the library sort half of the pairs, cleanup_driver.hip)."""
    same = outer is inner and co is ci
    inner, outer, ci, co = _rows(inner), _rows(outer), _coeff(ci), _coeff(co)
    assert inner.shape[1] == outer.shape[1]
    if inner.shape[0] == 0 or outer.shape[0] == 0:
        return np.empty((0, inner.shape[1]), dtype='<u8'), np.empty(0, dtype=np.complex128)
    with DeviceOp.upload(inner, ci) as a, (a if same else DeviceOp.upload(outer, co)) as b, \
            mul_cleanup_handles(a, b, inner_is_left, zero_threshold, max_pairs) as res:
        return res.download()


import functools
import math


@functools.lru_cache(maxsize=256)
def rotation_args(angle, threshold=1e-18):
    """(cos, sin, clifford_k) for ``_rotate_by_single_Pword`` (base.py:1146-1156): clifford_k = round(2*angle/pi) if the
    angle is a multiple of pi/2 to within ``threshold``, else -1.  Negative multiples keep the reference's behaviour
    (``int_part in [2,3]`` is not reduced mod 4): only the parity and membership in {2,3} matter, so a negative k is
    mapped to k & 1 (parity preserved, never 2 or 3)."""
    multiple = angle * 2 / np.pi
    k = round(multiple)
    if abs(k - multiple) <= threshold:
        ck = k if k in (2, 3) else (k % 2)
        return 0.0, 0.0, int(ck)             # the Clifford branch never uses cos / sin (base.py:1139-1154): not computed
    # (np.cos / np.sin of a Python float and math.cos / math.sin are the same libm call; the results are cached per angle: a Trotter circuit
    # repeats a handful of angles thousands of times)
    return float(np.cos(angle)), float(np.sin(angle)), -1


def rotate_single_resident(op, q_addr, angle, zero_threshold=1e-15, clifford_threshold=1e-18):
    """``rotate_single_dev`` for the drop-in class, without its per-call conveniences (the API call cost 1.6x the C-ABI
    step): the generator's packed row comes as an address the caller keeps, cos / sin come from the cache, and the result's term count is
    read once and returned.  -> (DeviceOp or None, all_commute, n_terms)."""
    cos_t, sin_t, k = rotation_args(angle, clifford_threshold)
    out = ctypes.c_void_p()
    allc, t = c_int(0), c_i64(0)
    check(_lib.lib().symgpu_rotate_single_dev_n(op.handle, q_addr, cos_t, sin_t, k, zero_threshold, ctypes.byref(out), ctypes.addressof(allc),
                                                ctypes.addressof(t)))
    if allc.value:
        return None, True, 0
    return DeviceOp(out), False, t.value


def rotate_single_dev(op, q_row, angle, zero_threshold=1e-15, clifford_threshold=1e-18):
    """Device-resident rotation: returns (DeviceOp or None, all_commute).  ``clifford_threshold`` is the reference's
    ``threshold`` argument (base.py:1146): how close 2*angle/pi must be to an integer for the Clifford branch."""
    q_row = np.ascontiguousarray(q_row, dtype='<u8').reshape(-1)
    cos_t, sin_t, k = rotation_args(angle, clifford_threshold)
    out = ctypes.c_void_p()
    allc = c_int(0)
    check(_lib.lib().symgpu_rotate_single_dev(op.handle, addr(q_row), cos_t, sin_t, k, float(zero_threshold), ctypes.byref(out),
                                              ctypes.addressof(allc)))
    if allc.value:
        return None, True
    return DeviceOp(out), False


# symgpu_rotate_clifford_chain_dev: when Wq = ceil(n / 64) is a power of two <= 32 (n <= 2048) the rows stay in registers and the accumulated partition
# bits are sorted once per 40 rotations (5.0 us per rotation at 10^5 terms, 1.1 us at 64).  Other rows: one LDS-resident or single-workgroup launch for the
# whole run up to 128 terms, two launches per rotation up to 262,144, the per-rotation kernels back to back without a host read-back above that.
CLIFFORD_CHAIN_MAX_TERMS = 1 << 22
CLIFFORD_CHAIN_KERNEL_LIMIT = 8192


def rotate_clifford_chain_dev(op, q_rows, ks):
    """K Clifford rotations of a CLEAN device operator (straight from a cleanup: no duplicate rows, |c| > 1e-15) with at most
    CLIFFORD_CHAIN_MAX_TERMS terms without any host round trip between them.  ``q_rows`` uint64[K, 2*Wq], ``ks`` the clifford_k of every rotation as
    returned by :func:`rotation_args` (0..3).  Returns a new DeviceOp."""
    q_rows = np.ascontiguousarray(q_rows, dtype='<u8')
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    assert q_rows.ndim == 2 and q_rows.shape[0] == ks.shape[0]
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_rotate_clifford_chain_dev(op.handle, addr(q_rows), addr(ks), q_rows.shape[0], ctypes.byref(out)))
    return DeviceOp(out)


def perform_rotations_dev(op, q_rows, cos_t, sin_t, ks, clean, zero_threshold=1e-15):
    """``perform_rotations`` on a device operator in one library call (``symgpu_perform_rotations_dev``): returns
    (new DeviceOp or None if nothing changed, rotations done, uint8 flags of the single rotations that acted, clean flag).
    The call processes all K rotations, also through the states "no terms" and "0 * I" (it follows the reference's alternation itself)."""
    q_rows = np.ascontiguousarray(q_rows, dtype='<u8')
    cos_t, sin_t = np.ascontiguousarray(cos_t, dtype=np.float64), np.ascontiguousarray(sin_t, dtype=np.float64)
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    K = q_rows.shape[0]
    acted = np.zeros(K, dtype=np.uint8)
    out = ctypes.c_void_p()
    n_done, clean_out = c_i64(0), c_int(0)
    check(_lib.lib().symgpu_perform_rotations_dev(op.handle, addr(q_rows), addr(cos_t), addr(sin_t), addr(ks), K, float(zero_threshold),
                                                  1 if clean else 0, ctypes.byref(out), addr(acted), ctypes.addressof(n_done), ctypes.addressof(clean_out)))
    return (DeviceOp(out) if out.value else None), n_done.value, acted, bool(clean_out.value)


def cleanup_dev(op, zero_threshold=1e-15):
    thr, use = _thr_args(zero_threshold)
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_cleanup_dev(op.handle, thr, use, ctypes.byref(out)))
    return DeviceOp(out)


def rref(matrix_words, want_pivots=False):
    """``_rref_binary`` on uint64[R, Wc] packed rows -> (reduced, xor_count[, pivot column per row or -1])."""
    m = np.array(matrix_words, dtype='<u8', order='C', copy=True)
    assert m.ndim == 2
    R, wc = m.shape
    count = c_i64(0)
    piv = np.full(R, -1, dtype=np.int64)
    if R and wc:
        check(_lib.lib().symgpu_rref(addr(m), R, wc, ctypes.addressof(count), addr(piv)))
    return (m, count.value, piv) if want_pivots else (m, count.value)


def symmetry_kernel(h_rows, n_qubits):
    """Packed generators of the Z2 symmetries of the operator with packed rows ``h_rows`` -> (rows, xor_count)."""
    h_rows = _rows(h_rows)
    wq = h_rows.shape[1] // 2
    out = np.zeros((2 * n_qubits, 2 * wq), dtype='<u8')
    k, count = c_i64(0), c_i64(0)
    check(_lib.lib().symgpu_symmetry_kernel(addr(h_rows), h_rows.shape[0], int(n_qubits), wq, addr(out), 2 * n_qubits,
                                            ctypes.addressof(k), ctypes.addressof(count)))
    return out[:k.value].copy(), count.value


def symmetry_kernel_handle(op, n_qubits):
    """The same on a device-resident operator (``symgpu_symmetry_kernel_dev``): only the generators come back."""
    wq = op.info()[1]
    out = np.zeros((2 * n_qubits, 2 * wq), dtype='<u8')
    k, count = c_i64(0), c_i64(0)
    check(_lib.lib().symgpu_symmetry_kernel_dev(op.handle, int(n_qubits), addr(out), 2 * n_qubits, ctypes.addressof(k), ctypes.addressof(count)))
    return out[:k.value].copy(), count.value


# ---- f2: generator routines on resident operators (csrc/genrec.hip) -----------------------------------------------------
def gf2_rank_dev(op):
    """Rank over GF(2) of the operator's symplectic rows (= non-zero rows of ``_rref_binary``, utils.py:292-315)."""
    r = c_i64(0)
    check(_lib.lib().symgpu_op_gf2_rank(op.handle, ctypes.addressof(r)))
    return r.value


def generators_dev(op):
    """``PauliwordOp.generators`` (base.py:1436-1456) -> new DeviceOp: non-zero rows of ``_rref_binary(symp_matrix)``, coefficients 1."""
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_generators_dev(op.handle, ctypes.byref(out)))
    return DeviceOp(out)


def generator_reconstruction_dev(gens, op, n_qubits):
    """``PauliwordOp.generator_reconstruction`` (base.py:523-560) of ``op`` in ``gens`` -> (int64[T, g], bool[T])."""
    g, t = gens.info()[0], op.info()[0]
    recon = np.empty((t, g), dtype=np.int64)
    mask = np.empty(t, dtype=np.uint8)
    check(_lib.lib().symgpu_generator_reconstruction_dev(gens.handle, op.handle, int(n_qubits), addr(recon), addr(mask)))
    return recon, mask.view(np.bool_)


# ---- f3 / f4: projection, noncontextuality test, state inner product -------------------------------------------------
def sector_signs(eigenvalues):
    """Stabiliser eigenvalues as ints in {-1, 0, +1}.  The reference multiplies by the eigenvalue itself (projection/base.py:68-71); the
    sign-mask form of the device kernel is that product only for these three values, so anything else is refused — with an exception, not
    an assert (`python -O`), and before anything has consumed the values; entries within 1e-12 of an allowed value (a sector that went
    through floating point) are rounded as the reference's own `IndependentOp` would store them."""
    ev = np.asarray(eigenvalues).ravel()
    if ev.size == 0:
        return np.zeros(0, dtype=np.int64)
    if np.iscomplexobj(ev):
        if np.any(np.abs(ev.imag) > 1e-12):
            raise ValueError(f'stabiliser eigenvalues must be -1, 0 or +1, got {ev}')
        ev = ev.real
    rounded = np.rint(np.asarray(ev, dtype=float))
    if np.any(np.abs(ev - rounded) > 1e-12) or not np.all(np.isin(rounded, (-1.0, 0.0, 1.0))):
        raise ValueError(f'stabiliser eigenvalues must be -1, 0 or +1, got {ev}')
    return rounded.astype(np.int64)


def project_dev(op, stab_rows, eigenvalues, keep_qubits, n_qubits, zero_threshold=1e-15):
    """``S3Projection._perform_projection`` (projection/base.py:44-84) on a device operator: ``stab_rows`` uint64[k, 2*Wq] the fixed
    single-qubit stabilisers, ``eigenvalues`` int[k] their sector, ``keep_qubits`` the ascending indices of the qubits that stay.
    Returns (cleaned projected DeviceOp, number of terms that commuted with every stabiliser)."""
    stab_rows = np.ascontiguousarray(stab_rows, dtype='<u8').reshape(-1, stab_rows.shape[-1]) if len(stab_rows) else np.zeros((0, 2), dtype='<u8')
    k = stab_rows.shape[0]
    wq = op.info()[1]
    neg = np.zeros(2 * wq, dtype='<u8')
    eigenvalues = sector_signs(eigenvalues)
    for row, ev in zip(stab_rows, eigenvalues):
        if ev == -1:
            neg |= row                                             # (projection/base.py:69: the column index list has one entry per stabiliser)
    keep = np.ascontiguousarray(keep_qubits, dtype=np.int32)
    thr, use = _thr_args(zero_threshold)
    out = ctypes.c_void_p()
    n_surv = c_i64(0)
    check(_lib.lib().symgpu_project_dev(op.handle, addr(stab_rows) if k else None, k, addr(neg), addr(keep), keep.shape[0], int(n_qubits), thr, use,
                                        ctypes.byref(out), ctypes.addressof(n_surv)))
    return DeviceOp(out), n_surv.value


def noncontextual_dev(op):
    res = c_int(0)
    check(_lib.lib().symgpu_noncontextual_dev(op.handle, ctypes.addressof(res)))
    return bool(res.value)


def state_inner_dev(a, b):
    """Inner product of two CLEANED device states (operators whose X blocks are the basis strings): sum of c_a * c_b over the rows present
    in both, added in the order of ``a``."""
    out = np.zeros(2, dtype=np.float64)
    check(_lib.lib().symgpu_state_inner_dev(a.handle, b.handle, addr(out)))
    return complex(out[0], out[1])


EXPVAL_LDS, EXPVAL_GLOBAL = 1, 2             # SYMGPU_EXPVAL_LDS / SYMGPU_EXPVAL_GLOBAL: where the look-up table of a call lived


def expval_terms_dev(op, phi, psi, want_terms=True):
    """``<phi|P_k|psi>`` for every term of the device operator ``op`` in one call (csrc/expval.hip): ``phi`` and ``psi`` are CLEANED device
    states (``phi is psi``: the expectation value), ``op`` is taken as it is.  Returns (terms complex128[T] without the terms' coefficients
    — None with ``want_terms=False`` —, total = sum of c_k * terms[k] in term order, the form that ran)."""
    t = op.n_terms
    terms = np.zeros(t, dtype=np.complex128) if want_terms else None
    total = np.zeros(2, dtype=np.float64)
    form = c_int(0)
    check(_lib.lib().symgpu_expval_terms_dev(op.handle, phi.handle, psi.handle, addr(terms), addr(total), ctypes.addressof(form)))
    return terms, complex(total[0], total[1]), form.value


def _host_available_bytes():
    """MemAvailable of /proc/meminfo (None where there is no such file)."""
    try:
        with open('/proc/meminfo') as f:
            for line in f:
                if line.startswith('MemAvailable:'):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def csr_index_dtype(nnz, n_qubits):
    """The index dtype scipy gives a ``2^n x 2^n`` CSR matrix of ``nnz`` entries: int32 while both fit, else int64."""
    return np.int32 if max(int(nnz), 1 << int(n_qubits)) <= np.iinfo(np.int32).max else np.int64


def csr_forced_index_dtype(nnz, n_qubits, index_dtype):
    """The index dtype of ``to_csr``: ``csr_index_dtype`` for None, else the forced int32 / int64; ValueError for any other dtype and for
    an int32 that cannot hold ``nnz`` or ``2^n``."""
    natural = csr_index_dtype(nnz, n_qubits)
    if index_dtype is None:
        return natural
    forced = np.dtype(index_dtype)
    if forced not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError(f'to_csr: index_dtype = {index_dtype!r} is neither int32 nor int64')
    if forced == np.dtype(np.int32) and natural is not np.int32:
        raise ValueError(f'to_csr: {int(nnz)} entries of a 2^{int(n_qubits)} x 2^{int(n_qubits)} matrix do not fit int32 indices')
    return forced.type


def to_csr(devop, n_qubits, index_dtype=None):
    """``PauliwordOp.to_sparse_matrix`` (base.py:1458-1507) of a device operator of 1 <= n_qubits <= 31 as ``(data, indices, indptr)``
    NumPy arrays of a canonical ``2^n x 2^n`` CSR matrix: entry (b, b ^ x_k) sums ``c_k (-i)^{Y_k} (-1)^{|b & z_k|}`` over the terms in
    operator order, qubit 0 the most significant bit of b; entries whose two components are both +-0 are not stored.  The exact entry
    count is known before the output is allocated: MemoryError if it does not fit the device or the host.  ``index_dtype``: None for
    the dtype scipy would choose (``csr_index_dtype``), ``np.int32`` / ``np.int64`` to force the width of ``indices`` and ``indptr``
    (ValueError if int32 is forced and cannot hold the result)."""
    n_qubits = int(n_qubits)
    csr_forced_index_dtype(0, n_qubits, index_dtype)          # a bad index_dtype is refused before any device work
    if not 1 <= n_qubits <= 31:
        raise ValueError(f'to_csr: n_qubits = {n_qubits} outside 1 .. 31 (column indices must fit an int32 index space)')
    nnz_c, scratch_c, plan = c_i64(0), c_i64(0), ctypes.c_void_p()
    check(_lib.lib().symgpu_to_csr_count(devop.handle, n_qubits, ctypes.addressof(nnz_c), ctypes.addressof(scratch_c), ctypes.byref(plan)))
    nnz, side = int(nnz_c.value), 1 << n_qubits
    try:
        idx_dtype = csr_forced_index_dtype(nnz, n_qubits, index_dtype)
    except ValueError:
        check(_lib.lib().symgpu_to_csr_fill(plan, None, None, None, 4))               # frees the plan
        raise
    ib = np.dtype(idx_dtype).itemsize
    host_need = nnz * (16 + ib) + (side + 1) * ib
    # what the fill allocates on the device: data + indices, the int32 copy of indptr (the int64 one is already held by the plan, so the
    # free memory read below has paid for it) and its slot scratch, as the count call reports it
    dev_need = nnz * (16 + ib) + ((side + 1) * 4 if ib == 4 else 0) + int(scratch_c.value)
    free_b, total_b = c_i64(0), c_i64(0)
    rc = _lib.lib().symgpu_mem_info(ctypes.addressof(free_b), ctypes.addressof(total_b))
    host_avail = _host_available_bytes()
    short = None
    if rc == 0 and dev_need > free_b.value:
        short = f'{dev_need / 2**30:.2f} GiB on the device, {free_b.value / 2**30:.2f} GiB free'
    elif host_avail is not None and host_need > host_avail:
        short = f'{host_need / 2**30:.2f} GiB on the host, {host_avail / 2**30:.2f} GiB available'
    if short is not None:
        check(_lib.lib().symgpu_to_csr_fill(plan, None, None, None, ib))          # frees the plan
        raise MemoryError(f'to_sparse_matrix: {nnz} entries of a {side} x {side} matrix need {short}')
    try:
        data = np.empty(nnz, dtype=np.complex128)
        indices = np.empty(nnz, dtype=idx_dtype)
        indptr = np.empty(side + 1, dtype=idx_dtype)
    except MemoryError:
        check(_lib.lib().symgpu_to_csr_fill(plan, None, None, None, ib))
        raise
    check(_lib.lib().symgpu_to_csr_fill(plan, addr(data), addr(indices), addr(indptr), ib))
    return data, indices, indptr


# ---- H x on dense statevectors and the vector kernels of exact_gs_energy (csrc/matvec.hip, csrc/lanczos.hip) --------------------------
MATVEC_DIRECT = 1                            # SYMGPU_MATVEC_DIRECT: the form a matvec_apply reports (0: no kernel ran, T = 0)
CHEB_DIRECT = 1                              # SYMGPU_CHEB_DIRECT: the form a cheb_apply reports, the only one


class DeviceBuffer:
    """Owner of a block of ``symgpu_dev_alloc``: ``nbytes`` bytes on the current device, freed by ``free()``, on leaving a ``with`` block
    or when collected."""

    def __init__(self, nbytes):
        self.ptr, self.nbytes = ctypes.c_void_p(), int(nbytes)
        rc = _lib.lib().symgpu_dev_alloc(self.nbytes, ctypes.byref(self.ptr))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)

    @classmethod
    def upload(cls, array):
        array = np.ascontiguousarray(array)
        buf = cls(array.nbytes)
        buf.write(array)
        return buf

    def write(self, array):
        """``array`` to the start of the block."""
        array = np.ascontiguousarray(array)
        assert array.nbytes <= self.nbytes
        check(_lib.lib().symgpu_dev_upload(self.ptr, addr(array), array.nbytes))

    def download(self, dtype, count, offset_bytes=0):
        out = np.empty(count, dtype=dtype)
        check(_lib.lib().symgpu_dev_download(ctypes.c_void_p(self.ptr.value + int(offset_bytes)), addr(out), out.nbytes))
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value:
            _lib.load().symgpu_dev_free(self.ptr)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MatvecPlan:
    """Owner of a ``symgpu_matvec_plan``: the terms of a device operator of 1 .. 32 qubits grouped by X-part, resident until ``free()``
    (also on leaving a ``with`` block, or when collected).  The operator itself is not referenced after the constructor returns."""

    def __init__(self, devop, n_qubits):
        n_qubits = int(n_qubits)
        if not 1 <= n_qubits <= 32:
            raise ValueError(f'matvec: n_qubits = {n_qubits} outside 1 .. 32')
        self.handle = ctypes.c_void_p()
        rc = _lib.lib().symgpu_matvec_plan(devop.handle, n_qubits, ctypes.byref(self.handle))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)
        self.n_qubits = n_qubits

    def info(self):
        """(n_qubits, n_terms, n_groups, device_bytes)."""
        n, t, g, b = c_int(0), c_i64(0), c_i64(0), c_i64(0)
        check(_lib.lib().symgpu_matvec_info(self.handle, ctypes.addressof(n), ctypes.addressof(t), ctypes.addressof(g), ctypes.addressof(b)))
        return n.value, t.value, g.value, b.value

    def apply(self, x, y):
        """``y = H x`` for two ``DeviceBuffer`` of ``2^n`` complex128 (not the same one); returns the form that ran."""
        form = c_int(0)
        check(_lib.lib().symgpu_matvec_apply(self.handle, x.ptr, y.ptr, ctypes.addressof(form)))
        return form.value

    def matvec(self, v):
        """``H v`` for a host vector of ``2^n`` numbers: upload, apply, download.  Returns (complex128[2^n], form)."""
        v = np.ascontiguousarray(v, dtype=np.complex128).reshape(-1)
        if v.shape[0] != 1 << self.n_qubits:
            raise ValueError(f'matvec: the vector has {v.shape[0]} elements, 2^{self.n_qubits} wanted')
        with DeviceBuffer.upload(v) as x, DeviceBuffer(v.nbytes) as y:
            form = self.apply(x, y)
            return y.download(np.complex128, v.shape[0]), form

    def sector_mask(self, n_particles, keep):
        """For the plan of a diagonal operator N: ``keep`` (``DeviceBuffer`` of ``2^n`` bytes) gets 1 where the nearest integer to
        ``Re N[b, b]`` is ``n_particles``, else 0; returns the number of kept states."""
        n_kept = c_i64(0)
        check(_lib.lib().symgpu_matvec_sector_mask(self.handle, int(n_particles), keep.ptr, ctypes.addressof(n_kept)))
        return n_kept.value

    def lanczos_step(self, keep, basis, capacity, j):
        """One Lanczos step with full reorthogonalisation on the resident ``basis`` (``DeviceBuffer`` of ``capacity`` vectors, slots
        0 .. j orthonormal; ``keep``: a sector mask or None): returns (alpha, beta) and leaves ``v_{j+1}`` in slot j + 1 if there is one
        and beta > 0."""
        alpha, beta = ctypes.c_double(0), ctypes.c_double(0)
        rc = _lib.lib().symgpu_lanczos_step(self.handle, None if keep is None else keep.ptr, basis.ptr, int(capacity), int(j),
                                            ctypes.addressof(alpha), ctypes.addressof(beta))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)
        return alpha.value, beta.value

    def chebyshev(self, centre, half_width, coeffs, psi, out):
        """``out = sum_k coeffs[k] T_k((H - centre) / half_width) psi`` for two ``DeviceBuffer`` of ``2^n`` complex128 (not the same
        one; ``psi`` is not written) and ``K + 1 >= 1`` complex coefficients: one launch per order (csrc/evolve.hip), in the arithmetic
        of include/symgpu.h f11.  The spectrum of ``H`` must lie in ``[centre - half_width, centre + half_width]``.  Returns the form
        that ran (``CHEB_DIRECT``)."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.complex128).reshape(-1)
        form = c_int(0)
        rc = _lib.lib().symgpu_cheb_apply(self.handle, float(centre), float(half_width), addr(coeffs), coeffs.shape[0] - 1,
                                          None if psi is None else psi.ptr, None if out is None else out.ptr, ctypes.addressof(form))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)
        return form.value

    def free(self):
        if self.handle is not None and self.handle.value:
            _lib.load().symgpu_matvec_free(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def vec_combine(basis, m, n_qubits, s, out=None, normalise=False):
    """``out = sum_j s[j] v_j`` over the first ``m`` vectors of ``basis`` (real ``s``), scaled to unit norm with ``normalise``.  ``out``:
    a ``DeviceBuffer`` of ``2^n`` complex128, or None for slot 0 of the basis (the restart)."""
    s = np.ascontiguousarray(s, dtype=np.float64)
    assert s.shape == (int(m),)
    check(_lib.lib().symgpu_vec_combine(basis.ptr, int(m), int(n_qubits), addr(s), (basis if out is None else out).ptr, 1 if normalise else 0))


# ---- exp(i theta P) rotations of a statevector, energy, adjoint gradient, pool gradient (csrc/ansatz.hip) --------------------------------
ANSATZ_DIRECT, ANSATZ_TILED = 1, 2           # SYMGPU_ANSATZ_*: the forms an ansatz_apply reports as a bit set (0: no rotation ran)


def _cos_sin(x, count):
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if x.shape[0] != count:
        raise ValueError(f'ansatz: {x.shape[0]} angles for {count} generators')
    return np.ascontiguousarray(np.cos(x)), np.ascontiguousarray(np.sin(x))


class AnsatzPlan:
    """Owner of a ``symgpu_ansatz_plan``: the rows of a device operator of 1 .. 32 qubits as the generators ``P_k`` of
    ``prod_k exp(i theta_k P_k)``, in operator order, resident until ``free()`` (also on leaving a ``with`` block, or when collected).
    The operator itself is not referenced after the constructor returns."""

    def __init__(self, devop, n_qubits):
        n_qubits = int(n_qubits)
        if not 1 <= n_qubits <= 32:
            raise ValueError(f'ansatz: n_qubits = {n_qubits} outside 1 .. 32')
        self.handle = ctypes.c_void_p()
        rc = _lib.lib().symgpu_ansatz_plan(devop.handle, n_qubits, ctypes.byref(self.handle))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)
        self.n_qubits = n_qubits
        self.n_generators = self.info()[1]

    def info(self):
        """(n_qubits, n_generators, n_runs, device_bytes)."""
        n, k, r, b = c_int(0), c_i64(0), c_i64(0), c_i64(0)
        check(_lib.lib().symgpu_ansatz_info(self.handle, ctypes.addressof(n), ctypes.addressof(k), ctypes.addressof(r), ctypes.addressof(b)))
        return n.value, k.value, r.value, b.value

    def apply(self, x, psi, k_begin=0, k_end=None, inverse=False):
        """Rotations ``k_begin .. k_end-1`` (default: all) with the angles ``x`` (one per generator of the plan) on ``psi``, a
        ``DeviceBuffer`` of ``2^n`` complex128, in place.  ``inverse``: the inverse rotations in reverse order.  Returns the forms that
        ran, ``ANSATZ_DIRECT | ANSATZ_TILED`` as a bit set (``SYMGPU_ANSATZ_FORM=direct`` forces direct passes; the bits are the same)."""
        k_end = self.n_generators if k_end is None else int(k_end)
        cos_t, sin_t = _cos_sin(x, self.n_generators)
        if inverse:
            sin_t = -sin_t
        form = c_int(0)
        check(_lib.lib().symgpu_ansatz_apply(self.handle, addr(cos_t), addr(sin_t), int(k_begin), k_end, 1 if inverse else 0, psi.ptr,
                                             ctypes.addressof(form)))
        return form.value

    def energy_grad(self, plan_H, x, ref, psi_out=None, want_grad=True):
        """``(E, grad)`` of ``<psi(x)|H|psi(x)>`` for ``psi(x)`` prepared from ``ref`` (``DeviceBuffer``, not changed): one state
        preparation, one ``H v`` and one reverse sweep.  ``grad`` is None without ``want_grad``; ``psi_out`` (``DeviceBuffer`` or
        None) receives the prepared state."""
        cos_t, sin_t = _cos_sin(x, self.n_generators)
        energy = ctypes.c_double(0)
        grad = np.zeros(self.n_generators, dtype=np.float64) if want_grad else None
        rc = _lib.lib().symgpu_ansatz_energy_grad(self.handle, plan_H.handle, addr(cos_t), addr(sin_t), ref.ptr,
                                                  None if psi_out is None else psi_out.ptr, ctypes.addressof(energy), addr(grad))
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        check(rc)
        return energy.value, grad

    def free(self):
        if self.handle is not None and self.handle.value:
            _lib.load().symgpu_ansatz_free(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pool_gradient(plan_H, pool_devop, psi, want_energy=False):
    """``<psi| i [H, P_j] |psi>`` for every row ``P_j`` of the device operator ``pool_devop`` from one ``H psi`` (``psi``: a
    ``DeviceBuffer`` of ``2^n`` complex128).  With ``want_energy``: ``(gradient, <psi|H|psi>)``."""
    grad = np.zeros(pool_devop.n_terms, dtype=np.float64)
    energy = ctypes.c_double(0)
    rc = _lib.lib().symgpu_pool_gradient(plan_H.handle, pool_devop.handle, psi.ptr, ctypes.addressof(energy) if want_energy else None, addr(grad))
    if rc == _lib.E_NOMEM:
        raise MemoryError(_lib.last_error())
    check(rc)
    return (grad, energy.value) if want_energy else grad


# ---- the reduced density matrix of a dense statevector (csrc/rdm.hip) -----------------------------------------------------------------
RDM_STREAM, RDM_TILED = 1, 2                 # SYMGPU_RDM_*: the form a symgpu_rdm reports in info[0]
RDM_MAX_QUBITS, RDM_MAX_KEPT = 32, 12        # the refusal bounds of symgpu_rdm


def rdm_dev(psi, n_qubits, kept, want_info=False):
    """The reduced density matrix of the ``2^n`` amplitudes ``psi`` (a ``DeviceBuffer``, or a complex array that is uploaded; qubit 0
    the most significant bit of the index) over the qubits ``kept`` — any iterable of ints, de-duplicated and sorted as the reference's
    ``get_rdm`` does through a set — as complex128 ``[2^k, 2^k]``; ``psi`` is not normalised.  The matrix is Hermitian to the bit.
    ``SYMGPU_RDM_FORM=stream|tiled`` forces a form where it is legal.  With ``want_info``: ``(rho, info)``, ``info`` the six int64 words of
    ``symgpu_rdm`` (form, KS, chunks, tile edge, workgroups, scratch bytes).  ValueError for a qubit outside ``0 .. n-1``, more than 32
    qubits or more than 12 kept ones; MemoryError when the scratch does not fit the device."""
    n_qubits = int(n_qubits)
    if not 1 <= n_qubits <= RDM_MAX_QUBITS:
        raise ValueError(f'rdm: n_qubits = {n_qubits} outside 1 .. {RDM_MAX_QUBITS}')
    qubits = sorted({int(q) for q in kept})
    if any(q < 0 or q >= n_qubits for q in qubits):
        raise ValueError(f'rdm: qubits {[q for q in qubits if q < 0 or q >= n_qubits]} outside 0 .. {n_qubits - 1}')
    k = len(qubits)
    if k > RDM_MAX_KEPT:
        raise ValueError(f'rdm: {k} kept qubits; at most {RDM_MAX_KEPT} are supported (a {1 << RDM_MAX_KEPT} x {1 << RDM_MAX_KEPT} matrix)')
    kept_arr = np.ascontiguousarray(qubits, dtype=np.int32)
    info = np.zeros(6, dtype=np.int64)
    own = None
    if not isinstance(psi, DeviceBuffer):
        host = np.ascontiguousarray(psi, dtype=np.complex128).reshape(-1)
        if host.shape[0] != 1 << n_qubits:
            raise ValueError(f'rdm: the vector has {host.shape[0]} elements, 2^{n_qubits} wanted')
        psi = own = DeviceBuffer.upload(host)
    try:
        if psi.nbytes < 16 << n_qubits:
            raise ValueError(f'rdm: the buffer holds {psi.nbytes} bytes, 2^{n_qubits} amplitudes need {16 << n_qubits}')
        with DeviceBuffer(16 << (2 * k)) as rho:
            rc = _lib.lib().symgpu_rdm(psi.ptr, n_qubits, addr(kept_arr) if k else None, k, rho.ptr, addr(info))
            if rc == _lib.E_NOMEM:
                raise MemoryError(_lib.last_error())
            check(rc)
            out = rho.download(np.complex128, 1 << (2 * k)).reshape(1 << k, 1 << k)
    finally:
        if own is not None:
            own.free()
    return (out, info) if want_info else out


# ---- measuring a vector of amplitudes (csrc/sample.hip, csrc/basis.hip) ----------------------------------------------------------------
SAMPLE_HIST, SAMPLE_SORT = 1, 2              # SYMGPU_SAMPLE_*: the counting form of a draw (info[4] of symgpu_sample_info)
BASIS_DIRECT, BASIS_TILED = 1, 2             # SYMGPU_BASIS_*: the form a symgpu_basis_change reports
SAMPLE_MAX_DRAWS = (1 << 31) - 1             # the refusal bound of symgpu_sample_draw


def philox_uniforms(seed, first_draw, count, out=None):
    """Draws ``first_draw .. first_draw + count - 1`` of the Philox4x64-10 stream of ``seed``, float64: the numbers of
    ``np.random.Generator(np.random.Philox(key=seed, counter=0)).random()`` at those positions, generated on the device.  ``out``: a
    ``DeviceBuffer`` that receives them (then nothing is downloaded and the buffer is returned)."""
    count = int(count)
    buf = out if out is not None else DeviceBuffer(max(8, 8 * max(count, 0)))
    try:
        check(_lib.lib().symgpu_philox_uniform(int(seed), int(first_draw), count, buf.ptr))
        return buf if out is not None else buf.download(np.float64, count) if count else np.zeros(0, dtype=np.float64)
    finally:
        if out is None:
            buf.free()


class SamplePlan:
    """Owner of a ``symgpu_sample_plan``: the radix-16 sum tree over the weights ``|a_i|^2`` of ``m`` complex128 amplitudes, resident
    until ``free()`` (also on leaving a ``with`` block, or when collected).  ``amp``: a ``DeviceBuffer``, which the plan references and
    keeps alive, or a host array, which is uploaded.  ValueError for weights that add up to zero or to something not finite."""

    def __init__(self, amp, m=None):
        self.handle, self._own = None, None
        if not isinstance(amp, DeviceBuffer):
            host = np.ascontiguousarray(amp, dtype=np.complex128).reshape(-1)
            m = host.shape[0] if m is None else int(m)
            if m < 1 or m > host.shape[0]:
                raise ValueError(f'sample: m = {m} for {host.shape[0]} amplitudes')
            amp = self._own = DeviceBuffer.upload(host)
        m = amp.nbytes // 16 if m is None else int(m)
        if m < 1 or 16 * m > amp.nbytes:
            raise ValueError(f'sample: m = {m} amplitudes do not fit the buffer of {amp.nbytes} bytes')
        self.amp, self.m = amp, m
        handle = ctypes.c_void_p()
        rc = _lib.lib().symgpu_sample_plan(amp.ptr, m, ctypes.byref(handle))
        if rc != _lib.OK and self._own is not None:
            self._own.free()
        if rc == _lib.E_NOMEM:
            raise MemoryError(_lib.last_error())
        if rc == _lib.E_INVALID:
            raise ValueError(_lib.last_error())
        check(rc)
        self.handle = handle

    def _info(self):
        total, info = ctypes.c_double(0), np.zeros(6, dtype=np.int64)
        check(_lib.lib().symgpu_sample_info(self.handle, ctypes.addressof(total), addr(info)))
        return total.value, info

    @property
    def total(self):
        """The root of the tree: the sum of the weights in the tree's order."""
        return self._info()[0]

    def info(self):
        """The six int64 words of ``symgpu_sample_info``: m, tree depth, device bytes, launches of the build, the counting form of the
        last draw, its launches."""
        return self._info()[1]

    def draw(self, n_samples, seed=0, first_draw=0, u=None, want_order=False):
        """``n_samples`` draws: ``(idx, count)``, the distinct samples ascending (int64) with their counts (int64); with ``want_order``
        ``(idx, count, order)``, ``order`` the sample of every draw.  ``u``: the caller's uniforms (float64 ``[n_samples]`` or a
        ``DeviceBuffer``) in place of the Philox stream of ``seed`` from ``first_draw`` on.  ``SYMGPU_SAMPLE_COUNT=hist|sort`` forces a
        counting form where it is legal; both give the same arrays."""
        n_samples = int(n_samples)
        with DeviceBuffer(8 * max(1, n_samples) if want_order else 8) as order:
            idx, cnt, nd = self.draw_dev(n_samples, seed, first_draw, u, order if want_order else None)
            with idx, cnt:
                if n_samples == 0:
                    return (np.zeros(0, dtype=np.int64),) * (3 if want_order else 2)
                out = (idx.download(np.int64, nd), cnt.download(np.int64, nd))
            return out + (order.download(np.int64, n_samples),) if want_order else out

    def draw_dev(self, n_samples, seed=0, first_draw=0, u=None, order=None):
        """``draw`` with the results left on the device: ``(idx, count, n_distinct)``, two ``DeviceBuffer`` of int64 that the caller
        frees.  ``order``: a ``DeviceBuffer`` of ``n_samples`` int64 that receives the sample of every draw, or None."""
        n_samples = int(n_samples)
        if not 0 <= n_samples <= SAMPLE_MAX_DRAWS:
            raise ValueError(f'sample: n_samples = {n_samples} outside 0 .. 2^31 - 1')
        cap = max(1, min(self.m, n_samples))
        own_u = None
        if u is not None and not isinstance(u, DeviceBuffer):
            u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
            if u.shape[0] != n_samples:
                raise ValueError(f'sample: {u.shape[0]} uniforms for {n_samples} draws')
            u = own_u = DeviceBuffer.upload(u) if n_samples else None
        idx, cnt = DeviceBuffer(8 * cap), DeviceBuffer(8 * cap)
        try:
            nd = c_i64(0)
            rc = _lib.lib().symgpu_sample_draw(self.handle, n_samples, int(seed), int(first_draw), None if u is None else u.ptr,
                                               None if order is None else order.ptr, idx.ptr, cnt.ptr, ctypes.addressof(nd))
            if rc == _lib.E_NOMEM:
                raise MemoryError(_lib.last_error())
            check(rc)
            return idx, cnt, nd.value
        except BaseException:
            idx.free()
            cnt.free()
            raise
        finally:
            if own_u is not None:
                own_u.free()

    def free(self):
        if self.handle is not None and self.handle.value:
            _lib.load().symgpu_sample_free(self.handle)
        self.handle = None
        if self._own is not None:
            self._own.free()
            self._own = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _qubit_mask(qubits, n_qubits, what):
    mask = 0
    for q in qubits:
        q = int(q)
        if not 0 <= q < n_qubits:
            raise ValueError(f'{what}: qubit {q} outside 0 .. {n_qubits - 1}')
        mask |= 1 << q
    return mask


def basis_change_dev(psi, n_qubits, x_qubits, y_qubits):
    """``H`` on ``x_qubits`` and ``H S^+`` on ``y_qubits`` of the ``2^n`` amplitudes in the ``DeviceBuffer`` ``psi``, in place: afterwards a
    Pauli with X on the former and Y on the latter reads as Z.  Returns the form that ran (``BASIS_DIRECT`` / ``BASIS_TILED``, 0: no qubit
    named); ``SYMGPU_BASIS_FORM=direct`` forces direct passes, the bits are the same."""
    n_qubits = int(n_qubits)
    if not 1 <= n_qubits <= 32:
        raise ValueError(f'basis_change: n_qubits = {n_qubits} outside 1 .. 32')
    if psi.nbytes < 16 << n_qubits:
        raise ValueError(f'basis_change: the buffer holds {psi.nbytes} bytes, 2^{n_qubits} amplitudes need {16 << n_qubits}')
    xm, ym = _qubit_mask(x_qubits, n_qubits, 'basis_change'), _qubit_mask(y_qubits, n_qubits, 'basis_change')
    if xm & ym:
        raise ValueError('basis_change: a qubit is named for both H and H S^+')
    form = c_int(0)
    check(_lib.lib().symgpu_basis_change(psi.ptr, n_qubits, xm, ym, ctypes.addressof(form)))
    return form.value


def counts_signed_sums(devop, n_qubits, idx, count, n_distinct=None):
    """``sum_j count_j (-1)^{|z_k & b_j|}`` for every row k of the Z-only device operator ``devop`` over the basis indices ``idx`` with the
    counts ``count`` — int64 arrays, or two ``DeviceBuffer`` (as ``SamplePlan.draw_dev`` leaves them) with ``n_distinct`` entries —:
    int64 ``[T]``, exact.  ValueError when a row has an X-part."""
    if isinstance(idx, DeviceBuffer):
        idx_buf, cnt_buf, n, own = idx, count, int(n_distinct), ()
    else:
        idx = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.int64).reshape(-1)
        assert idx.shape == count.shape
        n = idx.shape[0]
        idx_buf, cnt_buf = DeviceBuffer.upload(idx if n else np.zeros(1, np.int64)), DeviceBuffer.upload(count if n else np.zeros(1, np.int64))
        own = (idx_buf, cnt_buf)
    try:
        out = np.zeros(devop.n_terms, dtype=np.int64)
        rc = _lib.lib().symgpu_counts_signed_sums(devop.handle, int(n_qubits), idx_buf.ptr, cnt_buf.ptr, int(n), addr(out))
        if rc == _lib.E_INVALID:
            raise ValueError(_lib.last_error())
        check(rc)
        return out
    finally:
        for b in own:
            b.free()


def mem_info():
    """(free, total) bytes of the current device."""
    free_b, total_b = c_i64(0), c_i64(0)
    check(_lib.lib().symgpu_mem_info(ctypes.addressof(free_b), ctypes.addressof(total_b)))
    return free_b.value, total_b.value


# ---- PauliwordOp.from_matrix: Pauli decomposition on the device (csrc/pauli_decomp.hip) -----------------------------------------------
PAULI_ONE_PASS, PAULI_TWO_PASS = 1, 2        # SYMGPU_PAULI_ONE_PASS / SYMGPU_PAULI_TWO_PASS: the transform form a call reports


def _pauli_basis(basis_x, basis_z):
    if basis_x is None:
        return None, None, 0
    bx, bz = np.ascontiguousarray(basis_x, dtype='<u8'), np.ascontiguousarray(basis_z, dtype='<u8')
    assert bx.ndim == 1 and bx.shape == bz.shape
    return bx, bz, bx.shape[0]


def _pauli_call(fn, args, n_qubits, bx, bz, K):
    """The tail both entry points share: (DeviceOp, n_terms, form) without a basis, (complex128[K], form) with one."""
    out, n_out, form = ctypes.c_void_p(), c_i64(0), c_int(0)
    coeff = np.empty(K, dtype=np.complex128) if K else None
    rc = fn(*args, int(n_qubits), addr(bx), addr(bz), K, ctypes.byref(out), ctypes.addressof(n_out), addr(coeff), ctypes.addressof(form))
    if rc == _lib.E_NOMEM:
        raise MemoryError(f'from_matrix: {_lib.last_error()}')
    check(rc)
    if K:
        return coeff, form.value
    return DeviceOp(out), n_out.value, form.value


def pauli_decompose_dense(matrix, n_qubits, basis_x=None, basis_z=None):
    """Pauli coefficients ``c(x, z) = i^{|x & z|} 2^-n sum_b (-1)^{|b & z|} M[b, b ^ x]`` of a dense ``2^n x 2^n`` matrix (qubit 0 the most
    significant bit of b, x, z; the sum is the pinned radix-2 butterfly of ``symgpu_from_matrix_dense``).  Without a basis: a new
    DeviceOp with every coefficient that is not (+-0, +-0) in ascending (x, z) order, its term count and the transform form that ran.
    With ``basis_x`` / ``basis_z`` (uint64[K]): the K coefficients in basis order, zeros included, and the form."""
    m = np.ascontiguousarray(matrix, dtype=np.complex128)
    assert m.shape == (1 << int(n_qubits), 1 << int(n_qubits)), 'matrix must be 2^n x 2^n'
    bx, bz, K = _pauli_basis(basis_x, basis_z)
    return _pauli_call(_lib.lib().symgpu_from_matrix_dense, (addr(m),), n_qubits, bx, bz, K)


def pauli_decompose_csr(data, indices, indptr, n_qubits, basis_x=None, basis_z=None):
    """The same for a canonical CSR matrix (no duplicate entries; ``indices`` / ``indptr`` both int32 or both int64): only the
    XOR-diagonals ``row ^ col`` that hold a stored entry are transformed."""
    data = np.ascontiguousarray(data, dtype=np.complex128)
    idx_dtype = np.int64 if np.dtype(indptr.dtype).itemsize == 8 or np.dtype(indices.dtype).itemsize == 8 else np.int32
    indices, indptr = np.ascontiguousarray(indices, dtype=idx_dtype), np.ascontiguousarray(indptr, dtype=idx_dtype)
    assert indptr.shape == ((1 << int(n_qubits)) + 1,) and indices.shape == data.shape
    bx, bz, K = _pauli_basis(basis_x, basis_z)
    return _pauli_call(_lib.lib().symgpu_from_matrix_csr, (addr(data), addr(indices), addr(indptr), np.dtype(idx_dtype).itemsize, data.shape[0]),
                       n_qubits, bx, bz, K)


# ---- cleanups that also return the first-occurrence index of every output term (hash-partitioned multi-GPU cleanup, sharding.py) ----
def _first_index(op):
    t = op.n_terms
    first = np.zeros(t, dtype='<u8')
    check(_lib.lib().symgpu_op_first_index(op.handle, addr(first), t))
    return first


def mul_cleanup_indexed(inner, ci, outer, co, inner_is_left=True, zero_threshold=None):
    """Fused product + cleanup -> (rows, coeff, i_first, o_first): ``inner[i_first[t]] ^ outer[o_first[t]]`` is output row t, and
    ``o_first * Ni + i_first`` is the pair index of its first occurrence (base.py:783-792, utils.py:271)."""
    inner, outer, ci, co = _rows(inner), _rows(outer), _coeff(ci), _coeff(co)
    if inner.shape[0] == 0 or outer.shape[0] == 0:
        z = np.zeros(0, dtype=np.int64)
        return np.empty((0, inner.shape[1]), dtype='<u8'), np.empty(0, dtype=np.complex128), z, z
    with DeviceOp.upload(inner, ci) as a, DeviceOp.upload(outer, co) as b, mul_cleanup_indexed_dev(a, b, inner_is_left, zero_threshold) as res:
        rows, coeff = res.download()
        first = _first_index(res)
    return rows, coeff, (first & 0xFFFFFFFF).astype(np.int64), (first >> 32).astype(np.int64)


def cleanup_indexed(rows, coeff, zero_threshold=1e-15):
    """First-occurrence cleanup -> (rows, coeff, first): ``first[t]`` is the position of output term t's first input row."""
    rows, coeff = _rows(rows), _coeff(coeff)
    if rows.shape[0] == 0:
        return rows.copy(), coeff.copy(), np.zeros(0, dtype=np.int64)
    thr, use = _thr_args(zero_threshold)
    out = ctypes.c_void_p()
    with DeviceOp.upload(rows, coeff) as op:
        check(_lib.lib().symgpu_cleanup_indexed_dev(op.handle, thr, use, ctypes.byref(out)))
        with DeviceOp(out) as res:
            r, c = res.download()
            first = _first_index(res).astype(np.int64)
    return r, c, first


# ---- device-resident pieces of the hash-partitioned multi-GPU cleanup (csrc/partition.hip) -----------------------------------------
def op_gather(op, idx):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_op_gather(op.handle, addr(idx), idx.shape[0], ctypes.byref(out)))
    return DeviceOp(out)


def mul_cleanup_indexed_dev(inner, outer, inner_is_left=True, zero_threshold=None):
    thr, use = _thr_args(zero_threshold)
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_mul_cleanup_indexed_dev(inner.handle, outer.handle, 1 if inner_is_left else 0, thr, use, ctypes.byref(out)))
    return DeviceOp(out)


def part_global_index(part, inner_idx, outer_idx, ni_global):
    inner_idx = np.ascontiguousarray(inner_idx, dtype=np.int64); outer_idx = np.ascontiguousarray(outer_idx, dtype=np.int64)
    check(_lib.lib().symgpu_part_global_index(part.handle, addr(inner_idx), inner_idx.shape[0], addr(outer_idx), outer_idx.shape[0], int(ni_global)))


def merge_indexed_dev(parts, key_bits=0, do_cleanup=True, zero_threshold=1e-15):
    """Indexed device operators -> one, ordered by index; ``do_cleanup``: shared rows merged at their smallest index + threshold."""
    arr = (ctypes.c_void_p * len(parts))(*[p.handle for p in parts])
    thr, use = _thr_args(zero_threshold)
    out = ctypes.c_void_p()
    check(_lib.lib().symgpu_merge_indexed_dev(ctypes.addressof(arr), len(parts), int(key_bits), 1 if do_cleanup else 0, thr, use, ctypes.byref(out)))
    return DeviceOp(out)


def op_first_index(op):
    return _first_index(op)


def op_set_first_index(op, first):
    first = np.ascontiguousarray(first, dtype='<u8')
    assert first.shape[0] == op.n_terms
    check(_lib.lib().symgpu_op_set_first_index(op.handle, addr(first)))
