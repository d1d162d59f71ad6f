"""GPU: the radix sort and the two scans that cleanups, rotations and matrix conversions stand on (csrc/sort.hip), run directly through
symgpu_debug_sort / symgpu_debug_scan / symgpu_debug_popc_scan on device buffers, against NumPy, with no tolerance.

Sort: the expected order is np.argsort((keys >> begin_bit) & mask, kind='stable') applied to keys and values — stability is what makes
the reference's `np.add.at` order come out of a cleanup, and here it is asserted on the sort itself.  The sizes are the smallest at which
each mechanism can go wrong: the wavefront and tile edges, 9 tiles (the XCD-contiguous tile order has a short last eighth and idle
workgroups), 17 tiles (two column-scan chunks: the ticket path), and both sides of every threshold between the one launch and the launches
per step.  Which form ran is asserted in every case against the rule restated in `expected_form`.

The give-up path of the one-launch form's barrier is not exercised: that would need workgroups that are not co-resident.  If the form has
been switched off in this process (symgpu_degraded says so), a case that expects it is skipped, not failed."""
import ctypes

import numpy as np
import pytest

from symmer_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 4096
SIZES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 32769, 65537, 131072, 131073, 196608, 196609, 524288, 524289)
RANGES = ((0, 8), (16, 32), (40, 64))              # one pass / an even pass count (result in the input buffer) / an odd one (in the temporary)
LAUNCHES, ONE_IF_FITS, ONE_WHERE_PAYS = 0, 1, 2
FORM_CASES = ((LAUNCHES, False), (LAUNCHES, True), (ONE_IF_FITS, False), (ONE_WHERE_PAYS, False), (ONE_WHERE_PAYS, True))   # (form, with_first_hist)
FAMILIES = ('uniform', 'eight_distinct', 'all_equal', 'all_ones', 'descending', 'equal_inside_range')


def expected_form(n, with_vals, form, first_hist):
    """1: all passes in one launch, 0: a launch per step — the library's rule, restated"""
    if form == LAUNCHES or first_hist:
        return 0
    limit = 128 if form == ONE_IF_FITS else (32 if with_vals else 48)
    return 1 if (n + TILE - 1) // TILE <= limit else 0


class Dev:
    """a device buffer holding a copy of a NumPy array"""

    def __init__(self, arr):
        self.dtype, self.n = arr.dtype, arr.size
        self.p = ctypes.c_void_p()
        _lib.check(_lib.lib().symgpu_dev_alloc(max(arr.nbytes, 16), ctypes.byref(self.p)))
        self.upload(arr)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.size == self.n
        if arr.nbytes:
            _lib.check(_lib.lib().symgpu_dev_upload(self.p, arr.ctypes.data, arr.nbytes))

    def download(self):
        out = np.empty(self.n, dtype=self.dtype)
        if out.nbytes:
            _lib.check(_lib.lib().symgpu_dev_download(self.p, out.ctypes.data, out.nbytes))
        return out

    def free(self):
        _lib.lib().symgpu_dev_free(self.p)


def sort_switched_off():
    return any('one-launch radix sort' in d for d in _lib.degraded())


def make_keys(family, n, begin, end, rng):
    u = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if family == 'uniform':
        return u
    if family == 'eight_distinct':
        return rng.integers(0, 1 << 64, 8, dtype=np.uint64)[rng.integers(0, 8, n)]
    if family == 'all_equal':
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if family == 'all_ones':
        return np.full(n, ~np.uint64(0), dtype=np.uint64)       # the filler of the invalid lanes, here as data
    if family == 'descending':
        k = np.sort(u)[::-1].copy()
        assert np.all(k[:-1] > k[1:])
        return k
    assert family == 'equal_inside_range'
    inside = np.uint64(((1 << (end - begin)) - 1) << begin)
    return (u & ~inside) | (np.uint64(0x5A5A5A5A5A5A5A5A) & inside)


def stable_order(keys, begin, end):
    digits = (keys >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)
    return np.argsort(digits, kind='stable')


def run_sorts(family, n, with_vals, seed):
    """every bit range x every form of one (family, size, keys alone / with values); returns the number of one-launch cases skipped"""
    lib = _lib.lib()
    rng = np.random.default_rng(seed)
    skipped = 0
    dk = dv = None
    try:
        for begin, end in RANGES:
            keys = make_keys(family, n, begin, end, rng)
            vals = np.arange(n, dtype=np.uint32) if family != 'uniform' else rng.integers(0, 1 << 32, n, dtype=np.uint32)
            order = stable_order(keys, begin, end)
            if family == 'equal_inside_range':
                assert np.array_equal(order, np.arange(n))              # nothing to order by: the input order comes back
            want_k, want_v = keys[order], vals[order]
            if dk is None:
                dk = Dev(keys)
                dv = Dev(vals) if with_vals else None
            for form, first_hist in FORM_CASES:
                dk.upload(keys)
                if with_vals:
                    dv.upload(vals)
                ran = ctypes.c_int(-1)
                rc = lib.symgpu_debug_sort(dk.p, dv.p if with_vals else None, n, begin, end, form, int(first_hist), ctypes.addressof(ran))
                what = f'{family} n={n} bits [{begin}, {end}) form {form} first_hist={first_hist} vals={with_vals}'
                expect_form = expected_form(n, with_vals, form, first_hist)
                if expect_form == 1 and sort_switched_off() and (rc != _lib.OK or ran.value == 0):
                    skipped += 1                                        # the one launch gave up earlier in this process (or just now)
                    if rc != _lib.OK:
                        continue
                else:
                    _lib.check(rc)
                    assert ran.value == expect_form, f'{what}: form {ran.value} ran'
                assert np.array_equal(dk.download(), want_k), f'{what}: keys'
                if with_vals:
                    assert np.array_equal(dv.download(), want_v), f'{what}: values'
    finally:
        for d in (dk, dv):
            if d is not None:
                d.free()
    return skipped


@pytest.mark.parametrize('with_vals', [False, True], ids=['keys', 'pairs'])
@pytest.mark.parametrize('n', SIZES)
def test_sort_sizes(n, with_vals):
    skipped = run_sorts('uniform', n, with_vals, seed=1000 + n)
    if skipped:
        pytest.skip(f'{skipped} one-launch cases: the form is switched off in this process ({_lib.degraded()})')


@pytest.mark.parametrize('with_vals', [False, True], ids=['keys', 'pairs'])
@pytest.mark.parametrize('n', (65, 4097, 32769, 65537))
@pytest.mark.parametrize('family', FAMILIES[1:])
def test_sort_families(family, n, with_vals):
    skipped = run_sorts(family, n, with_vals, seed=2000 + n)
    if skipped:
        pytest.skip(f'{skipped} one-launch cases: the form is switched off in this process ({_lib.degraded()})')


def test_expected_form_at_the_thresholds():
    """the restated rule puts each pair of SIZES on the two sides of a threshold: one launch at the first size, launches at the second"""
    for form, with_vals, last in ((ONE_WHERE_PAYS, True, 131072), (ONE_WHERE_PAYS, False, 196608), (ONE_IF_FITS, False, 524288), (ONE_IF_FITS, True, 524288)):
        assert last in SIZES and last + 1 in SIZES
        assert expected_form(last, with_vals, form, False) == 1 and expected_form(last + 1, with_vals, form, False) == 0
        assert expected_form(last, with_vals, form, True) == 0 and expected_form(last, with_vals, LAUNCHES, False) == 0


# ---- exclusive scan ------------------------------------------------------------------------------------------------
_scan_inputs = {}


def scan_case(n):
    """(input, exclusive prefix, total) in uint32, built once per size and never written"""
    if n not in _scan_inputs:
        a = np.random.default_rng(3000 + n).integers(0, 512, n, dtype=np.uint32)         # below 512: no sum reaches 2^32
        incl = np.cumsum(a, dtype=np.uint32)
        excl = np.concatenate([np.zeros(1, np.uint32), incl[:-1]]) if n else incl
        for x in (a, excl):
            x.setflags(write=False)
        _scan_inputs[n] = (a, excl, int(incl[-1]) if n else 0)
    return _scan_inputs[n]


def run_scan(n, in_place, with_total):
    a, excl, total = scan_case(n)
    din, dout, dtot = Dev(a), None, None
    try:
        dout = din if in_place else Dev(np.full(n, 0xDEADBEEF, dtype=np.uint32))
        dtot = Dev(np.full(1, 0xDEADBEEF, dtype=np.uint32)) if with_total else None
        _lib.check(_lib.lib().symgpu_debug_scan(din.p, dout.p, n, dtot.p if with_total else None))
        assert np.array_equal(dout.download(), excl)
        if not in_place:
            assert np.array_equal(din.download(), a)
        if with_total:
            assert int(dtot.download()[0]) == total
    finally:
        for d in {id(d): d for d in (din, dout, dtot) if d is not None}.values():
            d.free()


@pytest.mark.parametrize('with_total', [False, True], ids=['no_total', 'total'])
@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('n', (0, 1, 2047, 2048, 2049, 8388608, 8388609))     # the last workgroup count of the two-launch form, the first of the recursive one
def test_scan(n, in_place, with_total, monkeypatch):
    monkeypatch.delenv('SYMGPU_SCAN_RECURSIVE', raising=False)
    run_scan(n, in_place, with_total)


@pytest.mark.parametrize('with_total', [False, True], ids=['no_total', 'total'])
@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('n', (2049, 4194305))                                  # two / three levels of the recursion
def test_scan_recursive_form(n, in_place, with_total, monkeypatch):
    monkeypatch.setenv('SYMGPU_SCAN_RECURSIVE', '1')                            # read per call by exclusive_scan_u32
    run_scan(n, in_place, with_total)


# ---- population-count scan of a bitmap -----------------------------------------------------------------------------
@pytest.mark.parametrize('n32_kind', ['none', 'even', 'odd'])
@pytest.mark.parametrize('n', (1, 8191, 8192))
def test_popc_scan(n, n32_kind):
    bits = np.random.default_rng(4000 + n).integers(0, 1 << 64, n, dtype=np.uint64)
    n32 = {'none': -1, 'even': 2 * n, 'odd': 2 * n - 1}[n32_kind]
    counted = bits.copy()
    if n32_kind == 'odd':
        bits[-1] |= np.uint64(0xFFFFFFFF00000000)                                # the unwritten half, full of ones ...
        counted[-1] &= np.uint64(0xFFFFFFFF)                                     # ... is not counted
    cnt = np.unpackbits(counted.view(np.uint8)).reshape(n, 64).sum(axis=1).astype(np.uint32)
    incl = np.cumsum(cnt, dtype=np.uint32)
    excl = np.concatenate([np.zeros(1, np.uint32), incl[:-1]])
    dbits, dout, dtot = Dev(bits), Dev(np.full(n, 0xDEADBEEF, dtype=np.uint32)), Dev(np.full(1, 0xDEADBEEF, dtype=np.uint32))
    try:
        _lib.check(_lib.lib().symgpu_debug_popc_scan(dbits.p, n, n32, dout.p, dtot.p))
        assert np.array_equal(dout.download(), excl)
        total = int(dtot.download()[0])
        assert total == int(incl[-1])
        if n32_kind == 'odd':
            with_upper = int(np.unpackbits(bits.view(np.uint8)).sum())
            assert with_upper == total + 32                                      # the 32 ones of the upper half were left out
    finally:
        for d in (dbits, dout, dtot):
            d.free()
