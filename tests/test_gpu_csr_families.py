"""PauliwordOp.to_sparse_matrix on the device (csrc/sparse_matrix.hip) on the families of tests/_csr_families.py: every case with int32
and with int64 indices, in the fill form the library chooses and in the forced global-scratch form, bit for bit against the NumPy
restatement (tests/_sparse_oracle.py); which form ran, and in how many launches, through the counters CSR_FILL_LDS / CSR_FILL_SCRATCH and the scratch
size that the count call reports.  tests/test_csr_families.py proves what each family is."""
import ctypes
import functools

import numpy as np
import pytest

import _csr_families as fam
import _sparse_oracle as so
from symmer_amd import PauliwordOp, kernels, _lib

pytestmark = pytest.mark.gpu

FILL_COUNTERS = ('CSR_FILL_LDS', 'CSR_FILL_SCRATCH')     # launches of k_csr_fill by form

BUILDERS = {'x_parts': fam.x_part_set, 'tiles': fam.term_tiles, 'large_n': fam.large_n, 'coeff': fam.coeff_kind}
CASES = ([('x_parts', D) for D in fam.X_PART_COUNTS] + [('tiles', T) for T in sorted(fam.TERM_TILE_SIZES)]
         + [('large_n', n) for n in fam.LARGE_N] + [('coeff', k) for k in fam.COEFF_KINDS])


@functools.lru_cache(maxsize=None)
def case(family, arg):
    """(symp, coeff, facts, the restatement's CSR): built once, shared, never written to."""
    symp, c, facts = BUILDERS[family](arg)
    with np.errstate(invalid='ignore'):                       # inf - inf inside a group is part of the 'nonfinite' case
        want = so.to_csr(symp, c)
    for a in (symp, c) + want:
        a.setflags(write=False)
    return symp, c, facts, want


def fill_scratch_bytes(op, n):
    """The count call's report of the fill's scratch (0: the slots stay in LDS); the plan is released unused."""
    nnz, scratch, plan = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p()
    _lib.check(_lib.lib().symgpu_to_csr_count(op._device().handle, n, ctypes.addressof(nnz), ctypes.addressof(scratch), ctypes.byref(plan)))
    _lib.check(_lib.lib().symgpu_to_csr_fill(plan, None, None, None, 4))
    return scratch.value


def assert_bit_equal(got, want, dtype):
    d, i, p = got
    wd, wi, wp = want
    assert i.dtype == np.dtype(dtype) and p.dtype == np.dtype(dtype) and d.dtype == np.complex128
    assert np.array_equal(p, wp), 'indptr'
    assert np.array_equal(i, wi), 'indices'
    g, w = d.view(np.float64), wd.view(np.float64)
    nan = np.isnan(w)                                         # a NaN equals a NaN (in the same component); payloads are not compared
    assert np.all(np.isnan(g[nan])), 'a NaN of the restatement is not a NaN here'
    assert np.array_equal(g.view(np.uint64)[~nan], w.view(np.uint64)[~nan]), 'data not bit-equal'


def expected_launches(op, facts, forced_scratch):
    """(launches in LDS, launches in scratch, scratch bytes > 0) by the restated arithmetic of csr_fill_form."""
    n, D = facts['n'], facts['D']
    if not forced_scratch and fam.fill_form(D, 1 << n) is not None:
        assert -(-(1 << n) // fam.fill_form(D, 1 << n)[0]) < 1 << 22         # one launch holds every workgroup
        return 1, 0, 0
    scratch = fill_scratch_bytes(op, n)
    per_launch = scratch // (256 * D * fam.SLOT_BYTES)                      # workgroups of 256 rows per launch
    assert scratch > 0 and scratch == per_launch * 256 * D * fam.SLOT_BYTES
    workgroups = -(-(1 << n) // 256)
    return 0, -(-workgroups // per_launch), scratch


def run(op, facts, dtype):
    before = kernels.counters(FILL_COUNTERS)
    got = kernels.to_csr(op._device(), facts['n'], index_dtype=dtype)
    return got, tuple((kernels.counters(FILL_COUNTERS) - before).tolist())


# ---- every family, both index widths, both forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize('family, arg', CASES, ids=[f'{f}-{a}' for f, a in CASES])
def test_family_matches_the_restatement(monkeypatch, family, arg):
    symp, c, facts, want = case(family, arg)
    n, D = facts['n'], facts['D']
    assert len(np.unique(fam.x_ints(symp))) == D
    op = PauliwordOp(symp.copy(), c.copy())
    monkeypatch.delenv('SYMGPU_CSR_SCRATCH_MIB', raising=False)
    for forced in (False, True):
        if forced:
            monkeypatch.setenv('SYMGPU_CSR_SCRATCH', '1')
        else:
            monkeypatch.delenv('SYMGPU_CSR_SCRATCH', raising=False)
        lds, scr, scratch = expected_launches(op, facts, forced)
        if not forced:
            assert (scratch == 0) == (D <= 115) == facts.get('lds', True), 'the library did not choose the form that D implies'
            assert fill_scratch_bytes(op, n) == scratch
        for dtype in (np.int32, np.int64):
            got, moved = run(op, facts, dtype)
            assert moved == (lds, scr), f'launches (LDS, scratch) = {moved}, expected {(lds, scr)}'
            assert_bit_equal(got, want, dtype)
    assert not any('k_csr_fill' in t for t in _lib.degraded())


def test_default_index_dtype_is_unchanged():
    symp, c, facts, want = case('coeff', 'dyadic')
    op = PauliwordOp(symp.copy(), c.copy())
    assert_bit_equal(kernels.to_csr(op._device(), facts['n']), want, np.int32)
    assert_bit_equal(kernels.to_csr(op._device(), facts['n'], None), want, np.int32)
    A = op.to_sparse_matrix
    assert A.indices.dtype == np.int32 and A.indptr.dtype == np.int32
    assert_bit_equal((A.data, A.indices, A.indptr), want, np.int32)
    with pytest.raises(ValueError):
        kernels.to_csr(op._device(), facts['n'], index_dtype=np.uint32)


# ---- the fill in several launches ----------------------------------------------------------------------------------------------------
def test_fill_in_several_launches(monkeypatch):
    """n = 19, D = 2 (the two X-parts of the large-n family without its I + Z pair): 2^11 workgroups of 256 rows.  One MiB of scratch
    holds 102 of them, the floor of four workgroups per compute unit more: the fill takes ceil(2^11 / c) >= 2 launches, and every
    launch after the first reads its rows at block0 + blockIdx.x and its slots at blockIdx.x."""
    n = 19
    full, c_full, _ = fam.large_n(n)
    keep = fam.x_ints(full) != 0
    symp, c = full[keep], c_full[keep]
    D = len(np.unique(fam.x_ints(symp)))
    assert D == 2 and len(c) == 4
    facts = {'n': n, 'D': D}
    want = so.to_csr(symp, c)
    op = PauliwordOp(symp, c)
    monkeypatch.setenv('SYMGPU_CSR_SCRATCH', '1')
    monkeypatch.delenv('SYMGPU_CSR_SCRATCH_MIB', raising=False)
    assert expected_launches(op, facts, True)[:2] == (0, 1)
    whole, moved = run(op, facts, np.int32)
    assert moved == (0, 1)
    monkeypatch.setenv('SYMGPU_CSR_SCRATCH_MIB', '1')
    per_launch = fill_scratch_bytes(op, n) // (256 * D * fam.SLOT_BYTES)
    launches = -(-(1 << 11) // per_launch)
    assert per_launch >= (1 << 20) // (256 * D * fam.SLOT_BYTES) and launches >= 2, (per_launch, launches)
    for dtype in (np.int32, np.int64):
        got, moved = run(op, facts, dtype)
        assert moved == (0, launches)
        assert_bit_equal(got, want, dtype)
        assert all(np.array_equal(a, b) for a, b in zip(got, whole)), 'the chunked fill differs from the fill in one launch'
    # the limit acts on the scratch form only: the LDS form has no scratch to limit
    monkeypatch.delenv('SYMGPU_CSR_SCRATCH')
    assert fill_scratch_bytes(op, n) == 0
    got, moved = run(op, facts, np.int32)
    assert moved == (1, 0)
    assert_bit_equal(got, want, np.int32)


# ---- the refusal in kernels.to_csr ------------------------------------------------------------------------------------------------------
def test_memory_refusal_releases_the_plan(monkeypatch):
    symp, c, facts, want = case('x_parts', 20)
    op = PauliwordOp(symp.copy(), c.copy())
    dev = op._device()
    monkeypatch.setattr(kernels, '_host_available_bytes', lambda: 1)
    before = kernels.counters(FILL_COUNTERS)
    for dtype in (None, np.int64):
        with pytest.raises(MemoryError, match='on the host'):
            kernels.to_csr(dev, facts['n'], index_dtype=dtype)
    assert np.array_equal(kernels.counters(FILL_COUNTERS), before), 'a refused call launched its fill'
    monkeypatch.undo()
    assert_bit_equal(kernels.to_csr(dev, facts['n']), want, np.int32)
    assert_bit_equal(kernels.to_csr(dev, facts['n'], index_dtype=np.int64), want, np.int64)
