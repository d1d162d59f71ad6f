"""GPU: the sums of csrc/lanczos.hip (symgpu_lanczos_step, symgpu_vec_combine) and csrc/ansatz.hip (the energy, the reverse sweep, the pool
gradient) against the ORDER include/symgpu.h states for them, restated in tests/_reduction_oracle.py: the device's scalars and vectors
are compared for equality, not within a bound.  H is one Pauli string with the coefficient 0.5, so H v is exact (asserted) and the
comparison does not rest on the rounding of the product.  Sizes (units = slots for the sweep, elements elsewhere): 1 and 16 units below
a workgroup, 256 one full chunk, 512 two chunks, 2^18 the last size with one unit per thread (1024 chunks of 256), 2^19 the first with
two (C = 512), 2^20 four (C = 1024).  tests/test_reduction_oracle.py shows on the CPU that the inputs of the two largest sizes give
other values in three other orders, and that every expected gradient component is at least 1e-3 in magnitude.
Dyadic inputs at 2^19 and 2^20 elements: every sum is exact in any order, so the device must give the integer result.
The pool is walked in slices of 32768 rows: one full slice, and one full slice and five rows."""
import itertools

import numpy as np
import pytest

import _ansatz_oracle as ao
import _matvec_oracle as mo
import _reduction_oracle as ro
from symmer_amd import kernels, packing
from test_gpu_ansatz import bits, device_energy_grad, device_pool_gradient, upload_rows
from test_gpu_ansatz import plans_and_buffers_are_balanced  # noqa: F401 — the module-scoped DEV_BLOCKS_LIVE balance, autouse here too
from test_gpu_exact_gs import number_operator

pytestmark = pytest.mark.gpu


def product_is_exact(h_symp, h_coeff, v):
    """The premise: H v of the oracle is 0.5 (P v) element by element, nothing rounded."""
    (x,), (z,), (y,) = ao.gens_of(h_symp)
    assert h_symp.shape[0] == 1 and h_coeff[0] == 0.5
    return np.array_equal(mo.matvec(h_symp, h_coeff, v), 0.5 * ao.apply_pauli(x, z, y, v))


# ---- energy, prepared state and sweep gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ro.SWEEP_SIZES)
def test_energy_and_sweep_gradient_in_the_stated_order(n, monkeypatch):
    h_symp, h_coeff, gens, theta, ref = ro.sweep_inputs(n)
    K = gens.shape[0]
    psi = ao.state(gens, theta, ref)
    assert product_is_exact(h_symp, h_coeff, psi)
    want_e, want_g = ro.energy_ordered(h_symp, h_coeff, psi), ro.sweep_grad_ordered(h_symp, h_coeff, gens, theta, ref)
    assert K == (2 if n == 21 else 4) and np.abs(want_g).min() >= ro.MIN_GRADIENT, want_g
    runs = [seg[3] for seg in ao.plan_runs(gens)]
    if n >= 14 and K == 4:
        assert runs == [True, False, True]                  # a direct pass between two tiled runs
    with upload_rows(gens) as op, kernels.AnsatzPlan(op, n) as plan:
        assert plan.info()[:3] == (n, K, sum(runs))
    for form in ('default', 'direct'):
        if form == 'direct':
            monkeypatch.setenv('SYMGPU_ANSATZ_FORM', 'direct')
        e, g, out = device_energy_grad(h_symp, h_coeff, gens, theta, ref, want_psi=True)
        print(f'n={n} {form}: E = {e!r} (ordered {want_e!r}), g = {g} (ordered {want_g})')
        assert np.array_equal(bits(out), bits(psi)), f'{form}: psi_out is not the state of the rotations'
        assert e == want_e, f'{form}: E = {e!r}, in the stated order {want_e!r}'
        assert np.array_equal(g, want_g), f'{form}: g = {g}, in the stated order {want_g}, differing at k = {np.flatnonzero(g != want_g)}'
    monkeypatch.delenv('SYMGPU_ANSATZ_FORM')
    e, g, _ = device_energy_grad(h_symp, h_coeff, gens, theta, ref, want_grad=False)
    assert g is None and e == want_e


# ---- pool gradient and energy on the prepared state ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ro.ELEMENT_SIZES)
def test_pool_gradient_in_the_stated_order(n):
    h_symp, h_coeff, pool, psi = ro.pool_inputs(n)
    assert product_is_exact(h_symp, h_coeff, psi)
    want_g, want_e = ro.pool_grad_ordered(h_symp, h_coeff, pool, psi), ro.energy_ordered(h_symp, h_coeff, psi)
    assert want_g.shape == (4,) and np.abs(want_g).min() >= ro.MIN_GRADIENT, want_g
    g, e = device_pool_gradient(h_symp, h_coeff, pool, psi, want_energy=True)
    print(f'n={n}: E = {e!r} (ordered {want_e!r}), g = {g} (ordered {want_g})')
    assert e == want_e, f'E = {e!r}, in the stated order {want_e!r}'
    assert np.array_equal(g, want_g), f'g = {g}, in the stated order {want_g}, differing at j = {np.flatnonzero(g != want_g)}'


# ---- Lanczos steps and the Ritz combination --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True], ids=['no_mask', 'sector_mask'])
@pytest.mark.parametrize('n', ro.ELEMENT_SIZES)
def test_lanczos_steps_and_combination_in_the_stated_order(n, masked):
    side, cap = 1 << n, 3
    h_symp, h_coeff = ro.symp_of([ro.masked_h_string(n) if masked else ro.h_string(n)]), ro.H_COEFF
    Nop = number_operator(n)
    with kernels.DeviceOp.upload(packing.pack_rows(h_symp), h_coeff.astype(complex)) as op, kernels.MatvecPlan(op, n) as plan, \
            kernels.DeviceOp.upload(packing.pack_rows(Nop.symp_matrix), np.asarray(Nop.coeff_vec, dtype=complex)) as nop, \
            kernels.MatvecPlan(nop, n) as plan_n, kernels.DeviceBuffer(side) as keep, kernels.DeviceBuffer(cap * side * 16) as basis, \
            kernels.DeviceBuffer(side * 16) as out:
        mask = None
        if masked:
            kept = plan_n.sector_mask(n // 2, keep)
            mask = keep.download(np.uint8, side).astype(bool)
            assert np.array_equal(mask, ro.particle_sector(n)) and kept == int(mask.sum()) >= 3
        basis.write(np.zeros(cap * side, dtype=np.complex128))
        basis.write(ro.lanczos_start(n, mask))
        for j in range(2):
            alpha, beta = plan.lanczos_step(keep if masked else None, basis, cap, j)
            V = basis.download(np.complex128, (j + 2) * side).reshape(j + 2, side)        # the DEVICE's slots 0 .. j: each step judged alone
            assert product_is_exact(h_symp, h_coeff, V[j])
            want_alpha, want_beta, want_next = ro.lanczos_step_ordered(h_symp, h_coeff, mask, V[:j + 1], j)
            print(f'n={n} j={j}: alpha = {alpha!r} (ordered {want_alpha!r}), beta = {beta!r} (ordered {want_beta!r})')
            assert alpha == want_alpha, f'j = {j}: alpha = {alpha!r}, in the stated order {want_alpha!r}'
            assert beta == want_beta, f'j = {j}: beta = {beta!r}, in the stated order {want_beta!r}'
            assert beta > 0.0 and np.array_equal(V[j + 1], want_next), f'j = {j}: slot {j + 1} differs in {np.count_nonzero(V[j + 1] != want_next)} elements'
            if masked:
                assert not V[j + 1][~mask].any()
        s = np.random.default_rng(n).standard_normal(cap)
        V = basis.download(np.complex128, cap * side).reshape(cap, side)
        kernels.vec_combine(basis, cap, n, s, out=out)
        assert np.array_equal(out.download(np.complex128, side), ro.combine_ordered(V, s)), 'the combination into a buffer'
        kernels.vec_combine(basis, cap, n, s, normalise=True)
        after = basis.download(np.complex128, cap * side).reshape(cap, side)
        assert np.array_equal(after[0], ro.combine_ordered(V, s, normalise=True)), 'the normalised combination into slot 0'
        assert np.array_equal(bits(after[1:]), bits(V[1:])), 'the combination into slot 0 changed another slot'


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ro.LARGE_ELEMENT)
def test_dyadic_inputs_give_the_integer_result(n):
    (h_symp, h_coeff), pool, v = ro.dyadic_operator(n), ro.dyadic_pool(n), ro.dyadic_vector(n)
    want_e, want_g = ro.integer_results(h_symp, h_coeff, pool, v)
    assert h_symp.shape[0] == 12 and pool.shape[0] == 6 and want_e != 0 and np.all(want_g != 0)
    g, e = device_pool_gradient(h_symp, h_coeff, pool, v, want_energy=True)
    assert e == want_e, f'pool_gradient: E = {e!r}, exactly {want_e!r}'
    assert np.array_equal(g, want_g), f'pool_gradient: g = {g}, exactly {want_g}'
    # theta = 0: no rotation changes psi or lambda, and the sweep's t_k (summed by slot) is the pool's sum (by element) of the same string
    e, g, out = device_energy_grad(h_symp, h_coeff, pool, np.zeros(6), v, want_psi=True)
    assert np.array_equal(out, v) and e == want_e, f'energy_grad: E = {e!r}, exactly {want_e!r}'
    assert np.array_equal(g, want_g), f'energy_grad at theta = 0: g = {g}, exactly {want_g}'
    with kernels.DeviceOp.upload(packing.pack_rows(h_symp), h_coeff.astype(complex)) as op, kernels.MatvecPlan(op, n) as plan, \
            kernels.DeviceBuffer.upload(v) as basis:
        alpha, _ = plan.lanczos_step(None, basis, 1, 0)                               # on the un-normalised vector: <v|H|v> itself
        assert alpha == want_e, f'lanczos_step: alpha = {alpha!r}, exactly {want_e!r}'


# ---- the pool in slices of 32768 rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [32768, 32768 + 5])
def test_pool_slices(M):
    n = 4
    strings = [''.join(s) for s in itertools.product('IXYZ', repeat=n)]              # the identity and the 255 others
    assert len(set(strings)) == 256 and strings[0] == 'I' * n
    distinct = ro.symp_of(strings)
    h_symp, h_coeff = ro.symp_of([ro.h_string(n)]), ro.H_COEFF
    psi = ro.unit(ro.gaussian(np.random.default_rng(4), 1 << n))
    assert product_is_exact(h_symp, h_coeff, psi)
    each = ro.pool_grad_ordered(h_symp, h_coeff, distinct, psi)
    assert np.count_nonzero(np.abs(each) >= ro.MIN_GRADIENT) >= 100                    # the strings that do not commute with H
    named = (32767, 32768, 32772)                                                      # the last row of the first slice, the first two of the second
    shift = next(k for k in range(256) if all(ro.anticommute(strings[(r + k) % 256], ro.h_string(n)) for r in named))
    row = (np.arange(M) + shift) % 256                                                # the named rows hold strings that do not commute with H
    want = each[row]
    assert len(set(row[:256])) == 256 and all(abs(each[(r + shift) % 256]) >= ro.MIN_GRADIENT for r in named)
    got, e = device_pool_gradient(h_symp, h_coeff, distinct[row], psi, want_energy=True)
    assert got.shape == (M,) and e == ro.energy_ordered(h_symp, h_coeff, psi)
    for r in named:
        if r < M:
            assert got[r] == want[r], f'row {r} ({strings[row[r]]}): {got[r]!r}, in the stated order {want[r]!r}'
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f'{wrong.size} rows differ, the first at {wrong[:8]}'
