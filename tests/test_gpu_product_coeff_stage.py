"""GPU: the coefficient stage of the phase-sum product path (product.hip k_mul_rows_e + k_mul_coeff_expand), bit-exact against the C
oracle.  The row kernel leaves the 2-bit phase sum of every pair, four pairs to a byte; the expansion writes one 256-term piece of one
outer row per workgroup.  The shapes below end packed bytes and 256-term pieces part-full, cut the inner operand into tiles, need more
outer rows than one launch's grid.y holds, and write a slab with o_begin > 0 into an output handle that already holds another slab.
The slab and grid.y cases also run with the switches that select the other paths of the product (word-major or wide coefficient kernel
followed by the plain row stream, rows only): each path has its own o_begin and batch-offset arithmetic; which path served a call is read from
the counters PRODUCT_* (one per ProductPath, bumped at the switch of symgpu_mul_allpairs_dev)."""

import numpy as np
import pytest
from symmer_amd import kernels, packing, _lib
from symmer_amd.kernels import DeviceOp
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu

# qubits -> 16-byte chunks per row Wq = 1, 2, 4, 8, 16, 32, 64: every row length the phase-sum path serves
QUBITS = [40, 100, 250, 500, 1000, 2000, 4090]


def dyadic(rng, t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 16.0


def gaussian(rng, t):
    return rng.standard_normal(t) + 1j * rng.standard_normal(t)


PATHS = ('rows only', 'phase stream', 'wide coefficients, then rows', 'word-major coefficients, then rows', 'word-major coefficients beside rows')
PATH_COUNTERS = ('PRODUCT_ROWS_ONLY', 'PRODUCT_PHASE_STREAM', 'PRODUCT_WIDE_COEFF_THEN_ROWS', 'PRODUCT_WORD_MAJOR_THEN_ROWS', 'PRODUCT_WORD_MAJOR_BESIDE_ROWS')
ROWS_ONLY, PHASE_STREAM, WIDE, WORD_MAJOR = 0, 1, 2, 3


def path_counters():
    return kernels.counters(PATH_COUNTERS)


def counted(call, path, what, calls=1):
    """Run `call` and assert that it went through symgpu_mul_allpairs_dev `calls` times, on the path `path` every time."""
    before = path_counters()
    out = call()
    delta = (path_counters() - before).tolist()
    assert delta == [calls if k == path else 0 for k in range(5)], f'{what}: expected [{PATHS[path]}] x {calls}, took {dict((PATHS[k], d) for k, d in enumerate(delta) if d)}'
    return out


def check_pairs(rng, n, Ni, No, left):
    a = packing.pack_rows(rng.random((Ni, 2 * n)) < 0.3); b = packing.pack_rows(rng.random((No, 2 * n)) < 0.3)
    erows = None
    for coeffs in (dyadic, gaussian):
        ca, cb = coeffs(rng, Ni), coeffs(rng, No)
        rows, coeff = kernels.mul_allpairs(a, ca, b, cb, left)
        er, ec = oc.mul_allpairs(a, ca, b, cb, left)
        if erows is None:
            assert np.array_equal(rows, er)
            erows = er
        assert np.array_equal(coeff, ec), (n, Ni, No, left, coeffs.__name__)


@pytest.mark.parametrize('left', [True, False])
@pytest.mark.parametrize('n', QUBITS)
def test_coeff_stage_ragged_shapes(n, left, monkeypatch):
    monkeypatch.setenv('SYMGPU_PRODUCT_FUSED', '1')
    rng = np.random.default_rng(1000 + n + left)
    for Ni in (1, 3, 5, 255, 257, 1025):
        for No in (1, 3):
            check_pairs(rng, n, Ni, No, left)


@pytest.mark.parametrize('n', QUBITS)
def test_coeff_stage_inner_tiles(n, monkeypatch):
    """SYMGPU_PRODUCT_TILE_MB=0.3: several inner tiles, the last one ragged; every tile is its own pair of launches."""
    monkeypatch.setenv('SYMGPU_PRODUCT_FUSED', '1')
    monkeypatch.setenv('SYMGPU_PRODUCT_TILE_MB', '0.3')
    wq = (n + 63) // 64
    Ni = 3 * (19661 // wq) + 257
    check_pairs(np.random.default_rng(1100 + n), n, Ni, 3, n % 2 == 0)


@pytest.mark.parametrize('fused', ['1', '0'])
def test_coeff_stage_more_outer_rows_than_one_grid(fused, monkeypatch):
    """70,000 outer rows: more than the 65,535 of one launch's grid.y, so the slab goes out in two launches of each kernel (fused = 0: of
    the plain row stream, behind the word-major coefficient kernel)."""
    monkeypatch.setenv('SYMGPU_PRODUCT_FUSED', fused)
    counted(lambda: check_pairs(np.random.default_rng(1200), 20, 3, 70000, True), PHASE_STREAM if fused == '1' else WORD_MAJOR, f'fused={fused}', calls=2)


# the paths of symgpu_mul_allpairs_dev by environment: phase-byte stream where the row length allows it / word-major coefficient kernel +
# plain row stream / wide coefficient kernel + plain row stream
PATH_ENVS = [{}, {'SYMGPU_PRODUCT_FUSED': '0'}, {'SYMGPU_PRODUCT_FUSED': '0', 'SYMGPU_WIDE': '1'}]


@pytest.mark.parametrize('env', PATH_ENVS, ids=['default', 'fused0', 'fused0-wide1'])
@pytest.mark.parametrize('n,Ni', [(1000, 257), (40, 1025), (4090, 5), (300, 257)])
def test_coeff_stage_slab_into_reused_handle(n, Ni, env, monkeypatch):
    """A slab [o_begin, o_end) with o_begin > 0 written into an output handle that already holds a longer slab of the same product; the
    same slabs into a handle without coefficients (rows only).  n = 300 is 5 chunks per row: the word-major path even in the default environment."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(1300 + n + Ni)
    No = 9
    a = packing.pack_rows(rng.random((Ni, 2 * n)) < 0.3); b = packing.pack_rows(rng.random((No, 2 * n)) < 0.3)
    ca, cb = gaussian(rng, Ni), gaussian(rng, No)
    A, B = DeviceOp.upload(a, ca), DeviceOp.upload(b, cb)
    out = DeviceOp.alloc(No * Ni, (n + 63) // 64, with_coeff=True)
    out_rows = DeviceOp.alloc(No * Ni, (n + 63) // 64, with_coeff=False)
    lib = _lib.lib()
    # the path of the calls with coefficients: the phase-byte stream serves a power-of-two number of chunks per row (n = 300 is 5 chunks: word-major)
    if not env:
        path = WORD_MAJOR if n == 300 else PHASE_STREAM
    else:
        path = WIDE if env.get('SYMGPU_WIDE') == '1' else WORD_MAJOR
    try:
        for o0, o1 in ((0, No), (4, 7), (8, 9)):
            counted(lambda: _lib.check(lib.symgpu_mul_allpairs_dev(A.handle, B.handle, o0, o1, 1, out.handle)), path, (n, Ni, o0, o1))
            assert out.n_terms == (o1 - o0) * Ni
            rows, coeff = out.download()
            er, ec = oc.mul_allpairs(a, ca, b[o0:o1], cb[o0:o1], True)
            assert np.array_equal(rows, er) and np.array_equal(coeff, ec), (o0, o1)
            counted(lambda: _lib.check(lib.symgpu_mul_allpairs_dev(A.handle, B.handle, o0, o1, 1, out_rows.handle)), ROWS_ONLY, (n, Ni, o0, o1, 'rows only'))
            assert out_rows.n_terms == (o1 - o0) * Ni
            assert np.array_equal(out_rows.download(with_coeff=False), er), (o0, o1, 'rows only')
    finally:
        for h in (A, B, out, out_rows):
            h.free()
