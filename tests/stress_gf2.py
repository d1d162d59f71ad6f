# randomised cross-check of the GF(2) elimination schedules (run on the GPU box): default against SYMGPU_GF2_FULL_PANEL=0,
# SYMGPU_GF2_FUSED_SELECT=0, SYMGPU_GF2_LOOKAHEAD=0, SYMGPU_GF2_SMALL=0 and — for small matrices — the NumPy restatement of the
# reference loop; the matrix kinds are the families of tests/_gf2_families.py (the ones tests/test_gpu_gf2_structure.py runs at fixed
# sizes), here at random sizes, densities, steps and band widths
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from symmer_amd import kernels, packing
from oracle import oracle_np as onp
import _gf2_families as fam
VARIANTS = fam.variants()
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 1
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rng = np.random.default_rng(seed)
bad = 0
t0 = time.time()
ENVS = [{}, {'SYMGPU_GF2_FUSED_SELECT': '0'}, {'SYMGPU_GF2_M4R': '0'}, {'SYMGPU_GF2_SMALL': '0'}, {'SYMGPU_GF2_FUSED_SELECT': '0', 'SYMGPU_GF2_SMALL': '0'}]
for case in range(n_cases):
    R = int(rng.choice([1, 2, 63, 64, 65, 100, 129, 300, 700, 1500, 2500]))
    C = int(rng.choice([1, 5, 64, 65, 200, 700, 3000, 9000, 16384, 16400, 30000]))
    if R * C > 3e7: C = int(3e7 // R)
    dens = float(rng.choice([0.001, 0.003, 0.02, 0.2, 0.5]))
    kind, fn, kw = VARIANTS[int(rng.integers(0, len(VARIANTS)))]
    if fn in (fam.dense, fam.low_rank, fam.identity_plus_noise): kw = dict(kw, density=max(dens, 0.02) if fn is fam.low_rank else dens)
    elif fn in (fam.staircase, fam.reverse_staircase): kw = dict(kw, step=int(rng.choice([1, 3, 67, 129, 300])))
    elif fn is fam.banded: kw = dict(kw, slope=None if rng.random() < 0.5 else kw['slope'], width=int(rng.integers(1, 40)))
    m = fn(rng, R, C, **kw)
    packed = packing.pack_bits(m)
    outs = []
    for env in ENVS:
        for k in ('SYMGPU_GF2_FUSED_SELECT', 'SYMGPU_GF2_M4R', 'SYMGPU_GF2_SMALL'): os.environ.pop(k, None)
        os.environ.update(env)
        outs.append(kernels.rref(packed, want_pivots=True))
    ok = all(np.array_equal(outs[0][0], o[0]) and outs[0][1] == o[1] and np.array_equal(outs[0][2], o[2]) for o in outs[1:])
    why = '' if ok else 'GPU schedules differ'
    if R * C <= 2e6:
        ered, ecnt = onp.rref_noswap(m, count_xors=True)
        if not (np.array_equal(packing.unpack_bits(outs[0][0], C), ered) and outs[0][1] == ecnt):
            ok = False; why += ' oracle differs'
    if not ok:
        bad += 1
        print(f'MISMATCH case {case}: R={R} C={C} kind={kind} dens={dens}: {why}', flush=True)
print(f'stress gf2: {n_cases} cases, {bad} mismatches, {time.time()-t0:.1f} s')
sys.exit(1 if bad else 0)
