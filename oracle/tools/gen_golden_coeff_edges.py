"""Generate ``tests/golden/coeff_edges.npz`` by RUNNING THE REFERENCE (imported through ``ref_shim``): cleanups, products and
single-Pauli rotations whose coefficients sit where the keep rule ``np.abs(c) > threshold`` (utils.py:275-278) is fragile.

BUILD CONTAINER ONLY (needs the reference).  Data only: seeded inputs and the reference's outputs.
Run:  python oracle/tools/gen_golden_coeff_edges.py        (the output is byte-identical from run to run)

Coefficient families (planted among ordinary dyadic terms, as single terms and as the first or last member of a merged segment):
  boundary  |c| exactly thr, one to four ulp on either side of it, one component exactly thr beside 0 or a subnormal, both components
            near thr / sqrt(2), and values where libm's hypot and NumPy's complex abs fall on different sides of thr;
  zeros     +0, -0, mixed signs, and segments that merge to zero;
  magnitude subnormal coefficients, and products that underflow to a subnormal or to 0;
  nonfinite NaN in re or im beside a component above or below thr, +-inf, merges that form inf - inf, and sums that overflow.
Each case carries ``exact``: whether the device's product rule gives NumPy's bits for every product the operation forms.  The device
forms the plain, unfused complex product and applies the phase exactly; NumPy's complex multiply on x86-64 contracts with FMA
(re = fma(ar, br, -(ai*bi)), im = fma(ar, bi, ai*br)) and multiplies by the phase, cos and -1j*sin as complex numbers.
The two agree for finite factors whose products the FMA does not round differently — planted values are dyadic, or one factor is real or
imaginary — and a few general products (Gaussian coefficients, ``family`` 'inexact') show where they do not: there ``exact`` is False
and the tests compare the device with the C oracle, which states its rule.  A cleanup forms no product: ``exact`` is True.
"""
import io, os, sys, warnings, zipfile
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: F401
warnings.simplefilter('ignore')
import numpy as np
from symmer.operators import PauliwordOp
from symmer.operators.utils import symplectic_cleanup

OUT = os.path.join(HERE, '..', '..', 'tests', 'golden', 'coeff_edges.npz')
rng = np.random.default_rng(8128)
cases, k = {}, 0
KIND = {'cleanup': 0, 'mul': 1, 'rotate': 2}
TINY = 5e-324


def add(**arrays):
    global k
    for key, val in arrays.items():
        a = np.asarray(val)
        cases[f'{k:04d}/{key}'] = a.astype(np.uint8) if a.dtype == bool else a
    k += 1


def save(path, arrays):
    """np.savez without the wall-clock time stamps of its zip entries: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            arr = io.BytesIO()
            np.lib.format.write_array(arr, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, arr.getvalue())
    with open(path, 'wb') as f:
        f.write(buf.getvalue())


def cabs(re, im):
    return float(np.abs(np.array([complex(re, im)]))[0])


def ulps(x, n):
    for _ in range(abs(n)):
        x = float(np.nextafter(x, np.inf if n > 0 else -np.inf))
    return x


def boundary(thr):
    """coefficients with |c| at and around thr, as NumPy's abs forms it"""
    out = [complex(thr, 0.0), complex(0.0, -thr), complex(-thr, TINY), complex(TINY, thr), complex(thr, -0.0)]
    out += [complex(ulps(thr, d), 0.0) for d in (-4, -2, -1, 1, 2, 4)]
    out += [complex(-0.0, ulps(thr, d)) for d in (-1, 1)]
    by_offset, split = {}, []
    x0 = thr / np.sqrt(2.0)
    for i in range(-12, 13):
        for j in range(-12, 13):
            re, im = ulps(x0, i), ulps(x0, j)
            a = cabs(re, im)
            off = 0 if a == thr else int(np.sign(a - thr)) * int(round(abs(a - thr) / np.spacing(thr)))
            if -4 <= off <= 4:
                by_offset.setdefault(off, complex(re, -im) if (i + j) % 2 else complex(-re, im))
            if (np.hypot(re, im) > thr) != (a > thr) and len(split) < 4:
                split.append(complex(re, im))
    t = 0
    while len(split) < 8 and t < 20000:                       # anywhere on the circle |c| = thr: libm hypot against NumPy's abs
        t += 1
        th = rng.random() * np.pi / 2
        re, im = ulps(thr * np.cos(th), int(rng.integers(-3, 4))), ulps(thr * np.sin(th), int(rng.integers(-3, 4)))
        if (np.hypot(re, im) > thr) != (cabs(re, im) > thr):
            split.append(complex(re, im))
    return out + [by_offset[o] for o in sorted(by_offset)] + split


ZEROS = [complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)]
MAGNITUDE = [complex(TINY, 0.0), complex(TINY, TINY), complex(-TINY, 0.0), complex(2.2e-308, 1e-310), complex(1e-310, -3e-320),
             complex(1.5e-323, -0.0)]


def nonfinite(thr):
    big, small = max(2.0 * thr, 5.0), thr / 8.0 if thr > 0 else 0.0
    nan, inf = np.nan, np.inf
    return [complex(nan, big), complex(big, nan), complex(nan, small), complex(small, nan), complex(inf, 0.0), complex(-inf, nan),
            complex(nan, -inf), complex(inf, -inf), complex(nan, nan), complex(0.0, inf), complex(-inf, small)]


def dyadic(t):
    return (rng.integers(-8, 9, t) + 1j * rng.integers(-8, 9, t)) / 16.0


def distinct_rows(t, n):
    while True:
        r = rng.random((t, 2 * n)) < 0.4
        if np.unique(r, axis=0).shape[0] == t:
            return r


def planted(edges, n, merges=()):
    """rows + coefficients: every edge value as a single term, as the first and as the last member of a two-term segment, among
    ordinary dyadic terms; `merges`: lists of coefficients that land on one row, in that order.  Shuffled."""
    m = len(edges)
    n_rows = 3 * m + len(merges) + 12
    base = distinct_rows(n_rows, n)
    rows, coeff = [], []
    for e, c in enumerate(edges):
        rows += [base[e], base[m + e], base[m + e], base[2 * m + e], base[2 * m + e]]
        coeff += [c, c, dyadic(1)[0], dyadic(1)[0], c]
    for s, seg in enumerate(merges):
        rows += [base[3 * m + s]] * len(seg); coeff += list(seg)
    rows += list(base[3 * m + len(merges):]); coeff += list(dyadic(12))
    order = rng.permutation(len(rows))
    return np.array(rows)[order], np.array(coeff, dtype=complex)[order]


def family_values(thr):
    fams = {'boundary': boundary(thr) if thr is not None and thr > 0 else [],
            'zeros': ZEROS, 'magnitude': MAGNITUDE, 'nonfinite': nonfinite(thr if thr is not None else 1.0)}
    merges = {'boundary': [], 'nonfinite': [[complex(np.inf, 1.0), complex(-np.inf, 1.0)], [complex(1.0, np.inf), complex(2.0, 0.0)],
                                             [complex(1e308, 0.0), complex(1e308, 0.0)], [complex(np.nan, 0.0), complex(1.0, 1.0)],
                                             [complex(2.0, -1.0), complex(np.nan, 0.0)], [complex(np.inf, 0.0), complex(np.nan, 3.0)]],
              'zeros': [[complex(0.5, -0.25), complex(-0.5, 0.25)], [complex(-0.0, 0.0), complex(0.0, -0.0)], [complex(-0.0, -0.0)] * 2],
              'magnitude': [[complex(TINY, 0.0), complex(TINY, 0.0)], [complex(TINY, -TINY), complex(-TINY, TINY)]]}
    if thr is not None and thr > 0:                                # a segment whose members are below thr and whose sum is at it / above it
        merges['boundary'] = [[complex(thr / 2, 0.0), complex(thr / 2, 0.0)], [complex(thr / 2, 0.0), complex(ulps(thr / 2, 1), 0.0)],
                              [complex(0.0, thr), complex(0.0, -0.0)]]
    return fams, merges


def exact_products(ca, cb):
    """finite factors, finite products, and NumPy's product (FMA) equal to the plain one for every pair"""
    with np.errstate(all='ignore'):
        p = np.outer(ca, cb)
        ar, ai, br, bi = ca.real[:, None], ca.imag[:, None], cb.real[None, :], cb.imag[None, :]
        plain = (ar * br - ai * bi) + 1j * (ar * bi + ai * br)
    finite = np.all(np.isfinite(ca)) and np.all(np.isfinite(cb)) and np.all(np.isfinite(p))
    return bool(finite and np.array_equal(p.real, plain.real) and np.array_equal(p.imag, plain.imag))


# ---- cleanup: symplectic_cleanup with and without a threshold ----------------------------------------------------------------------
for thr in (1e-15, 1e-18, 0.25, 1.0, 0.0, None):
    fams, merges = family_values(thr)
    for fam in ('boundary', 'zeros', 'magnitude', 'nonfinite'):
        if not fams[fam] and not merges[fam]:
            continue
        n = int(rng.choice([17, 40, 70]))
        symp, coeff = planted(fams[fam], n, merges[fam])
        if thr is None:
            rs, rc = symplectic_cleanup(symp, coeff)
        else:
            rs, rc = symplectic_cleanup(symp, coeff, zero_threshold=thr)
        add(kind=KIND['cleanup'], family=fam, has_thr=thr is not None, thr=0.0 if thr is None else thr, in_symp=symp, in_coeff=coeff,
            out_symp=rs, out_coeff=np.asarray(rc, dtype=complex), exact=True)

# ---- products: P * Q (general) and P * P ---------------------------------------------------------------------------------------------
for thr in (1e-15, 0.25):
    fams, _ = family_values(thr)
    for fam in ('boundary', 'zeros', 'magnitude', 'nonfinite'):
        n = int(rng.choice([9, 33]))
        edges = fams[fam] or ZEROS
        A_s = distinct_rows(len(edges) + 6, n)
        A_c = np.hstack([edges, dyadic(6)])
        for nb, bc in ((1, [1.0]), (3, [0.5, -1j, 2.0]), (5, dyadic(5))):
            if fam == 'magnitude':
                bc = [1e-160, 0.5e-160j, 1e-170, 1.0, -2.0][:nb]         # subnormal products, products that underflow to 0
            B_s = distinct_rows(nb, n)
            P, Q = PauliwordOp(A_s, A_c), PauliwordOp(B_s, bc)
            R = P._multiply_by_operator(Q, zero_threshold=thr)
            add(kind=KIND['mul'], family=fam, has_thr=True, thr=thr, in_symp=A_s, in_coeff=A_c, b_symp=B_s,
                b_coeff=np.asarray(bc, dtype=complex), out_symp=R.symp_matrix, out_coeff=np.asarray(R.coeff_vec, dtype=complex),
                exact=exact_products(A_c, np.asarray(bc, dtype=complex)))
        if fam in ('boundary', 'zeros'):                               # P * P: dyadic values, |c_i c_j| and twin sums at the threshold
            vals = np.array([0.5, 0.5j, -0.5, 0.25 + 0.25j, 0.75, 0.125, -0.25j, 1.0, 0.0, -0.0, 0.5 - 0.5j, 0.375j])
            t = int(rng.integers(8, 13))
            S = distinct_rows(t, n)
            c = vals[rng.integers(0, vals.size, t)]
            P = PauliwordOp(S, c)
            for pthr in (0.25, 0.125, 1e-15):
                R = P._multiply_by_operator(P, zero_threshold=pthr)
                add(kind=KIND['mul'], family='squared', has_thr=True, thr=pthr, in_symp=S, in_coeff=c, b_symp=S, b_coeff=c,
                    out_symp=R.symp_matrix, out_coeff=np.asarray(R.coeff_vec, dtype=complex), exact=exact_products(c, c))

    # general coefficients: NumPy's FMA product and the plain one differ in the last bit of many pairs
    n = 12
    A_s, B_s = distinct_rows(10, n), distinct_rows(4, n)
    A_c = rng.standard_normal(10) + 1j * rng.standard_normal(10)
    B_c = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    R = PauliwordOp(A_s, A_c)._multiply_by_operator(PauliwordOp(B_s, B_c), zero_threshold=thr)
    add(kind=KIND['mul'], family='inexact', has_thr=True, thr=thr, in_symp=A_s, in_coeff=A_c, b_symp=B_s, b_coeff=B_c,
        out_symp=R.symp_matrix, out_coeff=np.asarray(R.coeff_vec, dtype=complex), exact=exact_products(A_c, B_c))

# ---- rotations: _rotate_by_single_Pword, Clifford and not, 0-d ndarray angles, angles at the Clifford-detection threshold -----------
half = np.pi / 2
angles = [half, -half, np.pi, 3 * half, -3 * half, 2 * np.pi, 0.0, -0.0, 0.3, -1.1, half * 1e-18, half * 0.9e-18, half * 2e-18,
          -half * 1e-18, -half * 2e-18, 1e-18, -1e-18]
for trial, ang in enumerate(angles):
    n = int((5, 33, 70)[trial % 3])
    thr = 1e-15
    if trial % 2 == 0:                                               # coefficients at the cleanup threshold after the cos / sin scaling
        c0, s0 = abs(np.cos(ang)), abs(np.sin(ang))
        edges = boundary(thr)[:10]
        if c0 > 1e-3:
            edges += [complex(ulps(thr / c0, d), 0.0) for d in (-2, -1, 0, 1, 2)]
        if s0 > 1e-3:
            edges += [complex(0.0, ulps(thr / s0, d)) for d in (-2, -1, 0, 1, 2)]
        fam = 'boundary'
    elif trial % 4 == 1:
        edges, fam = ZEROS + MAGNITUDE, 'magnitude'
    else:
        edges, fam = nonfinite(thr), 'nonfinite'
    symp, coeff = planted(edges, n)
    q = rng.random(2 * n) < 0.45
    q[0] = True
    P, Q = PauliwordOp(symp, coeff), PauliwordOp(q.reshape(1, -1), [1])
    R = P._rotate_by_single_Pword(Q, np.array(ang))                   # a 0-d ndarray angle, as a caller may pass one
    add(kind=KIND['rotate'], family=fam, has_thr=True, thr=thr, in_symp=symp, in_coeff=coeff, q=q, angle=float(ang),
        out_symp=R.symp_matrix, out_coeff=np.asarray(R.coeff_vec, dtype=complex), same_object=np.array(R is P),
        exact=bool(np.all(np.isfinite(coeff))))          # cos, sin, -1j and the phase: one partial product of each component is 0

cases['n_cases'] = np.array(k)
save(OUT, cases)
print('coeff_edges:', k, 'cases,', os.path.getsize(OUT), 'bytes')
