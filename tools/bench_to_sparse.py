"""PauliwordOp.to_sparse_matrix on the device: the C-ABI call split into count (symgpu_to_csr_count: grouping, count pass, scan), fill
(symgpu_to_csr_fill minus its download) and download (symgpu_dev_download of the same number of bytes), the Python property, and a NumPy
baseline (the per-term loop of tests/_sparse_oracle.py), at the shapes of DESIGN §3.9.  Operators are synthetic and chemistry-like: a
third of the terms Z-only, the rest spread over a few hundred X-parts.  Kernel times belong to `rocprofv3 --kernel-trace --stats`; this
tool prints wall times of the calls, the output bytes per second of fill + count against the fill probe of the same run, one JSON line
per shape.  `fill_ms` is the fill call minus a separately timed download of as many bytes: a host-side estimate that can even come out
negative when the two downloads run at different rates; the fill kernel's own time comes from the profiler.

    python tools/bench_to_sparse.py [--reps 3] [--shapes 12:631,14:1086,16:3000,20:10000] [--numpy-max-n 16] [--scratch]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

from symmer_amd import PauliwordOp, _lib, kernels
import _sparse_oracle as so


def chemistry_like(n, T, x_parts=300, seed=0):
    rng = np.random.default_rng(seed)
    xs = rng.random((x_parts, n)) < 0.3
    x = xs[rng.integers(0, x_parts, T)]
    x[: T // 3] = False
    z = rng.random((T, n)) < 0.4
    return np.hstack([x, z]), rng.normal(size=T) + 1j * rng.normal(size=T)


def time_c_abi(dev, n):
    lib = _lib.lib()
    nnz_c, scratch_c, plan = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p()
    t0 = time.perf_counter()
    _lib.check(lib.symgpu_to_csr_count(dev.handle, n, ctypes.addressof(nnz_c), ctypes.addressof(scratch_c), ctypes.byref(plan)))
    t1 = time.perf_counter()
    nnz = nnz_c.value
    ib = np.dtype(kernels.csr_index_dtype(nnz, n)).itemsize
    data = np.empty(nnz, np.complex128); idx = np.empty(nnz, kernels.csr_index_dtype(nnz, n))
    ptr = np.empty((1 << n) + 1, kernels.csr_index_dtype(nnz, n))
    data.fill(0); idx.fill(0); ptr.fill(0)                                   # pages touched: the download is not timing page faults
    t2 = time.perf_counter()
    _lib.check(lib.symgpu_to_csr_fill(plan, data.ctypes.data, idx.ctypes.data, ptr.ctypes.data, ib))
    t3 = time.perf_counter()
    nbytes = nnz * (16 + ib) + ptr.nbytes
    buf = ctypes.c_void_p()
    _lib.check(lib.symgpu_dev_alloc(max(nbytes, 16), ctypes.byref(buf)))
    host = np.empty(max(nbytes, 16), np.uint8); host.fill(0)
    t4 = time.perf_counter()
    _lib.check(lib.symgpu_dev_download(buf, host.ctypes.data, nbytes))
    t5 = time.perf_counter()
    lib.symgpu_dev_free(buf)
    return nnz, ib, t1 - t0, (t3 - t2) - (t5 - t4), t5 - t4, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='12:631,14:1086,16:3000,20:10000')
    ap.add_argument('--numpy-max-n', type=int, default=16, help='larger shapes: the NumPy loop is timed on its first 200 terms and scaled')
    ap.add_argument('--scratch', action='store_true', help='force the global-scratch fill (SYMGPU_CSR_SCRATCH=1)')
    a = ap.parse_args()
    if a.scratch:
        os.environ['SYMGPU_CSR_SCRATCH'] = '1'
    _lib.init(0)
    lib = _lib.lib()
    fill_probe, copy_probe = ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(lib.symgpu_membw_probe(4 << 30, ctypes.addressof(fill_probe), ctypes.addressof(copy_probe)))
    for shape in a.shapes.split(','):
        n, T = (int(v) for v in shape.split(':'))
        symp, c = chemistry_like(n, T, seed=n)
        op = PauliwordOp(symp, c)
        dev = op._device()
        D = len(np.unique(so.bits_to_int(symp[:, :n])))
        best = None
        for _ in range(a.reps):
            r = time_c_abi(dev, n)
            best = r if best is None or r[2] + r[3] < best[2] + best[3] else best
        nnz, ib, t_count, t_fill, t_dl, nbytes = best
        t_prop = []
        for _ in range(a.reps):
            fresh = PauliwordOp(symp, c)
            fresh._device()
            t0 = time.perf_counter(); fresh.to_sparse_matrix; t_prop.append(time.perf_counter() - t0)
            del fresh
        if n <= a.numpy_max_n:
            t0 = time.perf_counter(); so.to_csr(symp, c); t_np, np_note = time.perf_counter() - t0, 'measured'
        else:
            k = 200
            t0 = time.perf_counter(); so.to_csr(symp[:k], c[:k]); t_np, np_note = (time.perf_counter() - t0) * T / k, f'first {k} terms, scaled'
        out = dict(n=n, T=T, D=D, nnz=nnz, index_bytes=ib, out_bytes=nbytes, count_ms=t_count * 1e3, fill_ms=t_fill * 1e3,
                   download_ms=t_dl * 1e3, property_ms=min(t_prop) * 1e3, numpy_ms=t_np * 1e3, numpy_note=np_note,
                   out_GBps_fill_plus_count=nbytes / max(t_fill + t_count, 1e-9) / 1e9, fill_probe_GBps=fill_probe.value,
                   scratch=bool(a.scratch))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
