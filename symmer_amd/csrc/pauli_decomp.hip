// pauli_decomp.hip — PauliwordOp.from_matrix (reference base.py:239-425): the Pauli decomposition of a 2^n x 2^n matrix, the inverse of
// sparse_matrix.hip, with its conventions (qubit 0 the MOST significant bit of a row / column index b and of x, z):
//   d_x[b]  = M[b, b ^ x]                                  the x-th XOR-diagonal
//   c(x, z) = i^{|x & z| mod 4} 2^-n WHT(d_x)[z],          WHT(d)[z] = sum_b (-1)^{|b & z|} d[b]
// Plan, one PdPlan per call, then stages that decide nothing:
//   1. diagonals: the sorted list xs[0..D) of the x values that are decomposed — all 2^n (dense, no basis), the distinct X-parts of the
//      basis (dense), or the distinct row ^ col of the stored entries (CSR; radix sort + head flags + scan on the device), intersected
//      with the basis's X-parts.
//   2. gather: scratch[j][b] = M[b, b ^ xs[j]], complex128 [D][2^n].  Dense: 32 x 32 tiles through LDS — for b and x in aligned
//      blocks of 32 the columns b ^ x fill one aligned block of 32, so the matrix is read and the scratch written in 512-byte runs.
//      CSR: scratch zeroed, every entry scattered to (rank(row ^ col), row).
//   3. transform: the radix-2 butterfly, stage s = 0 .. n-1 on index bit s, a' = a + b, b' = a - b (a: bit clear), per component in
//      fp64, three stages per LDS round trip in registers (the same additions in the same order).  ONE PASS: tiles of 2^L contiguous
//      slots in LDS (several rows per tile when n < L).  TWO PASS: bits [0, tile_bits) that way, the bits above them in strided tiles
//      (2^k values of the bits x 8 consecutive slots = full 128-byte lines), k <= L - 3 bits per launch.
//   4. select: c = i^{|x & z|} (2^-n v) (both exact).  No basis: keep what is not (+-0, +-0) (NaN, inf stay), compact in slot order
//      = ascending (x, z) into a new operator.  Basis: c(x_k, z_k) for the K terms in basis order, zeros included.
// Every form performs the same additions in the same order: all results are bit-reproducible.
#include "common.h"
#include "sort.h"
#include "block_scan.h"
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace symgpu {

constexpr int PD_TILE_MIN = 8;                    // the LDS index swizzle permutes within blocks of 256 slots
constexpr int PD_TILE_LDS = 13;                   // 2^13 complex128 = 128 KiB of the 160 KiB
constexpr int PD_TILE_STATIC = 12;                // 64 KiB: what a kernel may use without the attribute
constexpr int PD_CHUNK_BITS = 3;                  // strided tiles: 8 consecutive slots (128 B) per value of the transformed bits
constexpr int PD_SEL = 1024;                      // slots per workgroup of the select stage
constexpr u32 PD_BAD_INDEX = 1u, PD_BAD_INDPTR = 2u;

struct PdXBlock { u32 x0, first_rank, mask; u32 pad; };   // an aligned block of 32 x values: which are listed, and the rank of the first

// ---- 2. gather ---------------------------------------------------------------------------------------------------------------------
// grid (b-blocks, x-blocks); tile[r][c] = M[b0 + r][(b0 ^ x0) + c]; scratch[rank(x0 + xj)][b0 + r] = tile[r][r ^ xj].  The transposed
// read is conflict-free: a row of the tile is 512 B = two bank rows, and the 16 lanes of a ds_read_b128 group hold 16 distinct r mod 16.
__global__ __launch_bounds__(256) void k_pd_gather_dense(const f64x2 *__restrict__ M, int n, int tb, const PdXBlock *__restrict__ blocks,
                                                         f64x2 *__restrict__ scratch) {
    __shared__ f64x2 tile[32 * 32];
    const int TS = 1 << tb;
    const size_t N = (size_t)1 << n;
    PdXBlock xb;
    if (blocks) xb = blocks[blockIdx.y];
    else { xb.x0 = blockIdx.y << tb; xb.first_rank = xb.x0; xb.mask = TS == 32 ? 0xffffffffu : ((1u << TS) - 1u); }
    const size_t b0 = (size_t)blockIdx.x << tb;
    const size_t c0 = b0 ^ xb.x0;
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int r = i >> tb, c = i & (TS - 1);
        tile[r * TS + c] = M[(b0 + r) * N + c0 + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TS * TS; i += 256) {
        const int xj = i >> tb, r = i & (TS - 1);
        if ((xb.mask >> xj) & 1u) {
            const size_t rank = xb.first_rank + __popc(xb.mask & ((1u << xj) - 1u));
            scratch[rank * N + b0 + r] = tile[r * TS + (r ^ xj)];
        }
    }
}

// CSR: per stored entry its row (the last row whose indptr is <= e) and key row ^ col; bad column indices raise a flag
template <typename IDX>
__global__ __launch_bounds__(256) void k_pd_csr_keys(const IDX *__restrict__ indices, const IDX *__restrict__ indptr, i64 nnz, int n,
                                                     u64 *__restrict__ key, u32 *__restrict__ row_of, u32 *__restrict__ flags) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const i64 N = (i64)1 << n;
    i64 lo = 0, hi = N;                                   // first row r in [0, N) with indptr[r + 1] > e
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if ((i64)indptr[mid + 1] <= e) lo = mid + 1; else hi = mid;
    }
    const i64 row = lo < N ? lo : N - 1;
    const i64 col = (i64)indices[e];
    if (col < 0 || col >= N) atomicOr(flags, PD_BAD_INDEX);
    row_of[e] = (u32)row;
    key[e] = (u64)(row ^ col) & (u64)(N - 1);
}

template <typename IDX>
__global__ __launch_bounds__(256) void k_pd_csr_check_indptr(const IDX *__restrict__ indptr, i64 nnz, int n, u32 *__restrict__ flags) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 N = (i64)1 << n;
    if (r > N) return;
    const i64 v = (i64)indptr[r];
    bool bad = v < 0 || v > nnz || (r == 0 && v != 0) || (r == N && v != nnz);
    if (r < N && (i64)indptr[r + 1] < v) bad = true;
    if (bad) atomicOr(flags, PD_BAD_INDPTR);
}

// sorted keys -> 1 at the first of every run of equal keys (that the basis lists, when there is one)
__global__ __launch_bounds__(256) void k_pd_heads(const u64 *__restrict__ key, i64 T, const u64 *__restrict__ basis_xs, i64 Db, u32 *__restrict__ head) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= T) return;
    bool h = s == 0 || key[s] != key[s - 1];
    if (h && basis_xs) {
        const i64 p = lower_bound(basis_xs, Db, key[s]);
        h = p < Db && basis_xs[p] == key[s];
    }
    head[s] = h ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_pd_compact_xs(const u64 *__restrict__ key, const u32 *__restrict__ head, const u32 *__restrict__ excl, i64 T,
                                                       u64 *__restrict__ xs) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s < T && head[s]) xs[excl[s]] = key[s];
}

template <typename IDX>
__global__ __launch_bounds__(256) void k_pd_scatter(const f64x2 *__restrict__ data, const IDX *__restrict__ indices, const u32 *__restrict__ row_of, i64 nnz,
                                                    int n, const u64 *__restrict__ xs, i64 D, f64x2 *__restrict__ scratch) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const u64 N = (u64)1 << n;
    const u64 row = row_of[e];
    const u64 key = (row ^ (u64)indices[e]) & (N - 1);
    const i64 j = lower_bound(xs, D, key);
    if (j < D && xs[j] == key) scratch[(size_t)j * N + row] = data[e];
}

// ---- 3. transform ------------------------------------------------------------------------------------------------------------------
// LDS slot of tile index i (re and im in two planes of doubles, read and written with 8-byte accesses): bits 0-2 take bits 5-7, bits
// 3-4 take bits 6-7.  The 32 lanes of a half-wave then hit 32 distinct slots mod 32 (= all 64 banks of a ds_read_b64) in every round:
// round 0 (lanes over bits 3-7), round 1 (bits 0-2, 6-7), later rounds and the global load / store phases (bits 0-4).
__device__ __forceinline__ u32 pd_slot(u32 i) { return i ^ ((i >> 5) & 7u) ^ (((i >> 6) & 3u) << 3); }

// Butterfly stages on tile bits [lo, lo + nb) of a tile of 2^L slots already in LDS, up to three stages per round in registers.
__device__ __forceinline__ void pd_tile_butterfly(double *__restrict__ re, double *__restrict__ im, int L, int lo, int nb) {
    for (int p = lo; p < lo + nb; p += 3) {
        const int kk = lo + nb - p < 3 ? lo + nb - p : 3;
        const u32 groups = 1u << (L - kk), lowmask = (1u << p) - 1u;
        __syncthreads();
        for (u32 g = threadIdx.x; g < groups; g += blockDim.x) {
            const u32 base = (g & lowmask) | ((g >> p) << (p + kk));
            double vr[8], vi[8];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < (1 << kk)) {
                    const u32 s = pd_slot(base + ((u32)r << p));
                    vr[r] = re[s];
                    vi[r] = im[s];
                }
#pragma unroll
            for (int st = 0; st < 3; ++st)
                if (st < kk) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (!(r & (1 << st)) && r < (1 << kk)) {
                            const int q = r | (1 << st);
                            const double ar = vr[r], ai = vi[r], br = vr[q], bi = vi[q];
                            vr[r] = ar + br; vi[r] = ai + bi;
                            vr[q] = ar - br; vi[q] = ai - bi;
                        }
                }
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < (1 << kk)) {
                    const u32 s = pd_slot(base + ((u32)r << p));
                    re[s] = vr[r];
                    im[s] = vi[r];
                }
        }
    }
    __syncthreads();
}

// Contiguous tiles: slots [tile << L, (tile + 1) << L) of the flat scratch (`total` slots), stages on bits [0, nb), nb <= L.
__global__ __launch_bounds__(1024) void k_pd_wht_tile(f64x2 *__restrict__ scratch, u64 total, int L, int nb) {
    extern __shared__ __align__(16) double pd_lds[];
    const u32 S = 1u << (L < PD_TILE_MIN ? PD_TILE_MIN : L);
    double *re = pd_lds, *im = pd_lds + S;
    const u64 base = (u64)blockIdx.x << L;
    for (u32 l = threadIdx.x; l < (1u << L); l += blockDim.x) {
        const f64x2 v = base + l < total ? scratch[base + l] : f64x2{0.0, 0.0};
        const u32 s = pd_slot(l);
        re[s] = v.x;
        im[s] = v.y;
    }
    pd_tile_butterfly(re, im, L, 0, nb);
    for (u32 l = threadIdx.x; l < (1u << L); l += blockDim.x)
        if (base + l < total) {
            const u32 s = pd_slot(l);
            scratch[base + l] = f64x2{re[s], im[s]};
        }
}

// Strided tiles: stages on bits [s, s + k) of the flat slot index; a tile holds, for one value of the bits above s + k and one run of 8
// consecutive values below s (s >= 3), all 2^k values of the bits between: tile index = (bits value << 3) | position in the run.
__global__ __launch_bounds__(1024) void k_pd_wht_strided(f64x2 *__restrict__ scratch, int s, int k) {
    extern __shared__ __align__(16) double pd_lds[];
    const int L = k + PD_CHUNK_BITS;
    const u32 S = 1u << (L < PD_TILE_MIN ? PD_TILE_MIN : L);
    double *re = pd_lds, *im = pd_lds + S;
    const u64 w = blockIdx.x;
    const u64 run = w & (((u64)1 << (s - PD_CHUNK_BITS)) - 1), hi = w >> (s - PD_CHUNK_BITS);
    const u64 base = (hi << (s + k)) | (run << PD_CHUNK_BITS);
    for (u32 l = threadIdx.x; l < (1u << L); l += blockDim.x) {
        const f64x2 v = scratch[base + ((u64)(l >> PD_CHUNK_BITS) << s) + (l & 7u)];
        const u32 sl = pd_slot(l);
        re[sl] = v.x;
        im[sl] = v.y;
    }
    pd_tile_butterfly(re, im, L, PD_CHUNK_BITS, k);
    for (u32 l = threadIdx.x; l < (1u << L); l += blockDim.x) {
        const u32 sl = pd_slot(l);
        scratch[base + ((u64)(l >> PD_CHUNK_BITS) << s) + (l & 7u)] = f64x2{re[sl], im[sl]};
    }
}

// ---- 4. select ---------------------------------------------------------------------------------------------------------------------
// the coefficient of slot (x, z): i^{|x & z|} (2^-n v), both steps exact
__device__ __forceinline__ f64x2 pd_coefficient(f64x2 v, u64 x, u64 z, double scale) {
    double re, im;
    apply_phase(v.x * scale, v.y * scale, __popcll(x & z) & 3, re, im);
    return f64x2{re, im};
}
__device__ __forceinline__ bool pd_kept(f64x2 c) { return !(c.x == 0.0 && c.y == 0.0); }

struct PdSlots {
    const f64x2 *scratch;
    const u64 *xs;        // null: x = the row index itself (all diagonals)
    u64 total;            // D * 2^n
    int n;
    double scale;
};

__device__ __forceinline__ bool pd_slot_value(const PdSlots &P, u64 i, u64 *x, u64 *z, f64x2 *c) {
    if (i >= P.total) return false;
    const u64 j = i >> P.n;
    *z = i & (((u64)1 << P.n) - 1);
    *x = P.xs ? P.xs[j] : j;
    *c = pd_coefficient(P.scratch[i], *x, *z, P.scale);
    return pd_kept(*c);
}

__global__ __launch_bounds__(256) void k_pd_count(PdSlots P, u32 *__restrict__ counts) {
    __shared__ u32 s_wave[4];
    const u64 base = (u64)blockIdx.x * PD_SEL;
    u32 cnt = 0;
    for (int j = 0; j < PD_SEL / 256; ++j) {
        u64 x, z;
        f64x2 c;
        cnt += pd_slot_value(P, base + j * 256 + threadIdx.x, &x, &z, &c) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// kept slots of block b land at excl[b] + their position in the block, in slot order: row = [bit-reversed x, bit-reversed z] (Wq = 1)
__global__ __launch_bounds__(256) void k_pd_emit(PdSlots P, const u32 *__restrict__ excl, u64 T, u64 *__restrict__ rows, f64x2 *__restrict__ coeff) {
    __shared__ u32 s_wave[4];
    const u64 base = (u64)blockIdx.x * PD_SEL;
    u64 out = excl[blockIdx.x];
    for (int j = 0; j < PD_SEL / 256; ++j) {
        u64 x = 0, z = 0;
        f64x2 c = {0.0, 0.0};
        const bool keep = pd_slot_value(P, base + j * 256 + threadIdx.x, &x, &z, &c);
        u32 all;
        const u64 pos = out + block_compact_256(keep, s_wave, &all);
        if (keep && pos < T) {
            rows[2 * pos] = __brevll(x) >> (64 - P.n);
            rows[2 * pos + 1] = __brevll(z) >> (64 - P.n);
            coeff[pos] = c;
        }
        out += all;
    }
}

// basis: out[k] = c(x_k, z_k), zero where x_k is not among the diagonals
__global__ __launch_bounds__(256) void k_pd_pick(PdSlots P, i64 D, const u64 *__restrict__ bx, const u64 *__restrict__ bz, i64 K, f64x2 *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const u64 x = bx[k], z = bz[k];
    const i64 j = P.xs ? lower_bound(P.xs, D, x) : (i64)x;
    f64x2 c = {0.0, 0.0};
    if (j < D && (!P.xs || P.xs[j] == x)) c = pd_coefficient(P.scratch[((u64)j << P.n) + z], x, z, P.scale);
    out[k] = c;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
struct PdPass { bool strided; int L, s, k; u64 grid; int threads; };
struct PdPlan {
    int n = 0;
    u64 D = 0, total = 0;             // diagonals, slots
    int form = 0;                     // SYMGPU_PAULI_ONE_PASS / SYMGPU_PAULI_TWO_PASS
    int tile_bits = 0;                // bits transformed in contiguous tiles
    int n_pass = 0;
    PdPass pass[12];
};

static int pd_tile_switch() {
    const char *e = getenv("SYMGPU_PAULI_TILE_BITS");   // read per call: the tests force the two-pass form on small matrices
    return e ? atoi(e) : 0;
}

static int pd_threads(int L, int kk_first) {
    const int groups = 1 << (L - (kk_first < 1 ? 1 : kk_first));
    return groups < 64 ? 64 : (groups > 1024 ? 1024 : groups);
}

// A pure function of the shape (n, D), the switch and the device's answer to the LDS attribute.
static PdPlan pd_plan(int n, u64 D, int tile_switch, bool big_lds) {
    PdPlan p;
    p.n = n;
    p.D = D;
    p.total = D << n;
    const int cap = big_lds ? PD_TILE_LDS : PD_TILE_STATIC;
    int tb = tile_switch > 0 ? tile_switch : cap;
    if (tb < PD_CHUNK_BITS) tb = PD_CHUNK_BITS;
    if (tb > cap) tb = cap;
    p.form = n <= tb ? SYMGPU_PAULI_ONE_PASS : SYMGPU_PAULI_TWO_PASS;
    p.tile_bits = n <= tb ? n : tb;
    if (p.total == 0) return p;
    // contiguous tiles: several rows (or sub-tiles) per workgroup while the tile is small
    int L = p.tile_bits < 10 ? 10 : p.tile_bits;
    while (L > p.tile_bits && ((u64)1 << L) > p.total) --L;
    if (L < p.tile_bits) L = p.tile_bits;
    PdPass &a = p.pass[p.n_pass++];
    a = PdPass{false, L, 0, p.tile_bits, (p.total + ((u64)1 << L) - 1) >> L, pd_threads(L, p.tile_bits < 3 ? p.tile_bits : 3)};
    for (int s = p.tile_bits; s < n;) {
        const int k = n - s < cap - PD_CHUNK_BITS ? n - s : cap - PD_CHUNK_BITS;
        PdPass &b = p.pass[p.n_pass++];
        b = PdPass{true, k + PD_CHUNK_BITS, s, k, p.total >> (k + PD_CHUNK_BITS), pd_threads(k + PD_CHUNK_BITS, k < 3 ? k : 3)};
        s += k;
    }
    return p;
}

static bool pd_big_lds() {
    const bool ok = SG_DEVICE_ONCE(
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pd_wht_tile), hipFuncAttributeMaxDynamicSharedMemorySize, 16 << PD_TILE_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pd_wht_strided), hipFuncAttributeMaxDynamicSharedMemorySize, 16 << PD_TILE_LDS) == hipSuccess);
    if (!ok) note_degraded("from_matrix transform (k_pd_wht_tile) with 128 KiB tiles off: the runtime refused its LDS size; tiles of 64 KiB are used");
    return ok;
}

// device memory for `bytes` more?  (the cached allocator gives its parked blocks back first)
static int pd_require_memory(u64 bytes, const char *what) {
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (bytes > f) {
        dev_cache_release();
        HIP_TRY(hipMemGetInfo(&f, &t));
    }
    if (bytes > f) {
        set_error("from_matrix: %s needs %.2f GiB on the device, %.2f GiB free", what, (double)bytes / 1073741824.0, (double)f / 1073741824.0);
        return SYMGPU_E_NOMEM;
    }
    return SYMGPU_OK;
}

static int pd_upload(Scratch &dst, const void *host, size_t bytes) {
    SG_TRY(dst.alloc(bytes));
    if (bytes == 0) return SYMGPU_OK;
    HIP_TRY(hipMemcpyAsync(dst.p, host, bytes, hipMemcpyHostToDevice, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));          // host buffers are not retained past the call
    count_h2d(bytes);
    return SYMGPU_OK;
}

// ---- stages ------------------------------------------------------------------------------------------------------------------------
static int pd_transform(const PdPlan &p, f64x2 *scratch) {
    hipStream_t st = ctx().stream;
    for (int i = 0; i < p.n_pass; ++i) {
        const PdPass &q = p.pass[i];
        const size_t lds = (size_t)16 << (q.L < PD_TILE_MIN ? PD_TILE_MIN : q.L);
        if (q.strided) hipLaunchKernelGGL(k_pd_wht_strided, dim3((unsigned)q.grid), dim3(q.threads), lds, st, scratch, q.s, q.k);
        else hipLaunchKernelGGL(k_pd_wht_tile, dim3((unsigned)q.grid), dim3(q.threads), lds, st, scratch, p.total, q.L, q.k);
        KERNEL_CHECK();
    }
    return SYMGPU_OK;
}

static PdSlots pd_slots(const PdPlan &p, const f64x2 *scratch, const u64 *xs) {
    return PdSlots{scratch, xs, p.total, p.n, __builtin_ldexp(1.0, -p.n)};
}

// no basis: the kept coefficients, compacted in slot order, as a new operator
static int pd_select_all(const PdPlan &p, const f64x2 *scratch, const u64 *xs, symgpu_op_t *out, int64_t *n_out) {
    hipStream_t st = ctx().stream;
    u64 T = 0;
    Scratch counts, excl;
    const u64 nblk = (p.total + PD_SEL - 1) / PD_SEL;
    if (p.total > 0) {
        SG_TRY(counts.alloc((size_t)nblk * 4));
        SG_TRY(excl.alloc((size_t)nblk * 4 + 4));
        hipLaunchKernelGGL(k_pd_count, dim3((unsigned)nblk), dim3(256), 0, st, pd_slots(p, scratch, xs), counts.as<u32>());
        KERNEL_CHECK();
        u32 *d_total = excl.as<u32>() + nblk;
        SG_TRY(exclusive_scan_u32(counts.as<u32>(), excl.as<u32>(), (i64)nblk, d_total));
        u32 t32 = 0;
        SG_TRY(read_back_words(d_total, 1, nullptr, 0, &t32));
        T = t32;
    }
    SG_TRY(pd_require_memory(T * 32, "the operator"));
    OwnedOp op;
    SG_TRY(op.alloc((i64)T, (i64)T, 1, true));
    op->dup_free = 1;                                    // one term per (x, z)
    if (T > 0) {
        hipLaunchKernelGGL(k_pd_emit, dim3((unsigned)nblk), dim3(256), 0, st, pd_slots(p, scratch, xs), excl.as<u32>(), T, op->rows,
                           reinterpret_cast<f64x2 *>(op->coeff));
        KERNEL_CHECK();
    }
    op.hand_out(out);
    *n_out = (int64_t)T;
    return SYMGPU_OK;
}

// basis: the K coefficients in basis order, to the host
static int pd_select_basis(const PdPlan &p, const f64x2 *scratch, const u64 *xs, const u64 *bx_dev, const u64 *bz_dev, i64 K, double *coeff_out) {
    Scratch picked;
    SG_TRY(picked.alloc((size_t)K * 16));
    hipLaunchKernelGGL(k_pd_pick, dim3(grid_each(K)), dim3(256), 0, ctx().stream, pd_slots(p, scratch, xs), (i64)p.D, bx_dev, bz_dev, K, picked.as<f64x2>());
    KERNEL_CHECK();
    SG_TRY(download_any(picked.p, coeff_out, (size_t)K * 16));
    count_d2h((size_t)K * 16);
    return SYMGPU_OK;
}

// the basis on the device, and its distinct X-parts (ascending) on the host
struct PdBasis {
    i64 K = 0;
    Scratch bx, bz;
    std::vector<u64> xs;
    void list(const uint64_t *x, i64 K_) {               // host work only: an entry point checks the count before anything is allocated
        K = K_;
        if (K == 0) return;
        xs.assign(x, x + K);
        std::sort(xs.begin(), xs.end());
        xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    }
    int upload(const uint64_t *x, const uint64_t *z) {
        if (K == 0) return SYMGPU_OK;
        SG_TRY(pd_upload(bx, x, (size_t)K * 8));
        return pd_upload(bz, z, (size_t)K * 8);
    }
};

static bool pd_basis_in_range(const uint64_t *x, const uint64_t *z, i64 K, int n) {
    const u64 lim = (u64)1 << n;
    for (i64 k = 0; k < K; ++k)
        if (x[k] >= lim || z[k] >= lim) return false;
    return true;
}

static int pd_finish(const PdPlan &p, f64x2 *scratch, const u64 *xs_dev, const PdBasis &basis, symgpu_op_t *out, int64_t *n_out, double *coeff_out, int *form) {
    OwnedOp all;                                         // the operator of a call without a basis: the caller's once the stream has drained
    if (p.total > 0) SG_TRY(pd_transform(p, scratch));
    if (basis.K > 0) SG_TRY(pd_select_basis(p, scratch, xs_dev, basis.bx.as<u64>(), basis.bz.as<u64>(), basis.K, coeff_out));
    else SG_TRY(pd_select_all(p, scratch, xs_dev, all.slot(), n_out));
    if (form) *form = p.form;
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    if (basis.K == 0) all.hand_out(out);
    return SYMGPU_OK;
}

static int pd_dense(const double *matrix, int n, PdBasis &basis, symgpu_op_t *out, int64_t *n_out, double *coeff_out, int *form) {
    const u64 N = (u64)1 << n;
    const u64 D = basis.K > 0 ? (u64)basis.xs.size() : N;
    const PdPlan p = pd_plan(n, D, pd_tile_switch(), pd_big_lds());
    SG_TRY(pd_require_memory((N * N + p.total) * 16, "the matrix and its diagonals"));
    Scratch M, scratch, blocks, xs;
    SG_TRY(pd_upload(M, matrix, (size_t)(N * N) * 16));
    SG_TRY(scratch.alloc((size_t)p.total * 16));
    const int tb = n < 5 ? n : 5;
    std::vector<PdXBlock> xb;
    if (basis.K > 0) {
        for (size_t j = 0; j < basis.xs.size(); ++j) {
            const u32 x0 = (u32)(basis.xs[j] >> tb << tb);
            if (xb.empty() || xb.back().x0 != x0) xb.push_back(PdXBlock{x0, (u32)j, 0u, 0u});
            xb.back().mask |= 1u << (basis.xs[j] - x0);
        }
        SG_TRY(blocks.alloc(xb.size() * sizeof(PdXBlock)));
        HIP_TRY(hipMemcpyAsync(blocks.p, xb.data(), xb.size() * sizeof(PdXBlock), hipMemcpyHostToDevice, ctx().stream));
        SG_TRY(xs.alloc(basis.xs.size() * 8));
        HIP_TRY(hipMemcpyAsync(xs.p, basis.xs.data(), basis.xs.size() * 8, hipMemcpyHostToDevice, ctx().stream));
        HIP_TRY(hipStreamSynchronize(ctx().stream));     // the host vectors end with this scope
    }
    const unsigned gy = basis.K > 0 ? (unsigned)xb.size() : (unsigned)(N >> tb);
    hipLaunchKernelGGL(k_pd_gather_dense, dim3((unsigned)(N >> tb), gy), dim3(256), 0, ctx().stream, M.as<f64x2>(), n, tb,
                       basis.K > 0 ? blocks.as<PdXBlock>() : (const PdXBlock *)nullptr, scratch.as<f64x2>());
    KERNEL_CHECK();
    return pd_finish(p, scratch.as<f64x2>(), basis.K > 0 ? xs.as<u64>() : nullptr, basis, out, n_out, coeff_out, form);
}

template <typename IDX>
static int pd_csr(const double *data, const IDX *indices, const IDX *indptr, i64 nnz, int n, PdBasis &basis, symgpu_op_t *out, int64_t *n_out,
                  double *coeff_out, int *form) {
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << n;
    Scratch d_data, d_idx, d_ptr, key, key_tmp, row_of, head, excl, flags, bxs, xs;
    SG_TRY(pd_require_memory((u64)nnz * (16 + sizeof(IDX) + 8 + 8 + 4 + 4 + 4) + (N + 1) * sizeof(IDX), "the CSR arrays"));
    SG_TRY(pd_upload(d_data, data, (size_t)nnz * 16));
    SG_TRY(pd_upload(d_idx, indices, (size_t)nnz * sizeof(IDX)));
    SG_TRY(pd_upload(d_ptr, indptr, (size_t)(N + 1) * sizeof(IDX)));
    SG_TRY(flags.alloc(8));
    HIP_TRY(hipMemsetAsync(flags.p, 0, 8, st));
    u32 *d_D = flags.as<u32>() + 1;
    hipLaunchKernelGGL(k_pd_csr_check_indptr<IDX>, dim3(grid_each((i64)N + 1)), dim3(256), 0, st, d_ptr.as<IDX>(), nnz, n, flags.as<u32>());
    KERNEL_CHECK();
    u32 w[2] = {0, 0};
    if (nnz > 0) {
        // 1. the distinct row ^ col of the stored entries (that the basis lists), ascending
        SG_TRY(read_back_words(flags.as<u32>(), 1, nullptr, 0, w));      // a broken indptr must not steer the row search below
        if (w[0]) { set_error("invalid argument: from_matrix_csr: indptr does not ascend from 0 to nnz"); return SYMGPU_E_INVALID; }
        SG_TRY(key.alloc((size_t)nnz * 8));
        SG_TRY(key_tmp.alloc((size_t)nnz * 8));
        SG_TRY(row_of.alloc((size_t)nnz * 4));
        SG_TRY(head.alloc((size_t)nnz * 4));
        SG_TRY(excl.alloc((size_t)nnz * 4));
        hipLaunchKernelGGL(k_pd_csr_keys<IDX>, dim3(grid_each(nnz)), dim3(256), 0, st, d_idx.as<IDX>(), d_ptr.as<IDX>(), nnz, n, key.as<u64>(),
                           row_of.as<u32>(), flags.as<u32>());
        KERNEL_CHECK();
        SortResult by_x;
        SG_TRY(radix_sort({key.as<u64>(), key_tmp.as<u64>(), nullptr, nullptr, nnz, 0, (n + 7) / 8 * 8, nullptr, SortForm::Launches}, &by_x));
        const u64 *sorted = by_x.keys;
        if (basis.K > 0) {
            SG_TRY(bxs.alloc(basis.xs.size() * 8));
            HIP_TRY(hipMemcpyAsync(bxs.p, basis.xs.data(), basis.xs.size() * 8, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(k_pd_heads, dim3(grid_each(nnz)), dim3(256), 0, st, sorted, nnz, basis.K > 0 ? bxs.as<u64>() : (const u64 *)nullptr,
                           (i64)basis.xs.size(), head.as<u32>());
        KERNEL_CHECK();
        SG_TRY(exclusive_scan_u32(head.as<u32>(), excl.as<u32>(), nnz, d_D));
        SG_TRY(read_back_words(flags.as<u32>(), 2, nullptr, 0, w));
        if (w[0]) { set_error("invalid argument: from_matrix_csr: a column index lies outside [0, 2^n)"); return SYMGPU_E_INVALID; }
        SG_TRY(xs.alloc((size_t)w[1] * 8));
        hipLaunchKernelGGL(k_pd_compact_xs, dim3(grid_each(nnz)), dim3(256), 0, st, sorted, head.as<u32>(), excl.as<u32>(), nnz, xs.as<u64>());
        KERNEL_CHECK();
    } else {
        SG_TRY(read_back_words(flags.as<u32>(), 1, nullptr, 0, w));
        if (w[0]) { set_error("invalid argument: from_matrix_csr: indptr does not ascend from 0 to nnz"); return SYMGPU_E_INVALID; }
        SG_TRY(xs.alloc(8));
    }
    const u64 D = w[1];
    if ((D << n) >= ((u64)1 << 31)) {
        set_error("invalid argument: from_matrix_csr: %llu diagonals of 2^%d slots: 2^31 or more", (unsigned long long)D, n);
        return SYMGPU_E_INVALID;
    }
    const PdPlan p = pd_plan(n, D, pd_tile_switch(), pd_big_lds());
    // 2. gather: zeros, then every entry to (rank of its diagonal, row)
    Scratch scratch;
    SG_TRY(pd_require_memory(p.total * 16, "the diagonals"));
    SG_TRY(scratch.alloc((size_t)p.total * 16));
    if (p.total > 0) {
        HIP_TRY(hipMemsetAsync(scratch.p, 0, (size_t)p.total * 16, st));
        hipLaunchKernelGGL(k_pd_scatter<IDX>, dim3(grid_each(nnz)), dim3(256), 0, st, d_data.as<f64x2>(), d_idx.as<IDX>(), row_of.as<u32>(), nnz, n,
                           xs.as<u64>(), (i64)D, scratch.as<f64x2>());
        KERNEL_CHECK();
    }
    return pd_finish(p, scratch.as<f64x2>(), xs.as<u64>(), basis, out, n_out, coeff_out, form);
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_from_matrix_dense(const double *matrix, int n_qubits, const uint64_t *basis_x, const uint64_t *basis_z, int64_t K, symgpu_op_t *out,
                             int64_t *n_out, double *coeff_out, int *form) {
    SG_ENTER();
    SG_REQUIRE(matrix, "from_matrix_dense: null matrix");
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 31, "from_matrix_dense: 1 <= n_qubits <= 31");
    SG_REQUIRE(K >= 0 && K < ((i64)1 << 31), "from_matrix_dense: 0 <= K < 2^31");
    SG_REQUIRE(K == 0 ? (out && n_out) : (basis_x && basis_z && coeff_out), "from_matrix_dense: K = 0 needs out and n_out, K > 0 the basis arrays and coeff_out");
    SG_REQUIRE(n_qubits <= 16, "from_matrix_dense: a dense matrix of more than 16 qubits");
    SG_REQUIRE(pd_basis_in_range(basis_x, basis_z, K, n_qubits), "from_matrix_dense: a basis word has a bit at or above 2^n");
    SG_REQUIRE(K > 0 || n_qubits <= 15, "from_matrix_dense: all 4^n coefficients: 2^31 slots or more");
    if (out) *out = nullptr;
    PdBasis basis;
    basis.list(basis_x, K);
    SG_REQUIRE(((u64)(K > 0 ? basis.xs.size() : (size_t)1 << n_qubits) << n_qubits) < ((u64)1 << 31), "from_matrix_dense: diagonals x 2^n: 2^31 slots or more");
    SG_TRY(basis.upload(basis_x, basis_z));
    return pd_dense(matrix, n_qubits, basis, out, n_out, coeff_out, form);
}

int symgpu_from_matrix_csr(const double *data, const void *indices, const void *indptr, int index_bytes, int64_t nnz, int n_qubits,
                           const uint64_t *basis_x, const uint64_t *basis_z, int64_t K, symgpu_op_t *out, int64_t *n_out, double *coeff_out, int *form) {
    SG_ENTER();
    SG_REQUIRE(indptr && nnz >= 0 && nnz < ((i64)1 << 31) && (nnz == 0 || (data && indices)), "from_matrix_csr: arrays / 0 <= nnz < 2^31");
    SG_REQUIRE(index_bytes == 4 || index_bytes == 8, "from_matrix_csr: index_bytes is 4 or 8");
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 31, "from_matrix_csr: 1 <= n_qubits <= 31");
    SG_REQUIRE(K >= 0 && K < ((i64)1 << 31), "from_matrix_csr: 0 <= K < 2^31");
    SG_REQUIRE(K == 0 ? (out && n_out) : (basis_x && basis_z && coeff_out), "from_matrix_csr: K = 0 needs out and n_out, K > 0 the basis arrays and coeff_out");
    SG_REQUIRE(pd_basis_in_range(basis_x, basis_z, K, n_qubits), "from_matrix_csr: a basis word has a bit at or above 2^n");
    if (out) *out = nullptr;
    PdBasis basis;
    basis.list(basis_x, K);
    SG_TRY(basis.upload(basis_x, basis_z));
    if (index_bytes == 4)
        return pd_csr<int32_t>(data, (const int32_t *)indices, (const int32_t *)indptr, nnz, n_qubits, basis, out, n_out, coeff_out, form);
    return pd_csr<int64_t>(data, (const int64_t *)indices, (const int64_t *)indptr, nnz, n_qubits, basis, out, n_out, coeff_out, form);
}

}  // extern "C"
