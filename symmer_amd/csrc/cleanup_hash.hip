// cleanup_hash.hip — the row hashes the cleanup sorts by (cleanup_driver.hip): the GF(2)-linear tabulated hash (its tables, the host
// evaluation, k_hash_rows / k_hash_rows_long) and the mixing hash of rows that nothing XORs together (k_hash_rows_mix).
#include "cleanup_common.h"
#include <stdlib.h>
#include <vector>

namespace symgpu {

static u64 host_splitmix64(u64 &s) {
    u64 z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// k_hash_rows_long: columns of M^(2^j), M = the xorshift step of the per-lane Horner scheme (a linear map on GF(2)^64), j < 32
static u64 host_xorshift_step(u64 h) { h ^= h << 13; h ^= h >> 7; h ^= h << 17; return h; }
static int ensure_xs_pow() {
    if (ctx().xs_pow) return SYMGPU_OK;
    std::vector<u64> P(32 * 64);
    for (int i = 0; i < 64; ++i) P[i] = host_xorshift_step(1ULL << i);
    for (int j = 1; j < 32; ++j)
        for (int i = 0; i < 64; ++i) {                               // column i of M^(2^j) = M^(2^(j-1)) applied to column i of M^(2^(j-1))
            const u64 x = P[(j - 1) * 64 + i];
            u64 y = 0;
            for (int b = 0; b < 64; ++b)
                if ((x >> b) & 1) y ^= P[(j - 1) * 64 + b];
            P[j * 64 + i] = y;
        }
    HIP_TRY(hipMalloc((void **)&ctx().xs_pow, P.size() * sizeof(u64)));
    HIP_TRY(hipMemcpy(ctx().xs_pow, P.data(), P.size() * sizeof(u64), hipMemcpyHostToDevice));
    return SYMGPU_OK;
}

int ensure_hash_tables(u64 seed) {
    Context &c = ctx();
    if (c.hash_tab && c.hash_seed == seed) return SYMGPU_OK;
    if (!c.hash_tab) HIP_TRY(hipMalloc((void **)&c.hash_tab, 8 * 256 * 2 * sizeof(u64)));
    std::vector<u64> tab(8 * 256 * 2);
    u64 s = seed * 0x2545f4914f6cdd1dULL + 0x1234567ULL;
    u64 basis[2][64];
    for (int h = 0; h < 2; ++h)
        for (int b = 0; b < 64; ++b) basis[h][b] = host_splitmix64(s);
    // test hook: SYMGPU_HASH_WEAK_ODD=1 leaves an odd seed only the 4 top hash bits, so that different rows collide in bulk and the
    // exactness guard (row-against-row verification -> reseed -> retry; long mixed prefix runs -> full 64-bit sort) actually runs
    if (const char *e = getenv("SYMGPU_HASH_WEAK_ODD"))
        if (e[0] == '1' && (seed & 1))
            for (int h = 0; h < 2; ++h)
                for (int b = 0; b < 64; ++b) basis[h][b] &= 0xF000000000000000ULL;
    for (int k = 0; k < 8; ++k)
        for (int v = 0; v < 256; ++v)
            for (int h = 0; h < 2; ++h) {
                u64 x = 0;
                for (int b = 0; b < 8; ++b)
                    if ((v >> b) & 1) x ^= basis[h][8 * k + b];
                tab[((size_t)k * 256 + v) * 2 + h] = x;
            }
    HIP_TRY(hipMemcpyAsync(c.hash_tab, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));   // tab is a host temporary
    c.hash_seed = seed;
    c.host_hash_tab = tab;
    return SYMGPU_OK;
}

// host evaluation of the same linear hash h1 as k_hash_rows (per-lane Horner over 64-word blocks, XOR over lanes)
u64 host_row_hash(const u64 *row, int W) {
    const std::vector<u64> &tab = ctx().host_hash_tab;
    const int n_blk = (W + 63) / 64;
    u64 h = 0;
    for (int g = 0; g < 64; ++g) {
        u64 hg = 0;
        for (int b = 0; b < n_blk; ++b) {
            const int w = b * 64 + g;
            u64 a1 = 0;
            if (w < W) {
                const u64 x = row[w];
                for (int k = 0; k < 8; ++k) a1 ^= tab[((size_t)k * 256 + ((x >> (8 * k)) & 255)) * 2];
            }
            hg ^= hg << 13; hg ^= hg >> 7; hg ^= hg << 17;
            const int r = g & 63;
            hg ^= r ? ((a1 << r) | (a1 >> (64 - r))) : a1;
        }
        h ^= hg;
    }
    return h;
}

__device__ __forceinline__ u64 rotl64(u64 x, int r) { r &= 63; return r ? ((x << r) | (x >> (64 - r))) : x; }
__device__ __forceinline__ u64 xorshift_step(u64 h) { h ^= h << 13; h ^= h >> 7; h ^= h << 17; return h; }

// Row hash on row-major rows.  G (power of two, <= 64) lanes cooperate on one row; lane g handles words
// g, g+64, g+128, ... (only G == 64 has more than one).  Only the first of the two table columns is used (16 KiB of LDS).
__global__ __launch_bounds__(256) void k_hash_rows(const u64 *__restrict__ rows, i64 T, int W, int G, const u64 *__restrict__ tab_g,
                                                    u64 *__restrict__ out1) {
    __shared__ u64 tab[8 * 256];
    for (int k = threadIdx.x; k < 8 * 256; k += 256) tab[k] = tab_g[2 * k];
    __syncthreads();
    const int rows_per_block = 256 / G;
    const int g = threadIdx.x % G, rsub = threadIdx.x / G;
    const int n_blk = (W + 63) / 64;
    constexpr int HU = 4;                                           // row groups in flight per step (the loop is latency bound)
    for (i64 t0 = (i64)blockIdx.x * rows_per_block * HU; t0 < T; t0 += (i64)gridDim.x * rows_per_block * HU) {
        u64 h1[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) h1[u] = 0;
        // BU 64-word blocks of every row group are loaded before the (sequential) Horner steps consume them: a 1e8-qubit row is
        // 48,828 blocks long, and one dependent load per step made its hash 80 ms
        constexpr int BU = 4;
        for (int b0 = 0; b0 < n_blk; b0 += BU) {
            u64 x[BU][HU];
#pragma unroll
            for (int bu = 0; bu < BU; ++bu) {
                const int w = (b0 + bu) * 64 + g;
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    const i64 t = t0 + (i64)u * rows_per_block + rsub;
                    x[bu][u] = (t < T && w < W && g < 64) ? rows[t * W + w] : 0ULL;
                }
            }
#pragma unroll
            for (int bu = 0; bu < BU; ++bu) {
                if (b0 + bu >= n_blk) break;                            // uniform
                const int w = (b0 + bu) * 64 + g;
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    u64 a1 = 0;
                    if (w < W && g < 64) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) a1 ^= tab[k * 256 + (int)((x[bu][u] >> (8 * k)) & 255)];
                    }
                    h1[u] = xorshift_step(h1[u]) ^ rotl64(a1, g);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            for (int off = G >> 1; off > 0; off >>= 1) h1[u] ^= __shfl_xor(h1[u], off);
            const i64 t = t0 + (i64)u * rows_per_block + rsub;
            if (g == 0 && t < T) out1[t] = h1[u];
        }
    }
}

// ---- a hash for rows that nothing XORs together afterwards (plain cleanup, joins of two operators) ---------------------------------------
// The tabulated hash above is GF(2)-linear because the fused product needs h(a ^ b) = h(a) ^ h(b); it costs eight LDS look-ups per 64-bit
// word and runs at 1.0-1.8 TB/s (a plain cleanup of 1e7 rows of 1,000 qubits spent a third of its time in it).  Where linearity is not
// needed every word goes through an injective 64-bit mix salted with its position and the seed (two rounds of the murmur3 32-bit finaliser
// with the halves crossed: four v_mul_lo_u32), and the words of a row are XORed: memory bound.  Exactness never rests on it (equal
// keys are verified row against row, a mismatch reseeds).
__device__ __forceinline__ u32 fmix32(u32 h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16; return h; }
__device__ __forceinline__ u64 mix_word(u64 x, u32 w, u64 seed) {
    u32 a = (u32)x ^ (u32)seed ^ (w * 0x9E3779B1u);
    u32 b = (u32)(x >> 32) ^ (u32)(seed >> 32) ^ (w * 0x85EBCA77u + 0x165667B1u);
    a = fmix32(a + __builtin_amdgcn_alignbit(b, b, 17));             // (rotl 15)
    b = fmix32(b ^ a);
    return ((u64)b << 32) | a;
}
__global__ __launch_bounds__(256) void k_hash_rows_mix(const u64 *__restrict__ rows, i64 T, int W, int G, u64 seed, u64 keep_mask, u64 *__restrict__ out1,
                                                        u32 *__restrict__ iota /* null, or [T]: iota[t] = t (the index array the sort carries) */) {
    // G lanes per row, a lane takes 16-byte chunks g, g + G, ... (W = 2 Wq is even: a row is a whole number of chunks)
    const int rows_per_block = 256 / G;
    const int g = threadIdx.x % G, rsub = threadIdx.x / G;
    const int C = W / 2;                                             // chunks per row
    const u32x4 *rows16 = reinterpret_cast<const u32x4 *>(rows);
    constexpr int HU = 4;                                           // row groups in flight per step
    for (i64 t0 = (i64)blockIdx.x * rows_per_block * HU; t0 < T; t0 += (i64)gridDim.x * rows_per_block * HU) {
        u64 h[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) h[u] = 0;
        for (int c0 = 0; c0 < C; c0 += 2 * G) {                      // two chunks per lane and step (rows of up to 256 words: one step)
            u32x4 x[2][HU];
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    const i64 t = t0 + (i64)u * rows_per_block + rsub;
                    const int c = c0 + k * G + g;
                    const u32x4 z = {0u, 0u, 0u, 0u};
                    x[k][u] = (t < T && c < C) ? rows16[t * C + c] : z;
                }
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int u = 0; u < HU; ++u) {
                    const int c = c0 + k * G + g;
                    if (c < C) {
                        h[u] ^= mix_word(((u64)x[k][u].y << 32) | x[k][u].x, (u32)(2 * c), seed);
                        h[u] ^= mix_word(((u64)x[k][u].w << 32) | x[k][u].z, (u32)(2 * c + 1), seed);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            for (int off = G >> 1; off > 0; off >>= 1) h[u] ^= __shfl_xor(h[u], off);
            const i64 t = t0 + (i64)u * rows_per_block + rsub;
            if (g == 0 && t < T) { out1[t] = h[u] & keep_mask; if (iota) iota[t] = (u32)t; }
        }
    }
}

// The same hash for VERY long rows (>= 8192 words: > 262,144 qubits; the reference's "two 100,000,000-qubit Pauli terms",
// README.md:54).  The Horner scheme of k_hash_rows is one dependent step per 64 words — 48,828 steps, 37 ms, for a 1e8-qubit row on
// ONE wavefront.  It is linear:  h_g = sum_b M^(n_blk-1-b) v_(b,g),  so a wavefront can run it over a SEGMENT of LSEG blocks and
// shift its partial result to the end of the row with M^(n_blk - segment end) (square-and-multiply on the precomputed columns
// of M^(2^j): <= 16 bit-matrix products), and the segments of a row combine with XOR (atomicXor; out1 zeroed by the caller).
constexpr int LSEG = 64;
__global__ __launch_bounds__(256) void k_hash_rows_long(const u64 *__restrict__ rows, i64 t_base, int W, const u64 *__restrict__ tab_g,
                                                         const u64 *__restrict__ xs_pow, u64 *__restrict__ out1) {
    __shared__ u64 tab[8 * 256];
    for (int k = threadIdx.x; k < 8 * 256; k += 256) tab[k] = tab_g[2 * k];
    __syncthreads();
    const int g = threadIdx.x & 63;
    const int n_blk = (W + 63) / 64;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b_lo = seg * LSEG;
    if (b_lo >= n_blk) return;
    const int b_hi = b_lo + LSEG < n_blk ? b_lo + LSEG : n_blk;
    const i64 t = t_base + blockIdx.y;
    const u64 *row = rows + t * W;
    u64 h = 0;
    constexpr int BU = 8;
    for (int b0 = b_lo; b0 < b_hi; b0 += BU) {
        u64 x[BU];
#pragma unroll
        for (int bu = 0; bu < BU; ++bu) {
            const int w = (b0 + bu) * 64 + g;
            x[bu] = (b0 + bu < b_hi && w < W) ? row[w] : 0ULL;
        }
#pragma unroll
        for (int bu = 0; bu < BU; ++bu) {
            if (b0 + bu >= b_hi) break;                              // wave-uniform
            u64 a1 = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) a1 ^= tab[k * 256 + (int)((x[bu] >> (8 * k)) & 255)];   // padding words are zero: tab[..][0] = 0
            h = xorshift_step(h) ^ rotl64(a1, g);
        }
    }
    // h <- M^(n_blk - b_hi) h
    for (unsigned k = (unsigned)(n_blk - b_hi), j = 0; k; k >>= 1, ++j) {
        if (!(k & 1u)) continue;                                     // wave-uniform
        const u64 *P = xs_pow + j * 64;
        u64 y = 0;
#pragma unroll 8
        for (int i = 0; i < 64; ++i) y ^= P[i] & (0ULL - ((h >> i) & 1ULL));
        h = y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h ^= __shfl_xor(h, off);
    if (g == 0) atomicXor(reinterpret_cast<unsigned long long *>(out1 + t), (unsigned long long)h);
}

__global__ void k_iota_keys_plain(u32 *__restrict__ idx, i64 T) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) idx[t] = (u32)t;
}

static int pow2_group(int W) {
    int g = 1;
    while (g < W && g < 64) g <<= 1;
    return g;
}

// rows that are only compared with each other (see k_hash_rows_mix); `seed` as for the tables: a reseed changes the function
int hash_rows_any(const u64 *rows, i64 T, int W, u64 seed, u64 *out1, u32 *iota) {
    if (T == 0) return SYMGPU_OK;
    if (W >= 64 * 128) {                                            // very long rows: the segmented kernel of the linear hash
        if (iota) { hipLaunchKernelGGL(k_iota_keys_plain, dim3(grid_for(T)), dim3(256), 0, ctx().stream, iota, T); KERNEL_CHECK(); }
        return hash_rows(rows, T, W, out1);
    }
    u64 s = seed * 0x9E3779B97F4A7C15ULL + 0xD1B54A32D192ED03ULL;
    s ^= s >> 29; s *= 0xBF58476D1CE4E5B9ULL; s ^= s >> 32;
    u64 keep = ~0ULL;
    if (const char *e = getenv("SYMGPU_HASH_WEAK_ODD"))             // the tables' test hook: an odd seed keeps 4 bits, so rows collide in bulk
        if (e[0] == '1' && (seed & 1)) keep = 0xF000000000000000ULL;
    const int G = pow2_group(W / 2);                                // lanes per row: one 16-byte chunk each (rows of up to 128 words)
    const int rpb = 4 * (256 / G);
    i64 g = (T + rpb - 1) / rpb;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_hash_rows_mix, dim3((unsigned)g), dim3(256), 0, ctx().stream, rows, T, W, G, s, keep, out1, iota);
    KERNEL_CHECK();
    return SYMGPU_OK;
}
int hash_rows(const u64 *rows, i64 T, int W, u64 *out1) {
    if (T == 0) return SYMGPU_OK;
    if (W >= 64 * 128) {                                            // very long rows: segments in parallel (k_hash_rows_long)
        SG_TRY(ensure_xs_pow());
        hipStream_t st = ctx().stream;
        HIP_TRY(hipMemsetAsync(out1, 0, (size_t)T * sizeof(u64), st));
        const int n_seg = ((W + 63) / 64 + LSEG - 1) / LSEG;
        for (i64 t0 = 0; t0 < T; t0 += 65535) {
            const i64 nt = T - t0 < 65535 ? T - t0 : 65535;
            hipLaunchKernelGGL(k_hash_rows_long, dim3((unsigned)((n_seg + 3) / 4), (unsigned)nt), dim3(256), 0, st, rows, t0, W, ctx().hash_tab, ctx().xs_pow, out1);
            KERNEL_CHECK();
        }
        return SYMGPU_OK;
    }
    const int G = pow2_group(W);
    const int rpb = 4 * (256 / G);                                  // k_hash_rows: HU = 4 row groups per step
    i64 g = (T + rpb - 1) / rpb;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_hash_rows, dim3((unsigned)g), dim3(256), 0, ctx().stream, rows, T, W, G, ctx().hash_tab, out1);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
