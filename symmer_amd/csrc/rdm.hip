// rdm.hip — the reduced density matrix of a dense statevector over k kept qubits (conventions of matvec.hip: qubit q is bit
// n-1-q of a basis index b).  With KM / TM the index bits of the kept / traced qubits, a < 2^k and e < 2^(n-k) spread over them lowest bit
// to lowest bit (so the kept qubit of the lowest number is the most significant bit of a), b(a, e) = dep(a, KM) | dep(e, TM) and
//   rho[a][a'] = sum_e psi[b(a, e)] conj psi[b(a', e)]        — rho = M M^+ for the 2^k x 2^(n-k) matrix M[a][e] = psi[b(a, e)].
// One multiply-add, the same in both forms, p = psi[b(a, e)], q = psi[b(a', e)], every fma rounded once:
//   re <- fma(p.im, q.im, fma(p.re, q.re, re)),   im <- fma(-p.re, q.im, fma(p.im, q.re, im));   a = a': re only, im is stored as +0.0.
// Only a <= a' is summed; rho[a'][a] is written as the exact conjugate of the finished sum.  No floating-point atomics.
// STREAM (k <= 3): the tile bits S are KM and the min(8, n-k) lowest bits of TM; a workgroup stages the 2^|S| amplitudes that agree outside
//   S in LDS (global reads in index order: S holds the 4 lowest index bits) and thread t < 2^(|S|-k) takes e = tile * 2^(|S|-k) + t: it
//   reads its 2^k amplitudes from LDS and adds the products of the upper triangle to registers.  The 2^(n-|S|) tiles are cut into
//   C = min(tiles, 1024) chunks of consecutive tiles, one workgroup each, its tiles in ascending order; the 256 thread sums of every entry
//   are folded by halving (s[t] += s[t + 128], then 64, ... 1); one last launch adds the chunk sums to 0 in ascending chunk order.
// TILED (every other k; any k when forced): tiles of 64 x 64 entries (the whole matrix for k < 6), only the pairs (I, J), I <= J; the
//   2^(n-k) values of e go in blocks of 2^sk, sk = min(4, n-k), and C consecutive runs of blocks (chunks); C = the smaller of the number
//   of blocks and the largest power of two <= max(1, 1024 / pairs).  Workgroup (pair, chunk): per block it stages the panel
//   psi[b(64 I + r, e)] (and the panel of J unless I = J) in LDS as [e][r] — the amplitudes of a panel vary in the 6 lowest kept and
//   the sk lowest traced index bits, which hold the 4 lowest index bits, so the global reads go in index order — and thread (ty, tx)
//   adds to its 4 x 4 entries (rows ty + 16 i, columns tx + 16 j) for e ascending — on a diagonal tile only to the 10 with i <= j, the
//   others lie below the diagonal for every thread (the half is taken in steps of 16 there).  The tile of a chunk goes to scratch [C][2^k][2^k];
//   one launch adds the chunks to 0 in ascending order for a <= a' and writes both triangles.
// Both forms load the next tile / block into registers while the present one is used from LDS.
#include "matvec.h"
#include <stdlib.h>
#include <string.h>

namespace symgpu {

constexpr int RDM_WG = 256;
constexpr int RDM_KS = 3;              // STREAM takes k <= KS: 36 complex sums a thread
constexpr int RDM_MAX_K = 12;          // the refusal bound: 2^12 x 2^12 x 16 bytes = 256 MiB
constexpr int RDM_ST_E = 8;            // STREAM: 2^8 values of e a tile, one per thread
constexpr unsigned RDM_ST_CHUNKS = 1024;
constexpr int RDM_T = 6;               // TILED: tile edge 2^6 = 16 threads x 4 entries
constexpr int RDM_S = 4;               // TILED: 2^4 values of e a staged block
constexpr unsigned RDM_TL_WGS = 1024;  // TILED: pairs x chunks stays at or below this while the chunks are cut

// the bits of v, lowest first, to the set positions of mask, lowest first
__host__ __device__ __forceinline__ u64 rdm_deposit(u64 v, u64 mask) {
    u64 r = 0;
    while (mask) {
        const u64 low = mask & (~mask + 1);
        if (v & 1) r |= low;
        v >>= 1;
        mask ^= low;
    }
    return r;
}
// the bits of v at the set positions of mask, packed lowest first
__host__ __device__ __forceinline__ u64 rdm_extract(u64 v, u64 mask) {
    u64 r = 0;
    for (int at = 0; mask; mask &= mask - 1, ++at)
        if (v & mask & (~mask + 1)) r |= (u64)1 << at;
    return r;
}

__device__ __forceinline__ void rdm_mac(double &re, double &im, f64x2 p, f64x2 q) {
    re = __fma_rn(p.y, q.y, __fma_rn(p.x, q.x, re));
    im = __fma_rn(-p.x, q.y, __fma_rn(p.y, q.x, im));
}

// the sum of v over the workgroup by halving; the value is thread 0's
__device__ __forceinline__ double rdm_fold(double v, double *sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int h = RDM_WG / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = __dadd_rn(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    return sm[0];
}

// STREAM.  S: the tile bits (m of them), outside: the other index bits, LA: the kept bits among the tile bits (as bits of a tile slot).
// partial[chunk][entry]: the upper triangle row by row, entry (a, a'), a <= a'.
template <int K>
__global__ __launch_bounds__(RDM_WG) void k_rdm_stream(const f64x2 *__restrict__ psi, u64 S, u64 outside, u32 LA, int m, u64 tiles_per_chunk,
                                                       f64x2 *__restrict__ partial) {
    constexpr int D = 1 << K, E = D * (D + 1) / 2;
    extern __shared__ f64x2 rdm_tile[];
    __shared__ double sm[RDM_WG];
    const u32 L = 1u << m, t = threadIdx.x;
    const bool active = t < (L >> K);
    const u32 lt = (u32)rdm_deposit(t, (u64)((L - 1) & ~LA));
    u32 at[D];
    u64 g[D];                                             // L / 256 <= 2^K pieces a thread
    f64x2 next[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        at[a] = ((u32)rdm_deposit((u64)a, (u64)LA) | lt) & (L - 1);
        g[a] = rdm_deposit((u64)(t + RDM_WG * a), S);
    }
    double re[E], im[E];
#pragma unroll
    for (int e = 0; e < E; ++e) re[e] = im[e] = 0.0;
    const u64 T0 = (u64)blockIdx.x * tiles_per_chunk, T1 = T0 + tiles_per_chunk;
    u64 base = rdm_deposit(T0, outside);
#pragma unroll
    for (int i = 0; i < D; ++i)
        if (t + RDM_WG * i < L) next[i] = psi[base | g[i]];
    for (u64 T = T0; T < T1; ++T) {
#pragma unroll
        for (int i = 0; i < D; ++i)
            if (t + RDM_WG * i < L) rdm_tile[t + RDM_WG * i] = next[i];
        __syncthreads();
        if (T + 1 < T1) {
            base = rdm_deposit(T + 1, outside);
#pragma unroll
            for (int i = 0; i < D; ++i)
                if (t + RDM_WG * i < L) next[i] = psi[base | g[i]];
        }
        if (active) {
            f64x2 v[D];
#pragma unroll
            for (int a = 0; a < D; ++a) v[a] = rdm_tile[at[a]];
            int e = 0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                re[e] = __fma_rn(v[a].y, v[a].y, __fma_rn(v[a].x, v[a].x, re[e]));
                ++e;
#pragma unroll
                for (int b = a + 1; b < D; ++b, ++e) rdm_mac(re[e], im[e], v[a], v[b]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const double sr = rdm_fold(re[e], sm), si = rdm_fold(im[e], sm);
        if (t == 0) partial[(u64)blockIdx.x * E + e] = f64x2{sr, si};
    }
}

// rho from the chunk sums of STREAM: one thread an entry of the upper triangle
__global__ __launch_bounds__(RDM_WG) void k_rdm_stream_sum(const f64x2 *__restrict__ partial, unsigned chunks, int k, f64x2 *__restrict__ rho) {
    const u32 D = 1u << k, E = D * (D + 1) / 2;
    u32 e = blockIdx.x * RDM_WG + threadIdx.x;
    if (e >= E) return;
    const u32 entry = e;
    u32 a = 0;
    while (e >= D - a) { e -= D - a; ++a; }
    const u32 b = a + e;
    double sr = 0.0, si = 0.0;
    for (unsigned c = 0; c < chunks; ++c) {
        const f64x2 p = partial[(u64)c * E + entry];
        sr = __dadd_rn(sr, p.x);
        si = __dadd_rn(si, p.y);
    }
    if (a == b) {
        rho[(u64)a * D + a] = f64x2{sr, 0.0};
    } else {
        rho[(u64)a * D + b] = f64x2{sr, si};
        rho[(u64)b * D + a] = f64x2{sr, -si};
    }
}

// one staged block of TILED: the 4 x 4 entries of thread (ty, tx) over `count` values of e.  On a diagonal tile (DIAG) the entries
// with i > j lie below the diagonal for every thread (row - column = ty - tx + 16 (i - j) >= 1) and are left out: 10 of 16 remain.
template <bool DIAG>
__device__ __forceinline__ void rdm_block(const f64x2 *rows, const f64x2 *cols, int count, u32 tx, u32 ty, double (&re)[4][4], double (&im)[4][4]) {
    constexpr int EDGE = 1 << RDM_T;
    for (int e = 0; e < count; ++e) {
        f64x2 p[4], q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = rows[e * EDGE + ty + 16 * i];
            q[i] = cols[e * EDGE + tx + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!DIAG || i <= j) rdm_mac(re[i][j], im[i][j], p[i], q[j]);
    }
}

// TILED, the work of one workgroup on the tile pair (I, J), DIAG = (I == J): a path of its own for each, so that neither carries the
// other's tests in its loop.  KM / TM: the kept / traced index bits; V: the tk lowest of KM and the sk lowest of TM; LA: the kept bits
// among V (as bits of a panel slot); out: this chunk's [2^k][2^k] of the scratch.
template <bool DIAG>
__device__ __forceinline__ void rdm_tile_pair(const f64x2 *__restrict__ psi, u64 KM, u64 TM, u64 V, u32 LA, int tk, int sk, int k, u32 I, u32 J,
                                              u64 blocks_per_chunk, f64x2 *__restrict__ out, f64x2 *sA, f64x2 *sB) {
    constexpr int EDGE = 1 << RDM_T, EB = 1 << RDM_S, PIECES = EDGE * EB / RDM_WG;
    const u32 t = threadIdx.x, tx = t & 15, ty = t >> 4;
    for (u32 l = t; l < EB * EDGE; l += RDM_WG) sA[l] = sB[l] = f64x2{0.0, 0.0};      // rows from 2^tk on stay zero (k < 6)
    const u32 L = 1u << (tk + sk);
    u64 g[PIECES];
    u32 slot[PIECES];
    f64x2 nextA[PIECES], nextB[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const u32 l = t + RDM_WG * i;
        g[i] = rdm_deposit((u64)l, V);
        slot[i] = ((u32)rdm_extract((u64)l, (u64)((L - 1) & ~LA)) * EDGE + (u32)rdm_extract((u64)l, (u64)LA)) & (EB * EDGE - 1);
    }
    const u64 rowA = rdm_deposit((u64)I << tk, KM), rowB = rdm_deposit((u64)J << tk, KM);
    double re[4][4], im[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) re[i][j] = im[i][j] = 0.0;
    const u64 B0 = (u64)blockIdx.y * blocks_per_chunk, B1 = B0 + blocks_per_chunk;
    u64 ebase = rdm_deposit(B0 << sk, TM);
#pragma unroll
    for (int i = 0; i < PIECES; ++i)
        if (t + RDM_WG * i < L) {
            nextA[i] = psi[rowA | ebase | g[i]];
            if (!DIAG) nextB[i] = psi[rowB | ebase | g[i]];
        }
    __syncthreads();
    for (u64 blk = B0; blk < B1; ++blk) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i)
            if (t + RDM_WG * i < L) {
                sA[slot[i]] = nextA[i];
                if (!DIAG) sB[slot[i]] = nextB[i];
            }
        __syncthreads();
        if (blk + 1 < B1) {
            ebase = rdm_deposit((blk + 1) << sk, TM);
#pragma unroll
            for (int i = 0; i < PIECES; ++i)
                if (t + RDM_WG * i < L) {
                    nextA[i] = psi[rowA | ebase | g[i]];
                    if (!DIAG) nextB[i] = psi[rowB | ebase | g[i]];
                }
        }
        rdm_block<DIAG>(sA, DIAG ? sA : sB, 1 << sk, tx, ty, re, im);
        __syncthreads();
    }
    const u64 D = (u64)1 << k;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 row = (u64)I * EDGE + ty + 16 * i, col = (u64)J * EDGE + tx + 16 * j;
            if (row < D && col < D && !(DIAG && i > j)) out[row * D + col] = f64x2{re[i][j], im[i][j]};
        }
}

// TILED: workgroup (tile pair, chunk); nt: tiles a side; partial [chunks][2^k][2^k]
__global__ __launch_bounds__(RDM_WG) void k_rdm_tiled(const f64x2 *__restrict__ psi, u64 KM, u64 TM, u64 V, u32 LA, int tk, int sk, int k, int nt,
                                                      u64 blocks_per_chunk, f64x2 *__restrict__ partial) {
    __shared__ f64x2 sA[(1 << RDM_S) << RDM_T], sB[(1 << RDM_S) << RDM_T];
    u32 I = 0, J = blockIdx.x;
    while (J >= (u32)nt - I) { J -= (u32)nt - I; ++I; }
    J += I;
    f64x2 *out = partial + ((u64)blockIdx.y << (2 * k));
    if (I == J) rdm_tile_pair<true>(psi, KM, TM, V, LA, tk, sk, k, I, J, blocks_per_chunk, out, sA, sB);
    else rdm_tile_pair<false>(psi, KM, TM, V, LA, tk, sk, k, I, J, blocks_per_chunk, out, sA, sB);
}

// rho from the chunk tiles of TILED: one thread an entry, those of the upper triangle add and write both
__global__ __launch_bounds__(RDM_WG) void k_rdm_tiled_sum(const f64x2 *__restrict__ partial, unsigned chunks, int k, f64x2 *__restrict__ rho) {
    const u64 D = (u64)1 << k, at = (u64)blockIdx.x * RDM_WG + threadIdx.x;
    if (at >= D * D) return;
    const u64 a = at >> k, b = at & (D - 1);
    if (a > b) return;
    double sr = 0.0, si = 0.0;
    for (unsigned c = 0; c < chunks; ++c) {
        const f64x2 p = partial[(u64)c * D * D + at];
        sr = __dadd_rn(sr, p.x);
        si = __dadd_rn(si, p.y);
    }
    if (a == b) {
        rho[at] = f64x2{sr, 0.0};
    } else {
        rho[at] = f64x2{sr, si};
        rho[b * D + a] = f64x2{sr, -si};
    }
}

// what a call does, from (n, KM) and the form alone
struct RdmShape {
    int form = 0, n = 0, k = 0;
    u64 KM = 0, TM = 0;
    unsigned chunks = 1;
    u64 grid = 1, scratch = 0;
    // STREAM
    u64 S = 0;
    int m = 0;
    u64 tiles_per_chunk = 1;
    // TILED
    u64 V = 0;
    int tk = 0, sk = 0, nt = 1;
    u64 blocks_per_chunk = 1;
};

static u64 rdm_lowest_bits(u64 mask, int count) { return rdm_deposit(((u64)1 << count) - 1, mask); }

static RdmShape rdm_shape(int n, int k, u64 KM, int form) {
    RdmShape s;
    s.form = form;
    s.n = n;
    s.k = k;
    s.KM = KM;
    s.TM = (((u64)1 << n) - 1) & ~KM;
    if (form == SYMGPU_RDM_STREAM) {
        const int eb = n - k < RDM_ST_E ? n - k : RDM_ST_E;
        s.m = k + eb;
        s.S = KM | rdm_lowest_bits(s.TM, eb);
        const u64 tiles = (u64)1 << (n - s.m);
        s.chunks = tiles < RDM_ST_CHUNKS ? (unsigned)tiles : RDM_ST_CHUNKS;
        s.tiles_per_chunk = tiles / s.chunks;
        s.grid = s.chunks;
        s.scratch = (u64)s.chunks * (((u64)1 << k) * (((u64)1 << k) + 1) / 2) * 16;
    } else {
        s.tk = k < RDM_T ? k : RDM_T;
        s.sk = n - k < RDM_S ? n - k : RDM_S;
        s.nt = 1 << (k - s.tk);
        s.V = rdm_lowest_bits(KM, s.tk) | rdm_lowest_bits(s.TM, s.sk);
        const u64 pairs = (u64)s.nt * (s.nt + 1) / 2, blocks = (u64)1 << (n - k - s.sk);
        u64 want = 1;
        while (2 * want * pairs <= RDM_TL_WGS) want *= 2;
        s.chunks = (unsigned)(blocks < want ? blocks : want);
        s.blocks_per_chunk = blocks / s.chunks;
        s.grid = pairs * s.chunks;
        s.scratch = (u64)s.chunks * 16 << (2 * k);
    }
    return s;
}

static int rdm_form_of(int k) {
    const char *f = getenv("SYMGPU_RDM_FORM");
    if (f && !strcmp(f, "tiled")) return SYMGPU_RDM_TILED;
    if (f && !strcmp(f, "stream") && k <= RDM_KS) return SYMGPU_RDM_STREAM;
    return k <= RDM_KS ? SYMGPU_RDM_STREAM : SYMGPU_RDM_TILED;
}

static int rdm_launch(const RdmShape &s, const f64x2 *psi, f64x2 *partial, f64x2 *rho) {
    hipStream_t st = ctx().stream;
    if (s.form == SYMGPU_RDM_STREAM) {
        const u64 outside = (((u64)1 << s.n) - 1) & ~s.S;
        const u32 LA = (u32)rdm_extract(s.KM, s.S);
        const size_t lds = (size_t)16 << s.m;
        const dim3 grid((unsigned)s.grid), wg(RDM_WG);
        switch (s.k) {
        case 0: hipLaunchKernelGGL(k_rdm_stream<0>, grid, wg, lds, st, psi, s.S, outside, LA, s.m, s.tiles_per_chunk, partial); break;
        case 1: hipLaunchKernelGGL(k_rdm_stream<1>, grid, wg, lds, st, psi, s.S, outside, LA, s.m, s.tiles_per_chunk, partial); break;
        case 2: hipLaunchKernelGGL(k_rdm_stream<2>, grid, wg, lds, st, psi, s.S, outside, LA, s.m, s.tiles_per_chunk, partial); break;
        default: hipLaunchKernelGGL(k_rdm_stream<3>, grid, wg, lds, st, psi, s.S, outside, LA, s.m, s.tiles_per_chunk, partial); break;
        }
        const i64 E = ((i64)1 << s.k) * (((i64)1 << s.k) + 1) / 2;
        hipLaunchKernelGGL(k_rdm_stream_sum, dim3(grid_each(E, RDM_WG)), wg, 0, st, partial, s.chunks, s.k, rho);
    } else {
        const u32 LA = (u32)rdm_extract(rdm_lowest_bits(s.KM, s.tk), s.V);
        hipLaunchKernelGGL(k_rdm_tiled, dim3((unsigned)(s.grid / s.chunks), s.chunks), dim3(RDM_WG), 0, st, psi, s.KM, s.TM, s.V, LA, s.tk, s.sk, s.k, s.nt,
                           s.blocks_per_chunk, partial);
        hipLaunchKernelGGL(k_rdm_tiled_sum, dim3(grid_each((i64)1 << (2 * s.k), RDM_WG)), dim3(RDM_WG), 0, st, partial, s.chunks, s.k, rho);
    }
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_rdm(const double *psi_dev, int n_qubits, const int *kept_host, int k, double *rho_dev, int64_t *info) {
    SG_ENTER();
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32, "rdm: 1 <= n_qubits <= 32");
    SG_REQUIRE(k >= 0 && k <= n_qubits && k <= RDM_MAX_K, "rdm: 0 <= k <= min(n_qubits, 12) kept qubits");
    SG_REQUIRE(psi_dev && rho_dev && (kept_host || k == 0), "rdm: null arguments");
    u64 KM = 0;
    for (int i = 0; i < k; ++i) {
        SG_REQUIRE(kept_host[i] >= 0 && kept_host[i] < n_qubits && (i == 0 || kept_host[i] > kept_host[i - 1]),
                   "rdm: the kept qubits must be strictly ascending in 0 .. n_qubits-1");
        KM |= (u64)1 << (n_qubits - 1 - kept_host[i]);
    }
    const uintptr_t p0 = (uintptr_t)psi_dev, p1 = p0 + ((uintptr_t)16 << n_qubits), r0 = (uintptr_t)rho_dev, r1 = r0 + ((uintptr_t)16 << (2 * k));
    SG_REQUIRE(r1 <= p0 || p1 <= r0, "rdm: rho overlaps psi");
    const RdmShape s = rdm_shape(n_qubits, k, KM, rdm_form_of(k));
    SG_TRY(matvec_require_memory(s.scratch + 4096, "the reduced density matrix"));
    Scratch partial;
    SG_TRY(partial.alloc((size_t)s.scratch));
    SG_TRY(rdm_launch(s, reinterpret_cast<const f64x2 *>(psi_dev), partial.as<f64x2>(), reinterpret_cast<f64x2 *>(rho_dev)));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    if (info) {
        info[0] = s.form;
        info[1] = RDM_KS;
        info[2] = s.chunks;
        info[3] = s.form == SYMGPU_RDM_TILED ? 1 << RDM_T : 0;
        info[4] = (int64_t)s.grid;
        info[5] = (int64_t)s.scratch;
    }
    return SYMGPU_OK;
}

}  // extern "C"
