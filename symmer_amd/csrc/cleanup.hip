// cleanup.hip — the output stage of the cleanup (cleanup_driver.hip): the kept terms (the set bits of a bitmap over the input index space)
// written in input order, rows and summed coefficients.  k_emit_fused for rows of up to 64 chunks, k_emit_meta + k_emit_stream beyond.
#include "cleanup_common.h"
#include <stdlib.h>

namespace symgpu {

__global__ void k_popc_words(const u32 *__restrict__ bits, i64 n_words, u32 *__restrict__ counts) {
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (i64)gridDim.x * blockDim.x) counts[w] = (u32)__popc(bits[w]);
}

// Output stage without any scatter.  The kept terms are the set bits of `markbits` (input index space), and input order IS the
// output order.  Two kernels per BATCH of 2^17 bitmap words (4M input indices; emit_batch_words()):
//  * k_emit_meta: a wavefront takes up to 64 bitmap words, expands their set bits into a compact list in LDS (output slot of the
//    k-th one = word prefix + k), and every lane files one kept term: its summed coefficient (read from where k_heads_sums filed
//    it, nearly sequential) at its output slot and its source (i, o) — 8 bytes — in the batch's list, coalesced.
//  * k_emit_stream: the rows.  Block b writes the b-th 4 KiB of the batch's output — the sequential pattern of the product's row
//    stream (product.hip), which is what the HBM wants.
// Why batches: a saturated HBM write stream tolerates reads that hit in the L2s or in the Infinity Cache, but HBM READS mixed into
// it halve it (tools/ubench_fused.hip, S3: the same stream kernel writes 6.1-6.3 TB/s while its 8-byte-per-row list comes out of
// the Infinity Cache and 3.7-4.0 TB/s when the list was evicted by 256 MB of other traffic or is read with `nt` loads, which
// bypass that cache).  The first version streamed the rows from the wavefronts that decode the bitmap, next to their HBM reads of
// the filed sums (4.2 TB/s); a whole-operator list written first and streamed afterwards is out of the cache again by the time
// it is read (3.8 TB/s).  A batch's list is 32 MB at most, written by one kernel and read by the next.
// TRI (PAIR only): the index space is the compacted slot order of a squared operator (tri_slot / tri_pair).
static i64 emit_batch_words() {                                  // SYMGPU_EMIT_BATCH = log2(bitmap words per batch), default 17 (4M indices)
    const i64 w = [] { const char *e = SG_TUNE("SYMGPU_EMIT_BATCH"); const int l = e ? atoi(e) : 17; return (i64)1 << (l >= 6 && l <= 26 ? l : 17); }();
    return w;
}
template <bool PAIR, bool TRI>
__global__ __launch_bounds__(256) void k_emit_meta(const u32 *__restrict__ markbits, const u32 *__restrict__ wordprefix, i64 w_begin, i64 w_end,
                                                    const double *__restrict__ sum_of, int wpw, u32 Ni,
                                                    uint2 *__restrict__ meta, double *__restrict__ out_coeff, LazyEmit lz, u64 *__restrict__ out_first) {
    __shared__ unsigned short s_list[4][2048];                       // offsets inside the chunk (< 2048)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned short *list = s_list[wave];
    const u32 P0 = wordprefix[w_begin];                              // first output slot of the batch
    // wpw (power of two <= 64) bitmap words per wavefront and step: narrow chunks so that enough waves exist
    const i64 n_chunks = (w_end - w_begin + wpw - 1) / wpw;
    for (i64 chunk = (i64)blockIdx.x * 4 + wave; chunk < n_chunks; chunk += (i64)gridDim.x * 4) {
        const i64 w = w_begin + chunk * wpw + lane;
        const u32 bits = (lane < wpw && w < w_end) ? markbits[w] : 0u;
        const u32 cnt = (u32)__popc(bits);
        u32 incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        const u32 K = __shfl(incl, 63);
        if (K == 0) continue;                                        // wave-uniform
        const u32 p_base = __shfl(wordprefix[w_begin + chunk * wpw], 0);
        {
            u32 b = bits, k = incl - cnt;
            while (b) { list[k++] = (unsigned short)(lane * 32 + __builtin_ctz(b)); b &= b - 1; }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const u32 t_base = (u32)((w_begin + chunk * wpw) * 32);
        for (u32 k = lane; k < K; k += 64) {
            const u32 t = t_base + list[k];
            u32 ti = t, to = 0;
            if (PAIR && TRI) tri_pair(t, Ni, to, ti);
            else if (PAIR) { to = t / Ni; ti = t - to * Ni; }
            double2 cf;
            if (lz.mode == 0 || ((lz.patchbits[t >> 5] >> (t & 31u)) & 1u)) cf = reinterpret_cast<const double2 *>(sum_of)[t];
            else if (lz.mode == 1) {                                  // a single of a packed product: c_i * c_o * i^e from the operand tables
                const int e = (int)(((lz.e_lo[t >> 5] >> (t & 31u)) & 1u) | (((lz.e_hi[t >> 5] >> (t & 31u)) & 1u) << 1));
                double cx, cy;
                pair_coefficient(lz.ci[2 * ti], lz.ci[2 * ti + 1], lz.co[2 * to], lz.co[2 * to + 1], e, cx, cy);
                if (lz.squared && ti != to) {
                    if (e & 1) { cx = 0.0; cy = 0.0; }
                    else { cx = __dadd_rn(cx, cx); cy = __dadd_rn(cy, cy); }
                }
                cf.x = __dadd_rn(0.0, cx); cf.y = __dadd_rn(0.0, cy);
            } else {                                                  // a single of an indexed operator: 0.0 + its own coefficient
                const double2 c0 = reinterpret_cast<const double2 *>(lz.coeff)[t];
                cf.x = __dadd_rn(0.0, c0.x); cf.y = __dadd_rn(0.0, c0.y);
            }
            reinterpret_cast<double2 *>(out_coeff)[(i64)p_base + k] = cf;
            meta[(p_base - P0) + k] = make_uint2(ti, to);
            if (out_first) out_first[(i64)p_base + k] = PAIR ? (((u64)to << 32) | ti) : (u64)t;
        }
        __builtin_amdgcn_wave_barrier();                             // the list is rewritten by the next chunk
    }
}

// RC 16-byte chunks per lane, 256 apart: output chunk f = slot * Wq + c  <-  inner[i][c] ^ outer[o][c]   (plain mode: rows[i][c])
// for the slots [*p_begin, *p_end) of the batch; the grid is sized for a batch whose every index is kept, surplus blocks exit.
template <bool PAIR, int RC>
__global__ __launch_bounds__(256) void k_emit_stream(const uint2 *__restrict__ meta, const u32 *__restrict__ p_begin, const u32 *__restrict__ p_end,
                                                      int Wq, int wsh, const u32x4 *__restrict__ rows, const u32x4 *__restrict__ inner,
                                                      const u32x4 *__restrict__ outer, u32x4 *__restrict__ out_rows) {
    const i64 P0 = *p_begin;
    const i64 n_chunks16 = ((i64)*p_end - P0) * Wq;
    const i64 b0 = (i64)blockIdx.x * (256 * RC);
    if (b0 >= n_chunks16) return;
    const i64 f0 = b0 + threadIdx.x;
    const i64 last = n_chunks16 - 1;
    uint2 m[RC];
    int c[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        const i64 f = f0 + 256 * k < last ? f0 + 256 * k : last;      // clamped: every load is unconditional
        const i64 slot = wsh >= 0 ? f >> wsh : f / Wq;
        c[k] = (int)(f - slot * Wq);
        m[k] = meta[slot];                                            // plain load: served by the Infinity Cache (see above)
    }
    u32x4 v[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k)
        v[k] = PAIR ? (inner[(i64)m[k].x * Wq + c[k]] ^ outer[(i64)m[k].y * Wq + c[k]]) : rows[(i64)m[k].x * Wq + c[k]];
    u32x4 *dst = out_rows + P0 * Wq + f0;
    if (b0 + 256 * RC <= n_chunks16) {
#pragma unroll
        for (int k = 0; k < RC; ++k) __builtin_nontemporal_store(v[k], dst + 256 * k);
    } else {
#pragma unroll
        for (int k = 0; k < RC; ++k)
            if (f0 + 256 * k < n_chunks16) __builtin_nontemporal_store(v[k], dst + 256 * k);
    }
}

// Fused output stage (round 3): ONE launch, one 64-bit bitmap word (64 indices) per wavefront.  The set lanes file their term — source
// (i, o) into LDS, coefficient to its output slot — and the wavefront then streams the K kept rows, 64 consecutive 16-byte chunks per
// step, into [prefix, prefix + K): consecutive wavefronts and workgroups write consecutive pieces (a workgroup's four words make
// ~32 KB at n = 1000), so the chip still writes one moving window.  No list, no batches, no second launch: with the sums of the
// singles no longer read back from HBM (k_mark_singles) nothing but the bitmaps is read beside the row stream.
// NW = bitmap words per wavefront (4: the dependent chain bitmap -> prefix -> phase / patch bits -> operand tables is paid once per 256
// indices; a wavefront per word spent two thirds of its life in it: 4.5 TB/s), U = steps of 64 chunks in flight
template <bool PAIR, bool TRI, int NW, int U>
__global__ __launch_bounds__(256) void k_emit_fused(const u64 *__restrict__ markbits64, const u32 *__restrict__ wordprefix, i64 T, const double *__restrict__ sum_of,
                                                     u32 Ni, int Wq, int wsh, const u32x4 *__restrict__ rows, const u32x4 *__restrict__ inner,
                                                     const u32x4 *__restrict__ outer, u32x4 *__restrict__ out_rows, double *__restrict__ out_coeff, LazyEmit lz,
                                                     u64 *__restrict__ out_first, int pfx_shift /* prefix entries per 64 indices: 1 << pfx_shift */,
                                                     int interleaved) {
    __shared__ u32 s_i[4][64 * NW], s_o[4][64 * NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // XCD-aware order: workgroups go round-robin over the 8 XCDs; every XCD takes a CONTIGUOUS eighth of the bitmap (and of the output) in
    // order instead of every eighth 64 KB piece — 1.13-1.18 -> 1.04 ms at cfg3 (the output stage's write stream reaches 6.5 TB/s) on the
    // arenas that like it and 1.20 ms on those that do not (round 5: the mode follows the memory the driver hands out).  `interleaved`
    // is the plain order (1.10-1.19 ms everywhere); emit_order() measures both on the buffer at hand and keeps the faster.
    const i64 per_xcd = ((i64)gridDim.x + 7) / 8;
    const i64 blk = interleaved ? (i64)blockIdx.x : (i64)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const i64 w0 = (blk * 4 + wave) * NW;
    if (w0 * 64 >= T) return;
    u64 bits[NW];
    u32 off[NW + 1];
    off[0] = 0;
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const i64 w = w0 + u;
        bits[u] = w * 64 < T ? markbits64[w] : 0ULL;
        if (w * 64 < T && T - w * 64 < 64) bits[u] &= (1ULL << (T - w * 64)) - 1ULL;   // the bitmap's last word may be half written (32-bit words)
        off[u + 1] = off[u] + (u32)__popcll(bits[u]);
    }
    const u32 K = off[NW];
    if (K == 0) return;                                              // wave-uniform
    const i64 p_base = wordprefix[w0 << pfx_shift];
    u32 o_min = 0xFFFFFFFFu, o_max = 0u;                             // this lane's kept terms: range of their outer indices
    // Nothing the coefficients need depends on the bitmap's CONTENT: the pair (i, o) of an index, its patch / phase-exponent bits and its
    // operands' coefficients are addressed by the index alone.  They are therefore fetched for all NW x 64 indices at once, next to the
    // bitmap words and the prefix — one memory round trip per wavefront instead of two dependent ones (the prologue alone took 0.25 ms of the
    // stage's 1.19 at cfg3 and did not overlap the row stream).
    u32 ti_[NW], to_[NW], pw_[NW], el_[NW], eh_[NW];
    double2 ca_[NW], cb_[NW], cs_[NW];
    // The pair of the wavefront's FIRST index costs a square root (triangular slots) or a division; every other index of the wavefront is a
    // few additions away: consecutive indices walk along a row of the (o, i) plane and step to the next row when i reaches Ni (the per-index
    // tri_pair of all NW x 64 indices was most of the prologue's 0.25 ms: ~150 instructions each).
    u32 o_first = 0, i_first = 0;
    if (PAIR) {
        const u32 t0 = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(w0 * 64));
        if (TRI) tri_pair(t0, Ni, o_first, i_first);
        else { o_first = t0 / Ni; i_first = t0 - o_first * Ni; }
        o_first = (u32)__builtin_amdgcn_readfirstlane((int)o_first); i_first = (u32)__builtin_amdgcn_readfirstlane((int)i_first);
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        const i64 tt = (w0 + u) * 64 + lane;
        const u32 t = (u32)(tt < T ? tt : T - 1);                     // clamped: the surplus lanes of the last word load valid addresses
        ti_[u] = t; to_[u] = 0;
        if (PAIR) {
            u32 o = o_first;
            u64 i = (u64)i_first + (t - (u32)(w0 * 64));
            // row o holds the indices i in [TRI ? o : 0, Ni): step rows while i runs past the end (0 or 1 steps except in the last short rows)
            while (i >= Ni) { i -= Ni; ++o; if (TRI) i += o; }
            to_[u] = o; ti_[u] = (u32)i;
        }
        pw_[u] = lz.mode != 0 ? lz.patchbits[t >> 5] : 0xFFFFFFFFu;
        if (lz.mode == 1) {
            el_[u] = lz.e_lo[t >> 5]; eh_[u] = lz.e_hi[t >> 5];
            ca_[u] = reinterpret_cast<const double2 *>(lz.ci)[ti_[u]];
            cb_[u] = reinterpret_cast<const double2 *>(lz.co)[to_[u]];
        } else if (lz.mode == 2) {
            cs_[u] = reinterpret_cast<const double2 *>(lz.coeff)[t];
        }
    }
#pragma unroll
    for (int u = 0; u < NW; ++u) {
        if ((bits[u] >> lane) & 1ULL) {
            const u32 rank = off[u] + (u32)__popcll(bits[u] & ((1ULL << lane) - 1ULL));
            const u32 t = (u32)((w0 + u) * 64 + lane);
            const u32 ti = ti_[u], to = to_[u];
            double2 cf;
            if (lz.mode == 0 || ((pw_[u] >> (t & 31u)) & 1u)) cf = reinterpret_cast<const double2 *>(sum_of)[t];
            else if (lz.mode == 1) {                                  // a single of a packed product: c_i * c_o * i^e from the operand tables
                const int e = (int)(((el_[u] >> (t & 31u)) & 1u) | (((eh_[u] >> (t & 31u)) & 1u) << 1));
                double cx, cy;
                pair_coefficient(ca_[u].x, ca_[u].y, cb_[u].x, cb_[u].y, e, cx, cy);
                if (lz.squared && ti != to) {
                    if (e & 1) { cx = 0.0; cy = 0.0; }
                    else { cx = __dadd_rn(cx, cx); cy = __dadd_rn(cy, cy); }
                }
                cf.x = __dadd_rn(0.0, cx); cf.y = __dadd_rn(0.0, cy);
            } else {                                                  // a single of an indexed operator: 0.0 + its own coefficient
                cf.x = __dadd_rn(0.0, cs_[u].x); cf.y = __dadd_rn(0.0, cs_[u].y);
            }
            reinterpret_cast<double2 *>(out_coeff)[p_base + rank] = cf;
            if (out_first) out_first[p_base + rank] = PAIR ? (((u64)to << 32) | ti) : (u64)t;
            s_i[wave][rank] = ti; s_o[wave][rank] = to;
            o_min = to < o_min ? to : o_min; o_max = to > o_max ? to : o_max;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const u32 n_ch = K * (u32)Wq;
    u32x4 *dst = out_rows + p_base * Wq;
    // One outer row for the whole wavefront (a product's terms are ordered by their outer index, so 256 consecutive indices nearly always
    // share it) and a row length that divides 64: the lane's chunk of that row is loop invariant — one gather and one list read per
    // 16 bytes written instead of two each.
    bool one_outer = false;
    if (PAIR && wsh >= 0 && Wq <= 64 && lz.no_one_outer == 0) {
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) {
            const u32 a = (u32)__shfl_xor((int)o_min, sft), b = (u32)__shfl_xor((int)o_max, sft);
            o_min = a < o_min ? a : o_min; o_max = b > o_max ? b : o_max;
        }
        one_outer = o_min == o_max;                                   // wave-uniform
    }
    if (one_outer) {
        const u32x4 oc = outer[(i64)o_min * Wq + (lane & (Wq - 1))];
        for (u32 f0 = 0; f0 < n_ch; f0 += 64 * U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const u32 f = f0 + 64 * u + lane < n_ch ? f0 + 64 * u + lane : n_ch - 1;
                const u32 r = f >> wsh;
                v[u] = inner[(i64)s_i[wave][r] * Wq + (lane & (Wq - 1))] ^ oc;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (f0 + 64 * u + lane < n_ch) __builtin_nontemporal_store(v[u], dst + f0 + 64 * u + lane);
        }
        return;
    }
    for (u32 f0 = 0; f0 < n_ch; f0 += 64 * U) {
        u32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32 f = f0 + 64 * u + lane < n_ch ? f0 + 64 * u + lane : n_ch - 1;
            const u32 r = wsh >= 0 ? f >> wsh : f / (u32)Wq;
            const u32 c = f - r * (u32)Wq;
            v[u] = PAIR ? (inner[(i64)s_i[wave][r] * Wq + c] ^ outer[(i64)s_o[wave][r] * Wq + c]) : rows[(i64)s_i[wave][r] * Wq + c];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (f0 + 64 * u + lane < n_ch) __builtin_nontemporal_store(v[u], dst + f0 + 64 * u + lane);
    }
}

// Reads every 16-byte chunk of a buffer and keeps nothing: run right before the output stage on the bitmaps it decodes (written two
// gigabytes of traffic earlier, so out of the Infinity Cache again) — a saturated HBM WRITE stream tolerates cache hits, but every HBM
// read mixed into it costs the DRAM a turn-around.
struct TouchMaps { const u32x4 *p[5]; i64 n16[5]; };
__global__ __launch_bounds__(256) void k_touch(TouchMaps tm, u32 *__restrict__ sink) {
    u32 acc = 0;
#pragma unroll
    for (int m = 0; m < 5; ++m)
        for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < tm.n16[m]; i += (i64)gridDim.x * 256) { const u32x4 v = tm.p[m][i]; acc |= v.x & v.y & v.z & v.w; }
    if (acc == 0xDEADBEEFu) *sink = acc;                           // (never true for bitmaps of a real run; keeps the loads alive)
}

// T = size of the index space the kept terms are filed under (pair indices, or the slots of a squared operator: `tri`)
// word prefix of the kept-term bitmap (the output slot of every 32 indices' first kept term) + the number of kept terms, on the device
// wide: one prefix entry per 64 indices (all the fused output stage reads) instead of per 32: half the elements to count and scan
__global__ void k_popc_words64_tail(const u64 *__restrict__ bits, i64 n64, i64 n32, u32 *__restrict__ counts) {
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < n64; w += (i64)gridDim.x * blockDim.x) {
        u64 b = bits[w];
        if (w == n64 - 1 && (n32 & 1)) b &= 0xFFFFFFFFULL;           // the bitmap is written in 32-bit words: the last upper half may be unwritten
        counts[w] = (u32)__popcll(b);
    }
}
int emit_prefix(const u32 *markbits_p, i64 T, Scratch &wordprefix, Scratch &total, bool wide) {
    hipStream_t st = ctx().stream;
    const i64 n_words = (T + 31) / 32, n64 = (T + 63) / 64;
    const i64 n = wide ? n64 : n_words;
    SG_TRY(wordprefix.alloc((size_t)n * 4));
    SG_TRY(total.alloc(32));                                       // [0] the count, [2] k_touch's sink
    if (wide && n64 <= POPC_SCAN_SMALL_MAX) return popc_scan_small(reinterpret_cast<const u64 *>(markbits_p), n64, n_words, wordprefix.as<u32>(), total.as<u32>());
    if (wide) hipLaunchKernelGGL(k_popc_words64_tail, dim3(grid_for(n64)), dim3(256), 0, st, reinterpret_cast<const u64 *>(markbits_p), n64, n_words, wordprefix.as<u32>());
    else hipLaunchKernelGGL(k_popc_words, dim3(grid_for(n_words)), dim3(256), 0, st, markbits_p, n_words, wordprefix.as<u32>());
    KERNEL_CHECK();
    return exclusive_scan_u32(wordprefix.as<u32>(), wordprefix.as<u32>(), n, total.as<u32>());
}

// Which block order the fused output stage takes on THIS output buffer (the XCD-contiguous order is 15 % faster or 3 %
// slower than the plain one depending on the memory behind the buffer, which a process cannot choose).  A large output (>= 512 MB) is
// written into blocks the allocator hands out again and again (a loop of calls alternates between two of them): per block, the first four
// calls alternate the two orders under a pair of events, from the fifth on the block is written in the order whose faster sample won.
// Both orders write the same bytes.  SYMGPU_EMIT_ORDER=0 / 1 pins the contiguous / plain order (tests).
struct EmitOrder { int interleaved = 0; EmitProbe *probe = nullptr; };
static int emit_order_begin(const void *dst, size_t bytes, EmitOrder &eo) {
    Context &c = ctx();
    if (const char *e = getenv("SYMGPU_EMIT_ORDER")) { eo.interleaved = e[0] == '1'; return SYMGPU_OK; }
    if (bytes < ((size_t)512 << 20)) return SYMGPU_OK;
    EmitProbe *p = nullptr, *oldest = &c.emit_probe[0];
    for (auto &q : c.emit_probe) {
        if (q.key == dst) { p = &q; break; }
        if (q.stamp < oldest->stamp) oldest = &q;
    }
    if (!p) { p = oldest; p->key = dst; p->phase = 0; p->best[0] = p->best[1] = 1e30f; }
    p->stamp = ++c.emit_stamp;
    if (p->phase > 0 && p->phase <= 4) {                          // the sample of this block's previous call (two or more calls ago: complete)
        float ms = 0;
        if (hipEventSynchronize(p->ev[1]) == hipSuccess && hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) {
            const int o = (p->phase - 1) & 1;
            if (ms < p->best[o]) p->best[o] = ms;
        } else (void)hipGetLastError();
        if (p->phase == 4) { p->choice = p->best[1] < p->best[0] ? 1 : 0; p->phase = 5; }
    }
    if (p->phase >= 5) { eo.interleaved = p->choice; return SYMGPU_OK; }
    if (!p->ev[0]) { HIP_TRY(hipEventCreate(&p->ev[0])); HIP_TRY(hipEventCreate(&p->ev[1])); }
    eo.interleaved = p->phase & 1;                                // 0, 1, 0, 1
    eo.probe = p;
    HIP_TRY(hipEventRecord(p->ev[0], c.stream));
    return SYMGPU_OK;
}
static void emit_order_end(const EmitOrder &eo) {
    if (!eo.probe) return;
    (void)hipEventRecord(eo.probe->ev[1], ctx().stream);
    ++eo.probe->phase;
}

// one launch over the bitmaps the fused output stage decodes (five launches of 2 us each sat 6 us apart behind the host's read-back)
int emit_touch(const u32 *markbits_p, i64 T, const LazyEmit &lz, EmitPrefix &pre) {
    const i64 n16 = (T + 63) / 64 / 2;                              // whole 16-byte chunks of a T-bit map
    pre.touched = true;
    if (n16 <= 0 || T < ((i64)1 << 23)) return SYMGPU_OK;           // (five maps of < 1 MiB each: still cached from the kernels that wrote them)
    TouchMaps tm;
    const void *maps[5] = {markbits_p, pre.wordprefix.p, lz.mode ? (const void *)lz.patchbits : nullptr, lz.mode == 1 ? (const void *)lz.e_lo : nullptr,
                           lz.mode == 1 ? (const void *)lz.e_hi : nullptr};
    for (int m = 0; m < 5; ++m) {
        tm.p[m] = reinterpret_cast<const u32x4 *>(maps[m]);
        tm.n16[m] = maps[m] ? (m == 1 ? (pre.wide ? n16 / 2 : 2 * n16) : n16) : 0;     // (the prefix: 4 bytes per 64 or per 32 indices)
    }
    hipLaunchKernelGGL(k_touch, dim3(grid_for(2 * n16)), dim3(256), 0, ctx().stream, tm, pre.total.as<u32>() + 2);
    KERNEL_CHECK();
    return SYMGPU_OK;
}
// pre: the prefix over the kept-term bitmap and the count of kept terms (formed and read back by the attempt that succeeded)
int cleanup_finish(u32 *markbits_p, const double *sum_of_p, i64 T, bool pair, const u64 *rows, int W, const u64 *inner, i64 Ni,
                   const u64 *outer, symgpu_op_t *out, int Wq_out, bool tri, const LazyEmit &lz, bool want_first, const CleanupSwitches &sw,
                   EmitPrefix &pre) {
    hipStream_t st = ctx().stream;
    const i64 n_words = (T + 31) / 32;
    Scratch &wordprefix = pre.wordprefix, &total = pre.total;
    const i64 n_out = pre.n_out;
    OwnedOp res;
    SG_TRY(res.alloc(rows_or_one(n_out), n_out, Wq_out, true));
    if (want_first) SG_TRY(res.attach_first());
    if (n_out > 0) {
        const int Wq = W / 2;
        const int wsh = (Wq & (Wq - 1)) == 0 ? __builtin_ctz((unsigned)Wq) : -1;
        const u32x4 *pin = reinterpret_cast<const u32x4 *>(inner), *pout = reinterpret_cast<const u32x4 *>(outer);
        u32x4 *dst = reinterpret_cast<u32x4 *>(res->rows);
        // (rows of more than 64 chunks keep the batched stage: there every workgroup of the grid shares the chunks of a row, here a
        // wavefront streams its own rows alone — two 10^8-qubit terms: 2.9 ms against 8.5 ms)
        const bool fused = sw.fused(Wq);
        if (fused) {
            const i64 n_w64 = (T + 63) / 64;
            // wavefront shape: bitmap words per wavefront x 64-chunk steps in flight (SYMGPU_EMIT_SHAPE = "NW,U": experiments)
            const int shape = sw.emit_shape;
            const int NWs = shape / 16, Us = shape % 16;
            const int NWr = (NWs == 1 || NWs == 4 || NWs == 8) ? NWs : 2;   // 2 words per wavefront, 4 steps in flight: 1.20 ms at cfg3 (4,4: 1.30; 1,4: 1.24; 2,8: 1.22)
            const dim3 gfu((unsigned)(((n_w64 + 4 * NWr - 1) / (4 * NWr) + 7) / 8 * 8));     // a multiple of 8: the kernel's XCD-aware order is a bijection then
            if (sw.emit_touch != 0 && !pre.touched) SG_TRY(emit_touch(markbits_p, T, lz, pre));
            EmitOrder eo;
            SG_TRY(emit_order_begin(dst, (size_t)n_out * (size_t)(16 * Wq + 16), eo));
            ProfScope prof(3);
#define LAUNCH_FUSED_S(P, TR, NWV, UV) hipLaunchKernelGGL((k_emit_fused<P, TR, NWV, UV>), gfu, dim3(256), 0, st, reinterpret_cast<const u64 *>(markbits_p), wordprefix.as<u32>(), T, sum_of_p, \
                                               (u32)(pair ? Ni : 1), Wq, wsh, reinterpret_cast<const u32x4 *>(rows), pin, pout, dst, res->coeff, lz, res->first, pre.wide ? 0 : 1, eo.interleaved)
#define LAUNCH_FUSED_U(P, TR, NWV) do { if (Us == 8) LAUNCH_FUSED_S(P, TR, NWV, 8); else if (Us == 2) LAUNCH_FUSED_S(P, TR, NWV, 2); else LAUNCH_FUSED_S(P, TR, NWV, 4); } while (0)
#define LAUNCH_FUSED(P, TR) do { if (NWr == 1) LAUNCH_FUSED_U(P, TR, 1); else if (NWr == 4) LAUNCH_FUSED_U(P, TR, 4); else if (NWr == 8) LAUNCH_FUSED_U(P, TR, 8); \
                                 else LAUNCH_FUSED_U(P, TR, 2); } while (0)
            if (pair && tri) LAUNCH_FUSED(true, true); else if (pair) LAUNCH_FUSED(true, false); else LAUNCH_FUSED(false, false);
            emit_order_end(eo);
#undef LAUNCH_FUSED_S
#undef LAUNCH_FUSED_U
#undef LAUNCH_FUSED
        } else {
        const int rc_env = sw.emit_rc;                                    // chunks per lane: 1: 115, 2: 97, 4: 97 us per batch
        const int RCs = rc_env == 1 || rc_env == 4 ? rc_env : 2;
        const i64 EMIT_BATCH_WORDS = emit_batch_words();
        const i64 bw = n_words < EMIT_BATCH_WORDS ? n_words : EMIT_BATCH_WORDS;
        Scratch meta;
        SG_TRY(meta.alloc((size_t)bw * 32 * sizeof(uint2)));
        int wpw = 64;                                            // bitmap words per wavefront: aim at >= 16k wavefronts per batch
        while (wpw > 1 && (bw + wpw - 1) / wpw < 16384) wpw >>= 1;
        for (i64 w0 = 0; w0 < n_words; w0 += EMIT_BATCH_WORDS) {
            const i64 w1 = w0 + EMIT_BATCH_WORDS < n_words ? w0 + EMIT_BATCH_WORDS : n_words;
            i64 ge = ((w1 - w0 + wpw - 1) / wpw + 3) / 4;
            if (ge > 16384) ge = 16384;
#define LAUNCH_META(P, TR) hipLaunchKernelGGL((k_emit_meta<P, TR>), dim3((unsigned)ge), dim3(256), 0, st, markbits_p, wordprefix.as<u32>(), w0, w1, sum_of_p, wpw, \
                                              (u32)(pair ? Ni : 1), meta.as<uint2>(), res->coeff, lz, res->first)
            if (pair && tri) LAUNCH_META(true, true); else if (pair) LAUNCH_META(true, false); else LAUNCH_META(false, false);
#undef LAUNCH_META
            const u32 *p_begin = wordprefix.as<u32>() + w0;
            const u32 *p_end = w1 < n_words ? wordprefix.as<u32>() + w1 : total.as<u32>();
            const i64 gs = ((w1 - w0) * 32 * Wq + 256 * RCs - 1) / (256 * RCs);     // as if every index of the batch were kept
#define LAUNCH_STREAM(P, R) hipLaunchKernelGGL((k_emit_stream<P, R>), dim3((unsigned)gs), dim3(256), 0, st, meta.as<uint2>(), p_begin, p_end, Wq, wsh, \
                                               reinterpret_cast<const u32x4 *>(rows), pin, pout, dst)
            {
                ProfScope prof(3);
                if (pair) { if (RCs == 1) LAUNCH_STREAM(true, 1); else if (RCs == 4) LAUNCH_STREAM(true, 4); else LAUNCH_STREAM(true, 2); }
                else { if (RCs == 1) LAUNCH_STREAM(false, 1); else if (RCs == 4) LAUNCH_STREAM(false, 4); else LAUNCH_STREAM(false, 2); }
            }
#undef LAUNCH_STREAM
        }
        }
        KERNEL_CHECK();
        HIP_TRY(hipStreamSynchronize(st));                   // the scratch buffers are freed on return; keep ordering simple
    }
    res->dup_free = 1;                                          // merged: no two equal rows
    res.hand_out(out);
    return SYMGPU_OK;
}

}  // namespace symgpu
