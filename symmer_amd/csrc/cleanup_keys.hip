// cleanup_keys.hip — two stages of a cleanup attempt (cleanup_driver.hip).  Hash and key: row hashes, pair keys or key bytes, the marking
// of the single terms in index order.  Order: the complete radix sort, or a partial sort + flag pass (k_find_suspects, pair_dups.hip).
#include "cleanup_common.h"

namespace symgpu {

__global__ void k_pair_keys(const u64 *__restrict__ hI, i64 Ni, const u64 *__restrict__ hO, i64 T, u64 *__restrict__ keys, u32 *__restrict__ idx) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        const i64 o = t / Ni, i = t - o * Ni;
        keys[t] = hI[i] ^ hO[o];
        idx[t] = (u32)t;
    }
}

// ---- terms that merge with nothing ("singles") never pass through the sorted order ------------------------------------------------
// An operator product without repeated rows — the common case, and the benchmark's — merges nothing: every sorted key is a segment of
// its own.  Filing 2.5e7 sums under their first index from the SORTED order is a random 16-byte scatter plus a bitmap atomic per
// term (WRITE_SIZE 1.56 GB for 0.4 GB of sums: 1.0 of k_heads_sums' 1.36 ms at cfg3), and the output stage then reads them back.
// Instead the fate of a term AS IF IT WERE ALONE is decided here, in INDEX order and before the sort — strict |c| > thr on
// 0.0 + c, exactly the sum k_heads_sums forms for a one-element segment — with coalesced bitmap stores; the packed pair key's
// phase exponent goes to two more bitmaps (the sort scrambles the keys).  k_heads_sums then only touches the members of segments
// with MORE than one element: the followers clear their bits, the head files the sum and sets its `patch` bit; k_emit_meta takes a
// patched term's coefficient from the filed sum and rebuilds every other one from the operand tables (cache resident).  Nothing
// about the result changes: same kept set, same order, same sums.
// PACKED: keys[s] is the packed key of index s (pair index, or slot of a squared operator); otherwise coeff[s].
// One workgroup per tile of SORT_TILE indices (= the radix sort's tile).  hist != null (packed keys): the same pass forms the digit
// histograms of the sort's first pass, which reads these very keys in this very order (one HBM pass over the keys less).
// smallest max(|re|, |im|) over the terms of an operand (0 if a component is not finite), as the bit pattern of a non-negative double
// (ordered like the unsigned integer): *slot starts as all ones
__global__ __launch_bounds__(1024) void k_coeff_floor(const double *__restrict__ c0, i64 n0, const double *__restrict__ c1, i64 n1,
                                                      unsigned long long *__restrict__ slot0, int one_block) {
    const double *__restrict__ c = blockIdx.y ? c1 : c0;           // one_block: grid (1, 2) = operand 0 / operand 1 -> slot0[0] / slot0[1]
    const i64 n = blockIdx.y ? n1 : n0;
    unsigned long long *slot = slot0 + blockIdx.y;
    __shared__ unsigned long long s_min;
    if (one_block) { if (threadIdx.x == 0) s_min = ~0ULL; __syncthreads(); }
    double m = __builtin_inf();
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 t0 = (i64)blockIdx.x * blockDim.x + threadIdx.x; t0 < n; t0 += 4 * stride) {      // four loads in flight
        double2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const i64 t = t0 + k * stride; v[k] = reinterpret_cast<const double2 *>(c)[t < n ? t : n - 1]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = fabs(v[k].x), b = fabs(v[k].y);
            const double mx = (a <= __DBL_MAX__ && b <= __DBL_MAX__) ? (a > b ? a : b) : 0.0;
            m = mx < m ? mx : m;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(m, d); m = o < m ? o : m; }
    if ((threadIdx.x & 63) == 0) atomicMin(one_block ? &s_min : slot, (unsigned long long)__double_as_longlong(m));
    if (one_block) { __syncthreads(); if (threadIdx.x == 0) *slot = s_min; }
}
// floor_i / floor_o (packed keys; null: none): k_coeff_floor of the two operands.  |c_i c_o| >= floor_i * floor_o, the larger component of
// the computed product is at least 0.7 of that, so when half of it exceeds thr every pair of non-zero weight is kept WHATEVER its
// coefficient: the two table gathers, the complex product and the comparison (50 of the kernel's 70 instructions per key) are skipped
// — the decision is the same, it is just not computed (cfg3: 0.19 -> see DESIGN 3.3).  It needs finite operands (a product of finite
// factors never has two NaN components, and an inf component is kept) and a normal floor product (no subnormal rounding eats the 0.7).
__device__ __forceinline__ bool floors_clear(double fi, double fo, double thr) { return 0.5 * fi * fo > thr && fi * fo > 0x1p-1000; }
template <bool PACKED>
__global__ __launch_bounds__(256) void k_mark_singles(const u64 *__restrict__ keys, const double *__restrict__ coeff, i64 space, PackedLayout L,
                                                       const double *__restrict__ ci, const double *__restrict__ co, int squared, double thr, int use_thr,
                                                       u64 *__restrict__ markbits64, u64 *__restrict__ e_lo64, u64 *__restrict__ e_hi64,
                                                       u32 *__restrict__ hist, int hist_shift, i64 n_tiles, const double *__restrict__ floor_i,
                                                       const double *__restrict__ floor_o) {
    __shared__ u32 s_h[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool all_kept = PACKED && (!use_thr || (floor_i && floor_o && floors_clear(floor_i[0], floor_o[0], thr)));   // block-uniform
    if (hist) { s_h[threadIdx.x] = 0; __syncthreads(); }
    const i64 tile_base = (i64)blockIdx.x * SORT_TILE;
#pragma unroll 1
    for (int step = 0; step < SORT_TILE / 1024; ++step) {             // four 64-index chunks per wavefront and step, their loads in flight together
        const i64 g0 = tile_base + step * 1024 + wave * 256;
        if (g0 >= space) break;                                       // wave-uniform
        u64 k[4];
        double2 cf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i64 sidx = g0 + 64 * j + lane;
            k[j] = 0ULL; cf[j].x = 0.0; cf[j].y = 0.0;
            if (sidx < space) {
                if (PACKED) k[j] = keys[sidx];
                else cf[j] = reinterpret_cast<const double2 *>(coeff)[sidx];
            }
        }
        // the operand coefficients of all four chunks are fetched before the first one is used (gathers from the cache-resident tables:
        // one after the other they were four dependent round trips per step, and the kernel was bound by them)
        double2 ca[4], cb[4];
        if (PACKED && !all_kept) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32 i = L.i(k[j]), o = L.o(k[j]);                // (lanes past the end hold key 0: term 0 of both tables)
                ca[j] = reinterpret_cast<const double2 *>(ci)[i];
                cb[j] = reinterpret_cast<const double2 *>(co)[o];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i64 sidx = g0 + 64 * j + lane;
            if (g0 + 64 * j >= space) break;                          // wave-uniform
            const bool valid = sidx < space;
            double cx = cf[j].x, cy = cf[j].y;
            int e = 0;
            bool keep;
            if (PACKED && all_kept) {
                if (valid && hist) atomicAdd(&s_h[(u32)(k[j] >> hist_shift) & 255u], 1u);
                e = L.e(k[j]);
                // the weight-0 pairs of a squared operator (anticommuting, off the diagonal) are exact zeros: kept only without a threshold
                keep = valid && !(use_thr && squared && (e & 1) && L.i(k[j]) != L.o(k[j]) && !(0.0 > thr));
            } else {
            if (PACKED && valid) {
                if (hist) atomicAdd(&s_h[(u32)(k[j] >> hist_shift) & 255u], 1u);
                const u32 i = L.i(k[j]), o = L.o(k[j]);
                e = L.e(k[j]);
                pair_coefficient(ca[j].x, ca[j].y, cb[j].x, cb[j].y, e, cx, cy);
                if (squared && i != o) {
                    if (e & 1) { cx = 0.0; cy = 0.0; }
                    else { cx = __dadd_rn(cx, cx); cy = __dadd_rn(cy, cy); }
                }
            }
            // strict |c| > thr as NumPy decides it (common.h)
            keep = valid && (!use_thr || above_thr(cx, cy, thr));
            }
            const u64 mk = __ballot(keep);
            const i64 chunk = (g0 + 64 * j) / 64;
            if (PACKED) {
                const u64 lo = __ballot(e & 1), hi = __ballot(e & 2);
                if (lane == 0) { markbits64[chunk] = mk; e_lo64[chunk] = lo; e_hi64[chunk] = hi; }
            } else if (lane == 0) markbits64[chunk] = mk;
        }
    }
    if (hist) {
        __syncthreads();
        hist[(i64)blockIdx.x * 256 + threadIdx.x] = s_h[threadIdx.x];         // tile-major, as k_rs_hist files it
    }
}

// Round 6: the same marking from ONE BYTE per pair (PairKeyArgs::ebytes: e | (i == o) << 2, written by the key kernel in index order in
// place of the keys) — where the pairs that share a key are found from the operand hash tables (pair_dups.hip) the marking was the only
// reader of the 400 MB of keys (0.14 ms at cfg3: bound by the latency of its 8-byte loads).  A lane takes 16 consecutive indices (one 16-byte
// load), forms its 16 bits of the three bitmaps with byte-parallel arithmetic and stores them as 2 bytes each (a wavefront: 128 contiguous
// bytes per bitmap): 50 MB in, 19 MB out.  When the operands' coefficient floors do not settle the decision (all_kept false) the sixteen
// pairs are decided one by one from the operand tables like k_mark_singles does.
// index -> (i, o) of a pair: general o * Ni + i; squared operator: the compacted slot of PairKeyArgs
__device__ __forceinline__ void pair_of_index(i64 pos, i64 Ni, int squared, i64 &i, i64 &o) {
    if (!squared) { o = pos / Ni; i = pos - o * Ni; return; }
    // row o starts at s(o) = o (2 Ni - o + 1) / 2: the largest o with s(o) <= pos
    const double b = 2.0 * (double)Ni + 1.0;
    i64 oo = (i64)((b - sqrt(b * b - 8.0 * (double)pos)) * 0.5);
    if (oo < 0) oo = 0;
    if (oo >= Ni) oo = Ni - 1;
    while (oo > 0 && oo * (2 * Ni - oo + 1) / 2 > pos) --oo;
    while (oo + 1 < Ni && (oo + 1) * (2 * Ni - oo) / 2 <= pos) ++oo;
    o = oo;
    i = pos - oo * (2 * Ni - oo + 1) / 2 + oo;
}
__device__ __forceinline__ u32 pack_bit0_of_bytes(u32 w) { return ((w & 0x01010101u) * 0x01020408u) >> 24 & 0xFu; }   // bit 0 of the four bytes -> four bits
__global__ __launch_bounds__(256) void k_mark_bytes(const u32x4 *__restrict__ eb, i64 space, i64 n_groups, i64 Ni, const double *__restrict__ ci,
                                                     const double *__restrict__ co, int squared, double thr, int use_thr, unsigned short *__restrict__ mark16,
                                                     unsigned short *__restrict__ lo16, unsigned short *__restrict__ hi16, const double *__restrict__ floor_i,
                                                     const double *__restrict__ floor_o) {
    const bool all_kept = !use_thr || (floor_i && floor_o && floors_clear(floor_i[0], floor_o[0], thr));     // uniform
    const bool drop_rule = use_thr && squared && !(0.0 > thr);           // the anticommuting off-diagonal pairs of a squared operator are exact zeros
    for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (i64)gridDim.x * blockDim.x) {
        const i64 p0 = g * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (p0 < space) v = __builtin_nontemporal_load(eb + g);
        u32 valid = 0xFFFFu;
        if (p0 + 16 > space) valid = p0 < space ? (1u << (int)(space - p0)) - 1u : 0u;
        u32 lo = 0, hi = 0, drop = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const u32 w = v[q];
            lo |= pack_bit0_of_bytes(w) << (4 * q);
            hi |= pack_bit0_of_bytes(w >> 1) << (4 * q);
            drop |= pack_bit0_of_bytes(w & ~(w >> 2)) << (4 * q);        // e odd and not the diagonal
        }
        lo &= valid; hi &= valid;
        u32 keep;
        if (all_kept) keep = valid & (drop_rule ? ~drop : 0xFFFFu);
        else {
            keep = 0;
            for (int k = 0; k < 16; ++k) {
                if (!((valid >> k) & 1u)) continue;
                i64 i, o;
                pair_of_index(p0 + k, Ni, squared, i, o);
                const int e = (int)(((lo >> k) & 1u) | (((hi >> k) & 1u) << 1));
                double cx, cy;
                pair_coefficient(ci[2 * i], ci[2 * i + 1], co[2 * o], co[2 * o + 1], e, cx, cy);
                if (squared && i != o) {
                    if (e & 1) { cx = 0.0; cy = 0.0; }
                    else { cx = __dadd_rn(cx, cx); cy = __dadd_rn(cy, cy); }
                }
                const bool kp = !use_thr || above_thr(cx, cy, thr);
                keep |= (kp ? 1u : 0u) << k;
            }
        }
        mark16[g] = (unsigned short)keep; lo16[g] = (unsigned short)lo; hi16[g] = (unsigned short)hi;
    }
}
// the flagged pairs' packed keys rebuilt in place from their indices (k_compact_suspects with keys == null leaves those), the byte and the
// operand hash tables; *n_flagged is the device-side count (the host does not know it yet)
__global__ __launch_bounds__(256) void k_keys_of_indices(u64 *__restrict__ out, const u32 *__restrict__ n_flagged, const unsigned char *__restrict__ eb, i64 Ni, int squared,
                                                          PackedLayout L, const u64 *__restrict__ hI, const u64 *__restrict__ hO) {
    const u64 hmask = ~((1ULL << L.F()) - 1ULL);
    const i64 n = n_flagged[0];
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (i64)gridDim.x * blockDim.x) {
        const i64 pos = (i64)out[t];
        i64 i, o;
        pair_of_index(pos, Ni, squared, i, o);
        const u64 e = eb[pos] & 3u;
        out[t] = ((hI[i] ^ hO[o]) & hmask) | (e << (L.bi + L.bo)) | ((u64)o << L.bi) | (u64)i;
    }
}

// ---- products without repeated rows: the keys that COULD merge are few — find them after a partial sort, sort only them ---------------
// The radix sort exists to bring equal keys together, but a product of operators without repeated rows merges next to nothing (cfg3:
// the N diagonal pairs of P * P and nothing else), and the lazy flow has already decided every other term in index order
// (k_mark_singles).  So the sort stops early: after `run_bits` / 8 passes the keys are ordered by hash bits [lo, lo + run_bits), a RUN of
// equal bits holds ~Tk / 2^run_bits keys still in ascending index order (LSD passes are stable), and equal FULL keys can only sit in
// one run.  k_find_suspects flags every key that has an equal full key somewhere in its run — both partners — plus every key whose hash
// field is zero (the identity segment of a squared operator, N keys in one run).  The flagged keys are compacted IN ARRAY ORDER (so equal
// keys stay in index order), sorted completely — a few thousand keys instead of 5e7 — and handed to the unchanged segment machinery
// (fix-up, identity segment, k_heads_sums), which only ever acts on segments of more than one key.  Inputs full of repeated rows flag
// most keys: the caller then finishes the remaining passes on the whole array and carries on as before (the partial sort is the old
// sort's first passes, nothing is wasted but the flag pass).
// Round 4 stopped ONE pass early (runs of 3 keys, each key compared with its 12 predecessors in registers).  Round 5 stops when a run
// holds <= 1,024 keys on average (cfg3: two passes of four, runs of 763) and finds the partners inside a run through LDS: one scatter,
// one histogram and one scan pass over 5e7 keys less (0.27 ms), for a flag pass of the same cost.
//
// A workgroup owns the runs that START in its tile of 4,096 positions: it skips the head of the tile that continues the previous tile's
// run and reads on past the end of the tile until its last run ends (the neighbour skips exactly those keys).  The words w = key bits
// [32, 64) of the owned keys go through a pair of LDS bitmaps (2^17 bits each): `seen`, and `dup` for a bit that was already set.  Every
// key whose `dup` bit is set — the keys that have a partner, plus ~6 % chance hits — is listed, the listed words are compared all against
// all from LDS (two lanes per key, no memory access in the loop), and an equal word is followed up with the hash field and then the full
// 64-bit keys rebuilt from the operand hash tables, exactly the test the segment machinery makes.  A list that overflows flags every key
// the workgroup owns; a run longer than SUS_MAX_EXT extension steps raises `giveup` (the caller finishes the sort).  The kernel is bound
// by its LDS atomics and the chain of dependent phases of a workgroup, not by bandwidth (the loads alone: 0.09 ms of its 0.17).
constexpr int SUS_TILE = 4096;
constexpr int SUS_BLOOM = 17;                                          // log2 bits per bitmap: 16 KB each
constexpr int SUS_CAND = 960;                                          // (four workgroups' LDS per CU: 4 x 40.4 KB)
constexpr int SUS_MAX_EXT = 64;                                        // steps of 1,024 keys a workgroup reads past its tile
constexpr int SUS_WAVES = 8;                                           // 512 threads: eight keys of the tile and two of an extension step per lane
constexpr int SUS_ROWS = SUS_TILE / (64 * SUS_WAVES), SUS_XROWS = 1024 / (64 * SUS_WAVES);
__device__ __forceinline__ u32 wave_shr1(u32 v, u32 lane0) {            // lane L <- v[L - 1], lane 0 <- lane0 (DPP wave_shr:1, one VALU instruction)
    return (u32)__builtin_amdgcn_update_dpp((int)lane0, (int)v, 0x138, 0xf, 0xf, false);
}
// w = the upper half of a key: run bits v below, sixteen more hash bits u above.  Inside a workgroup's range v takes a handful of consecutive
// values: the slot of a word is (u, v mod 2) (one v_alignbit + one v_and).  ~6 % of the keys are listed without having a partner (another
// run of the same parity holds their u).  A second slot (u / 8, v mod 8) in the same bitmaps brings that down to 1 %, but its two LDS
// atomics per key cost more than the longer comparison of the listed words: 0.20 against 0.167 ms.
__device__ __forceinline__ u32 sus_slot(u32 w) { return __builtin_amdgcn_alignbit(w, w, 16) & ((1u << SUS_BLOOM) - 1u); }
static_assert(SUS_BLOOM == 17 && SUS_RUN_BITS == 16, "sus_slot is written for these");
__global__ __launch_bounds__(64 * SUS_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_find_suspects(const u64 *__restrict__ keys, i64 T, PackedLayout L, const u64 *__restrict__ hI,
                                                                   const u64 *__restrict__ hO, u64 *__restrict__ suspect64, u32 *__restrict__ giveup) {
    constexpr int NT = 64 * SUS_WAVES;
    __shared__ u32 s_seen[1 << (SUS_BLOOM - 5)], s_dup[1 << (SUS_BLOOM - 5)];
    __shared__ __attribute__((aligned(16))) u32 s_cw[SUS_CAND];
    __shared__ u32 s_cpos[SUS_CAND];
    __shared__ u32 s_start, s_end[2], s_nc;                             // s_end by step parity: a wavefront is at most one barrier ahead
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 lt_mask = (1ULL << lane) - 1ULL;
    const i64 t0 = (i64)blockIdx.x * SUS_TILE;
    const u64 *kt = keys + t0;
    const u32 n_rel = T - t0 < (i64)0x0fffffff ? (u32)(T - t0) : 0x0fffffffu;          // positions from t0 on, as far as this workgroup could ever reach
    const u32 t1_rel = n_rel < (u32)SUS_TILE ? n_rel : (u32)SUS_TILE;
    const u32 rmask = (1u << SUS_RUN_BITS) - 1u;
    const int F = L.F();
    typedef unsigned long long ull;
    // clamped, unconditional; a 32-bit byte offset from the workgroup's (scalar) base: one address register per load instead of two
    auto at = [&](u32 rel) -> u64 { return *reinterpret_cast<const u64 *>(reinterpret_cast<const char *>(kt) + (size_t)((rel < n_rel ? rel : n_rel - 1) << 3)); };
    auto hash0 = [&](u64 k) -> bool { return (k >> F) == 0ULL; };                      // the identity segment
    // the tile — a wavefront holds 512 consecutive keys — and the first 1,024 keys behind it (a run of 763 keys on average ends there):
    // all loads in flight together
    constexpr int NK = SUS_ROWS + SUS_XROWS;
    u64 key[NK];
    const u32 wrel = (u32)wave * (64 * SUS_ROWS), xrel = (u32)SUS_TILE + (u32)wave * (64 * SUS_XROWS);
    auto rel_of = [&](int r) -> u32 { return (r < SUS_ROWS ? wrel + r * 64 : xrel + (r - SUS_ROWS) * 64) + lane; };
#pragma unroll
    for (int r = 0; r < NK; ++r) key[r] = at(rel_of(r));
    // only the upper half of a key (run bits + sixteen hash bits) and one bit "hash field zero" are kept from here on: ten registers less
    u32 w[NK], zmask = 0;
    const u64 kprev = wrel > 0 ? at(wrel - 1) : (t0 > 0 ? keys[t0 - 1] : 0ULL);      // (clamped: a wavefront's segment may lie behind the end)
    const u64 kpe = at(xrel - 1);
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < (1 << (SUS_BLOOM - 5)) / (4 * NT); ++k) {
            reinterpret_cast<u32x4 *>(s_seen)[k * NT + threadIdx.x] = z;
            reinterpret_cast<u32x4 *>(s_dup)[k * NT + threadIdx.x] = z;
        }
    }
    if (threadIdx.x == 0) { s_start = ~0u; s_end[0] = ~0u; s_end[1] = ~0u; s_nc = 0u; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NK; ++r) { w[r] = (u32)(key[r] >> 32); zmask |= (hash0(key[r]) ? 1u : 0u) << r; }
    // first position of the tile where a run starts, and first one behind the tile
    {
        u32 carry = (u32)(kprev >> 32) & rmask;
        u32 first_b = ~0u, first_e = ~0u;
#pragma unroll
        for (int r = 0; r < NK; ++r) {
            if (r == SUS_ROWS) carry = (u32)(kpe >> 32) & rmask;
            const u32 v = w[r] & rmask;
            const u32 pv = wave_shr1(v, carry);
            carry = (u32)__builtin_amdgcn_readlane((int)v, 63);
            const u32 rel = rel_of(r);
            if (r < SUS_ROWS) {
                const u64 bm = __ballot(rel < t1_rel && (v != pv || (t0 == 0 && rel == 0)));
                if (bm && first_b == ~0u) first_b = rel - lane + (u32)__builtin_ctzll(bm);
            } else {
                const u64 bm = __ballot(rel < n_rel && v != pv);
                if (bm && first_e == ~0u) first_e = rel - lane + (u32)__builtin_ctzll(bm);
            }
        }
        if (lane == 0 && first_b != ~0u) atomicMin(&s_start, first_b);
        if (lane == 0 && first_e != ~0u) atomicMin(&s_end[0], first_e);
    }
    __syncthreads();
    const u32 s_rel = s_start;
    if (s_rel == ~0u) return;                                           // the whole tile continues a run that started earlier (block-uniform)
    // the end of the last run that starts in the tile: in the first 1,024 keys behind it, or (rare) further on, in steps of 1,024 keys
    u32 e_rel = t1_rel;
    bool closed = n_rel <= (u32)SUS_TILE;
    if (!closed) {
        const u32 end_now = s_end[0];
        const u32 step_end = (u32)SUS_TILE + 1024u;
        if (end_now != ~0u) { e_rel = end_now; closed = true; }
        else if (step_end >= n_rel) { e_rel = n_rel; closed = true; }
        else e_rel = step_end;
    }
    auto flag_chunk = [&](u64 m, i64 chunk) {
        if (lane == 0 && m) atomicOr(reinterpret_cast<ull *>(suspect64 + chunk), (ull)m);
    };
    // `seen` bits of a lane's keys back to back (a lane that owns nothing ORs a zero), then the `dup` bits
    {
        u32 ins = 0;                                                    // bit r = key r of this lane goes into the bitmaps
#pragma unroll
        for (int r = 0; r < NK; ++r) {
            const u32 rel = rel_of(r);
            const bool own = rel >= s_rel && rel < e_rel;
            const bool zh = own && ((zmask >> r) & 1u);
            flag_chunk(__ballot(zh), (t0 + rel - lane) / 64);
            ins |= ((own && !zh) ? 1u : 0u) << r;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                   // five keys at a time: ten atomics with return in flight
            constexpr int HB = NK / 2;
            u32 old[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int r = h * HB + q;
                const u32 slot = sus_slot(w[r]), in = (ins >> r) & 1u;
                old[q] = atomicOr(&s_seen[slot >> 5], in << (slot & 31));
            }
#pragma unroll
            for (int q = 0; q < HB; ++q) {
                const int r = h * HB + q;
                const u32 slot = sus_slot(w[r]), in = (ins >> r) & 1u;
                atomicOr(&s_dup[slot >> 5], old[q] & (in << (slot & 31)));
            }
        }
    }
    for (int step = 1; !closed; ++step) {
        if (step == SUS_MAX_EXT) {                                      // block-uniform
            if (threadIdx.x == 0) atomicOr(giveup, 1u);
            return;
        }
        const u32 q0 = xrel + (u32)step * 1024u;
        u64 kq[SUS_XROWS];
#pragma unroll
        for (int r = 0; r < SUS_XROWS; ++r) kq[r] = at(q0 + r * 64 + lane);
        const u64 kp = at(q0 - 1);
        u32 carry = (u32)(kp >> 32) & rmask, first_e = ~0u;
#pragma unroll
        for (int r = 0; r < SUS_XROWS; ++r) {
            const u32 rel = q0 + r * 64 + lane;
            const u32 v = (u32)(kq[r] >> 32) & rmask;
            const u32 pv = wave_shr1(v, carry);
            carry = (u32)__builtin_amdgcn_readlane((int)v, 63);
            const u64 bm = __ballot(rel < n_rel && v != pv);
            if (bm && first_e == ~0u) first_e = q0 + r * 64 + (u32)__builtin_ctzll(bm);
        }
        if (lane == 0 && first_e != ~0u) atomicMin(&s_end[step & 1], first_e);
        __syncthreads();
        const u32 end_now = s_end[step & 1];
        const u32 step_end = (u32)SUS_TILE + (u32)(step + 1) * 1024u;
        if (end_now != ~0u) { e_rel = end_now; closed = true; }
        else if (step_end >= n_rel) { e_rel = n_rel; closed = true; }
        else e_rel = step_end;
#pragma unroll
        for (int r = 0; r < SUS_XROWS; ++r) {
            const u32 rel = q0 + r * 64 + lane;
            const bool own = rel < e_rel;
            const bool zh = own && hash0(kq[r]);
            flag_chunk(__ballot(zh), (t0 + q0) / 64 + r);
            const u32 wq = (u32)(kq[r] >> 32), slot = sus_slot(wq);
            const u32 bit = (own && !zh) ? 1u << (slot & 31) : 0u;
            const u32 old = atomicOr(&s_seen[slot >> 5], bit);
            atomicOr(&s_dup[slot >> 5], old & bit);
        }
    }
    __syncthreads();
    // the owned keys whose bit was set twice: one counter update per wavefront
    auto listed = [&](u32 rel, u32 wk, bool zh) -> bool {
        const u32 slot = sus_slot(wk);
        return rel >= s_rel && rel < e_rel && ((s_dup[slot >> 5] >> (slot & 31)) & 1u) && !zh;
    };
    {
        u64 m[NK];
        u32 total = 0;
#pragma unroll
        for (int r = 0; r < NK; ++r) {
            m[r] = __ballot(listed(rel_of(r), w[r], (zmask >> r) & 1u));
            total += (u32)__popcll(m[r]);
        }
        if (total) {                                                    // wave-uniform
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&s_nc, total);
            base = (u32)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
            for (int r = 0; r < NK; ++r) {
                const u32 n = base + (u32)__popcll(m[r] & lt_mask);
                if (((m[r] >> lane) & 1ULL) && n < (u32)SUS_CAND) { s_cpos[n] = rel_of(r); s_cw[n] = w[r]; }
                base += (u32)__popcll(m[r]);
            }
        }
    }
    for (u32 rel = (u32)SUS_TILE + 1024u + threadIdx.x; rel < e_rel; rel += NT) {      // (the steps that were not kept in registers)
        const u64 k = kt[rel];
        if (listed(rel, (u32)(k >> 32), hash0(k))) {
            const u32 n = atomicAdd(&s_nc, 1u);
            if (n < (u32)SUS_CAND) { s_cpos[n] = rel; s_cw[n] = (u32)(k >> 32); }
        }
    }
    __syncthreads();
    const u32 nc = s_nc;
    if (nc > (u32)SUS_CAND) {                                           // (repeated rows all over: the caller gives the partial sort up anyway)
        // whole flag words (a bit at a time this path took 1.5 ms on the hash-partitioned products, where every key has its twin)
        const i64 g0 = t0 + s_rel, g1 = t0 + e_rel - 1;                // first and last owned position
        for (i64 wd = (g0 >> 6) + threadIdx.x; wd <= (g1 >> 6); wd += NT) {
            u64 m = ~0ULL;
            if (wd == (g0 >> 6)) m &= ~0ULL << (g0 & 63);
            if (wd == (g1 >> 6)) m &= ~0ULL >> (63 - (g1 & 63));
            atomicOr(reinterpret_cast<ull *>(suspect64 + wd), (ull)m);
        }
        return;
    }
    // listed keys all against all by their words (a broadcast 16-byte read serves four) — no memory access in the loop: a lane that
    // followed an equal word up with loads made the whole wavefront wait for every such lane in turn (a run of 763 keys holds four pairs
    // with equal 32-bit words), and that was two thirds of the kernel.  One partner: the rest of the hash field, then the 64-bit keys
    // rebuilt from the operand hash tables decide, all lanes at once (a run holds 0.02 triples of equal words on average: 3,000 keys of
    // 5e7, and flagged without looking they cost the fix-up pass of the flagged keys 0.15 ms); more than two: flagged without looking.
    // (two lanes per listed key, each on half of the list: the tail of a workgroup is a handful of lanes at work)
    const u32 nc4 = (nc + 3u) & ~3u, half = ((nc4 / 4 + 1) / 2) * 4;
    for (u32 a0 = 0; a0 < nc; a0 += NT / 2) {
        const u32 a = a0 + threadIdx.x / 2, part = threadIdx.x & 1u;
        const bool live = a < nc;
        const u32 wa = live ? s_cw[a] : 0u;
        u32 n_eq = 0, first = 0, last = 0;
        const u32 b0 = part ? half : 0u, b1 = part ? nc : (half < nc ? half : nc);
#pragma unroll 4
        for (u32 b = b0; b < b1; b += 4) {
            const u32x4 wl = *reinterpret_cast<const u32x4 *>(&s_cw[b]);
#pragma unroll
            for (u32 j = 0; j < 4; ++j)
                if (live && wl[j] == wa && b + j != a && b + j < b1) {
                    if (n_eq == 0) first = b + j;
                    last = b + j;
                    ++n_eq;
                }
        }
        {   // both halves together: with up to two partners (first, last) are all of them
            const u32 n_o = (u32)__shfl_xor((int)n_eq, 1), f_o = (u32)__shfl_xor((int)first, 1), l_o = (u32)__shfl_xor((int)last, 1);
            const u32 n_lo = part ? n_o : n_eq, f_lo = part ? f_o : first, l_lo = part ? l_o : last;
            const u32 n_hi = part ? n_eq : n_o, f_hi = part ? first : f_o, l_hi = part ? last : l_o;
            first = n_lo ? f_lo : f_hi;
            last = n_hi ? l_hi : l_lo;
            n_eq = n_lo + n_hi;
        }
        bool hit = n_eq > 2;                                            // (four equal 32-bit words in one run: flagged without looking)
        if (n_eq >= 1 && n_eq <= 2 && part == 0) {
            const u64 ka = kt[s_cpos[a]], kb = kt[s_cpos[first]], kc = kt[s_cpos[last]];      // (from the L2: the lists hold words only)
            const u64 fa = L.full_key(hI, hO, ka);
            hit = (((ka ^ kb) >> F) == 0ULL && fa == L.full_key(hI, hO, kb)) || (((ka ^ kc) >> F) == 0ULL && fa == L.full_key(hI, hO, kc));
        }
        if (hit && part == 0) {
            const i64 p = t0 + s_cpos[a];
            atomicOr(reinterpret_cast<ull *>(suspect64 + (p >> 6)), 1ULL << (p & 63));
        }
    }
}
__global__ void k_popc_words64(const u64 *__restrict__ bits, i64 n_words, u32 *__restrict__ counts) {
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (i64)gridDim.x * blockDim.x) counts[w] = (u32)__popcll(bits[w]);
}
// flagged keys, in array order, to the front of `out`
__global__ __launch_bounds__(256) void k_compact_suspects(const u64 *__restrict__ keys, const u64 *__restrict__ suspect64, const u32 *__restrict__ prefix,
                                                           i64 n_chunks, u64 *__restrict__ out) {
    // sixteen flag words per wavefront (lanes 0..15 load them), then the few words that have a flag set one after the other with the whole
    // wavefront (a product without repeated rows flags a few thousand of 5e7 keys: a wavefront per word spent 41 us reading zeros; 64 words
    // per wavefront left the 10^4 consecutive flagged keys of a squared operator's identity segment to three wavefronts: 31 us)
    const int lane = threadIdx.x & 63;
    for (i64 base = ((i64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16; base < n_chunks; base += (i64)gridDim.x * 64) {
        const i64 mine = base + (lane & 15);
        const u64 b = mine < n_chunks ? suspect64[mine] : 0ULL;
        u64 nz = __ballot(b != 0ULL) & 0xFFFFULL;
        while (nz) {                                                             // wave-uniform
            const int l = __builtin_ctzll(nz);
            nz &= nz - 1;
            const u64 bb = __shfl(b, l);
            const i64 c = base + l;
            if ((bb >> lane) & 1ULL) out[(i64)prefix[c] + __popcll(bb & ((1ULL << lane) - 1ULL))] = keys ? keys[c * 64 + lane] : (u64)(c * 64 + lane);   // (no keys: the index)
        }
    }
}

// ---- hash and key -----------------------------------------------------------------------------------------------------------------
static int pair_keys(const CleanupRun &r, bool bytes) {
    const PairOperands &p = r.rq.p;
    PairKeyArgs ka;
    ka.hI = r.hI.as<u64>(); ka.hO = r.hO_p; ka.keys = r.keys.as<u64>(); ka.bi = r.pl.L.bi; ka.bo = r.pl.L.bo; ka.o_base = 0; ka.squared = r.pl.squared ? 1 : 0;
    if (bytes) ka.ebytes = r.keys.as<unsigned char>();
    return mul_keys_dev(p.inner, p.Ni, p.outer, p.No, r.rq.W / 2, p.inner_is_left, ka);
}

// the single terms of packed pair keys, decided while the keys are still in index order
static int mark_singles_packed(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; const PairOperands &p = r.rq.p;
    const i64 Ni = p.Ni, No = p.No, Tk = pl.Tk; const double *ci = p.ci, *co = p.co; hipStream_t st = r.st;
    const i64 n_tiles = (Tk + SORT_TILE - 1) / SORT_TILE;
    // how small the operands' coefficients get: decides whether the marking has to look at them at all
    SG_TRY(r.cfloor.alloc(16));
    const bool one_block = Ni <= 65536 && No <= 65536;       // a single workgroup stores its minimum: nothing to initialise
    if (!one_block) HIP_TRY(hipMemsetAsync(r.cfloor.p, 0xFF, 16, st));
    const bool two_ops = co != ci || No != Ni;
    if (one_block)                                         // (blockIdx.y selects the operand: one launch for both)
        hipLaunchKernelGGL(k_coeff_floor, dim3(1, two_ops ? 2 : 1), dim3(1024), 0, st, ci, Ni, co, No, r.cfloor.as<unsigned long long>(), 1);
    else {
        hipLaunchKernelGGL(k_coeff_floor, dim3(grid_for(Ni, 256, 256)), dim3(256), 0, st, ci, Ni, ci, Ni, r.cfloor.as<unsigned long long>(), 0);
        if (two_ops)
            hipLaunchKernelGGL(k_coeff_floor, dim3(grid_for(No, 256, 256)), dim3(256), 0, st, co, No, co, No, r.cfloor.as<unsigned long long>() + 1, 0);
    }
    const double *fl_i = r.cfloor.as<double>(), *fl_o = two_ops ? r.cfloor.as<double>() + 1 : r.cfloor.as<double>();
    if (r.sw.nofloor) fl_i = fl_o = nullptr;     // tests: every coefficient looked at
    if (pl.key_bytes) {
        bump_counter(SYMGPU_CTR_FLOW_MARKED_FROM_BYTES);   // the single terms marked from bytes
        const i64 n_groups = (Tk + 63) / 64 * 4;           // whole 64-bit words of the bitmaps
        hipLaunchKernelGGL(k_mark_bytes, dim3((unsigned)grid_for(n_groups, 256, 1 << 16)), dim3(256), 0, st, r.keys.as<u32x4>(), Tk, n_groups, Ni, ci, co,
                           pl.squared ? 1 : 0, r.rq.thr, r.rq.use_thr, r.markbits.as<unsigned short>(), r.e_lo.as<unsigned short>(), r.e_hi.as<unsigned short>(), fl_i, fl_o);
    } else {
        SG_TRY(r.sort_hist.alloc((size_t)n_tiles * 256 * sizeof(u32)));
        r.a.first_hist = r.sort_hist.as<u32>();
        hipLaunchKernelGGL(k_mark_singles<true>, dim3((unsigned)n_tiles), dim3(256), 0, st, r.keys.as<u64>(), (const double *)nullptr, Tk, pl.L, ci, co,
                           pl.squared ? 1 : 0, r.rq.thr, r.rq.use_thr, r.markbits.as<u64>(), r.e_lo.as<u64>(), r.e_hi.as<u64>(), r.a.first_hist, 64 - pl.nbits, n_tiles, fl_i, fl_o);
    }
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// row hashes; pair keys (packed, or only their bytes) or 64-bit keys + indices; the single terms of the lazy flow
int cleanup_hash_keys(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; const CleanupRequest &rq = r.rq; const PairOperands &p = rq.p; hipStream_t st = r.st;
    if (!rq.pair) {
        SG_TRY(hash_rows_any(rq.rows, rq.T, rq.W, r.seed, r.keys.as<u64>(), r.idx.as<u32>()));      // (and idx[t] = t, the array the sort carries)
    } else {
        SG_TRY(hash_rows(p.inner, p.Ni, rq.W, r.hI.as<u64>()));
        if (!r.same_rows) SG_TRY(hash_rows(p.outer, p.No, rq.W, r.hO.as<u64>()));     // (one operand used twice: hO_p is hI)
        if (pl.packed) {
            SG_TRY(pair_keys(r, pl.key_bytes));
            if (pl.lazy) SG_TRY(mark_singles_packed(r));
        } else {
            if (!r.idx.p) {
                SG_TRY(r.idx.alloc((size_t)rq.T * 4));
                SG_TRY(r.idx2.alloc((size_t)rq.T * 4));
            }
            if (!r.pair_coeff.p) {
                SG_TRY(r.pair_coeff.alloc((size_t)rq.T * 16));
                SG_TRY(mul_coeff_dev(p.inner, p.ci, p.Ni, p.outer, p.co, 0, p.No, rq.W / 2, p.inner_is_left, r.pair_coeff.as<double>()));
                r.coeff = r.pair_coeff.as<double>();
            }
            hipLaunchKernelGGL(k_pair_keys, dim3(grid_for(rq.T)), dim3(256), 0, st, r.hI.as<u64>(), p.Ni, r.hO_p, rq.T, r.keys.as<u64>(), r.idx.as<u32>());
            KERNEL_CHECK();
        }
    }
    if (!pl.packed && pl.lazy) {
        hipLaunchKernelGGL(k_mark_singles<false>, dim3((unsigned)((rq.T + SORT_TILE - 1) / SORT_TILE)), dim3(256), 0, st, (const u64 *)nullptr, r.coeff, rq.T, pl.L, (const double *)nullptr,
                           (const double *)nullptr, 0, rq.thr, rq.use_thr, r.markbits.as<u64>(), (u64 *)nullptr, (u64 *)nullptr, (u32 *)nullptr, 0, (i64)0, (const double *)nullptr,
                           (const double *)nullptr);
        KERNEL_CHECK();
    }
    return SYMGPU_OK;
}

// ---- order ------------------------------------------------------------------------------------------------------------------------
// packed keys, sus_try: the keys that have a partner found (partial sort + k_find_suspects, or the direct flag pass from the operand hash
// tables), compacted and sorted alone — or, if most keys are flagged, the sort of all keys finished after all
static int order_flagged(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; const PairOperands &p = r.rq.p; CleanupRun::Attempt &a = r.a; hipStream_t st = r.st;
    const i64 Tk = pl.Tk;
    // two passes before the flag pass, on key bits [32, 48): a run then holds <= 2,048 keys on average (products of up to 2^27 keys)
    const int sus_pass = SUS_RUN_BITS / 8;
    const int lo = 64 - pl.nbits, hi = lo + 8 * sus_pass;
    const i64 n_sc = (Tk + 63) / 64;
    Scratch susbits, susprefix;
    SG_TRY(susbits.alloc((size_t)n_sc * 8 + 16));
    SG_TRY(susprefix.alloc((size_t)n_sc * 4));
    u32 *sustotal = susbits.as<u32>() + 2 * n_sc;          // [0] flagged keys, [1] the flag pass gave up (one memset with the flags)
    SG_TRY(zero_two(susbits.p, (size_t)n_sc * 8 + 16, nullptr, 0));
    // round 6: operands whose bucketed hash words fit a workgroup's LDS — the flags come from the operand hash tables, the
    // keys are never sorted (pair_dups.hip); they stay in index order and the flags are indexed likewise.
    // (Measured and dropped: the marking pass folded into the key kernel — three bitmaps ORed from its epilogue, an atomic per
    // 64 indices, or per 256 with the inner words stored: the conditional memory operations of the epilogue drain the kernel's
    // memory counter one by one, 0.28 -> 0.48 / 0.58 ms for the 0.14 ms pass it would replace; and the marking pass without the
    // first-pass histograms, which only the fall-back needs: 0.139 -> 0.141 ms, it is bound by reading the keys.)
    bool direct = false;
    SG_TRY(pair_dups_dev(r.hI.as<u64>(), p.Ni, r.hO_p, p.No, pl.squared, Tk, susbits.as<u64>(), sustotal + 1, &direct));
    u64 *part = r.keys.as<u64>(), *spare = r.keys2.as<u64>();
    bump_counter(direct ? SYMGPU_CTR_FLOW_FLAGS_HASH_TABLES : SYMGPU_CTR_FLOW_FLAGS_PARTIAL_SORT);   // which flag pass this attempt launches
    if (!direct) {
        if (pl.key_bytes) SG_TRY(pair_keys(r, false));     // (the flag pass was refused: keys after all)
        SortResult res;
        SG_TRY(radix_sort({part, spare, nullptr, nullptr, Tk, lo, hi, a.first_hist, SortForm::Launches}, &res));
        part = res.keys; spare = res.spare_keys;
        hipLaunchKernelGGL(k_find_suspects, dim3((unsigned)((Tk + SUS_TILE - 1) / SUS_TILE)), dim3(64 * SUS_WAVES), 0, st, part, Tk, pl.L, r.hI.as<u64>(),
                           r.hO_p, susbits.as<u64>(), sustotal + 1);
    }
    if (n_sc <= POPC_SCAN_SMALL_MAX) SG_TRY(popc_scan_small(susbits.as<u64>(), n_sc, -1, susprefix.as<u32>(), sustotal));
    else {
        hipLaunchKernelGGL(k_popc_words64, dim3(grid_for(n_sc)), dim3(256), 0, st, susbits.as<u64>(), n_sc, susprefix.as<u32>());
        KERNEL_CHECK();
        SG_TRY(exclusive_scan_u32(susprefix.as<u32>(), susprefix.as<u32>(), n_sc, sustotal));
    }
    // the compaction does not need the count: it is queued behind the count's way home and runs while the host waits for it (in
    // the rare give-up case its output is simply overwritten)
    u32 h_sus2[2] = {0, 0};
    {
        ReadBack rb;
        SG_TRY(read_back_post(sustotal, 2, nullptr, 0, &rb));
        const bool from_bytes = pl.key_bytes && direct;       // only bytes in the key buffer: the indices are compacted, the keys rebuilt from them
        hipLaunchKernelGGL(k_compact_suspects, dim3((unsigned)grid_for((n_sc + 63) / 64, 1, 1 << 16)), dim3(256), 0, st, from_bytes ? (const u64 *)nullptr : part,
                           susbits.as<u64>(), susprefix.as<u32>(), n_sc, spare);
        if (from_bytes)
            hipLaunchKernelGGL(k_keys_of_indices, dim3(64), dim3(256), 0, st, spare, sustotal, r.keys.as<unsigned char>(), p.Ni, pl.squared ? 1 : 0, pl.L, r.hI.as<u64>(), r.hO_p);
        KERNEL_CHECK();
        SG_TRY(read_back_wait(&rb, h_sus2));
    }
    const u32 h_sus = h_sus2[0];
    if (h_sus2[1]) {                                       // the flag pass gave up; the hash-table pass says why (the bits of k_pd_bucket / k_pair_dups)
        bump_counter(SYMGPU_CTR_FLOW_FLAGS_GAVE_UP);
        for (u32 bit : PD_GIVEUP_BITS) if (direct && (h_sus2[1] & bit)) bump_counter(counter_of_giveup(bit));
    }
    if ((i64)h_sus * 16 > Tk || r.sw.suspects == 2 || h_sus2[1]) {
        bump_counter(SYMGPU_CTR_FLOW_SORTED_WHOLE);        // the sort finished on the whole array
        // repeated rows all over: the last pass on the whole array after all (LSD: the order so far is its first passes; the
        // direct flag pass left the keys in index order: all passes)
        if (pl.key_bytes && direct) SG_TRY(pair_keys(r, false));   // (only bytes so far: the keys after all)
        SortResult res;
        SG_TRY(radix_sort({part, spare, nullptr, nullptr, Tk, direct ? lo : hi, 64, direct ? a.first_hist : nullptr, SortForm::Launches}, &res));
        a.ks = res.keys;
        return SYMGPU_OK;
    }
    bump_counter(SYMGPU_CTR_FLOW_SORTED_FLAGGED);          // the flagged keys sorted alone (none flagged: nothing to sort)
    a.sus_active = true;
    a.Tsort = h_sus;
    a.ks = part;
    if (a.Tsort == 0) return SYMGPU_OK;
    // the flagged keys, sorted completely (the same rule for the number of sorted bits, now for a few thousand keys);
    // `part` is not needed any more and serves as the sort's second buffer
    a.fix_bits = sorted_bits(a.Tsort, 64 - pl.L.F());                   // (a packed key carries 64 - F hash bits)
    // the compaction kept the array order, i.e. the flagged keys are ordered by key bits [lo, hi) already: when the bits to
    // order start inside that range only the passes above it are left (LSD: stable passes on more significant bits)
    const int sort_from = (!direct && 64 - a.fix_bits >= lo && 64 - a.fix_bits < hi) ? hi : 64 - a.fix_bits;
    SortResult res;
    SG_TRY(radix_sort({spare, part, nullptr, nullptr, a.Tsort, sort_from, 64, nullptr, SortForm::OneLaunchIfFits}, &res));
    a.sus_coop = res.one_launch;
    a.ks = res.keys;
    return SYMGPU_OK;
}

// the keys (and, unpacked, their indices) in sorted order: r.a.ks / r.a.is
int cleanup_order(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; CleanupRun::Attempt &a = r.a; const i64 Tk = pl.Tk;
    if (pl.sus_try) return order_flagged(r);
    // (plain cleanups of up to 1.3e5 rows: the index sort in ONE launch — its three passes were nine launches, launch bound;
    // small products — up to 2e5 keys, no first-pass histograms at hand —: the sort in ONE launch; its passes were three launches each)
    if (pl.packed) bump_counter(SYMGPU_CTR_FLOW_COMPLETE_SORT);   // the complete sort of the packed keys, no flag pass
    SortResult res;
    SG_TRY(radix_sort({r.keys.as<u64>(), r.keys2.as<u64>(), pl.packed ? nullptr : r.idx.as<u32>(), pl.packed ? nullptr : r.idx2.as<u32>(), Tk, 64 - pl.nbits, 64,
                       a.first_hist, SortForm::OneLaunchWherePays}, &res));
    a.sus_coop = res.one_launch;
    a.ks = res.keys;
    a.is = res.vals;
    return SYMGPU_OK;
}

}  // namespace symgpu
