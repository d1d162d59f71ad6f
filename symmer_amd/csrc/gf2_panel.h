// gf2_panel.h — the panel of the blocked GF(2) elimination: the reference loop on the rows of one block (device code; gf2.hip includes it)
#pragma once
#include "gf2_common.h"

namespace symgpu {

__device__ __forceinline__ u64 readlane64(u64 v, int l) {
    const u32 lo = __builtin_amdgcn_readlane((u32)v, l), hi = __builtin_amdgcn_readlane((u32)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// Where the 4-word window starts: at the smallest leading word of the block's rows, but never so far left that the first non-zero
// row (lane jf) falls out of it.  (Round 2 started it AT the first row's leading word: when the pivots cross a word boundary some
// rows still lead in the word before — a dense matrix then lost a one-row block every 64 columns.)
__device__ __forceinline__ int window_start(int a, bool valid, int jf) {
    const int a_first = __builtin_amdgcn_readlane(a, jf);
    int lo = (valid && a != NOLEAD) ? a : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(lo, off); lo = o < lo ? o : lo; }
    const int floor_w = a_first - (WN - 1);
    return lo > floor_w ? lo : floor_w;
}

// the reference loop on a window of WNT words per block row (registers of ONE wavefront, lane = block row).
// Rows still to process, in order (genuinely zero rows have no pivot and are never modified: skipped).  ONE exit test per pivot:
// the row's leading word lies outside the window, or the row cancelled to zero inside it -> it opens the next block (re-windowed).
template <int WNT>
__device__ __forceinline__ void panel_loop(const u64 *__restrict__ rows, i64 Wc, i64 i0, int lane, bool valid, int w_lo, u64 in_m, u64 todo,
                                           int &kk, int &pw, int &pb, u64 &my_mask, u64 &tv, const u64 *spec, int w_spec, int &w_max) {
    // spec: the window words loaded speculatively at w_spec (the previous block's guess), beside the leads instead of behind them
    u64 C[WNT];
    if (w_spec == w_lo) {
#pragma unroll
        for (int k = 0; k < WNT; ++k) C[k] = spec[k];
    } else {
#pragma unroll
        for (int k = 0; k < WNT; ++k) C[k] = (valid && (i64)w_lo + k < Wc) ? rows[(i0 + lane) * Wc + w_lo + k] : 0ULL;
    }
    while (todo) {
        const int j = __builtin_ctzll(todo);
        u64 p[WNT];
#pragma unroll
        for (int k = 0; k < WNT; ++k) p[k] = readlane64(C[k], j);
        if (!((in_m >> j) & 1ULL)) { kk = j; break; }
        int k0 = 0, b;
        u64 mk;
        if (p[0] != 0) {                                            // common case: the pivot sits in the first window word
            b = __builtin_ctzll(p[0]);
            mk = __ballot((C[0] >> b) & 1ULL);
        } else {
            k0 = -1;
#pragma unroll
            for (int k = WNT - 1; k >= 1; --k) if (p[k] != 0) k0 = k;
            if (k0 < 0) { kk = j; break; }
            u64 pk = p[1], ck = C[1];
#pragma unroll
            for (int k = 2; k < WNT; ++k) if (k == k0) { pk = p[k]; ck = C[k]; }
            b = __builtin_ctzll(pk);
            mk = __ballot((ck >> b) & 1ULL);
        }
        mk &= ~(1ULL << j);
        todo &= todo - 1;
        if (lane == j) { pw = w_lo + k0; pb = b; my_mask = mk; }
        w_max = w_lo + k0 > w_max ? w_lo + k0 : w_max;
        const u64 tj = readlane64(tv, j);
        if ((mk >> lane) & 1ULL) {
#pragma unroll
            for (int k = 0; k < WNT; ++k) C[k] ^= p[k];
            tv ^= tj;
        }
    }
}

// The same loop on a TWO-word window, written for its DEPENDENT CHAIN (round 4: the panel is the critical path of every block — 64 pivots,
// one after the other, 560 cycles each in the generic loop, nearly all of it pipeline latency between the vector and the scalar unit:
// readlane -> scalar find -> vector test -> ballot -> scalar mask -> EXEC -> vector update -> readlane ...).  Here the chain of a pivot is
// six v_readlane (issued together) -> branch-free scalar arithmetic (s_ff1 on the two window words, one-hot masks) -> ONE vector block:
// the holders of the pivot column as an all-ones / zero word per lane (four and/or, compare, select) and the update as six v_bitop3
// x ^= p & m — no EXEC-masked update, no ballot on the way to the next pivot.  Row j itself is kept out with EXEC (it holds the column it
// pivots on); the holder mask for the records is the compare's VCC, filed into lane j afterwards (off the chain).
__device__ __forceinline__ void panel_loop_narrow(const u64 *__restrict__ rows, i64 Wc, i64 i0, int lane, bool valid, int w_lo, u64 in_m, u64 todo,
                                                  int &kk, int &pw, int &pb, u64 &my_mask, u64 &tv, const u64 *spec, int w_spec, int &w_max) {
    u64 C[2];
    if (w_spec == w_lo) { C[0] = spec[0]; C[1] = spec[1]; }
    else {
#pragma unroll
        for (int k = 0; k < 2; ++k) C[k] = (valid && (i64)w_lo + k < Wc) ? rows[(i0 + lane) * Wc + w_lo + k] : 0ULL;
    }
    u32 c0 = (u32)C[0], c1 = (u32)(C[0] >> 32), c2 = (u32)C[1], c3 = (u32)(C[1] >> 32), t0 = (u32)tv, t1 = (u32)(tv >> 32);
    u32 pw_v = (u32)pw, pb_v = (u32)pb, mlo_v = (u32)my_mask, mhi_v = (u32)(my_mask >> 32);
    const int w_lo_s = __builtin_amdgcn_readfirstlane(w_lo);
    while (todo) {
        const int j = __builtin_ctzll(todo);
        const u32 p0 = __builtin_amdgcn_readlane(c0, j), p1 = __builtin_amdgcn_readlane(c1, j), p2 = __builtin_amdgcn_readlane(c2, j),
                  p3 = __builtin_amdgcn_readlane(c3, j), q0 = __builtin_amdgcn_readlane(t0, j), q1 = __builtin_amdgcn_readlane(t1, j);
        const u64 P0 = ((u64)p1 << 32) | p0, P1 = ((u64)p3 << 32) | p2;
        // (rare exits, one test: the row leads outside the window, or it cancelled to zero inside it)
        if (!((in_m >> j) & 1ULL) || (P0 | P1) == 0ULL) { kk = j; break; }
        const int hiw = P0 == 0ULL ? 1 : 0;                                     // the pivot sits in the second window word
        const int b = __builtin_ctzll(hiw ? P1 : P0);
        const u64 oh = 1ULL << b, M0 = hiw ? 0ULL : oh, M1 = hiw ? oh : 0ULL;   // one-hot over the window
        const u64 onej = 1ULL << j;
        u64 mk;
        u32 t;
        asm volatile("s_andn2_b64 exec, -1, %[onej]\n\t"
                     "v_and_b32 %[t], %[m0], %[c0]\n\t"
                     "v_and_or_b32 %[t], %[c1], %[m1], %[t]\n\t"
                     "v_and_or_b32 %[t], %[c2], %[m2], %[t]\n\t"
                     "v_and_or_b32 %[t], %[c3], %[m3], %[t]\n\t"
                     "v_cmp_ne_u32 vcc, 0, %[t]\n\t"
                     "v_cndmask_b32_e64 %[t], 0, -1, vcc\n\t"
                     "v_bitop3_b32 %[c0], %[c0], %[p0], %[t] bitop3:0x78\n\t"
                     "v_bitop3_b32 %[c1], %[c1], %[p1], %[t] bitop3:0x78\n\t"
                     "v_bitop3_b32 %[c2], %[c2], %[p2], %[t] bitop3:0x78\n\t"
                     "v_bitop3_b32 %[c3], %[c3], %[p3], %[t] bitop3:0x78\n\t"
                     "v_bitop3_b32 %[t0], %[t0], %[q0], %[t] bitop3:0x78\n\t"
                     "v_bitop3_b32 %[t1], %[t1], %[q1], %[t] bitop3:0x78\n\t"
                     "s_mov_b64 %[mk], vcc\n\t"
                     "s_mov_b64 exec, -1"
                     : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [t0] "+v"(t0), [t1] "+v"(t1), [t] "=&v"(t), [mk] "=&s"(mk)
                     : [onej] "s"(onej), [m0] "s"((u32)M0), [m1] "s"((u32)(M0 >> 32)), [m2] "s"((u32)M1), [m3] "s"((u32)(M1 >> 32)),
                       [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [p3] "s"(p3), [q0] "s"(q0), [q1] "s"(q1)
                     : "vcc");
        todo &= todo - 1;
        const int wabs = w_lo_s + hiw;
        w_max = wabs > w_max ? wabs : w_max;
        // the pivot's records into lane j (EXEC = {j}); nothing of the next pivot depends on them
        asm volatile("s_mov_b64 exec, %[onej]\n\t"
                     "v_mov_b32 %[pw], %[vw]\n\t"
                     "v_mov_b32 %[pb], %[vb]\n\t"
                     "v_mov_b32 %[ml], %[vl]\n\t"
                     "v_mov_b32 %[mh], %[vh]\n\t"
                     "s_mov_b64 exec, -1"
                     : [pw] "+v"(pw_v), [pb] "+v"(pb_v), [ml] "+v"(mlo_v), [mh] "+v"(mhi_v)
                     : [onej] "s"(onej), [vw] "s"(wabs), [vb] "s"(b), [vl] "s"((u32)mk), [vh] "s"((u32)(mk >> 32)));
    }
    pw = (int)pw_v; pb = (int)pb_v; my_mask = ((u64)mhi_v << 32) | mlo_v; tv = ((u64)t1 << 32) | t0;
}

// publish the block (one wavefront, lane = block row): only rows < kk belong to it.  pw / pb: the lane's pivot, mask: mask_j for j = lane
// (bits >= kk already cleared), tv: the lane's row of T, w_next: BlockInfo::w_next.
__device__ __forceinline__ void publish_block(BlockInfo *__restrict__ info, SweepState *__restrict__ st, i64 *__restrict__ pivots,
                                              Gf2Counters *__restrict__ counters, i64 i0, int kk, int lane, int pw, int pb, u64 mask, u64 tv, int w_next) {
    const bool mine = lane < kk;
    info->pivw[lane] = mine ? pw : -1;
    info->pivb[lane] = mine ? pb : 0;
    info->mask[lane] = mine ? mask : 0ULL;
    info->T[lane] = mine ? tv : 0ULL;
    if (mine && pivots) pivots[i0 + lane] = pw < 0 ? -1 : (i64)pw * 64 + pb;
    unsigned long long c = mine ? (unsigned long long)__popcll(mask) : 0ULL;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) {
        info->i0 = i0;
        info->kk = kk;
        info->w_next = w_next;
        st->next_i0 = i0 + kk;
        if (c) atomicAdd(&counters->xors, c);
    }
}

// the panel proper: ONE wavefront (lane = block row), `a` = this lane's leading word (lead[] semantics), block starts at i0
__device__ __forceinline__ void panel_wave(const u64 *__restrict__ rows, i64 R, i64 Wc, i64 i0, int a, int lane, SweepState *__restrict__ st,
                                           BlockInfo *__restrict__ info, i64 *__restrict__ pivots, Gf2Counters *__restrict__ counters,
                                           const u64 *spec = nullptr, int w_spec = -1, int lean = 1) {
    if (i0 >= R) { if (lane == 0) { info->i0 = i0; info->kk = 0; info->w_next = -1; } return; }
    int w_max = -1;
    u64 no_spec[WN] = {0, 0, 0, 0};
    if (!spec) { spec = no_spec; w_spec = -1; }
    const bool valid = a >= 0;
    const int n_valid = __popcll(__ballot(valid));                 // rows i0 .. i0+n_valid-1 exist
    const u64 zero_m = __ballot(valid && a == NOLEAD);
    const u64 fin_m = __ballot(valid && a != NOLEAD);
    int kk = n_valid;
    int pw = -1, pb = 0;                                            // this lane's (= block row's) pivot
    u64 my_mask = 0;                                                // mask_j for j = lane
    u64 tv = 1ULL << lane;                                          // T row of this lane
    bool narrow_ran = false;
    if (fin_m != 0) {
        const int jf = __builtin_ctzll(fin_m);
        const int w_lo = window_start(a, valid, jf);
        // narrow window (round 3): when every row of the block leads inside the first TWO words — a dense matrix, whose 64 pivots
        // are 64 consecutive columns — the panel keeps two words per row instead of four: 4 v_readlane + 4 v_xor less per pivot.
        // A row that cancels to zero inside the two words ends the block (as it does with four), so the result is unchanged.
        const bool narrow = __ballot(valid && a != NOLEAD && !(a >= w_lo && a < w_lo + 2)) == 0ULL;
        const int wn = narrow ? 2 : WN;
        narrow_ran = narrow;
        const u64 in_m = __ballot(valid && a != NOLEAD && a >= w_lo && a < w_lo + wn);
        const u64 todo0 = (n_valid >= 64 ? ~0ULL : ((1ULL << n_valid) - 1ULL)) & ~zero_m;
        static_assert(WN >= 2, "narrow window");
        if (narrow && lean) panel_loop_narrow(rows, Wc, i0, lane, valid, w_lo, in_m, todo0, kk, pw, pb, my_mask, tv, spec, w_spec, w_max);
        else if (narrow) panel_loop<2>(rows, Wc, i0, lane, valid, w_lo, in_m, todo0, kk, pw, pb, my_mask, tv, spec, w_spec, w_max);
        else panel_loop<WN>(rows, Wc, i0, lane, valid, w_lo, in_m, todo0, kk, pw, pb, my_mask, tv, spec, w_spec, w_max);
    }
    // block statistics {blocks | two-word windows << 32}: one add per block, issued ahead of the publication so that nothing waits behind it
    if (lane == 0 && kk > 0) atomicAdd(&counters->blocks, 1ULL | ((unsigned long long)narrow_ran << 32));
    const u64 low = (kk >= 64) ? ~0ULL : ((1ULL << kk) - 1ULL);
    publish_block(info, st, pivots, counters, i0, kk, lane, pw, pb, my_mask & low, tv, w_max);   // w_max is wave-uniform (scalar running maximum)
}

// Does the panel of the block whose rows lead at `a` (one wavefront, lead[] semantics) run on the full rows in LDS?  When the four-word window
// would end the block early: a row leads outside it, and the first such row is below min(rows of the block, 32).
__device__ __forceinline__ bool full_row_panel_wanted(int a) {
    const bool valid = a >= 0;
    const u64 fin_m = __ballot(valid && a != NOLEAD);
    if (fin_m == 0) return false;
    const int w_lo = window_start(a, valid, __builtin_ctzll(fin_m));
    const u64 bad = __ballot(valid && a != NOLEAD && !(a >= w_lo && a < w_lo + WN));   // rows that lead outside the window
    const int n_valid = __popcll(__ballot(valid));
    return bad != 0 && __builtin_ctzll(bad) < (n_valid < 32 ? n_valid : 32);
}

// the window words of row `row` at the guess w_spec (< 0: none) of the block before: loaded beside the leads, not behind them
__device__ __forceinline__ void load_spec_window(const u64 *__restrict__ rows, i64 Wc, i64 row, int w_spec, u64 (&spec)[WN]) {
    if (w_spec < 0) return;
#pragma unroll
    for (int k = 0; k < WN; ++k) spec[k] = (i64)w_spec + k < Wc ? rows[row * Wc + w_spec + k] : 0ULL;
}

// ---- full-row panel (round 3): sparse rows lead at scattered words, and the 4-word window then ends a block after a row or two
// (700 x 700 at density 0.003: 450 blocks instead of 11, 8.7x the dense time).  When the window would end the block early and the
// rows are at most FULL_WC words long, the whole workgroup runs the reference loop on the 64 FULL rows in LDS (<= 128 KiB, the
// sweep's table area): wavefront 0 finds the pivot of row j and the block rows that hold its column and keeps T, everybody XORs
// row j into those rows.  Two barriers per pivot (~0.5 us) instead of ~0.25 us in registers, but the block never ends early.
constexpr int FULL_WC = 256;
__device__ __forceinline__ void panel_full(const u64 *__restrict__ rows, i64 R, i64 Wc, i64 i0, int a, u64 *__restrict__ m /* LDS [64][Wc] */,
                                           u64 *__restrict__ s_bc /* LDS [4] */, SweepState *__restrict__ st, BlockInfo *__restrict__ info,
                                           i64 *__restrict__ pivots, Gf2Counters *__restrict__ counters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nt = blockDim.x;
    const int W = (int)Wc;
    const int n_valid = (int)(R - i0 < WK ? R - i0 : WK);
    for (int x = threadIdx.x; x < n_valid * W; x += nt) m[x] = rows[i0 * Wc + x];
    __syncthreads();
    int pw = -1, pb = 0;                                            // wavefront 0, lane = block row
    u64 my_mask = 0, tv = 1ULL << lane;
    if (threadIdx.x == 0) atomicAdd(&counters->blocks, 1ULL);       // block statistics: a block (the full-row ones are counted where the choice is made)
    for (int j = 0; j < n_valid; ++j) {
        if (wave == 0) {
            int jw = -1, jb = 0;
            if (__builtin_amdgcn_readlane(a, j) != NOLEAD) {        // rows that were zero when phase 0 looked stay zero: nothing touches them
                for (int w0 = 0; w0 < W; w0 += 64) {
                    const int w = w0 + lane;
                    const u64 v = w < W ? m[j * W + w] : 0ULL;
                    const u64 nz = __ballot(v != 0);
                    if (nz) {
                        const int l = __builtin_ctzll(nz);
                        jw = w0 + l;
                        jb = __builtin_ctzll(readlane64(v, l));
                        break;
                    }
                }
            }
            u64 mk = 0;
            if (jw >= 0) mk = __ballot(lane < n_valid && lane != j && ((m[lane * W + jw] >> jb) & 1ULL));
            if (lane == j) { pw = jw; pb = jb; my_mask = mk; }
            const u64 tj = readlane64(tv, j);
            if ((mk >> lane) & 1ULL) tv ^= tj;
            if (lane == 0) s_bc[0] = mk;
        }
        __syncthreads();
        const u64 mk = s_bc[0];
        // a wavefront per flagged row (wave-uniform test: unflagged rows cost nothing), lanes over the words
        for (int r = wave; r < n_valid; r += nt / 64)
            if ((mk >> r) & 1ULL)
                for (int w = lane; w < W; w += 64) m[r * W + w] ^= m[j * W + w];
        __syncthreads();
    }
    if (wave == 0) publish_block(info, st, pivots, counters, i0, n_valid, lane, pw, pb, my_mask, tv, -1);
}

}  // namespace symgpu
