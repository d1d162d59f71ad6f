// gf2.hip — GF(2) row reduction without row swaps (reference: _rref_binary, symmer/operators/utils.py:292-315)
// and the symmetry-generator kernel built on it (IndependentOp.symmetry_generators,
// symmer/operators/independent_op.py:124-126).
//
// Reference loop: for i = 0..R-1: if row i != 0: pivot = leftmost set column of row i; XOR row i into every
// OTHER row that has that column set.  Sequential in i.  Blocked form used here (bit-exact by construction), up to
// 64 consecutive rows per block:
//   lead    — first non-zero word of each block row (one wave per row, coalesced, early exit).
//   panel   — ONE wavefront, lane = block row.  It holds a WINDOW of 4 words (256 columns) of every block row,
//             starting at the leading word of the block's first non-zero row, runs the reference loop on the window
//             (pivot row broadcast with v_readlane, pivot-column flags of all 64 rows with ONE __ballot, row updates
//             lane-predicated: ~50 instructions per pivot) and records, besides the pivots, the transformation
//             T (new_row_r = XOR_{i in T_r} old_row_i).  The window is exact as long as every processed row has its
//             leading word inside it and does not cancel to zero inside it; the first row that violates this ENDS the
//             block (it opens the next one, whose window starts at its own leading word), so any matrix is handled.
//   select  — for every row r outside the block: f(r) = its bits at the block's pivot columns BEFORE the block is
//             applied.  The reduced block is the identity on its pivot columns, so the unique combination of reduced
//             block rows that clears those bits is f(r) itself — exactly the row the sequential loop produces; in terms
//             of the OLD block rows the selector is g = f*T.  Block rows use g = T_r (minus themselves).
//   sweep   — row ^= XOR_{i in g(row)} old_block_row_i for ALL rows, one pass over the matrix per block (old block
//             rows snapshotted first; 64 of them live in VGPRs; wave-uniform selector -> scalar branches).
// Row-XORs are COUNTED as the reference performs them: with mask_j = set of block rows that held pivot j's column at
// time j, the sequential-time selector of an outside row is t_j = f_j ^ parity(f & mask_j & (2^j-1)), so the count is
// sum_j |mask_j| + sum_r |t(r)|  (derivation in DESIGN.md §3.5).
#include "common.h"
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

namespace symgpu {

constexpr int WK = 64;        // max rows per block = lanes of the panel wave
constexpr int WN = 4;         // window width in 64-bit words
constexpr int NOLEAD = 0x7fffffff;
__global__ void k_fill_nolead(int *__restrict__ lead) { lead[threadIdx.x] = NOLEAD; }

struct BlockInfo {
    i64 i0;                   // first row of the block
    int kk;                   // rows in the block (0: nothing left)
    int pivw[WK];             // absolute pivot word per block row, -1 = no pivot (zero row)
    int pivb[WK];
    u64 mask[WK];             // block rows (bit r < kk, r != j) holding pivot j's column at time j
    u64 T[WK];                // new_row_r = XOR_{i in T[r]} old_row_i
    int w_next;               // the largest pivot word of the block: where the NEXT block's window most likely starts (-1: no guess)
};

struct SweepState {
    i64 next_i0;              // first row not yet processed
};

// lead[r] = index of the first non-zero word of row next_i0 + r (NOLEAD if the row is zero, -1 if beyond the matrix)
__global__ __launch_bounds__(256) void k_lead(const u64 *__restrict__ rows, i64 R, i64 Wc, const SweepState *__restrict__ st, int *__restrict__ lead) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const i64 row = st->next_i0 + r;
    if (r >= WK) return;
    if (row >= R) { if (lane == 0) lead[r] = -1; return; }
    const u64 *p = rows + row * Wc;
    int found = NOLEAD;
    for (i64 w0 = 0; w0 < Wc; w0 += 64) {
        const i64 w = w0 + lane;
        const u64 nz = __ballot(w < Wc && p[w] != 0);
        if (nz) { found = (int)(w0 + __builtin_ctzll(nz)); break; }
    }
    if (lane == 0) lead[r] = found;
}

__global__ void k_sum_u32(const u32 *__restrict__ p, i64 n, unsigned long long *__restrict__ out) {
    unsigned long long s = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

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

// the panel proper: ONE wavefront (lane = block row), `a` = this lane's leading word (lead[] semantics), block starts at i0
__device__ __forceinline__ void panel_wave(const u64 *__restrict__ rows, i64 R, i64 Wc, i64 i0, int a, int lane, SweepState *__restrict__ st,
                                           BlockInfo *__restrict__ info, i64 *__restrict__ pivots, unsigned long long *__restrict__ xor_count,
                                           const u64 *spec = nullptr, int w_spec = -1, int lean = 1, int *kk_out = nullptr, int *pw_out = nullptr,
                                           int *pb_out = nullptr) {
    if (kk_out) { *kk_out = 0; *pw_out = -1; *pb_out = 0; }
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
    if (lane == 0 && kk > 0) atomicAdd(xor_count + 2, 1ULL | ((unsigned long long)narrow_ran << 32));
    // publish: only rows < kk belong to the block
    const u64 low = (kk >= 64) ? ~0ULL : ((1ULL << kk) - 1ULL);
    const bool mine = lane < kk;
    if (kk_out) { *kk_out = kk; *pw_out = mine ? pw : -1; *pb_out = pb; }
    info->pivw[lane] = mine ? pw : -1;
    info->pivb[lane] = mine ? pb : 0;
    info->mask[lane] = mine ? (my_mask & low) : 0ULL;
    info->T[lane] = mine ? tv : 0ULL;
    if (mine && pivots) pivots[i0 + lane] = pw < 0 ? -1 : (i64)pw * 64 + pb;
    unsigned long long c = mine ? (unsigned long long)__popcll(my_mask & low) : 0ULL;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane == 0) {
        info->i0 = i0;
        info->kk = kk;
        info->w_next = w_max;                                        // w_max is wave-uniform (scalar running maximum)
        st->next_i0 = i0 + kk;
        if (c) atomicAdd(xor_count, c);
    }
}

// ---- full-row panel (round 3): sparse rows lead at scattered words, and the 4-word window then ends a block after a row or two
// (700 x 700 at density 0.003: 450 blocks instead of 11, 8.7x the dense time).  When the window would end the block early and the
// rows are at most FULL_WC words long, the whole workgroup runs the reference loop on the 64 FULL rows in LDS (<= 128 KiB, the
// sweep's table area): wavefront 0 finds the pivot of row j and the block rows that hold its column and keeps T, everybody XORs
// row j into those rows.  Two barriers per pivot (~0.5 us) instead of ~0.25 us in registers, but the block never ends early.
constexpr int FULL_WC = 256;
__device__ __forceinline__ void panel_full(const u64 *__restrict__ rows, i64 R, i64 Wc, i64 i0, int a, u64 *__restrict__ m /* LDS [64][Wc] */,
                                           u64 *__restrict__ s_bc /* LDS [4] */, SweepState *__restrict__ st, BlockInfo *__restrict__ info,
                                           i64 *__restrict__ pivots, unsigned long long *__restrict__ xor_count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nt = blockDim.x;
    const int W = (int)Wc;
    const int n_valid = (int)(R - i0 < WK ? R - i0 : WK);
    for (int x = threadIdx.x; x < n_valid * W; x += nt) m[x] = rows[i0 * Wc + x];
    __syncthreads();
    int pw = -1, pb = 0;                                            // wavefront 0, lane = block row
    u64 my_mask = 0, tv = 1ULL << lane;
    if (threadIdx.x == 0) atomicAdd(xor_count + 2, 1ULL);           // block statistics: a block (the full-row ones are counted where the choice is made)
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
    if (wave == 0) {
        const bool mine = lane < n_valid;
        info->pivw[lane] = mine ? pw : -1;
        info->pivb[lane] = mine ? pb : 0;
        info->mask[lane] = mine ? my_mask : 0ULL;
        info->T[lane] = mine ? tv : 0ULL;
        if (mine && pivots) pivots[i0 + lane] = pw < 0 ? -1 : (i64)pw * 64 + pb;
        unsigned long long c = mine ? (unsigned long long)__popcll(my_mask) : 0ULL;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0) {
            info->i0 = i0;
            info->kk = n_valid;
            info->w_next = -1;
            st->next_i0 = i0 + n_valid;
            if (c) atomicAdd(xor_count, c);
        }
    }
}

__global__ __launch_bounds__(64) void k_wpanel(const u64 *__restrict__ rows, i64 R, i64 Wc, SweepState *__restrict__ st, const int *__restrict__ lead,
                                                BlockInfo *__restrict__ info, i64 *__restrict__ pivots, unsigned long long *__restrict__ xor_count, int lean) {
    const i64 i0 = st->next_i0;
    panel_wave(rows, R, Wc, i0, i0 < R ? lead[threadIdx.x] : -1, threadIdx.x, st, info, pivots, xor_count, nullptr, -1, lean);
}

// selectors of all rows (in terms of the OLD block rows), reference-order XOR count, snapshot of the old block rows.
// One wavefront per row, lane j <-> pivot j: the 64 pivot-column bits are fetched in parallel and f is ONE __ballot.
// one wavefront, one row: its selector in terms of the OLD block rows, and the row's share of the reference-order XOR count
__device__ __forceinline__ u64 select_row(const u64 *__restrict__ rows, i64 Wc, i64 r, int lane, i64 i0, int kk, int pw, int pb, u64 mj, u64 Tj,
                                          u32 *__restrict__ rowcnt) {
    if (r >= i0 && r < i0 + kk) {
        // new_r = XOR_{i in T_r} old_i = old_r ^ XOR_{i in T_r xor {r}} old_i
        return readlane64(Tj, (int)(r - i0)) ^ (1ULL << (r - i0));
    }
    const bool bit = (lane < kk && pw >= 0) ? ((rows[r * Wc + pw] >> pb) & 1ULL) : false;
    const u64 f = __ballot(bit);
    // sequential-time selector t_j = f_j ^ parity(f & mask_j & (2^j-1)): |t| row-XORs in the reference loop
    const bool tj = bit ^ (bool)(__popcll(f & mj) & 1);
    const u64 t = __ballot(tj);
    if (lane == 0 && rowcnt) atomicAdd(&rowcnt[r], (u32)__popcll(t));  // fire and forget (a load + store pair puts a round trip in front of the selector)
    u64 x = bit ? Tj : 0ULL;                                          // g = XOR_{j in f} T_j
    for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off);
    return x;
}

__global__ __launch_bounds__(256) void k_select(const u64 *__restrict__ rows, i64 R, i64 Wc, const BlockInfo *__restrict__ info,
                                                 u64 *__restrict__ sel, u64 *__restrict__ snap, u32 *__restrict__ rowcnt) {
    const int kk = info->kk;
    if (kk == 0) return;
    const int lane = threadIdx.x & 63;
    const i64 i0 = info->i0;
    const int pw = info->pivw[lane], pb = info->pivb[lane];
    const u64 mj = info->mask[lane] & ((1ULL << lane) - 1ULL);      // earlier block rows that held pivot `lane`'s column
    const u64 Tj = info->T[lane];
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r < R) {
        const u64 g = select_row(rows, Wc, r, lane, i0, kk, pw, pb, mj, Tj, rowcnt);
        if (lane == 0) sel[r] = g;
    }
    // snapshot of the old block rows (the sweep overwrites them while other workgroups still read them)
    const i64 total = (i64)kk * Wc;
    for (i64 k = (i64)blockIdx.x * 256 + threadIdx.x; k < total; k += (i64)gridDim.x * 256) snap[k] = rows[i0 * Wc + k];
}


// Each lane owns one word column of SW_ROWS rows (kept in registers); the old block rows stream past once
// (independent loads, no dependent load->xor->store chain per row) and are XORed in under wave-uniform selector bits.
template <int SW_ROWS, int UNR>
__device__ __forceinline__ void sweep_tile(u64 *__restrict__ rows, i64 R, i64 Wc, int kk, const u64 *__restrict__ sel, const u64 *__restrict__ snap,
                                           i64 col_block, i64 row_group) {
    if (kk == 0) return;
    const i64 w = col_block * 256 + threadIdx.x;
    const bool live = w < Wc;
    const i64 wl = live ? w : Wc - 1;                               // dead lanes load a valid column and never store
    const i64 rb = row_group * SW_ROWS;
    const bool full = rb + SW_ROWS <= R;                             // uniform: branch-free loads and stores for full tiles
    u32 slo[SW_ROWS], shi[SW_ROWS];
    u64 x[SW_ROWS];
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < SW_ROWS; ++k) {
        const i64 r = (full || rb + k < R) ? rb + k : R - 1;          // clamped: rows past the end are loaded but never stored
        const u64 sv = (rb + k < R) ? sel[r] : 0ULL;
        slo[k] = __builtin_amdgcn_readfirstlane((u32)sv);
        shi[k] = __builtin_amdgcn_readfirstlane((u32)(sv >> 32));
        any |= slo[k] | shi[k];
        x[k] = rows[r * Wc + wl];
    }
    if (any == 0) return;                                            // uniform
    const u64 *sp = snap + wl;
#pragma unroll UNR
    for (int j = 0; j < kk; ++j) {
        const u64 b = sp[(i64)j * Wc];
        const u32 blo = (u32)b, bhi = (u32)(b >> 32);
#pragma unroll
        for (int k = 0; k < SW_ROWS; ++k) {
            // all-ones / zero from selector bit j in ONE VALU op (v_bfe_i32): the CU's single scalar unit would otherwise
            // be the bottleneck (3 SALU per (j, row))
            const u32 sbits = (j < 32) ? slo[k] : shi[k];
            const u32 m = (u32)__builtin_amdgcn_sbfe((int)sbits, j & 31, 1);
            const u32 lo = __builtin_amdgcn_bitop3_b32((u32)x[k], blo, m, 0x78);
            const u32 hi = __builtin_amdgcn_bitop3_b32((u32)(x[k] >> 32), bhi, m, 0x78);
            x[k] = ((u64)hi << 32) | lo;
        }
    }
    if (!live) return;
    if (full) {
        // unconditional back-to-back stores (a conditional store per row made the compiler wait for the previous store:
        // s_waitcnt vmcnt(0) before each of the 16 stores serialised them)
        u64 *dst = rows + rb * Wc + w;
#pragma unroll
        for (int k = 0; k < SW_ROWS; ++k) dst[(i64)k * Wc] = x[k];
    } else {
#pragma unroll
        for (int k = 0; k < SW_ROWS; ++k)
            if (rb + k < R) rows[(rb + k) * Wc + w] = x[k];
    }
}

template <int SW_ROWS, int UNR>
__global__ __launch_bounds__(256) void k_sweep(u64 *__restrict__ rows, i64 R, i64 Wc, const BlockInfo *__restrict__ info,
                                                const u64 *__restrict__ sel, const u64 *__restrict__ snap) {
    sweep_tile<SW_ROWS, UNR>(rows, R, Wc, info->kk, sel, snap, blockIdx.x, blockIdx.y);
}

// ---- Method-of-Four-Russians sweep ------------------------------------------------------------------------------
// The flag-per-block-row sweep above costs 3 VALU instructions per (block row, matrix row, word): ~200 per word of a matrix
// row for a 64-row block, which makes the sweep VALU-bound.  Here a workgroup owns a 64-word column tile and FIRST tabulates,
// in LDS, all 16 XOR combinations of every group of 4 old block rows (16 groups x 16 entries x 64 words x 8 B = 128 KiB of the
// CU's 160 KiB).  A matrix row then needs 16 table look-ups (ds_read_b64, wave-uniform entry index taken from 4 selector bits,
// consecutive lanes -> consecutive words: conflict free) and 16 XORs per word instead of 64 conditional ones.
// PHASE as in k_sweep_lookahead: 0 = only the rows of the next block, 1 = workgroup 0 runs the panel of the next block and the
// others sweep all remaining rows.
constexpr int M4_TW = 64;                       // words per column tile = lanes
constexpr int M4_NT = 1024;                     // threads per workgroup (16 waves; one workgroup per CU because of the table)
constexpr int M4_U = 4;                         // rows in flight per wave
constexpr size_t M4_LDS = (size_t)16 * 16 * M4_TW * sizeof(u64);

// PHASE 3 (round 3) = phase 0 and the selector launch in ONE grid: blocks 0..3 compute the selectors of the next block's 64 rows and
// publish them (agent-scope stores, one tagged flag per row), the next n_tiles blocks are phase 0's tile workgroups — they build their
// tables straight from the old block rows (nobody writes those in this launch) and wait for the 64 flags before they touch the next
// block's rows — and the remaining blocks compute the selectors of all other rows (which phase 0 never touches) and the snapshot.
// One kernel boundary less on the critical path of every block: select 5 us -> hidden behind phase 0.
constexpr int SEL_PRI = 4;                      // priority blocks: 16 rows (wavefronts) each = the next block's 64 rows
struct FusedSelect {
    u64 *sel;                                   // writable view of the selectors
    u64 *snap;
    u32 *rowcnt;
    u64 *ready;                                 // [64][2] granules {epoch 32 | half of the row's selector 32}: the data is the flag
    u32 epoch;
    u32 *fail;                                  // a tile workgroup gave up waiting
    int full_panel;                             // 1: the panel may switch to the full rows in LDS (panel_full)
    int lean_panel;                             // 1: two-word windows run panel_loop_narrow (0: the generic loop; tests)
};
template <int PHASE>
__global__ __launch_bounds__(M4_NT) void k_sweep_m4r(u64 *__restrict__ rows, i64 R, i64 Wc, const BlockInfo *__restrict__ info,
                                                      const u64 *__restrict__ sel, const u64 *__restrict__ snap, int n_tiles, int n_chunks,
                                                      BlockInfo *__restrict__ info_next, SweepState *__restrict__ st, i64 *__restrict__ pivots,
                                                      unsigned long long *__restrict__ xor_count, int *__restrict__ lead, FusedSelect fs) {
    extern __shared__ u64 tab[];                                    // [16 groups][16 entries][64 words]
    __shared__ u64 s_sel[WK];
    __shared__ int s_ok;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kk = info->kk;
    const i64 i0n = info->i0 + kk;                                  // first row of the next block
    // rows of the next block: [nb, ne)   (PHASE 2: plain sweep of all rows, no lookahead)
    const i64 nb = PHASE == 2 ? 0 : (i0n < R ? i0n : R), ne = PHASE == 2 ? 0 : (i0n + WK < R ? i0n + WK : R);
    int k = blockIdx.x;
    if (PHASE == 3) {
        if (k < SEL_PRI || k >= SEL_PRI + n_tiles) {
            // ---- selector role: one wavefront per row ----
            if (kk == 0) return;
            const i64 i0 = info->i0;
            const int pw = info->pivw[lane], pb = info->pivb[lane];
            const u64 mj = info->mask[lane] & ((1ULL << lane) - 1ULL);
            const u64 Tj = info->T[lane];
            i64 r = -1;
            if (k < SEL_PRI) { r = nb + (i64)k * 16 + wave; if (r >= ne) r = -1; }
            else {
                const i64 v = (i64)(k - SEL_PRI - n_tiles) * 16 + wave, n_other = R - (ne - nb);
                if (v < n_other) r = v < nb ? v : v + (ne - nb);
            }
            if (r >= 0) {
                const u64 g = select_row(rows, Wc, r, lane, i0, kk, pw, pb, mj, Tj, fs.rowcnt);
                if (lane == 0) {
                    if (k < SEL_PRI) {
                        __hip_atomic_store(&fs.ready[2 * (r - nb)], ((u64)fs.epoch << 32) | (u32)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(&fs.ready[2 * (r - nb) + 1], ((u64)fs.epoch << 32) | (u32)(g >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else fs.sel[r] = g;
                }
            }
            // snapshot of the old block rows for phase 1 (which overwrites them while other workgroups still read them)
            const i64 n_sel = (i64)gridDim.x - n_tiles, me = k < SEL_PRI ? k : k - n_tiles;
            const i64 total = (i64)kk * Wc;
            for (i64 x = me * M4_NT + threadIdx.x; x < total; x += n_sel * M4_NT) fs.snap[x] = rows[i0 * Wc + x];
            return;
        }
        k -= SEL_PRI;
    }
    if (PHASE == 1) {
        if (k == 0) {
            // ---- panel workgroup; the leading words were collected by phase 0 (reset for the next block).  One wavefront on a 4-word
            //      window — or, when the window would end the block early and the rows fit, the whole workgroup on the full rows ----
            int a = -1;
            u64 spec[WN] = {0, 0, 0, 0};
            const int w_spec = info->w_next;                         // the block that was just panelled guessed this block's window
            if (wave == 0 && i0n + lane < R) {
                a = lead[lane];
                if (w_spec >= 0) {                                   // the window words at the guess: loaded beside the leads, not behind them
#pragma unroll
                    for (int k = 0; k < WN; ++k) spec[k] = (i64)w_spec + k < Wc ? rows[(i0n + lane) * Wc + w_spec + k] : 0ULL;
                }
            }
            if (wave == 0) {
                bool full = false;
                if (fs.full_panel && Wc <= FULL_WC && i0n < R) {
                    const bool valid = a >= 0;
                    const u64 fin_m = __ballot(valid && a != NOLEAD);
                    if (fin_m != 0) {
                        const int w_lo = window_start(a, valid, __builtin_ctzll(fin_m));
                        const u64 bad = __ballot(valid && a != NOLEAD && !(a >= w_lo && a < w_lo + WN));   // rows that lead outside the window
                        const int n_valid = __popcll(__ballot(valid));
                        full = bad != 0 && __builtin_ctzll(bad) < (n_valid < 32 ? n_valid : 32);
                    }
                }
                if (lane == 0) { s_ok = full ? 1 : 0; if (full) atomicAdd(fs.fail + 1, 1u); }
                if (i0n + lane < R) lead[lane] = NOLEAD;
            }
            __syncthreads();
            if (s_ok) {
                if (wave != 0) a = 0;
                panel_full(rows, R, Wc, i0n, a, tab, s_sel, st, info_next, pivots, xor_count);
            } else if (wave == 0) panel_wave(rows, R, Wc, i0n, a, lane, st, info_next, pivots, xor_count, spec, w_spec, fs.lean_panel);
            return;
        }
        --k;
    }
    constexpr bool P0 = PHASE == 0 || PHASE == 3;
    if (kk == 0 && !P0) return;
    const int tile = k % n_tiles, chunk = k / n_tiles;
    // rows of this chunk: PHASE 0 the next block's rows, PHASE 1 / 2 the virtual index space of all OTHER rows
    const i64 n_rows = P0 ? ne - nb : R - (ne - nb);
    const i64 per = (n_rows + n_chunks - 1) / n_chunks;
    const i64 v_lo = (i64)chunk * per, v_hi = v_lo + per < n_rows ? v_lo + per : n_rows;
    if (v_lo >= v_hi) return;
    const i64 w = (i64)tile * M4_TW + lane;
    const bool live = w < Wc;
    const i64 wl = live ? w : Wc - 1;
    // ---- stream the rows: M4_U per wave and step, software pipelined (the loads of step i+1 are in flight while step i
    //      does its table look-ups: a wave only runs a handful of steps, so nothing else would hide the load latency) ----
    const i64 shift = ne - nb;
    const i64 step = M4_U * (M4_NT / 64);
    i64 rn[M4_U];
    u64 xn[M4_U], sn[M4_U];
    auto fetch = [&](i64 v0, bool with_sel) {
#pragma unroll
        for (int u = 0; u < M4_U; ++u) {
            const i64 v = v0 + u < v_hi ? v0 + u : (v0 < v_hi ? v0 : v_lo);   // tail: surplus slots repeat a valid row, never stored
            rn[u] = P0 ? nb + v : (v < nb ? v : v + shift);
            if (with_sel) sn[u] = kk != 0 ? (PHASE == 3 ? s_sel[rn[u] - nb] : sel[rn[u]]) : 0ULL;
            xn[u] = rows[rn[u] * Wc + wl];
        }
    };
    i64 v0 = v_lo + M4_U * wave;
    // phases 1 / 2: the first rows and their selectors are on their way while the tables are built (round 4: the loads used to start behind
    // the table build and its barrier, 2-3 us of every 15 us launch with nothing in flight)
    if (PHASE != 3 && v0 < v_hi) fetch(v0, true);
    // ---- tabulate the XOR combinations of the old block rows ----
    if (kk != 0) {
        for (int g = wave; g < 16; g += M4_NT / 64) {
            u64 sv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                sv[i] = (4 * g + i < kk) ? (PHASE == 3 ? rows[(info->i0 + 4 * g + i) * Wc + wl] : snap[(i64)(4 * g + i) * Wc + wl]) : 0ULL;
            u64 t[16];
            t[0] = 0; t[1] = sv[0]; t[2] = sv[1]; t[3] = sv[0] ^ sv[1];
#pragma unroll
            for (int e = 0; e < 4; ++e) t[4 + e] = t[e] ^ sv[2];
#pragma unroll
            for (int e = 0; e < 8; ++e) t[8 + e] = t[e] ^ sv[3];
#pragma unroll
            for (int e = 0; e < 16; ++e) tab[(g * 16 + e) * M4_TW + lane] = t[e];
        }
    }
    if (PHASE == 3) {
        // the rows themselves do not depend on the selectors: their loads are issued before the wait
        if (v0 < v_hi) fetch(v0, false);
        if (kk != 0) {
            // the selectors of the next block's rows come from blocks 0..3 of this launch: wait for their flags (bounded), then read them
            if (wave == 0) {
                const int nr = (int)(ne - nb);
                bool ok = true;
                u64 g0 = 0, g1 = 0;
                for (u32 spins = 0;; ++spins) {
                    const u64 tagged = (u64)fs.epoch << 32;
                    g0 = lane < nr ? __hip_atomic_load(&fs.ready[2 * lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tagged;
                    g1 = lane < nr ? __hip_atomic_load(&fs.ready[2 * lane + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tagged;
                    if (__ballot((u32)(g0 >> 32) == fs.epoch && (u32)(g1 >> 32) == fs.epoch) == ~0ULL) break;
                    if (spins >= (1u << 22)) { ok = false; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                s_sel[lane] = (ok && lane < nr) ? (((u64)(u32)g1 << 32) | (u32)g0) : 0ULL;
                if (lane == 0) { s_ok = ok ? 1 : 0; if (!ok) atomicOr(fs.fail, 1u); }
            }
        }
    }
    __syncthreads();
    if (PHASE == 3 && kk != 0 && !s_ok) return;                      // flagged: the call fails loudly
    if (PHASE == 3) {
#pragma unroll
        for (int u = 0; u < M4_U; ++u) sn[u] = (kk != 0 && v0 < v_hi) ? s_sel[rn[u] - nb] : 0ULL;
    }
    for (; v0 < v_hi; v0 += step) {
        i64 r[M4_U];
        u64 x[M4_U];
        u32 slo[M4_U], shi[M4_U];
#pragma unroll
        for (int u = 0; u < M4_U; ++u) {
            r[u] = rn[u]; x[u] = xn[u];
            slo[u] = __builtin_amdgcn_readfirstlane((u32)sn[u]);
            shi[u] = __builtin_amdgcn_readfirstlane((u32)(sn[u] >> 32));
        }
        if (v0 + step < v_hi) fetch(v0 + step, true);                // uniform
#pragma unroll
        for (int u = 0; u < M4_U; ++u) {
            const bool mine = (u == 0 || v0 + u < v_hi);
            if ((slo[u] | shi[u]) != 0u) {                           // uniform; untouched rows are not rewritten
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const u32 e = ((g < 8 ? slo[u] : shi[u]) >> (4 * (g & 7))) & 15u;
                    x[u] ^= tab[(g * 16 + (int)e) * M4_TW + lane];
                }
                if (live && mine) rows[r[u] * Wc + w] = x[u];
            }
            if (P0 && mine) {
                // leading word of the next block's rows for its panel: minimum over the column tiles
                const u64 nz = __ballot(live && x[u] != 0);
                if (nz && lane == 0) atomicMin(&lead[r[u] - nb], tile * M4_TW + (int)__builtin_ctzll(nz));
            }
        }
    }
}

// ---- small matrices: the whole reduction in ONE workgroup -------------------------------------------------------------
// R <= 64 rows and Wc <= 64 words (32 KiB of LDS): the reference loop verbatim — for every row in order: leftmost set column,
// flags of the rows holding it (one ballot), XOR — without the 3 launches per block of the blocked path.  Stabiliser sets,
// generator reconstructions and the symmetry matrices of molecules with <= 32 qubits land here (their rows are sparse and lead
// at scattered columns, which the windowed panel handles poorly).
constexpr int SMALL_R = 64, SMALL_WC = 64;     // wider dense matrices are faster on the blocked path (measured)

__global__ __launch_bounds__(256) void k_rref_small(u64 *__restrict__ rows, int R, int Wc, i64 *__restrict__ pivots,
                                                    unsigned long long *__restrict__ xor_count) {
    extern __shared__ u64 m[];                                      // [R][Wc]
    __shared__ u64 s_mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = R * Wc;
    for (int k = threadIdx.x; k < total; k += 256) m[k] = rows[k];
    __syncthreads();
    unsigned long long count = 0;                                   // kept by thread 0
    for (int j = 0; j < R; ++j) {
        if (wave == 0) {
            int pw = -1, pb = 0;
            for (int w0 = 0; w0 < Wc; w0 += 64) {
                const int w = w0 + lane;
                const u64 v = w < Wc ? m[j * Wc + w] : 0ULL;
                const u64 nz = __ballot(v != 0);
                if (nz) {
                    const int l = __builtin_ctzll(nz);
                    pw = w0 + l;
                    pb = __builtin_ctzll(__shfl(v, l));
                    break;
                }
            }
            u64 mask = 0;
            if (pw >= 0) mask = __ballot(lane < R && lane != j && ((m[lane * Wc + pw] >> pb) & 1ULL));
            if (lane == 0) {
                s_mask = mask;
                count += (unsigned long long)__popcll(mask);
                if (pivots) pivots[j] = pw < 0 ? -1 : (i64)pw * 64 + pb;
            }
        }
        __syncthreads();
        const u64 mask = s_mask;
        if (mask) {
            for (int k = threadIdx.x; k < total; k += 256) {
                const int r = k / Wc, w = k - r * Wc;
                if ((mask >> r) & 1ULL) m[k] ^= m[j * Wc + w];
            }
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < total; k += 256) rows[k] = m[k];
    if (threadIdx.x == 0 && xor_count) *xor_count = count;
}

// ---- in-place reduction of a device matrix -------------------------------------------------------
// fused_select: launch A carries the selectors of the next block's rows to its tile workgroups through in-launch flags (one launch less per
// block).  *timed_out: a tile workgroup gave up waiting (its workgroups were not co-resident) — the matrix is then partly updated: the caller
// restores it and runs the schedule with separate launches.
static int rref_dev_impl(u64 *rows, i64 R, i64 Wc, i64 *xor_count, i64 *pivots_host, bool fused_select_allowed, bool *timed_out) {
    hipStream_t st = ctx().stream;
    *timed_out = false;
    if (xor_count) *xor_count = 0;
    if (R <= 0 || Wc <= 0) return SYMGPU_OK;
    if (Wc >= ((i64)1 << 31) - 64) { set_error("rref: Wc too large"); return SYMGPU_E_INVALID; }
    {   // one-workgroup path for small matrices (SYMGPU_GF2_SMALL=0 disables it: tests)
        const char *env_small = getenv("SYMGPU_GF2_SMALL");
        const bool small_attr = SG_DEVICE_ONCE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rref_small), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                   SMALL_R * SMALL_WC * 8) == hipSuccess);
        if (R <= SMALL_R && Wc <= SMALL_WC && small_attr && !(env_small && env_small[0] == '0')) {
            Scratch piv, count;
            SG_TRY(piv.alloc((size_t)R * 8));
            SG_TRY(count.alloc(16));
            HIP_TRY(hipMemsetAsync(count.p, 0, 16, st));
            hipLaunchKernelGGL(k_rref_small, dim3(1), dim3(256), (size_t)R * Wc * 8, st, rows, (int)R, (int)Wc, piv.as<i64>(),
                               count.as<unsigned long long>());
            KERNEL_CHECK();
            unsigned long long h = 0;
            HIP_TRY(hipMemcpyAsync(&h, count.p, 8, hipMemcpyDeviceToHost, st));
            if (pivots_host) HIP_TRY(hipMemcpyAsync(pivots_host, piv.p, (size_t)R * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (xor_count) *xor_count = (i64)h;
            return SYMGPU_OK;
        }
    }
    Scratch info, state, lead, sel, snap, count, piv, rowcnt, ready;
    SG_TRY(info.alloc(2 * sizeof(BlockInfo)));
    SG_TRY(state.alloc(sizeof(SweepState)));
    SG_TRY(lead.alloc(WK * sizeof(int)));
    SG_TRY(sel.alloc((size_t)R * 8));
    SG_TRY(snap.alloc((size_t)WK * Wc * 8));
    SG_TRY(count.alloc(32));                                        // {XOR count, time-out flag | full-row panels << 32, blocks | two-word windows << 32, -}
    SG_TRY(piv.alloc((size_t)R * 8));
    SG_TRY(rowcnt.alloc((size_t)R * 4));
    HIP_TRY(hipMemsetAsync(rowcnt.p, 0, (size_t)R * 4, st));
    HIP_TRY(hipMemsetAsync(count.p, 0, 32, st));
    SG_TRY(ready.alloc(2 * WK * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(ready.p, 0, 2 * WK * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(state.p, 0, sizeof(SweepState), st));
    HIP_TRY(hipMemsetAsync(info.p, 0, 2 * sizeof(BlockInfo), st));   // {i0 = 0, kk = 0}: "nothing swept yet, next block starts at row 0"
    constexpr int SW_ROWS = 16;                                     // rows per sweep workgroup, held in VGPRs
    const unsigned gx = (unsigned)((Wc + 255) / 256), gy = (unsigned)((R + SW_ROWS - 1) / SW_ROWS);
    const unsigned gsel = (unsigned)((R + 3) / 4);
    BlockInfo *binfo = info.as<BlockInfo>();
    // Four-Russians sweep (128 KiB of LDS per workgroup) unless disabled or refused by the runtime
    const bool m4r_attr = SG_DEVICE_ONCE(
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess);
    const char *env_m4r = getenv("SYMGPU_GF2_M4R"), *env_la = SG_TUNE("SYMGPU_GF2_LOOKAHEAD");   // read per call: the tests switch paths
    const bool m4r = m4r_attr && !(env_m4r && env_m4r[0] == '0'), m4r_plain = m4r;
    const int m4_tiles = (int)((Wc + M4_TW - 1) / M4_TW);
    int m4_chunks = 256 / m4_tiles;                              // one workgroup per CU: about one round of workgroups
    if ((i64)m4_chunks > (R + 127) / 128) m4_chunks = (int)((R + 127) / 128);   // the table costs about 100 rows of work
    if (m4_chunks < 1) m4_chunks = 1;
    const bool lookahead = !(env_la && env_la[0] == '0');
    // SYMGPU_GF2_FUSED_SELECT=0: the selector launch on its own in front of phase 0 (three launches per block instead of two)
    const bool fused_select = fused_select_allowed;
    FusedSelect fs;
    fs.sel = sel.as<u64>(); fs.snap = snap.as<u64>(); fs.rowcnt = rowcnt.as<u32>(); fs.ready = ready.as<u64>(); fs.epoch = 0;
    fs.fail = reinterpret_cast<u32 *>(count.p) + 2;
    fs.full_panel = [] { const char *e = SG_TUNE("SYMGPU_GF2_FULL_PANEL"); return !(e && e[0] == '0'); }() ? 1 : 0;
    fs.lean_panel = [] { const char *e = SG_TUNE("SYMGPU_GF2_LEAN_PANEL"); return !(e && e[0] == '0'); }() ? 1 : 0;
    if (lookahead && m4r && (i64)m4_tiles * m4_chunks + 1 < ((i64)1 << 31)) {
        // Pipeline, three launches per block: select(b) -> phase 0: sweep of the rows of block b+1 + their leading words ->
        // phase 1: panel of block b+1 (-> the other info buffer) inside the sweep of all remaining rows.  The very first
        // iteration has nothing to sweep (zeroed info): it only collects the leading words of rows 0..63 and panels block 0.
        // `it` keeps counting across batches.
        hipLaunchKernelGGL(k_fill_nolead, dim3(1), dim3(WK), 0, st, lead.as<int>());
        i64 it = 0, done = 0, prev = -1;
        bool finished = false;
        while (!finished) {
            i64 n_iter = (R - done + WK - 1) / WK + 1;
            if (n_iter > 4096) n_iter = 4096;
            for (i64 k = 0; k < n_iter; ++k, ++it) {
                BlockInfo *cur = binfo + ((it + 1) & 1), *next = binfo + (it & 1);      // cur: block it-1 (to sweep), next: block it (to panel)
                fs.epoch = (u32)(it + 1);
                if (fused_select) {
                    // selectors of block it-1 and phase 0 in one grid (the very first iteration has no block to select for: kk == 0)
                    const unsigned g3 = (unsigned)(SEL_PRI + m4_tiles + (R + 15) / 16);
                    hipLaunchKernelGGL(k_sweep_m4r<3>, dim3(g3), dim3(M4_NT), M4_LDS, st, rows, R, Wc, cur, sel.as<u64>(), snap.as<u64>(),
                                       m4_tiles, 1, next, state.as<SweepState>(), piv.as<i64>(), count.as<unsigned long long>(), lead.as<int>(), fs);
                } else {
                    if (it > 0)
                        hipLaunchKernelGGL(k_select, dim3(gsel), dim3(256), 0, st, rows, R, Wc, cur, sel.as<u64>(), snap.as<u64>(), rowcnt.as<u32>());
                    hipLaunchKernelGGL(k_sweep_m4r<0>, dim3(m4_tiles), dim3(M4_NT), M4_LDS, st, rows, R, Wc, cur, sel.as<u64>(), snap.as<u64>(),
                                       m4_tiles, 1, next, state.as<SweepState>(), piv.as<i64>(), count.as<unsigned long long>(), lead.as<int>(), fs);
                }
                ProfScope prof(2);
                hipLaunchKernelGGL(k_sweep_m4r<1>, dim3(m4_tiles * m4_chunks + 1), dim3(M4_NT), M4_LDS, st, rows, R, Wc, cur, sel.as<u64>(),
                                   snap.as<u64>(), m4_tiles, m4_chunks, next, state.as<SweepState>(), piv.as<i64>(), count.as<unsigned long long>(),
                                   lead.as<int>(), fs);
                KERNEL_CHECK();
            }
            // the block that has been panelled but not swept yet: kk == 0 means the matrix is exhausted
            struct { i64 i0; int kk; } pending;
            {
                u32 w[3] = {0, 0, 0};                                   // (i0 low, i0 high, kk: the head of a BlockInfo)
                SG_TRY(read_back_words(reinterpret_cast<const u32 *>(binfo + ((it + 1) & 1)), 3, nullptr, 0, w));
                pending.i0 = (i64)(((u64)w[1] << 32) | w[0]);
                pending.kk = (int)w[2];
            }
            if (pending.kk == 0) finished = true;
            else if (pending.i0 <= prev) { set_error("rref: no progress (internal error)"); return SYMGPU_E_INVALID; }
            prev = pending.i0;
            done = pending.i0;
        }
    } else {
    i64 done = 0;
    while (done < R) {
        // optimistic batch: every block consumes up to 64 rows; blocks that end early are caught by the read-back
        i64 n_iter = (R - done + WK - 1) / WK;
        if (n_iter > 4096) n_iter = 4096;
        for (i64 it = 0; it < n_iter; ++it) {
            hipLaunchKernelGGL(k_lead, dim3(WK / 4), dim3(256), 0, st, rows, R, Wc, state.as<SweepState>(), lead.as<int>());
            hipLaunchKernelGGL(k_wpanel, dim3(1), dim3(64), 0, st, rows, R, Wc, state.as<SweepState>(), lead.as<int>(), binfo,
                               piv.as<i64>(), count.as<unsigned long long>(), fs.lean_panel);
            hipLaunchKernelGGL(k_select, dim3(gsel), dim3(256), 0, st, rows, R, Wc, binfo, sel.as<u64>(), snap.as<u64>(),
                               rowcnt.as<u32>());
            ProfScope prof(2);
            if (m4r_plain)
                hipLaunchKernelGGL(k_sweep_m4r<2>, dim3(m4_tiles * m4_chunks), dim3(M4_NT), M4_LDS, st, rows, R, Wc, binfo, sel.as<u64>(), snap.as<u64>(),
                                   m4_tiles, m4_chunks, binfo, state.as<SweepState>(), piv.as<i64>(), count.as<unsigned long long>(), lead.as<int>(), fs);
            else
            hipLaunchKernelGGL((k_sweep<SW_ROWS, 4>), dim3(gx, gy), dim3(256), 0, st, rows, R, Wc, binfo, sel.as<u64>(), snap.as<u64>());
            KERNEL_CHECK();
        }
        SweepState hs;
        {
            u32 w[2] = {0, 0};
            SG_TRY(read_back_words(state.as<u32>(), 2, nullptr, 0, w));
            hs.next_i0 = (i64)(((u64)w[1] << 32) | w[0]);
        }
        if (hs.next_i0 <= done) { set_error("rref: no progress (internal error)"); return SYMGPU_E_INVALID; }
        done = hs.next_i0;
    }
    }
    hipLaunchKernelGGL(k_sum_u32, dim3(256), dim3(256), 0, st, rowcnt.as<u32>(), R, count.as<unsigned long long>());
    KERNEL_CHECK();
    unsigned long long hb[3] = {0, 0, 0};
    if (pivots_host) {
        HIP_TRY(hipMemcpyAsync(hb, count.p, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pivots_host, piv.p, (size_t)R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        u32 w[6] = {0, 0, 0, 0, 0, 0};
        SG_TRY(read_back_words(reinterpret_cast<const u32 *>(count.p), 6, nullptr, 0, w));
        for (int k = 0; k < 3; ++k) hb[k] = ((unsigned long long)w[2 * k + 1] << 32) | w[2 * k];
    }
    // which panel the blocks of this run took (symgpu_debug_counter 15 / 16 / 17; a run that is redone after a time-out counts twice)
    bump_counter(15, (i64)(u32)hb[2]);
    bump_counter(16, (i64)(u32)(hb[1] >> 32));
    bump_counter(17, (i64)(u32)(hb[2] >> 32));
    if (SG_TUNE("SYMGPU_GF2_DEBUG")) fprintf(stderr, "rref %lld x %lld words: full-row panels %u\n", (long long)R, (long long)Wc, (u32)(hb[1] >> 32));
    if ((u32)hb[1] != 0) { *timed_out = true; return SYMGPU_OK; }
    if (xor_count) *xor_count = (i64)hb[0];
    return SYMGPU_OK;
}

static bool g_gf2_fused_off = false;         // a launch-A wait timed out once: the process keeps to the separate-launch schedule

int rref_dev(u64 *rows, i64 R, i64 Wc, i64 *xor_count, i64 *pivots_host) {
    hipStream_t st = ctx().stream;
    if (xor_count) *xor_count = 0;
    if (R <= 0 || Wc <= 0) return SYMGPU_OK;
    const bool env_fused = [] { const char *e = getenv("SYMGPU_GF2_FUSED_SELECT"); return !(e && e[0] == '0'); }();
    const bool inject = [] { const char *e = getenv("SYMGPU_GF2_FUSED_SELECT"); return e && e[0] == '2'; }();      // 2 = tests: pretend the first attempt timed out
    const bool fused = env_fused && !g_gf2_fused_off;
    // The fused schedule waits inside a launch for flags of other workgroups (bounded, ~1 s).  Should that wait ever give up, the matrix
    // is half updated in place — so a copy of the input is kept (2 x 27 MB at 5 TB/s = 11 us of a 2 ms call at cfg4) and the reduction is
    // redone from it with separate launches; the fused form stays off for the rest of the process.
    Scratch orig;
    const bool big = R > SMALL_R || Wc > SMALL_WC;
    bool fused_now = fused;
    if (fused && big) {
        if (orig.alloc((size_t)R * Wc * 8) != SYMGPU_OK) {
            // no room for the safety copy (a matrix near the memory limit): the separate-launch schedule needs none and has no wait to time out
            orig.p = nullptr;
            set_error("");
            fused_now = false;
        } else {
            HIP_TRY(hipMemcpyAsync(orig.p, rows, (size_t)R * Wc * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    bool timed_out = false;
    SG_TRY(rref_dev_impl(rows, R, Wc, xor_count, pivots_host, fused_now, &timed_out));
    if (inject && fused_now && big) timed_out = true;
    if (!timed_out) return SYMGPU_OK;
    if (!orig.p) { set_error("rref: an in-launch wait timed out on a schedule that has none (internal error)"); return SYMGPU_E_HIP; }
    g_gf2_fused_off = !inject;
    if (!inject) note_degraded("GF(2) fused selector launch off: an in-kernel wait timed out (workgroups not co-resident?); the elimination takes three launches per block");
    HIP_TRY(hipMemcpyAsync(rows, orig.p, (size_t)R * Wc * 8, hipMemcpyDeviceToDevice, st));
    if (xor_count) *xor_count = 0;
    SG_TRY(rref_dev_impl(rows, R, Wc, xor_count, pivots_host, false, &timed_out));
    if (timed_out) { set_error("rref: time-out on the separate-launch schedule (internal error)"); return SYMGPU_E_HIP; }
    return SYMGPU_OK;
}

// ---- symmetry-generator matrix build / read-out ----------------------------------------------------
// mat is (2n) x Wc, Wc = Wm + 2*Wq, Wm = ceil(M/64):  row c < n  = [ Z[:,c] | e_c ],  row n+c = [ X[:,c] | e_{n+c} ]
// (the transpose of independent_op.py:124's  vstack([hstack([Z, X]), eye(2n)])  with zero padding columns,
// which can never become pivots).  One wave transposes a 64-term x 64-qubit bit tile with 64 ballots.
__global__ __launch_bounds__(256) void k_build_symmat(const u64 *__restrict__ H, i64 M, int n, int Wq, u64 *__restrict__ mat, i64 Wc) {
    const int lane = threadIdx.x & 63;
    const i64 tile = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);   // 64-term tile index
    const int sw = blockIdx.y;                                   // source word 0..2Wq-1
    const i64 n_tiles = (M + 63) / 64;
    if (tile >= n_tiles) return;
    const i64 t = tile * 64 + lane;
    const u64 word = (t < M) ? H[t * 2 * Wq + sw] : 0ULL;
    u64 mine = 0;
    for (int b = 0; b < 64; ++b) {
        const u64 m = __ballot((word >> b) & 1ULL);
        if (lane == b) mine = m;
    }
    const int q = 64 * (sw % Wq) + lane;
    if (q < n) {
        const i64 c = (sw >= Wq) ? q : (i64)n + q;   // Z words feed rows 0..n-1, X words rows n..2n-1
        mat[c * Wc + tile] = mine;
    }
}

__global__ void k_set_identity(u64 *__restrict__ mat, int n, int Wq, i64 Wc, i64 Wm) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 2 * n) return;
    const int q = c < n ? c : c - n;
    const i64 w = Wm + (c < n ? 0 : Wq) + q / 64;
    mat[(i64)c * Wc + w] |= 1ULL << (q % 64);
}

// flag[c] = 1 iff the first Wm words of row c are all zero (one wave per row)
__global__ __launch_bounds__(256) void k_rowzero_flags(const u64 *__restrict__ mat, i64 R, i64 Wc, i64 Wm, u32 *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    bool nz = false;
    for (i64 w = lane; w < Wm; w += 64) nz |= (mat[r * Wc + w] != 0);
    const u64 any = __ballot(nz);
    if (lane == 0) flag[r] = any ? 0u : 1u;
}

__global__ void k_copy_generators(const u64 *__restrict__ mat, i64 R, i64 Wc, i64 Wm, int W, const u32 *__restrict__ pos, u32 total,
                                  u64 *__restrict__ out) {
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * W) return;
    const i64 r = idx / W;
    const int w = (int)(idx - r * W);
    const u32 p = pos[r];
    const u32 nxt = (r + 1 < R) ? pos[r + 1] : total;
    if (nxt == p + 1) out[(i64)p * W + w] = mat[r * Wc + Wm + w];
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_rref_dev(uint64_t *rows_dev, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots_host) {
    SG_ENTER();
    SG_REQUIRE(R >= 0 && Wc >= 0 && (rows_dev || R * Wc == 0), "rref_dev");
    return rref_dev(rows_dev, R, Wc, xor_count, pivots_host);
}

int symgpu_rref(uint64_t *rows, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots) {
    SG_ENTER();
    SG_REQUIRE(R >= 0 && Wc >= 0 && (rows || R * Wc == 0), "rref");
    if (xor_count) *xor_count = 0;
    if (R == 0 || Wc == 0) {
        if (pivots) for (i64 r = 0; r < R; ++r) pivots[r] = -1;
        return SYMGPU_OK;
    }
    Scratch d;
    SG_TRY(d.alloc((size_t)R * Wc * 8));
    HIP_TRY(hipMemcpyAsync(d.p, rows, (size_t)R * Wc * 8, hipMemcpyHostToDevice, ctx().stream));
    count_h2d((size_t)R * Wc * 8); count_d2h((size_t)R * Wc * 8);
    SG_TRY(rref_dev(d.as<u64>(), R, Wc, xor_count, pivots));
    HIP_TRY(hipMemcpyAsync(rows, d.p, (size_t)R * Wc * 8, hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

int symgpu_symmetry_kernel_dev(symgpu_op_t H, int n_qubits, uint64_t *out, int64_t capacity, int64_t *k, int64_t *xor_count) {
    SG_ENTER(H);
    SG_REQUIRE(H && k && n_qubits >= 1, "symmetry_kernel_dev");
    SG_REQUIRE((n_qubits + 63) / 64 == H->Wq, "symmetry_kernel_dev: n_qubits does not match Wq");
    hipStream_t st = ctx().stream;
    const int n = n_qubits, Wq = H->Wq, W = 2 * Wq;
    const i64 M = H->T, Wm = (M + 63) / 64, Wc = Wm + W, R = 2 * (i64)n;
    Scratch mat, flag, total, gens;
    SG_TRY(mat.alloc((size_t)R * Wc * 8));
    HIP_TRY(hipMemsetAsync(mat.p, 0, (size_t)R * Wc * 8, st));
    if (M > 0) {
        dim3 grid((unsigned)((Wm + 3) / 4), (unsigned)W);
        hipLaunchKernelGGL(k_build_symmat, grid, dim3(256), 0, st, H->rows, M, n, Wq, mat.as<u64>(), Wc);
        KERNEL_CHECK();
    }
    hipLaunchKernelGGL(k_set_identity, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, mat.as<u64>(), n, Wq, Wc, Wm);
    KERNEL_CHECK();
    SG_TRY(rref_dev(mat.as<u64>(), R, Wc, xor_count, nullptr));
    SG_TRY(flag.alloc((size_t)R * 4));
    SG_TRY(total.alloc(16));
    hipLaunchKernelGGL(k_rowzero_flags, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, mat.as<u64>(), R, Wc, Wm, flag.as<u32>());
    KERNEL_CHECK();
    SG_TRY(exclusive_scan_u32(flag.as<u32>(), flag.as<u32>(), R, total.as<u32>()));
    u32 kcount = 0;
    SG_TRY(read_back_words(total.as<u32>(), 1, nullptr, 0, &kcount));
    *k = kcount;
    if ((i64)kcount > capacity) {
        set_error("symmetry_kernel: capacity %lld < %u generators", (long long)capacity, kcount);
        return SYMGPU_E_CAPACITY;
    }
    if (kcount == 0) return SYMGPU_OK;
    SG_REQUIRE(out, "symmetry_kernel: null output");
    SG_TRY(gens.alloc((size_t)kcount * W * 8));
    hipLaunchKernelGGL(k_copy_generators, dim3((unsigned)((R * W + 255) / 256)), dim3(256), 0, st, mat.as<u64>(), R, Wc, Wm, W,
                       flag.as<u32>(), kcount, gens.as<u64>());
    KERNEL_CHECK();
    HIP_TRY(hipMemcpyAsync(out, gens.p, (size_t)kcount * W * 8, hipMemcpyDeviceToHost, st));
    count_d2h((size_t)kcount * W * 8);
    HIP_TRY(hipStreamSynchronize(st));
    return SYMGPU_OK;
}

int symgpu_symmetry_kernel(const uint64_t *H, int64_t M, int n_qubits, int Wq, uint64_t *out, int64_t capacity, int64_t *k,
                           int64_t *xor_count) {
    SG_ENTER();
    SG_REQUIRE(M >= 0 && n_qubits >= 1 && Wq == (n_qubits + 63) / 64 && k, "symmetry_kernel: sizes");
    SG_REQUIRE(H || M == 0, "symmetry_kernel: null input");
    symgpu_op_t op = nullptr;
    SG_TRY(symgpu_op_upload(H, nullptr, M, Wq, &op));
    int rc = symgpu_symmetry_kernel_dev(op, n_qubits, out, capacity, k, xor_count);
    symgpu_op_free(op);
    return rc;
}

}  // extern "C"
