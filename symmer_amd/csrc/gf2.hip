// gf2.hip — GF(2) row reduction without row swaps (reference: _rref_binary, symmer/operators/utils.py:292-315)
// (the symmetry-generator kernel built on it: gf2_symmetry.hip).
//
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
#include "gf2_panel.h"
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

namespace symgpu {

__global__ void k_fill_nolead(int *__restrict__ lead) { lead[threadIdx.x] = NOLEAD; }

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

__global__ __launch_bounds__(64) void k_wpanel(const u64 *__restrict__ rows, i64 R, i64 Wc, SweepState *__restrict__ st, const int *__restrict__ lead,
                                                BlockInfo *__restrict__ info, i64 *__restrict__ pivots, Gf2Counters *__restrict__ counters, int lean) {
    const i64 i0 = st->next_i0;
    panel_wave(rows, R, Wc, i0, i0 < R ? lead[threadIdx.x] : -1, threadIdx.x, st, info, pivots, counters, nullptr, -1, lean);
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
// PHASE: one of M4_NEXT, M4_PANEL_REST, M4_ALL, M4_SELECT_NEXT (gf2_common.h).

// M4_SELECT_NEXT (round 3) = phase 0 (M4_NEXT) and the selector launch in ONE grid: blocks 0..3 compute the selectors of the next block's 64 rows and
// publish them (agent-scope stores, one tagged flag per row), the next n_tiles blocks are phase 0's tile workgroups — they build their
// tables straight from the old block rows (nobody writes those in this launch) and wait for the 64 flags before they touch the next
// block's rows — and the remaining blocks compute the selectors of all other rows (which phase 0 never touches) and the snapshot.
// One kernel boundary less on the critical path of every block: select 5 us -> hidden behind phase 0.
template <int PHASE>
__global__ __launch_bounds__(M4_NT) void k_sweep_m4r(u64 *__restrict__ rows, i64 R, i64 Wc, const BlockInfo *__restrict__ info,
                                                      const u64 *__restrict__ sel, const u64 *__restrict__ snap, int n_tiles, int n_chunks,
                                                      BlockInfo *__restrict__ info_next, SweepState *__restrict__ st, i64 *__restrict__ pivots,
                                                      Gf2Counters *__restrict__ counters, int *__restrict__ lead, FusedSelect fs) {
    extern __shared__ u64 tab[];                                    // [16 groups][16 entries][64 words]
    __shared__ u64 s_sel[WK];
    __shared__ int s_ok;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kk = info->kk;
    const i64 i0n = info->i0 + kk;                                  // first row of the next block
    // rows of the next block: [nb, ne)   (M4_ALL: none)
    const i64 nb = PHASE == M4_ALL ? 0 : (i0n < R ? i0n : R), ne = PHASE == M4_ALL ? 0 : (i0n + WK < R ? i0n + WK : R);
    int k = blockIdx.x;
    if (PHASE == M4_SELECT_NEXT) {
        if (k < SEL_PRI || k >= SEL_PRI + n_tiles) {
            // ---- selector role: one wavefront per row (k_select's body with this grid's row and workgroup numbering) ----
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
    if (PHASE == M4_PANEL_REST) {
        if (k == 0) {
            // ---- panel workgroup; the leading words were collected by phase 0 (reset for the next block).  One wavefront on a 4-word
            //      window — or, when the window would end the block early and the rows fit, the whole workgroup on the full rows ----
            int a = -1;
            u64 spec[WN] = {0, 0, 0, 0};
            const int w_spec = info->w_next;                         // the block that was just panelled guessed this block's window
            if (wave == 0 && i0n + lane < R) {
                a = lead[lane];
                load_spec_window(rows, Wc, i0n + lane, w_spec, spec);
            }
            if (wave == 0) {
                const bool full = fs.full_panel && Wc <= FULL_WC && i0n < R && full_row_panel_wanted(a);
                if (lane == 0) { s_ok = full ? 1 : 0; if (full) atomicAdd(&fs.counters->full_panels, 1u); }
                if (i0n + lane < R) lead[lane] = NOLEAD;
            }
            __syncthreads();
            if (s_ok) {
                if (wave != 0) a = 0;
                panel_full(rows, R, Wc, i0n, a, tab, s_sel, st, info_next, pivots, counters);
            } else if (wave == 0) panel_wave(rows, R, Wc, i0n, a, lane, st, info_next, pivots, counters, spec, w_spec, fs.lean_panel);
            return;
        }
        --k;
    }
    constexpr bool P0 = PHASE == M4_NEXT || PHASE == M4_SELECT_NEXT;
    if (kk == 0 && !P0) return;
    const int tile = k % n_tiles, chunk = k / n_tiles;
    // rows of this chunk: M4_NEXT / M4_SELECT_NEXT the next block's rows, M4_PANEL_REST / M4_ALL the virtual index space of all OTHER rows
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
            if (with_sel) sn[u] = kk != 0 ? (PHASE == M4_SELECT_NEXT ? s_sel[rn[u] - nb] : sel[rn[u]]) : 0ULL;
            xn[u] = rows[rn[u] * Wc + wl];
        }
    };
    i64 v0 = v_lo + M4_U * wave;
    // phases 1 / 2: the first rows and their selectors are on their way while the tables are built (round 4: the loads used to start behind
    // the table build and its barrier, 2-3 us of every 15 us launch with nothing in flight)
    if (PHASE != M4_SELECT_NEXT && v0 < v_hi) fetch(v0, true);
    // ---- tabulate the XOR combinations of the old block rows ----
    if (kk != 0) {
        for (int g = wave; g < 16; g += M4_NT / 64) {
            u64 sv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                sv[i] = (4 * g + i < kk) ? (PHASE == M4_SELECT_NEXT ? rows[(info->i0 + 4 * g + i) * Wc + wl] : snap[(i64)(4 * g + i) * Wc + wl]) : 0ULL;
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
    if (PHASE == M4_SELECT_NEXT) {
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
                if (lane == 0) { s_ok = ok ? 1 : 0; if (!ok) atomicOr(&fs.counters->timed_out, 1u); }
            }
        }
    }
    __syncthreads();
    if (PHASE == M4_SELECT_NEXT && kk != 0 && !s_ok) return;                      // flagged: the call fails loudly
    if (PHASE == M4_SELECT_NEXT) {
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

// ---- launches ------------------------------------------------------------------------------------------------------------
bool gf2_small_attr_ok() {
    return SG_DEVICE_ONCE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rref_small), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              SMALL_R * SMALL_WC * 8) == hipSuccess);
}

bool gf2_m4r_attr_ok() {
    return SG_DEVICE_ONCE(
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sweep_m4r<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M4_LDS) == hipSuccess);
}

int launch_rref_small(u64 *rows, i64 R, i64 Wc, i64 *pivots, unsigned long long *xor_count) {
    hipLaunchKernelGGL(k_rref_small, dim3(1), dim3(256), (size_t)R * Wc * 8, ctx().stream, rows, (int)R, (int)Wc, pivots, xor_count);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

void launch_fill_nolead(const Gf2Run &g) { hipLaunchKernelGGL(k_fill_nolead, dim3(1), dim3(WK), 0, ctx().stream, g.lead.as<int>()); }

// one launch of the Four-Russians sweep: `cur` is swept, `next` receives the panel of M4_PANEL_REST
template <int PHASE>
static void launch_m4r(const Gf2Run &g, unsigned grid, int n_chunks, BlockInfo *cur, BlockInfo *next, u32 epoch) {
    const FusedSelect fs{g.sel.as<u64>(), g.snap.as<u64>(), g.rowcnt.as<u32>(), g.ready.as<u64>(), epoch, g.counters.as<Gf2Counters>(),
                         g.full_panel, g.lean_panel};
    hipLaunchKernelGGL(k_sweep_m4r<PHASE>, dim3(grid), dim3(M4_NT), M4_LDS, ctx().stream, g.rows, g.R, g.Wc, cur, g.sel.as<u64>(), g.snap.as<u64>(),
                       g.m4_tiles, n_chunks, next, g.state.as<SweepState>(), g.piv.as<i64>(), g.counters.as<Gf2Counters>(), g.lead.as<int>(), fs);
}

static void launch_select(const Gf2Run &g, const BlockInfo *info) {
    hipLaunchKernelGGL(k_select, dim3((unsigned)((g.R + 3) / 4)), dim3(256), 0, ctx().stream, g.rows, g.R, g.Wc, info, g.sel.as<u64>(), g.snap.as<u64>(),
                       g.rowcnt.as<u32>());
}

int launch_lookahead_step(const Gf2Run &g, i64 it, bool fused) {
    BlockInfo *binfo = g.info.as<BlockInfo>();
    BlockInfo *cur = binfo + ((it + 1) & 1), *next = binfo + (it & 1);      // cur: block it-1 (to sweep), next: block it (to panel)
    const u32 epoch = (u32)(it + 1);
    if (fused) {
        // selectors of block it-1 and phase 0 in one grid (the very first iteration has no block to select for: kk == 0)
        launch_m4r<M4_SELECT_NEXT>(g, (unsigned)(SEL_PRI + g.m4_tiles + (g.R + 15) / 16), 1, cur, next, epoch);
    } else {
        if (it > 0) launch_select(g, cur);
        launch_m4r<M4_NEXT>(g, (unsigned)g.m4_tiles, 1, cur, next, epoch);
    }
    ProfScope prof(2);
    launch_m4r<M4_PANEL_REST>(g, (unsigned)(g.m4_tiles * g.m4_chunks + 1), g.m4_chunks, cur, next, epoch);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

int launch_plain_step(const Gf2Run &g, bool m4r) {
    hipStream_t st = ctx().stream;
    constexpr int SW_ROWS = 16;                                     // rows per workgroup of the flag sweep, held in VGPRs
    BlockInfo *binfo = g.info.as<BlockInfo>();
    hipLaunchKernelGGL(k_lead, dim3(WK / 4), dim3(256), 0, st, g.rows, g.R, g.Wc, g.state.as<SweepState>(), g.lead.as<int>());
    hipLaunchKernelGGL(k_wpanel, dim3(1), dim3(64), 0, st, g.rows, g.R, g.Wc, g.state.as<SweepState>(), g.lead.as<int>(), binfo, g.piv.as<i64>(),
                       g.counters.as<Gf2Counters>(), g.lean_panel);
    launch_select(g, binfo);
    ProfScope prof(2);
    if (m4r) launch_m4r<M4_ALL>(g, (unsigned)(g.m4_tiles * g.m4_chunks), g.m4_chunks, binfo, binfo, 0);
    else
        hipLaunchKernelGGL((k_sweep<SW_ROWS, 4>), dim3((unsigned)((g.Wc + 255) / 256), (unsigned)((g.R + SW_ROWS - 1) / SW_ROWS)), dim3(256), 0, st, g.rows,
                           g.R, g.Wc, binfo, g.sel.as<u64>(), g.snap.as<u64>());
    KERNEL_CHECK();
    return SYMGPU_OK;
}

int launch_row_xor_sum(const Gf2Run &g) {
    hipLaunchKernelGGL(k_sum_u32, dim3(256), dim3(256), 0, ctx().stream, g.rowcnt.as<u32>(), g.R, &g.counters.as<Gf2Counters>()->xors);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
