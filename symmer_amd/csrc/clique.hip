// clique.hip — measurement grouping (reference: symmer/operators/base.py:985-1009 qubitwise_commutes_termwise, :1266-1364 clique_cover):
// the three termwise relations on packed rows, the table of one of them (QWC) as bytes, per-term relation degrees, and the first-fit
// colouring that both `sorted_insertion` and networkx's `largest_first` reduce to.
//
// Relations of two rows a = (xa | za), b = (xb | zb), X words then Z words, Wq words each:
//   C    related iff the parity of popcount(xa & zb ^ za & xb) over the row is even
//   AC   related iff that parity is odd
//   QWC  related iff no word has (xa | za) & (xb | zb) & ((xa ^ xb) | (za ^ zb)) != 0
// Two terms CONFLICT when they are not related; a term never meets itself (the same index) in the degrees or in the colouring.
//
// First fit: walk the terms in `order`; each takes the lowest colour none of whose members it conflicts with.  The walk is blocked, CQ_BLOCK
// terms of the order at a time, two launches a block and no host read-back between them:
//   wide     every thread holds one row of what is already coloured and meets it with CQ_WIDE_SLICE terms of the block; a conflict ORs bit `colour`
//            into the block term's forbidden-colour bitmap (global_atomic_or on 32-bit words, skipped where a plain load already shows the
//            bit).  Form PAIRS (C, AC): the rows are the s0 terms coloured so far.  Form UNIONS (QWC): the rows are the K merged Pauli
//            strings of the cliques so far — a term qubit-wise commutes with every member of a clique iff it does with their union —
//            so the work is T K instead of T^2 / 2.
//   resolve  one workgroup, thread u = block term u: the conflicts among the block's terms as 256 x 256 bits in LDS, then in order: term s
//            publishes its first free colour, every later term that conflicts with s sets that bit and moves on if it had the same colour
//            in mind.  Then the colours, the colour count and (UNIONS) the clique unions are written and the block's bitmap words are
//            cleared for the next block.
// Device memory of a colouring of T terms: the rows in colouring order 16 Wq T bytes, (UNIONS) the clique unions 16 Wq T, the order 8 T,
// the colours 4 T + 4, and the block's bitmaps CQ_BLOCK (T / 32 + 2) words = 32 T + 2 KiB: a bitmap is as wide as colours can become (T),
// but only one block of them exists.  No T x T table.  The degrees take 8 T bytes beside the operator.
#include "common.h"
#include <string.h>

namespace symgpu {

constexpr int CQ_BLOCK = 256;            // terms of the order resolved by one launch = threads of the resolve workgroup
constexpr int CQ_WIDE_SLICE = 32;        // terms of the block that one thread of the wide phase meets

// WQ > 0: row length known at compile time (a row held by a thread stays in registers); WQ = 0: Wq words, read where they are
template <int WQ>
__device__ __forceinline__ bool rows_related(const u64 *__restrict__ a, const u64 *__restrict__ b, int Wq_rt, int rel) {
    const int Wq = WQ ? WQ : Wq_rt;
    u64 p = 0, q = 0;
#pragma unroll
    for (int w = 0; w < Wq; ++w) {
        const u64 xa = a[w], za = a[Wq + w], xb = b[w], zb = b[Wq + w];
        p ^= (xa & zb) ^ (za & xb);
        q |= (xa | za) & (xb | zb) & ((xa ^ xb) | (za ^ zb));
    }
    if (rel == SYMGPU_REL_QWC) return q == 0;
    return (__popcll(p) & 1) == (rel == SYMGPU_REL_AC ? 1 : 0);
}

// out[i * M + j] = A[i] related to B[j]; 64 columns x 4 rows a workgroup, the rows of a launch strided over gridDim.y
template <int WQ>
__global__ __launch_bounds__(256) void k_rel_table(const u64 *__restrict__ A, i64 N, const u64 *__restrict__ B, i64 M, int Wq_rt, int rel,
                                                   uint8_t *__restrict__ out) {
    const int Wq = WQ ? WQ : Wq_rt;
    const i64 j = (i64)blockIdx.x * 64 + (threadIdx.x & 63);
    if (j >= M) return;
    for (i64 i = (i64)blockIdx.y * 4 + (threadIdx.x >> 6); i < N; i += (i64)gridDim.y * 4)
        out[i * M + j] = rows_related<WQ>(B + j * 2 * Wq, A + i * 2 * Wq, Wq, rel) ? 1 : 0;
}

// deg[i] += the terms j != i of the slice blockIdx.y that term i is related to
template <int WQ>
__global__ __launch_bounds__(256) void k_rel_degrees(const u64 *__restrict__ rows, i64 T, int Wq_rt, int rel, i64 slice,
                                                     unsigned long long *__restrict__ deg) {
    const int Wq = WQ ? WQ : Wq_rt;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const i64 j0 = (i64)blockIdx.y * slice, j1 = j0 + slice < T ? j0 + slice : T;
    const u64 *mine = rows + i * 2 * Wq;
    unsigned long long cnt = 0;
    for (i64 j = j0; j < j1; ++j)
        if (j != i && rows_related<WQ>(mine, rows + j * 2 * Wq, Wq, rel)) ++cnt;
    if (cnt) atomicAdd(deg + i, cnt);
}

// out[s] = rows[order[s]]
__global__ __launch_bounds__(256) void k_cq_gather(const u64 *__restrict__ rows, const i64 *__restrict__ order, i64 T, int W, u64 *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= T * W) return;
    out[k] = rows[order[k / W] * W + k % W];
}

// Wide phase.  ref: m rows (m = *m_dev if given, else m_host) with colours ref_col[j] (null: colour j); blk: the nb rows of the block;
// bitmap[t * Wb + c / 32] bit c % 32 = colour c is forbidden for block term t.  Colours are below T and Wb = T / 32 + 2.
template <int WQ>
__global__ __launch_bounds__(256) void k_cq_wide(const u64 *__restrict__ ref, const int *__restrict__ ref_col, const int *__restrict__ m_dev, i64 m_host,
                                                 const u64 *__restrict__ blk, int nb, int Wq_rt, int rel, u32 *bitmap, i64 Wb) {
    const int Wq = WQ ? WQ : Wq_rt;
    const i64 m = m_dev ? (i64)*m_dev : m_host;
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int c = ref_col ? ref_col[j] : (int)j;
    const u32 bit = 1u << (c & 31);
    u32 *col_word = bitmap + (c >> 5);
    const u64 *mine = ref + j * 2 * Wq;
    // blockIdx.y: CQ_WIDE_SLICE terms of the block each, so that a thread's chain of bitmap look-ups stays short
    const int t0 = (int)blockIdx.y * CQ_WIDE_SLICE, t1 = t0 + CQ_WIDE_SLICE < nb ? t0 + CQ_WIDE_SLICE : nb;
    for (int t = t0; t < t1; ++t) {
        if (rows_related<WQ>(mine, blk + (i64)t * 2 * Wq, Wq, rel)) continue;
        u32 *p = col_word + (i64)t * Wb;
        if (!(__atomic_load_n(p, __ATOMIC_RELAXED) & bit)) atomicOr(p, bit);      // bits are only ever set here: a stale read costs an atomic, no more
    }
}

// Resolve phase: one workgroup of CQ_BLOCK threads.  colour_out: the colours of the block's terms; K_dev: colours in use, read and updated;
// unions (or null): [colour][2 Wq] OR of the members' rows.
__global__ __launch_bounds__(CQ_BLOCK) void k_cq_resolve(const u64 *__restrict__ blk, int nb, int Wq, int rel, u32 *bitmap, i64 Wb,
                                                         int *__restrict__ colour_out, int *K_dev, u64 *unions) {
    __shared__ u32 s_conf[CQ_BLOCK / 32][CQ_BLOCK];      // [s / 32][u] bit s % 32: block terms s < u that u conflicts with
    __shared__ int s_col[CQ_BLOCK];
    __shared__ int s_K;
    const int u = threadIdx.x;
    const bool live = u < nb;
    const u64 *mine = blk + (i64)u * 2 * Wq;
    if (u == 0) s_K = *K_dev;
    for (int w = 0; w < CQ_BLOCK / 32; ++w) {
        u32 mask = 0;
        const int s_end = (w + 1) * 32 < nb ? (w + 1) * 32 : nb;
        for (int s = w * 32; s < s_end; ++s)
            if (live && s < u && !rows_related<0>(mine, blk + (i64)s * 2 * Wq, Wq, rel)) mask |= 1u << (s & 31);
        s_conf[w][u] = mask;
    }
    // The candidate colour c = the first zero bit of the term's bitmap row.  It only moves up, so the word that holds it lives in a register
    // (`cur` = row[cw], cw = c / 32, the term's own updates included) and only bits of later words go to memory, as atomics nobody waits
    // for; a word is read (past the L1, where those atomics do not show) when the candidate reaches it.  The row holds fewer set bits than
    // there are terms before its owner, so a zero exists below T, inside the row; the scan stops at the row's end all the same.
    u32 *row = bitmap + (i64)u * Wb;
    const auto row_word = [&](i64 w) { return __hip_atomic_load(row + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    i64 cw = 0;
    u32 cur = live ? row_word(0) : 0;
    const auto candidate = [&](u32 free_bits) {
        while (!free_bits && cw + 1 < Wb) { cur = row_word(++cw); free_bits = ~cur; }
        return free_bits ? (int)(cw * 32 + __ffs((int)free_bits) - 1) : (int)(Wb * 32 - 1);
    };
    int c = live ? candidate(~cur) : 0;
    for (int s = 0; s < nb; ++s) {
        if (u == s) s_col[s] = c;
        __syncthreads();
        if (live && u > s && ((s_conf[s >> 5][u] >> (s & 31)) & 1)) {
            const int cs = s_col[s];
            if (cs >= c) {                                       // a colour below the candidate cannot matter any more
                if ((cs >> 5) == cw) cur |= 1u << (cs & 31);
                else atomicOr(row + (cs >> 5), 1u << (cs & 31));
                if (cs == c) c = candidate(~cur & (~0u << (c & 31)));
            }
        }
    }
    if (live) {
        colour_out[u] = c;
        atomicMax(&s_K, c + 1);
        if (unions)
            for (int w = 0; w < 2 * Wq; ++w)
                if (mine[w]) atomicOr(reinterpret_cast<unsigned long long *>(unions + (i64)c * 2 * Wq + w), (unsigned long long)mine[w]);
    }
    __threadfence();                                     // the atomics on the rows have landed before anybody clears the rows
    __syncthreads();
    const int K = s_K;
    if (u == 0) *K_dev = K;
    const i64 nw = (K >> 5) + 1 < Wb ? (K >> 5) + 1 : Wb;   // every bit set in this block's rows is below K
    for (i64 k = u; k < nb * nw; k += CQ_BLOCK) bitmap[(k / nw) * Wb + k % nw] = 0;
}

#define CQ_BY_WQ(Wq, call_1, call_2, call_n) \
    do { if ((Wq) == 1) { call_1; } else if ((Wq) == 2) { call_2; } else { call_n; } } while (0)

static int relation_table_dev(const u64 *A, i64 N, const u64 *B, i64 M, int Wq, int rel, uint8_t *out) {
    if (N == 0 || M == 0) return SYMGPU_OK;
    hipStream_t st = ctx().stream;
    const i64 gy = (N + 3) / 4;
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)(gy < 16384 ? gy : 16384));
    CQ_BY_WQ(Wq, hipLaunchKernelGGL(k_rel_table<1>, grid, dim3(256), 0, st, A, N, B, M, Wq, rel, out),
             hipLaunchKernelGGL(k_rel_table<2>, grid, dim3(256), 0, st, A, N, B, M, Wq, rel, out),
             hipLaunchKernelGGL(k_rel_table<0>, grid, dim3(256), 0, st, A, N, B, M, Wq, rel, out));
    KERNEL_CHECK();
    return SYMGPU_OK;
}

static int launch_wide(const u64 *ref, const int *ref_col, const int *m_dev, i64 m_host, const u64 *blk, int nb, int Wq, int rel, u32 *bitmap, i64 Wb) {
    hipStream_t st = ctx().stream;
    const dim3 grid((unsigned)((m_host + 255) / 256), (unsigned)((nb + CQ_WIDE_SLICE - 1) / CQ_WIDE_SLICE));
    CQ_BY_WQ(Wq, hipLaunchKernelGGL(k_cq_wide<1>, grid, dim3(256), 0, st, ref, ref_col, m_dev, m_host, blk, nb, Wq, rel, bitmap, Wb),
             hipLaunchKernelGGL(k_cq_wide<2>, grid, dim3(256), 0, st, ref, ref_col, m_dev, m_host, blk, nb, Wq, rel, bitmap, Wb),
             hipLaunchKernelGGL(k_cq_wide<0>, grid, dim3(256), 0, st, ref, ref_col, m_dev, m_host, blk, nb, Wq, rel, bitmap, Wb));
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// the walk over the order: rows in colouring order in, colours by position and the colour count (colour[T]) out, all on the device
static int colour_blocks(const u64 *prow, i64 T, int Wq, int rel, bool by_unions, u64 *unions, u32 *bitmap, i64 Wb, int *colour, i64 *n_blocks) {
    hipStream_t st = ctx().stream;
    int *K_dev = colour + T;
    for (i64 s0 = 0; s0 < T; s0 += CQ_BLOCK, ++*n_blocks) {
        const int nb = (int)(T - s0 < CQ_BLOCK ? T - s0 : CQ_BLOCK);
        const u64 *blk = prow + s0 * 2 * Wq;
        if (s0 > 0) {
            // at most s0 colours exist before position s0: the launch covers that many union rows, the threads past *K_dev leave at once
            if (by_unions) SG_TRY(launch_wide(unions, nullptr, K_dev, s0, blk, nb, Wq, rel, bitmap, Wb));
            else SG_TRY(launch_wide(prow, colour, nullptr, s0, blk, nb, Wq, rel, bitmap, Wb));
        }
        hipLaunchKernelGGL(k_cq_resolve, dim3(1), dim3(CQ_BLOCK), 0, st, blk, nb, Wq, rel, bitmap, Wb, colour + s0, K_dev, by_unions ? unions : nullptr);
        KERNEL_CHECK();
    }
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_qwc_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint8_t *out_dev) {
    SG_ENTER(A, B);
    SG_REQUIRE(A && B && A->Wq == B->Wq, "qwc_dev: operands must share Wq");
    SG_REQUIRE(0 <= a_begin && a_begin <= a_end && a_end <= A->T, "qwc_dev: bad row range");
    SG_REQUIRE(out_dev || a_end == a_begin || B->T == 0, "qwc_dev: null output");
    return relation_table_dev(A->rows + a_begin * 2 * A->Wq, a_end - a_begin, B->rows, B->T, A->Wq, SYMGPU_REL_QWC, out_dev);
}

int symgpu_relation_degrees_dev(symgpu_op_t op, int relation, int64_t *deg_host) {
    SG_ENTER(op);
    SG_REQUIRE(op, "relation_degrees_dev: null handle");
    SG_REQUIRE(relation == SYMGPU_REL_C || relation == SYMGPU_REL_AC || relation == SYMGPU_REL_QWC, "relation_degrees_dev: relation out of range");
    const i64 T = op->T;
    SG_REQUIRE(deg_host || T == 0, "relation_degrees_dev: null output");
    if (T == 0) return SYMGPU_OK;
    const int Wq = op->Wq;
    hipStream_t st = ctx().stream;
    Scratch deg;
    SG_TRY(deg.alloc((size_t)T * 8));
    HIP_TRY(hipMemsetAsync(deg.p, 0, (size_t)T * 8, st));
    // enough workgroups to fill the device: the other axis of the pair space is cut into slices where the terms alone give too few
    const i64 gx = (T + 255) / 256, want = (i64)4 * ctx().num_cu;
    i64 gy = gx >= want ? 1 : (want + gx - 1) / gx;
    if (gy > (T + 63) / 64) gy = (T + 63) / 64;
    const i64 slice = (T + gy - 1) / gy;
    gy = (T + slice - 1) / slice;
    SG_REQUIRE(gx < ((i64)1 << 31), "relation_degrees_dev: too many terms");
    const dim3 grid((unsigned)gx, (unsigned)gy);
    unsigned long long *d = deg.as<unsigned long long>();
    CQ_BY_WQ(Wq, hipLaunchKernelGGL(k_rel_degrees<1>, grid, dim3(256), 0, st, op->rows, T, Wq, relation, slice, d),
             hipLaunchKernelGGL(k_rel_degrees<2>, grid, dim3(256), 0, st, op->rows, T, Wq, relation, slice, d),
             hipLaunchKernelGGL(k_rel_degrees<0>, grid, dim3(256), 0, st, op->rows, T, Wq, relation, slice, d));
    KERNEL_CHECK();
    SG_TRY(download_any(deg.p, deg_host, (size_t)T * 8));
    count_d2h((size_t)T * 8);
    return SYMGPU_OK;
}

int symgpu_clique_colour_dev(symgpu_op_t op, int relation, const int64_t *order_host, int32_t *colour_host, int64_t *n_colours, int64_t *info) {
    SG_ENTER(op);
    if (n_colours) *n_colours = 0;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    SG_REQUIRE(op && n_colours, "clique_colour_dev: null handle or null colour count");
    SG_REQUIRE(relation == SYMGPU_REL_C || relation == SYMGPU_REL_AC || relation == SYMGPU_REL_QWC, "clique_colour_dev: relation out of range");
    const i64 T = op->T;
    SG_REQUIRE(T < ((i64)1 << 31) - CQ_BLOCK, "clique_colour_dev: too many terms");
    SG_REQUIRE((order_host && colour_host) || T == 0, "clique_colour_dev: null order or colour array");
    {
        std::vector<uint8_t> seen((size_t)T, 0);
        for (i64 s = 0; s < T; ++s) {
            const i64 t = order_host[s];
            SG_REQUIRE(0 <= t && t < T, "clique_colour_dev: order is not a permutation, an entry is out of range");
            SG_REQUIRE(!seen[(size_t)t], "clique_colour_dev: order is not a permutation, an entry is repeated");
            seen[(size_t)t] = 1;
        }
    }
    if (T == 0) return SYMGPU_OK;
    const int Wq = op->Wq, W = 2 * Wq;
    const bool by_unions = relation == SYMGPU_REL_QWC;
    const i64 Wb = T / 32 + 2;
    hipStream_t st = ctx().stream;

    Scratch order, prow, unions, bitmap, colour;                       // colour: [T] by position, then the colour count
    SG_TRY(order.alloc((size_t)T * 8));
    SG_TRY(prow.alloc((size_t)T * W * 8));
    if (by_unions) SG_TRY(unions.alloc((size_t)T * W * 8));
    SG_TRY(bitmap.alloc((size_t)CQ_BLOCK * Wb * 4));
    SG_TRY(colour.alloc((size_t)(T + 1) * 4));
    HIP_TRY(hipMemcpyAsync(order.p, order_host, (size_t)T * 8, hipMemcpyHostToDevice, st));
    count_h2d((size_t)T * 8);
    hipLaunchKernelGGL(k_cq_gather, dim3((unsigned)((T * W + 255) / 256)), dim3(256), 0, st, op->rows, order.as<i64>(), T, W, prow.as<u64>());
    KERNEL_CHECK();
    if (by_unions) HIP_TRY(hipMemsetAsync(unions.p, 0, (size_t)T * W * 8, st));
    HIP_TRY(hipMemsetAsync(bitmap.p, 0, (size_t)CQ_BLOCK * Wb * 4, st));
    HIP_TRY(hipMemsetAsync(colour.p, 0, (size_t)(T + 1) * 4, st));

    i64 n_blocks = 0;
    SG_TRY(colour_blocks(prow.as<u64>(), T, Wq, relation, by_unions, unions.as<u64>(), bitmap.as<u32>(), Wb, colour.as<int>(), &n_blocks));

    std::vector<int32_t> by_pos((size_t)T + 1);                        // the one read-back
    SG_TRY(download_any(colour.p, by_pos.data(), (size_t)(T + 1) * 4));
    count_d2h((size_t)(T + 1) * 4);
    for (i64 s = 0; s < T; ++s) colour_host[order_host[s]] = by_pos[(size_t)s];
    *n_colours = by_pos[(size_t)T];
    if (info) {
        info[0] = by_unions ? SYMGPU_CLIQUE_UNIONS : SYMGPU_CLIQUE_PAIRS;
        info[1] = n_blocks;
        info[2] = CQ_BLOCK;
        info[3] = Wb;
    }
    return SYMGPU_OK;
}

}  // extern "C"
