// noncon_sweep.hip — the noncontextual sweep (reference: symmer/operators/utils.py:592-616 perform_noncontextual_sweep, the loop under
// NoncontextualOp._single_sweep_noncontextual_operator, _dfs_noncontextual_op and _diag_first_noncontextual_op).
//
// A sweep walks the terms in a given order and keeps a term whenever the kept set stays noncontextual.  The kept set of a noncontextual
// operator is a set SYM of terms that commute with every kept term, and m cliques (m = 0 or m >= 2): kept terms outside SYM commute
// iff they are in the same clique.  With v = the candidate's commutation bits against the kept terms the verdict is
//   1. v all ones                                   keep, SYM
//   2. m == 0, v not all ones                       keep: the kept terms that anticommute with t become clique 0, t becomes clique 1
//   3. m >= 2, t anticommutes with a SYM term       reject
//   4. m >= 2, t commutes with no clique term       keep, new clique m
//   5. m >= 2 otherwise                             j = the clique of a clique term that commutes with t; keep in clique j iff v on the
//                                                   clique terms is exactly clique j's membership mask, else reject
// (in 5 every commuting clique term names the same j whenever the term is kept, so which one is looked up does not change the result).
//
// Layout.  The T x T commutation bits are computed once (symgpu_commutes_bits_dev) on the operator's rows permuted into `order`, so
// row p of the table is position p of the order and a roll is an offset.  k_nsw_sweep: one workgroup runs one sweep; a persistent grid
// strides over the sweeps.  The kept, SYM and clique-term masks of the running sweep are bit vectors in LDS (3 T / 8 bytes); the
// membership mask of every clique and the labels live in global scratch of the WORKGROUP (not of the sweep).  A step is word-wide:
// thread i owns words i, i + blockDim, ... of the row (at most NSW_WPT of them; the next row is loaded while this one is judged), ANDs
// them with the masks, and the workgroup meets in two LDS words (a flag word, the lowest commuting clique term); rule 5 adds one more
// meeting for the comparison against one membership mask.  Everything is integer work in a fixed order: two runs give identical bytes.
#include "common.h"
#include <algorithm>
#include <string.h>

namespace symgpu {

constexpr int NSW_THREADS = 256;
constexpr int NSW_WPT = 8;                                    // words a thread owns at most
constexpr i64 NSW_MAX_T = (i64)NSW_THREADS * NSW_WPT * 64;    // 131,072 terms: a 2 GiB table, 48 KiB of masks in LDS (SYMGPU_NONCON_SWEEP_MAX_T)
static_assert(NSW_MAX_T == SYMGPU_NONCON_SWEEP_MAX_T, "the header states the cap");
constexpr int NSW_WG_PER_CU = 4;                              // resident grid: workgroups a CU is given
constexpr size_t NSW_SCRATCH_BUDGET = (size_t)1 << 30;        // the membership masks of all resident workgroups stay below this
constexpr i64 NSW_SLAB_PAIRS = (i64)1 << 31;                  // pairs a commutation call computes
constexpr u32 NSW_F_ANTI = 1u, NSW_F_ANTI_SYM = 2u, NSW_F_DIFFERS = 4u, NSW_NONE = 0xffffffffu;
constexpr int32_t NSW_REJECTED = -2, NSW_SYM = -1;

struct NswArgs {
    const u64 *table;        // [T][Wt] commutation bits in order positions
    i64 T, Wt;
    const i64 *starts;       // [n_starts]
    i64 n_starts;
    u64 *member;             // [gridDim.x][max_cliques][Wt] membership masks
    i64 max_cliques;
    int32_t *lab_scratch;    // [gridDim.x][T], used when labels == null
    u64 *kept_bits;          // [n_starts][Wt]
    int32_t *labels;         // [n_starts][T] or null
    int32_t *n_cliques;      // [n_starts]: the cliques the sweep ended with, -1 if it ran out of membership masks
};

__global__ __launch_bounds__(NSW_THREADS) void k_nsw_sweep(const NswArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 nsw_lds[];
    __shared__ u32 s_flags[2], s_pos[2];
    const i64 T = a.T, Wt = a.Wt;
    u64 *kept = nsw_lds, *sym = nsw_lds + Wt, *clq = nsw_lds + 2 * Wt;
    const int t = threadIdx.x, nt = blockDim.x;
    u64 *member = a.member + (size_t)blockIdx.x * (size_t)a.max_cliques * (size_t)Wt;
    for (i64 s = blockIdx.x; s < a.n_starts; s += gridDim.x) {
        int32_t *lab = a.labels ? a.labels + s * T : a.lab_scratch + (i64)blockIdx.x * T;
        const i64 start = a.starts[s];
        for (i64 w = t; w < Wt; w += nt) kept[w] = sym[w] = clq[w] = 0;
        if (t == 0) { s_flags[0] = s_flags[1] = 0; s_pos[0] = s_pos[1] = NSW_NONE; }
        __syncthreads();
        // the first visited term is kept as SYM
        if (t == 0) {
            kept[start >> 6] = sym[start >> 6] = (u64)1 << (start & 63);
            lab[start] = NSW_SYM;
        }
        i64 m = 0;
        bool overflow = false;
        u64 v[NSW_WPT], nxt[NSW_WPT];
        {
            const i64 p1 = start + 1 < T ? start + 1 : start + 1 - T;
#pragma unroll
            for (int k = 0; k < NSW_WPT; ++k) { const i64 w = t + (i64)k * nt; nxt[k] = w < Wt ? a.table[p1 * Wt + w] : 0; }
        }
        __syncthreads();
        for (i64 i = 1; i < T; ++i) {
            const int b = (int)(i & 1);
            i64 p = start + i;
            if (p >= T) p -= T;
#pragma unroll
            for (int k = 0; k < NSW_WPT; ++k) v[k] = nxt[k];
            if (i + 1 < T) {
                i64 pn = p + 1;
                if (pn >= T) pn -= T;
#pragma unroll
                for (int k = 0; k < NSW_WPT; ++k) { const i64 w = t + (i64)k * nt; nxt[k] = w < Wt ? a.table[pn * Wt + w] : 0; }
            }
            // meeting 1: does t anticommute with a kept term, with a SYM term; the lowest clique term it commutes with
            u32 flags = 0, pos = NSW_NONE;
#pragma unroll
            for (int k = 0; k < NSW_WPT; ++k) {
                const i64 w = t + (i64)k * nt;
                if (w >= Wt) break;
                if (~v[k] & kept[w]) flags |= NSW_F_ANTI;
                if (~v[k] & sym[w]) flags |= NSW_F_ANTI_SYM;
                const u64 c = v[k] & clq[w];
                if (c && pos == NSW_NONE) pos = (u32)(w * 64 + __ffsll((unsigned long long)c) - 1);
            }
            if (flags) atomicOr(&s_flags[b], flags);
            if (pos != NSW_NONE) atomicMin(&s_pos[b], pos);
            __syncthreads();
            flags = s_flags[b];
            pos = s_pos[b];
            if (t == 0) { s_flags[b ^ 1] = 0; s_pos[b ^ 1] = NSW_NONE; }      // the words of the next step (nobody reads them before the step's last barrier)
            const i64 pw = p >> 6;
            const u64 pbit = (u64)1 << (p & 63);
            const bool owner = (pw % nt) == t;                                // the thread that owns word pw
            int32_t label = NSW_REJECTED;
            if (!(flags & NSW_F_ANTI)) {
                label = NSW_SYM;                                              // rule 1
                if (owner) sym[pw] |= pbit;
            } else if (m == 0) {
                if (a.max_cliques < 2) overflow = true;                       // (cannot happen: T >= 2 gives max_cliques >= 2)
                else {
                    // rule 2: the demotion, once a sweep
#pragma unroll
                    for (int k = 0; k < NSW_WPT; ++k) {
                        const i64 w = t + (i64)k * nt;
                        if (w >= Wt) break;
                        const u64 anti = ~v[k] & kept[w];
                        sym[w] = kept[w] & ~anti;
                        clq[w] = anti;
                        member[w] = anti;
                        member[Wt + w] = 0;
                        for (u64 r = anti; r; r &= r - 1) lab[w * 64 + __ffsll((unsigned long long)r) - 1] = 0;
                    }
                    label = 1;
                    m = 2;
                }
            } else if (flags & NSW_F_ANTI_SYM) {
                // rule 3
            } else if (pos == NSW_NONE) {
                if (m >= a.max_cliques) overflow = true;                      // (more pairwise anticommuting terms than 2 n + 1: cannot happen)
                else {
                    for (i64 w = t; w < Wt; w += nt) member[m * Wt + w] = 0;  // rule 4
                    label = (int32_t)m;
                    m += 1;
                }
            } else {
                // rule 5: meeting 2
                const i64 j = lab[pos];
                const u64 *mj = member + j * Wt;
                bool differs = false;
#pragma unroll
                for (int k = 0; k < NSW_WPT; ++k) {
                    const i64 w = t + (i64)k * nt;
                    if (w >= Wt) break;
                    differs |= (v[k] & clq[w]) != mj[w];
                }
                if (differs) atomicOr(&s_flags[b], NSW_F_DIFFERS);
                __syncthreads();
                if (!(s_flags[b] & NSW_F_DIFFERS)) label = (int32_t)j;
            }
            if (label >= 0) __syncthreads();                                  // a membership mask zeroed above (rules 2, 4) before its bit is set
            if (owner) {
                if (label != NSW_REJECTED) kept[pw] |= pbit;
                if (label >= 0) { clq[pw] |= pbit; member[(i64)label * Wt + pw] |= pbit; }
                lab[p] = label;
            }
            __syncthreads();
        }
        for (i64 w = t; w < Wt; w += nt) a.kept_bits[s * Wt + w] = kept[w];
        if (t == 0) a.n_cliques[s] = overflow ? -1 : (int32_t)m;
        __syncthreads();                                                      // the masks and the scratch go to the next sweep
    }
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_noncon_sweep_dev(symgpu_op_t op, const int64_t *order, int64_t n_starts, const int64_t *starts,
                            uint64_t *kept_bits, int32_t *labels, int64_t *info) {
    SG_ENTER(op);
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    SG_REQUIRE(op, "noncon_sweep_dev: null handle");
    const i64 T = op->T;
    SG_REQUIRE(T <= NSW_MAX_T, "noncon_sweep_dev: more than 131,072 terms, the commutation table would pass 2 GiB");
    SG_REQUIRE(n_starts >= 0 && n_starts < ((i64)1 << 31), "noncon_sweep_dev: the number of sweeps is negative or too large");
    SG_REQUIRE((starts && kept_bits) || n_starts == 0 || T == 0, "noncon_sweep_dev: null starts or null output");
    for (i64 s = 0; s < n_starts && T > 0; ++s) SG_REQUIRE(0 <= starts[s] && starts[s] < T, "noncon_sweep_dev: a start outside [0, T)");
    if (order) {
        std::vector<uint8_t> seen((size_t)T, 0);
        for (i64 p = 0; p < T; ++p) {
            const i64 k = order[p];
            SG_REQUIRE(0 <= k && k < T, "noncon_sweep_dev: order is not a permutation, an entry is out of range");
            SG_REQUIRE(!seen[(size_t)k], "noncon_sweep_dev: order is not a permutation, an entry is repeated");
            seen[(size_t)k] = 1;
        }
    }
    if (T == 0 || n_starts == 0) return SYMGPU_OK;
    const i64 Wt = (T + 63) / 64;
    if (T == 1) {
        for (i64 s = 0; s < n_starts; ++s) { kept_bits[s] = 1; if (labels) labels[s] = NSW_SYM; }
        return SYMGPU_OK;
    }
    hipStream_t st = ctx().stream;

    // the table, in order positions
    OwnedOp permuted;
    symgpu_op_t rows = op;
    if (order) {
        SG_TRY(symgpu_op_gather(op, order, T, permuted.slot()));
        rows = permuted.op;
    }
    const size_t table_bytes = (size_t)T * (size_t)Wt * 8;
    Scratch table;
    SG_TRY(table.alloc(table_bytes));
    const i64 slab = std::max<i64>(1, NSW_SLAB_PAIRS / T);
    for (i64 r = 0; r < T; r += slab)
        SG_TRY(symgpu_commutes_bits_dev(rows, r, std::min(T, r + slab), rows, table.as<u64>() + r * Wt));

    // the grid: what is resident, what the membership masks of its workgroups may take
    const i64 max_cliques = std::min<i64>(T, (i64)128 * op->Wq + 1);           // pairwise anticommuting terms on n qubits: 2 n + 1 at most
    const size_t member_wg = (size_t)max_cliques * (size_t)Wt * 8;
    i64 n_wg = std::min<i64>(n_starts, (i64)NSW_WG_PER_CU * ctx().num_cu);
    n_wg = std::max<i64>(1, std::min<i64>(n_wg, (i64)(NSW_SCRATCH_BUDGET / member_wg)));
    const int threads = (int)std::min<i64>(NSW_THREADS, 64 * ((Wt + 63) / 64));

    Scratch d_starts, d_member, d_lab, d_kept, d_labels, d_cliques;
    SG_TRY(d_starts.alloc((size_t)n_starts * 8));
    HIP_TRY(hipMemcpyAsync(d_starts.p, starts, (size_t)n_starts * 8, hipMemcpyHostToDevice, st));
    count_h2d((size_t)n_starts * 8);
    SG_TRY(d_member.alloc((size_t)n_wg * member_wg));
    if (labels) SG_TRY(d_labels.alloc((size_t)n_starts * (size_t)T * 4));
    else SG_TRY(d_lab.alloc((size_t)n_wg * (size_t)T * 4));
    SG_TRY(d_kept.alloc((size_t)n_starts * (size_t)Wt * 8));
    SG_TRY(d_cliques.alloc((size_t)n_starts * 4));

    NswArgs a;
    a.table = table.as<u64>(); a.T = T; a.Wt = Wt;
    a.starts = d_starts.as<i64>(); a.n_starts = n_starts;
    a.member = d_member.as<u64>(); a.max_cliques = max_cliques;
    a.lab_scratch = labels ? nullptr : d_lab.as<int32_t>();
    a.kept_bits = d_kept.as<u64>();
    a.labels = labels ? d_labels.as<int32_t>() : nullptr;
    a.n_cliques = d_cliques.as<int32_t>();
    hipLaunchKernelGGL(k_nsw_sweep, dim3((unsigned)n_wg), dim3(threads), (size_t)3 * Wt * 8, st, a);
    KERNEL_CHECK();

    std::vector<int32_t> cliques((size_t)n_starts);
    SG_TRY(download_any(d_kept.p, kept_bits, (size_t)n_starts * (size_t)Wt * 8));
    SG_TRY(download_any(d_cliques.p, cliques.data(), (size_t)n_starts * 4));
    count_d2h((size_t)n_starts * ((size_t)Wt * 8 + 4));
    if (labels) {
        SG_TRY(download_any(d_labels.p, labels, (size_t)n_starts * (size_t)T * 4));
        count_d2h((size_t)n_starts * (size_t)T * 4);
    }
    i64 most = 0;
    for (int32_t c : cliques) {
        if (c < 0) { set_error("noncon_sweep_dev: a sweep met more than %lld cliques", (long long)max_cliques); return SYMGPU_E_INVALID; }
        most = std::max<i64>(most, c);
    }
    if (info) {
        info[0] = (i64)table_bytes;
        info[1] = n_wg;
        info[2] = (n_starts + n_wg - 1) / n_wg;
        info[3] = most;
    }
    return SYMGPU_OK;
}

}  // extern "C"
