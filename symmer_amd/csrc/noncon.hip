// noncon.hip — the noncontextual seam (reference: symmer/operators/noncontextual_op.py:502-531 noncontextual_reconstruction, :533-554 get_energy,
// :686-704 energy_via_brute_force): the sign of every term's generator product, and the brute-force search over all 2^f eigenvalue
// assignments of the free symmetry generators.
//
// Objective, per assignment m (bit b set <=> free generator f-1-b is -1):
//   E(m) = sum_{k in S0} c_k s_k(m) - sqrt( sum_i ( sum_{k in C_i} c_k s_k(m) )^2 ),   s_k(m) = (-1)^popcount(mask_k & m)
// Every inner sum is the Walsh-Hadamard transform of the vector v[x] = sum_{k: mask_k = x} c_k, read at m.  The f bits are split into
// l = min(f, L) low bits and h = f - l high bits: for a fixed high part m_hi the terms fold onto their low masks with the sign
// (-1)^popcount(hi(mask_k) & m_hi), and an l-stage transform of that 2^l vector gives the sums of all 2^l assignments that share m_hi.
// Cost (Q + 1) l 2^(l-1) butterflies + T signed adds per 2^l assignments, nothing but the T entries read from memory.
//
// k_nc_search: workgroups stride over the 2^h high parts.  LDS holds three double[2^L] vectors: w (work), acc (sum of squares over the cliques)
// and part (partial sums of the fold).  Per high part, for every non-empty clique and then for S0:
//   fold       the group's entries are sorted by low mask (host, stable in term order) and cut into ITEMS of at most `chunk` entries that
//              never cross a low mask; a thread adds one item's signed coefficients in order.  A low mask that is one item goes
//              straight to w[low]; one that was cut leaves its item sums in part[], and one thread per such mask then adds those in order.
//              Every slot of w is therefore written by one thread in a fixed order: no floating-point atomics, bit-identical reruns;
//              `chunk` only bounds the longest serial chain (all masks in the high bits put a whole group on slot 0).
//   transform  in place, three stages a pass in registers (eight values a thread), a barrier a pass
//   use        clique: acc[j] += w[j]^2;  S0 (last): E[j] = w[j] - sqrt(acc[j])
// and every thread keeps the best (E, m) it saw: lower E, and among equal E the LARGER m — the reference's `min` over
// itertools.product([-1, 1]) keeps the first minimum, and -1 (bit set) sorts first.  One winner a workgroup, reduced by k_nc_reduce.
#include "common.h"
#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace symgpu {

constexpr int NC_L = 11;                 // low bits held in LDS: 3 * 8 * 2^11 = 48 KiB a workgroup, three workgroups a CU (measured against 10 and 12: DESIGN.md §3.13)
constexpr bool NC_SWIZZLE = true;        // w is stored bank-swizzled (nc_slot)
constexpr int NC_THREADS = 256;
constexpr int NC_MAX_FREE = 40;
constexpr double NC_MAX_MAGNITUDE = 1e154;  // sum|c| a call accepts: its square is still a double
constexpr int NC_CHUNK_MIN = 16;         // entries an item holds at most, doubled until a group's item sums fit part[]
constexpr u32 NC_TO_PART = 0x80000000u;  // item target: bit 31 set = index into part[], else the slot of w

struct NcItem { u32 begin, count, target, pad; };             // entries [begin, begin + count) -> w[target] or part[target & ~NC_TO_PART]
struct NcJoin { u32 begin, count, slot, pad; };               // part[begin, begin + count) -> w[slot]
struct NcGroup { u32 item_begin, item_end, join_begin, join_end; };

struct NcArgs {
    const double *coeff;     // [T] entries in (group, low mask, term) order
    const u32 *high;         // [T] mask >> l
    const NcItem *items;
    const NcJoin *joins;
    const NcGroup *groups;   // [n_groups], S0 last (always present, may be empty)
    int n_groups, l;
    i64 n_high;              // 2^h
    double *energies;        // [2^f] or null
    double *wg_energy;       // [gridDim.x]
    u64 *wg_mask;
};

__device__ __forceinline__ bool nc_better(double e, u64 m, double be, u64 bm) { return e < be || (e == be && m > bm); }

// the workgroup's best of every thread's (e, m), valid in thread 0; se / sm: NC_THREADS words of LDS each
__device__ __forceinline__ void nc_block_best(double &e, u64 &m, double *se, u64 *sm) {
    const int t = threadIdx.x;
    se[t] = e; sm[t] = m;
    __syncthreads();
    for (int s = NC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s && nc_better(se[t + s], sm[t + s], se[t], sm[t])) { se[t] = se[t + s]; sm[t] = sm[t + s]; }
        __syncthreads();
    }
    e = se[0]; m = sm[0];
}

// Where value i of w lives.  SWZ: bits 0 .. 4 (the 32 eight-byte banks) are XORed with bits 5 .. 9, so that the threads of a pass whose
// values lie 8 or 64 doubles apart (the passes at s = 0 and s = 3) spread over the banks instead of meeting on a quarter of them.
template <bool SWZ>
__device__ __forceinline__ u32 nc_slot(u32 i) { return SWZ ? i ^ ((i >> 5) & 31u) : i; }

// stages s .. s + R - 1 of the transform of w[0 .. 2^l): unit u owns the 2^R values whose index has the bits of u around R free bits at s
template <int R, bool SWZ>
__device__ __forceinline__ void nc_wht_pass(double *w, int l, int s) {
    constexpr int V = 1 << R;
    const u32 units = 1u << (l - R), lo_mask = (1u << s) - 1;
    for (u32 u = threadIdx.x; u < units; u += NC_THREADS) {
        const u32 base = ((u >> s) << (s + R)) | (u & lo_mask);
        double v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = w[nc_slot<SWZ>(base + ((u32)k << s))];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (!(k & (1 << r))) {
                    const double a = v[k], b = v[k | (1 << r)];
                    v[k] = a + b;
                    v[k | (1 << r)] = a - b;
                }
#pragma unroll
        for (int k = 0; k < V; ++k) w[nc_slot<SWZ>(base + ((u32)k << s))] = v[k];
    }
}

template <int L, bool SWZ>
__global__ __launch_bounds__(NC_THREADS) void k_nc_search(const NcArgs a) {
    static_assert(L >= 9, "part[] doubles as the 2 * NC_THREADS words of the workgroup reduction");
    extern __shared__ __attribute__((aligned(16))) double nc_lds[];
    double *w = nc_lds, *acc = nc_lds + (1 << L), *part = nc_lds + (2 << L);
    const int t = threadIdx.x, l = a.l;
    const u32 n_low = 1u << l;
    double best_e = __builtin_inf();
    u64 best_m = 0;
    for (i64 hi = blockIdx.x; hi < a.n_high; hi += gridDim.x) {
        for (u32 j = t; j < n_low; j += NC_THREADS) acc[j] = 0.0;
        for (int g = 0; g < a.n_groups; ++g) {
            const NcGroup G = a.groups[g];
            for (u32 j = t; j < n_low; j += NC_THREADS) w[nc_slot<SWZ>(j)] = 0.0;      // the slots this thread read last
            __syncthreads();                                   // also: the previous group's (or high part's) readers of w and part are done
            for (u32 i = G.item_begin + t; i < G.item_end; i += NC_THREADS) {
                const NcItem it = a.items[i];
                double s = 0.0;
                for (u32 e = it.begin; e < it.begin + it.count; ++e) {
                    const double c = a.coeff[e];
                    s += (__popc(a.high[e] & (u32)hi) & 1) ? -c : c;
                }
                if (it.target & NC_TO_PART) part[it.target & ~NC_TO_PART] = s;
                else w[nc_slot<SWZ>(it.target)] = s;
            }
            if (G.join_begin < G.join_end) {
                __syncthreads();
                for (u32 i = G.join_begin + t; i < G.join_end; i += NC_THREADS) {
                    const NcJoin jn = a.joins[i];
                    double s = 0.0;
                    for (u32 p = jn.begin; p < jn.begin + jn.count; ++p) s += part[p];
                    w[nc_slot<SWZ>(jn.slot)] = s;
                }
            }
            for (int s = 0; s < l;) {
                __syncthreads();
                const int r = l - s >= 3 ? 3 : l - s;
                if (r == 3) nc_wht_pass<3, SWZ>(w, l, s);
                else if (r == 2) nc_wht_pass<2, SWZ>(w, l, s);
                else nc_wht_pass<1, SWZ>(w, l, s);
                s += r;
            }
            __syncthreads();
            if (g + 1 < a.n_groups) {
                for (u32 j = t; j < n_low; j += NC_THREADS) { const double x = w[nc_slot<SWZ>(j)]; acc[j] += x * x; }
            } else {
                for (u32 j = t; j < n_low; j += NC_THREADS) {
                    const double e = w[nc_slot<SWZ>(j)] - sqrt(acc[j]);
                    const u64 m = ((u64)hi << l) | j;
                    if (a.energies) a.energies[m] = e;
                    if (nc_better(e, m, best_e, best_m)) { best_e = e; best_m = m; }
                }
            }
        }
    }
    __syncthreads();
    nc_block_best(best_e, best_m, part, reinterpret_cast<u64 *>(part + NC_THREADS));
    if (t == 0) { a.wg_energy[blockIdx.x] = best_e; a.wg_mask[blockIdx.x] = best_m; }
}

// out_energy[0], out_mask[0] = the best of the n workgroup winners
__global__ __launch_bounds__(NC_THREADS) void k_nc_reduce(const double *__restrict__ wg_energy, const u64 *__restrict__ wg_mask, i64 n,
                                                          double *__restrict__ out_energy, u64 *__restrict__ out_mask) {
    __shared__ double se[NC_THREADS];
    __shared__ u64 sm[NC_THREADS];
    double best_e = __builtin_inf();
    u64 best_m = 0;
    for (i64 i = threadIdx.x; i < n; i += NC_THREADS)
        if (nc_better(wg_energy[i], wg_mask[i], best_e, best_m)) { best_e = wg_energy[i]; best_m = wg_mask[i]; }
    nc_block_best(best_e, best_m, se, sm);
    if (threadIdx.x == 0) { *out_energy = best_e; *out_mask = best_m; }
}

// signs[k] = +-1 if the product, in generator order from the identity, of the generators that sel row k selects is +-terms[k], else 0.
// The phase e = 3 (Y_a + Y_b) + Y_out + 2 |x_a & z_b| mod 4 of a product a * b is a sum over the words of the row, so the words are
// independent: NC_SIGN_LANES adjacent lanes share a term, lane i walks words i, i + NC_SIGN_LANES, ... with the running product of its
// word in two registers (adjacent lanes read adjacent words of the term and of every generator), over the set bits of the selection a
// 64-bit word at a time; the lanes' phase sums and row comparisons meet in three shuffle steps.
constexpr int NC_SIGN_LANES = 8;
__global__ __launch_bounds__(256) void k_nc_signs(const u64 *__restrict__ terms, i64 T, const u64 *__restrict__ gens, int g, int Wq,
                                                  const u64 *__restrict__ sel, int sel_words, int8_t *__restrict__ signs) {
    const i64 k = ((i64)blockIdx.x * 256 + threadIdx.x) / NC_SIGN_LANES;
    const int lane = threadIdx.x % NC_SIGN_LANES;
    const bool live = k < T;                                   // the lanes past the last term still take part in the shuffles
    const u64 *mine = terms + (live ? k : 0) * 2 * Wq, *pick = sel + (live ? k : 0) * sel_words;
    u32 e = 0, differs = 0;
    for (int w = lane; live && w < Wq; w += NC_SIGN_LANES) {
        u64 ax = 0, az = 0;
        for (int j0 = 0; j0 < g; j0 += 64) {
            u64 bits = pick[j0 >> 6];
            if (g - j0 < 64) bits &= ((u64)1 << (g - j0)) - 1;                  // bits at or above the generator count are not read
            for (; bits; bits &= bits - 1) {
                const i64 j = j0 + __ffsll((unsigned long long)bits) - 1;
                const u64 bx = gens[j * 2 * Wq + w], bz = gens[j * 2 * Wq + Wq + w];
                const u64 ox = ax ^ bx, oz = az ^ bz;
                e += 3u * (u32)(__popcll(ax & az) + __popcll(bx & bz)) + (u32)__popcll(ox & oz) + 2u * (u32)__popcll(ax & bz);
                ax = ox; az = oz;
            }
        }
        differs |= (ax != mine[w] || az != mine[Wq + w]) ? 1u : 0u;
    }
#pragma unroll
    for (int d = NC_SIGN_LANES / 2; d > 0; d >>= 1) {
        e += (u32)__shfl_xor((int)e, d);
        differs |= (u32)__shfl_xor((int)differs, d);
    }
    e &= 3u;
    if (live && lane == 0) signs[k] = differs || (e & 1u) ? 0 : (e == 0 ? 1 : -1);
}

// What the host prepares for k_nc_search: the entries in (group, low mask, term) order and their cut into items (see the head of the file)
struct NcPlan {
    std::vector<double> coeff;
    std::vector<u32> high;
    std::vector<NcItem> items;
    std::vector<NcJoin> joins;
    std::vector<NcGroup> groups;
    u32 chunk = NC_CHUNK_MIN;
};

static void nc_build_plan(const double *coeff, const u64 *mask, const int32_t *clique, i64 T, int l, int n_cliques, u32 part_cap, NcPlan &plan) {
    const u64 low_mask = ((u64)1 << l) - 1;
    // S0 (clique -1) sorts last: key = group << l | low mask
    const auto key_of = [&](i64 k) { return ((u64)(clique[k] < 0 ? n_cliques : clique[k]) << l) | (mask[k] & low_mask); };
    std::vector<i64> order((size_t)T);
    for (i64 k = 0; k < T; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](i64 x, i64 y) { return key_of(x) < key_of(y); });
    plan.coeff.resize((size_t)T);
    plan.high.resize((size_t)T);
    for (i64 e = 0; e < T; ++e) {
        plan.coeff[(size_t)e] = coeff[order[(size_t)e]];
        plan.high[(size_t)e] = (u32)(mask[order[(size_t)e]] >> l);
    }
    // runs of one (group, low mask): [begin, end) in entry order, the group boundaries among them
    struct Run { u32 begin, end; u64 key; };
    std::vector<Run> runs;
    for (i64 e = 0; e < T; ++e) {
        const u64 key = key_of(order[(size_t)e]);
        if (runs.empty() || runs.back().key != key) runs.push_back({(u32)e, (u32)e + 1, key});
        else runs.back().end = (u32)e + 1;
    }
    // the smallest chunk at which no group needs more item sums than part[] holds
    for (plan.chunk = NC_CHUNK_MIN;; plan.chunk *= 2) {
        u64 worst = 0, here = 0, group = ~(u64)0;
        for (const Run &r : runs) {
            if ((r.key >> l) != group) { group = r.key >> l; here = 0; }
            const u32 len = r.end - r.begin;
            if (len > plan.chunk) here += (len + plan.chunk - 1) / plan.chunk;
            worst = std::max(worst, here);
        }
        if (worst <= part_cap) break;
    }
    size_t r = 0;
    const auto emit_group = [&](u64 group) {
        NcGroup G{(u32)plan.items.size(), 0, (u32)plan.joins.size(), 0};
        u32 n_part = 0;
        for (; r < runs.size() && (runs[r].key >> l) == group; ++r) {
            const u32 len = runs[r].end - runs[r].begin, slot = (u32)(runs[r].key & low_mask);
            if (len <= plan.chunk) { plan.items.push_back({runs[r].begin, len, slot, 0}); continue; }
            const u32 pieces = (len + plan.chunk - 1) / plan.chunk;
            plan.joins.push_back({n_part, pieces, slot, 0});
            for (u32 p = 0; p < pieces; ++p)
                plan.items.push_back({runs[r].begin + p * plan.chunk, std::min(plan.chunk, len - p * plan.chunk), NC_TO_PART | n_part++, 0});
        }
        G.item_end = (u32)plan.items.size();
        G.join_end = (u32)plan.joins.size();
        plan.groups.push_back(G);
    };
    while (r < runs.size() && (runs[r].key >> l) < (u64)n_cliques) emit_group(runs[r].key >> l);      // the cliques that have terms
    emit_group((u64)n_cliques);                                                                      // S0, terms or none
}

template <typename V>
static int nc_upload(Scratch &s, const std::vector<V> &v) {
    SG_TRY(s.alloc(v.size() * sizeof(V)));
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(s.p, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice, ctx().stream));
    count_h2d(v.size() * sizeof(V));
    return SYMGPU_OK;
}

template <int L, bool SWZ>
static int nc_launch(const NcArgs &a, i64 n_wg) {
    constexpr size_t lds = (size_t)3 * sizeof(double) << L;
    if (lds > 64 * 1024) {
        const bool ok = SG_DEVICE_ONCE(hipFuncSetAttribute(reinterpret_cast<const void *>((&k_nc_search<L, SWZ>)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess);
        if (!ok) { set_error("noncon_search: the runtime refused %zu bytes of LDS", lds); return SYMGPU_E_HIP; }
    }
    hipLaunchKernelGGL((k_nc_search<L, SWZ>), dim3((unsigned)n_wg), dim3(NC_THREADS), lds, ctx().stream, a);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_noncon_signs_dev(symgpu_op_t terms, symgpu_op_t gens, const uint64_t *sel, int sel_words, int8_t *signs) {
    SG_ENTER(terms, gens);
    SG_REQUIRE(terms && gens && terms->Wq == gens->Wq, "noncon_signs_dev: null handle, or the operands do not share Wq");
    const i64 T = terms->T, g = gens->T;
    SG_REQUIRE(g < ((i64)1 << 31) && sel_words >= 0 && (i64)sel_words * 64 >= g, "noncon_signs_dev: the selection rows are shorter than the generator count");
    SG_REQUIRE((sel && signs) || T == 0, "noncon_signs_dev: null selection or null output");
    if (T == 0) return SYMGPU_OK;
    hipStream_t st = ctx().stream;
    const size_t sel_bytes = (size_t)T * (size_t)sel_words * 8;
    Scratch sel_dev, signs_dev;
    SG_TRY(sel_dev.alloc(sel_bytes));
    SG_TRY(signs_dev.alloc((size_t)T));
    if (sel_bytes) HIP_TRY(hipMemcpyAsync(sel_dev.p, sel, sel_bytes, hipMemcpyHostToDevice, st));
    count_h2d(sel_bytes);
    hipLaunchKernelGGL(k_nc_signs, dim3((unsigned)((T * NC_SIGN_LANES + 255) / 256)), dim3(256), 0, st, terms->rows, T, gens->rows, (int)g, terms->Wq,
                       sel_dev.as<u64>(), sel_words, signs_dev.as<int8_t>());
    KERNEL_CHECK();
    SG_TRY(download_any(signs_dev.p, signs, (size_t)T));
    count_d2h((size_t)T);
    return SYMGPU_OK;
}

int symgpu_noncon_search(const double *coeff, const uint64_t *mask, const int32_t *clique, int64_t T, int n_free, int64_t n_cliques,
                         double *best_energy, uint64_t *best_mask, double *energies_or_null, int64_t *info) {
    SG_ENTER();
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    SG_REQUIRE(best_energy && best_mask, "noncon_search: null output");
    SG_REQUIRE(0 <= n_free && n_free <= NC_MAX_FREE, "noncon_search: the number of free generators must be 0 .. 40");
    SG_REQUIRE(n_cliques >= 0 && n_cliques < ((i64)1 << 31), "noncon_search: the number of cliques is negative or too large");
    SG_REQUIRE(T >= 0 && T < ((i64)1 << 31), "noncon_search: the number of terms is negative or too large");
    SG_REQUIRE((coeff && mask && clique) || T == 0, "noncon_search: null input");
    double magnitude = 0.0;
    for (i64 k = 0; k < T; ++k) {
        SG_REQUIRE(clique[k] >= -1 && clique[k] < n_cliques, "noncon_search: a clique number outside -1 .. n_cliques - 1");
        SG_REQUIRE((mask[k] >> n_free) == 0, "noncon_search: a mask has a bit at or above n_free");
        SG_REQUIRE(isfinite(coeff[k]), "noncon_search: a coefficient is not finite");
        magnitude += fabs(coeff[k]);
    }
    // every partial sum is at most sum|c| and every sum of squares at most its square: below sqrt(DBL_MAX) no energy is inf or NaN
    SG_REQUIRE(magnitude <= NC_MAX_MAGNITUDE, "noncon_search: the coefficients' magnitudes sum beyond 1e154, the squares would overflow");
    int L = NC_L;
    if (const char *e = SG_TUNE("SYMGPU_NONCON_L")) L = atoi(e);
    SG_REQUIRE(L == 10 || L == 11 || L == 12, "noncon_search: SYMGPU_NONCON_L must be 10, 11 or 12");
    bool swizzle = NC_SWIZZLE;
    if (const char *e = SG_TUNE("SYMGPU_NONCON_SWIZZLE")) swizzle = e[0] != '0';
    const int l = n_free < L ? n_free : L, h = n_free - l;
    const i64 n_high = (i64)1 << h;
    hipStream_t st = ctx().stream;

    NcPlan plan;
    nc_build_plan(coeff, mask, clique, T, l, (int)n_cliques, (u32)1 << L, plan);
    Scratch d_coeff, d_high, d_items, d_joins, d_groups, d_energies, d_wg, d_out;
    SG_TRY(nc_upload(d_coeff, plan.coeff));
    SG_TRY(nc_upload(d_high, plan.high));
    SG_TRY(nc_upload(d_items, plan.items));
    SG_TRY(nc_upload(d_joins, plan.joins));
    SG_TRY(nc_upload(d_groups, plan.groups));
    const bool want_energies = energies_or_null && n_free <= 24;
    const size_t e_bytes = sizeof(double) << n_free;
    if (want_energies) SG_TRY(d_energies.alloc(e_bytes));
    // LDS bounds the workgroups a CU holds: two rounds of them, so that an uneven tail costs little
    const i64 per_cu = (160 * 1024) / ((i64)3 * 8 << L), fill = 2 * per_cu * ctx().num_cu;
    const i64 n_wg = n_high < fill ? n_high : fill;
    SG_TRY(d_wg.alloc((size_t)n_wg * 16));
    SG_TRY(d_out.alloc(16));

    NcArgs a;
    a.coeff = d_coeff.as<double>(); a.high = d_high.as<u32>();
    a.items = d_items.as<NcItem>(); a.joins = d_joins.as<NcJoin>(); a.groups = d_groups.as<NcGroup>();
    a.n_groups = (int)plan.groups.size(); a.l = l; a.n_high = n_high;
    a.energies = want_energies ? d_energies.as<double>() : nullptr;
    a.wg_energy = d_wg.as<double>(); a.wg_mask = d_wg.as<u64>() + n_wg;
    if (L == 10) SG_TRY((swizzle ? nc_launch<10, true>(a, n_wg) : nc_launch<10, false>(a, n_wg)));
    else if (L == 11) SG_TRY((swizzle ? nc_launch<11, true>(a, n_wg) : nc_launch<11, false>(a, n_wg)));
    else SG_TRY((swizzle ? nc_launch<12, true>(a, n_wg) : nc_launch<12, false>(a, n_wg)));
    hipLaunchKernelGGL(k_nc_reduce, dim3(1), dim3(NC_THREADS), 0, st, a.wg_energy, a.wg_mask, n_wg, d_out.as<double>(), d_out.as<u64>() + 1);
    KERNEL_CHECK();

    u64 out[2];
    SG_TRY(download_any(d_out.p, out, 16));
    count_d2h(16);
    memcpy(best_energy, &out[0], 8);
    *best_mask = out[1];
    if (want_energies) {
        SG_TRY(download_any(d_energies.p, energies_or_null, e_bytes));
        count_d2h(e_bytes);
    }
    if (info) {
        info[0] = L;
        info[1] = n_high;
        info[2] = T;
        info[3] = n_wg;
    }
    return SYMGPU_OK;
}

}  // extern "C"
