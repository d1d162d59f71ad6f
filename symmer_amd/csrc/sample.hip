// sample.hip — measuring a vector of m complex128 amplitudes (include/symgpu.h, section f10): uniforms of Philox4x64-10 in
// NumPy's order, a radix-16 sum tree over the weights w[i] = re re + im im kept as a plan, draws that walk the tree, the distinct samples
// with their counts in two forms (integer atomics + compaction, or sort + run lengths) that give the same bytes, and the signed sums
// sum_j count_j (-1)^{|z_k & b_j|} of a Z-only operator over the counted basis indices.
// Tree: level 0 = the weights (never stored: recomputed from the amplitudes, two products and one sum, each rounded once), an entry of
// level j+1 = 0 + its up to 16 consecutive children of level j in ascending order; levels 1 .. depth are stored, level `depth` is the
// total.  k_sp_leaf reads 4,096 amplitudes a workgroup, once, and writes their entries of levels 1, 2 and 3 (4,096 = 16^3, so the groups
// do not straddle workgroups; entries past the end count as +0.0, which changes no sum of non-negative terms); k_sp_up forms each
// further level from the one below.  No floating-point atomics.
// Draw: r = u total; at a node acc_k = acc_{k-1} + c_k (acc_{-1} = 0: the partial sums of the construction), the first k with r < acc_k
// is taken, else the last child with c_k > 0; r <- r - acc_{k-1}.  A draw is a pure function of (seed, first_draw + i) or of u[i].
#include "matvec.h"
#include "sort.h"
#include <math.h>
#include <memory>
#include <stdlib.h>
#include <string.h>

namespace symgpu {

constexpr int SP_WG = 256;
constexpr int SP_RADIX = 16;
constexpr int SP_LEAF = 4096;               // amplitudes a workgroup of k_sp_leaf: three levels of the tree
constexpr int SP_MAX_LEVELS = 17;           // 16^16 > 2^62
constexpr i64 SP_MAX_SAMPLES = ((i64)1 << 31) - 1;

// Philox4x64-10 (Salmon et al., SC'11; the constants of Random123 and of NumPy)
constexpr u64 PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;
constexpr u64 PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;

// word (s mod 4) of the block with counter (s div 4 + 1, 0, 0, 0) and key (seed, 0), as a double (word >> 11) 2^-53
__device__ __forceinline__ double philox_uniform(u64 seed, u64 s) {
    u64 c0 = (s >> 2) + 1, c1 = 0, c2 = 0, c3 = 0, k0 = seed, k1 = 0;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const u64 hi0 = __umul64hi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const u64 hi1 = __umul64hi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    const u32 word = (u32)(s & 3);
    const u64 v = word == 0 ? c0 : word == 1 ? c1 : word == 2 ? c2 : c3;
    return __dmul_rn((double)(v >> 11), 1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(SP_WG) void k_sp_uniform(u64 seed, u64 first, i64 count, double *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i < count) out[i] = philox_uniform(seed, first + (u64)i);
}

__device__ __forceinline__ double sp_weight(f64x2 a) { return __dadd_rn(__dmul_rn(a.x, a.x), __dmul_rn(a.y, a.y)); }

// levels 1, 2, 3 of the 4,096 amplitudes of a workgroup.  LDS slots are padded by one per 16 so that the 16 consecutive reads of a
// thread do not meet its neighbours' in one bank.
__global__ __launch_bounds__(SP_WG) void k_sp_leaf(const f64x2 *__restrict__ amp, i64 m, double *__restrict__ L1, i64 n1, double *__restrict__ L2, i64 n2,
                                                   double *__restrict__ L3) {
    __shared__ double w[SP_LEAF + SP_LEAF / SP_RADIX];
    __shared__ double s1[SP_WG + SP_WG / SP_RADIX];
    __shared__ double s2[SP_RADIX];
    const u32 t = threadIdx.x;
    const i64 base = (i64)blockIdx.x * SP_LEAF;
#pragma unroll
    for (int i = 0; i < SP_LEAF / SP_WG; ++i) {
        const u32 l = t + SP_WG * i;
        const i64 g = base + l;
        w[l + (l >> 4)] = g < m ? sp_weight(amp[g]) : 0.0;
    }
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SP_RADIX; ++k) s = __dadd_rn(s, w[17 * t + k]);
    s1[t + (t >> 4)] = s;
    const i64 g1 = (i64)blockIdx.x * SP_WG + t;
    if (g1 < n1) L1[g1] = s;
    __syncthreads();
    if (t < SP_RADIX) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < SP_RADIX; ++k) v = __dadd_rn(v, s1[17 * t + k]);
        s2[t] = v;
        const i64 g2 = (i64)blockIdx.x * SP_RADIX + t;
        if (L2 && g2 < n2) L2[g2] = v;
    }
    __syncthreads();
    if (t == 0 && L3) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < SP_RADIX; ++k) v = __dadd_rn(v, s2[k]);
        L3[blockIdx.x] = v;
    }
}

// one further level: out[i] = 0 + in[16 i] + ... in ascending order
__global__ __launch_bounds__(SP_WG) void k_sp_up(const double *__restrict__ in, i64 n_in, double *__restrict__ out, i64 n_out) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i >= n_out) return;
    double s = 0.0;
    for (int k = 0; k < SP_RADIX; ++k) {
        const i64 c = i * SP_RADIX + k;
        if (c < n_in) s = __dadd_rn(s, in[c]);
    }
    out[i] = s;
}

// what the walk reads: lev[j] = level j (j >= 1), n[j] its length (n[0] = m)
struct SpTree {
    const f64x2 *amp;
    const double *lev[SP_MAX_LEVELS];
    i64 n[SP_MAX_LEVELS];
    int depth;
    double total;
};

__device__ __forceinline__ i64 sp_walk(const SpTree &t, double u) {
    double r = __dmul_rn(u, t.total);
    i64 node = 0;
    for (int j = t.depth - 1; j >= 0; --j) {
        const i64 base = node * SP_RADIX;
        const i64 left = t.n[j] - base;
        const int cnt = left < SP_RADIX ? (int)left : SP_RADIX;
        double acc = 0.0, sub = 0.0, last_sub = 0.0;
        int chosen = -1, last = -1;
        for (int k = 0; k < cnt; ++k) {
            const double c = j == 0 ? sp_weight(t.amp[base + k]) : t.lev[j][base + k];
            const double a = __dadd_rn(acc, c);
            if (c > 0.0) {
                last = k;
                last_sub = acc;
            }
            if (r < a) {
                chosen = k;
                sub = acc;
                break;
            }
            acc = a;
        }
        if (chosen < 0) {
            chosen = last < 0 ? 0 : last;
            sub = last < 0 ? 0.0 : last_sub;
        }
        if (chosen > 0) r = __dsub_rn(r, sub);
        node = base + chosen;
    }
    return node;
}

__global__ __launch_bounds__(SP_WG) void k_sp_draw(SpTree t, i64 n_samples, u64 seed, u64 first, const double *__restrict__ u_in, u64 *__restrict__ keys,
                                                   i64 *__restrict__ order) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i >= n_samples) return;
    const double u = u_in ? u_in[i] : philox_uniform(seed, first + (u64)i);
    const i64 s = sp_walk(t, u);
    keys[i] = (u64)s;
    if (order) order[i] = s;
}

// ---- counting, histogram form ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_WG) void k_sp_hist(const u64 *__restrict__ keys, i64 n_samples, u32 *__restrict__ cnt) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i < n_samples) atomicAdd(&cnt[keys[i]], 1u);
}
__global__ __launch_bounds__(SP_WG) void k_sp_hist_flags(const u32 *__restrict__ cnt, i64 m, u32 *__restrict__ flag) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i < m) flag[i] = cnt[i] != 0;
}
__global__ __launch_bounds__(SP_WG) void k_sp_hist_emit(const u32 *__restrict__ cnt, const u32 *__restrict__ pos, i64 m, i64 *__restrict__ idx,
                                                        i64 *__restrict__ count) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i >= m || cnt[i] == 0) return;
    idx[pos[i]] = i;
    count[pos[i]] = (i64)cnt[i];
}

// ---- counting, sort form: run lengths of the sorted draws ---------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_WG) void k_sp_run_heads(const u64 *__restrict__ keys, i64 n_samples, u32 *__restrict__ head) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i < n_samples) head[i] = i == 0 || keys[i] != keys[i - 1];
}
// the head of run d writes the run's sample and its start
__global__ __launch_bounds__(SP_WG) void k_sp_run_starts(const u64 *__restrict__ keys, const u32 *__restrict__ pos, i64 n_samples, i64 *__restrict__ idx,
                                                         u64 *__restrict__ start) {
    const i64 i = (i64)blockIdx.x * SP_WG + threadIdx.x;
    if (i >= n_samples) return;
    if (i == 0 || keys[i] != keys[i - 1]) {
        idx[pos[i]] = (i64)keys[i];
        start[pos[i]] = (u64)i;
    }
}
__global__ __launch_bounds__(SP_WG) void k_sp_run_lengths(const u64 *__restrict__ start, const u32 *__restrict__ n_runs, i64 n_samples, i64 *__restrict__ count) {
    const i64 d = (i64)blockIdx.x * SP_WG + threadIdx.x;
    const i64 D = (i64)*n_runs;
    if (d >= D) return;
    count[d] = (d + 1 < D ? (i64)start[d + 1] : n_samples) - (i64)start[d];
}

// ---- signed sums ------------------------------------------------------------------------------------------------------------------------
// workgroup k: out[k] = sum_j count_j (-1)^{|zi_k & idx_j|}, zi_k the Z-part of row k moved to index bits (qubit q -> bit n-1-q);
// out[T] is raised when a row has an X-part
__global__ __launch_bounds__(SP_WG) void k_sp_signed(const u64 *__restrict__ rows, int n, const i64 *__restrict__ idx, const i64 *__restrict__ count, i64 D,
                                                     i64 *__restrict__ out, i64 T) {
    __shared__ i64 sm[SP_WG];
    const i64 k = blockIdx.x;
    const u64 x = rows[2 * k], z = rows[2 * k + 1];
    const u64 zi = __brevll(z) >> (64 - n);
    i64 s = 0;
    for (i64 j = threadIdx.x; j < D; j += SP_WG) s += (__popcll(zi & (u64)idx[j]) & 1) ? -count[j] : count[j];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int h = SP_WG / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[k] = sm[0];
        if (x != 0) out[T] = 1;
    }
}

}  // namespace symgpu

// a plan: the stored levels of the tree over a vector the caller keeps alive and unchanged
struct symgpu_sample_s {
    int device = 0;
    const f64x2 *amp = nullptr;
    i64 m = 0;
    int depth = 0;
    i64 n[symgpu::SP_MAX_LEVELS] = {0};
    i64 off[symgpu::SP_MAX_LEVELS] = {0};       // level j at tree + off[j], j >= 1
    i64 tree_doubles = 0;
    symgpu::Scratch tree;
    double total = 0.0;
    int build_launches = 0, last_form = 0, last_launches = 0;
};

namespace symgpu {

// the one place that chooses the counting form, from bytes moved: the histogram clears m counters, writes and scans m flags and reads
// both again (28 m bytes) beside an atomic a draw; the sort moves every 8-byte key three times a pass (histogram read, scatter read and
// write), one pass per byte of the sample.  UNMEASURED until tools/bench_sample.py has run on the target.
static int sp_sort_passes(i64 m) {
    int bits = 1;
    while (bits < 63 && ((i64)1 << bits) < m) ++bits;
    return (bits + 7) / 8;
}
static bool sp_hist_legal(i64 m) { return m < ((i64)1 << 31); }
static int sp_count_form(i64 m, i64 n_samples) {
    const char *f = getenv("SYMGPU_SAMPLE_COUNT");
    if (f && !strcmp(f, "sort")) return SYMGPU_SAMPLE_SORT;
    if (f && !strcmp(f, "hist") && sp_hist_legal(m)) return SYMGPU_SAMPLE_HIST;
    if (!sp_hist_legal(m)) return SYMGPU_SAMPLE_SORT;
    const double hist = 28.0 * (double)m + 8.0 * (double)n_samples, sort = 24.0 * sp_sort_passes(m) * (double)n_samples;
    return hist <= sort ? SYMGPU_SAMPLE_HIST : SYMGPU_SAMPLE_SORT;
}

static SpTree sp_tree_of(const symgpu_sample_s *p) {
    SpTree t;
    t.amp = p->amp;
    t.depth = p->depth;
    t.total = p->total;
    for (int j = 0; j < SP_MAX_LEVELS; ++j) {
        t.n[j] = p->n[j];
        t.lev[j] = j >= 1 && j <= p->depth ? p->tree.as<double>() + p->off[j] : nullptr;
    }
    return t;
}

static int sp_build(symgpu_sample_s *p) {
    hipStream_t st = ctx().stream;
    p->n[0] = p->m;
    int j = 0;
    do {
        p->n[j + 1] = (p->n[j] + SP_RADIX - 1) / SP_RADIX;
        ++j;
        p->off[j] = p->tree_doubles;
        p->tree_doubles += p->n[j];
    } while (p->n[j] > 1);
    p->depth = j;
    SG_TRY(matvec_require_memory((u64)p->tree_doubles * 8 + 4096, "the sampling plan"));
    SG_TRY(p->tree.alloc((size_t)p->tree_doubles * 8));
    double *tree = p->tree.as<double>();
    auto level = [&](int l) { return l <= p->depth ? tree + p->off[l] : (double *)nullptr; };
    hipLaunchKernelGGL(k_sp_leaf, dim3(grid_each(p->m, SP_LEAF)), dim3(SP_WG), 0, st, p->amp, p->m, level(1), p->n[1], level(2), p->n[2], level(3));
    p->build_launches = 1;
    for (int l = 3; l < p->depth; ++l) {
        hipLaunchKernelGGL(k_sp_up, dim3(grid_each(p->n[l + 1], SP_WG)), dim3(SP_WG), 0, st, level(l), p->n[l], level(l + 1), p->n[l + 1]);
        ++p->build_launches;
    }
    KERNEL_CHECK();
    SG_TRY(download_any(level(p->depth), &p->total, 8));
    if (!(p->total > 0.0) || !__builtin_isfinite(p->total)) {
        set_error("invalid argument: sample_plan: the weights add up to %g (zero, negative or not finite)", p->total);
        return SYMGPU_E_INVALID;
    }
    return SYMGPU_OK;
}

// the distinct samples of keys[0 .. S), ascending, with their counts; *n_runs_dev (device u32) their number
static int sp_count_hist(const symgpu_sample_s *p, const u64 *keys, i64 S, i64 *idx, i64 *count, u32 *n_runs_dev, int *launches) {
    hipStream_t st = ctx().stream;
    Scratch cnt, pos;
    SG_TRY(cnt.alloc((size_t)p->m * 4));
    SG_TRY(pos.alloc((size_t)p->m * 4));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, (size_t)p->m * 4, st));
    hipLaunchKernelGGL(k_sp_hist, dim3(grid_each(S, SP_WG)), dim3(SP_WG), 0, st, keys, S, cnt.as<u32>());
    hipLaunchKernelGGL(k_sp_hist_flags, dim3(grid_each(p->m, SP_WG)), dim3(SP_WG), 0, st, cnt.as<u32>(), p->m, pos.as<u32>());
    KERNEL_CHECK();
    SG_TRY(exclusive_scan_u32(pos.as<u32>(), pos.as<u32>(), p->m, n_runs_dev));
    hipLaunchKernelGGL(k_sp_hist_emit, dim3(grid_each(p->m, SP_WG)), dim3(SP_WG), 0, st, cnt.as<u32>(), pos.as<u32>(), p->m, idx, count);
    KERNEL_CHECK();
    *launches += 3;
    HIP_TRY(hipStreamSynchronize(st));           // the scratch of this form is read until here
    return SYMGPU_OK;
}

static int sp_count_sort(const symgpu_sample_s *p, u64 *keys, i64 S, i64 *idx, i64 *count, u32 *n_runs_dev, int *launches) {
    hipStream_t st = ctx().stream;
    Scratch tmp, pos;
    SG_TRY(tmp.alloc((size_t)S * 8));
    SG_TRY(pos.alloc((size_t)S * 4));
    SortResult res;
    SG_TRY(radix_sort({keys, tmp.as<u64>(), nullptr, nullptr, S, 0, 8 * sp_sort_passes(p->m), nullptr, SortForm::Launches}, &res));
    hipLaunchKernelGGL(k_sp_run_heads, dim3(grid_each(S, SP_WG)), dim3(SP_WG), 0, st, res.keys, S, pos.as<u32>());
    KERNEL_CHECK();
    SG_TRY(exclusive_scan_u32(pos.as<u32>(), pos.as<u32>(), S, n_runs_dev));
    hipLaunchKernelGGL(k_sp_run_starts, dim3(grid_each(S, SP_WG)), dim3(SP_WG), 0, st, res.keys, pos.as<u32>(), S, idx, res.spare_keys);
    hipLaunchKernelGGL(k_sp_run_lengths, dim3(grid_each(S, SP_WG)), dim3(SP_WG), 0, st, res.spare_keys, n_runs_dev, S, count);
    KERNEL_CHECK();
    *launches += 3;
    HIP_TRY(hipStreamSynchronize(st));
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_philox_uniform(uint64_t seed, int64_t first_draw, int64_t count, double *out_dev) {
    SG_ENTER();
    SG_REQUIRE(out_dev, "philox_uniform: null output");
    SG_REQUIRE(first_draw >= 0 && count >= 0 && first_draw <= INT64_MAX - count, "philox_uniform: first_draw, count >= 0 and first_draw + count < 2^63");
    if (count == 0) return SYMGPU_OK;
    hipLaunchKernelGGL(k_sp_uniform, dim3(grid_each(count, SP_WG)), dim3(SP_WG), 0, ctx().stream, (u64)seed, (u64)first_draw, (i64)count, out_dev);
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

int symgpu_sample_plan(const double *amp_dev, int64_t m, struct symgpu_sample_s **plan) {
    SG_ENTER();
    SG_REQUIRE(plan, "sample_plan: null plan pointer");
    *plan = nullptr;
    SG_REQUIRE(amp_dev, "sample_plan: null amplitudes");
    SG_REQUIRE(m >= 1 && m <= ((i64)1 << 40), "sample_plan: 1 <= m <= 2^40");
    std::unique_ptr<symgpu_sample_s> p(new symgpu_sample_s());
    p->device = ctx().device;
    p->amp = reinterpret_cast<const f64x2 *>(amp_dev);
    p->m = m;
    SG_TRY(sp_build(p.get()));
    *plan = p.release();
    return SYMGPU_OK;
}

int symgpu_sample_free(struct symgpu_sample_s *plan) {
    SG_REQUIRE(plan, "sample_free: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    delete plan;
    return SYMGPU_OK;
}

int symgpu_sample_info(struct symgpu_sample_s *plan, double *total, int64_t *info) {
    SG_REQUIRE(plan, "sample_info: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (total) *total = plan->total;
    if (info) {
        info[0] = plan->m;
        info[1] = plan->depth;
        info[2] = plan->tree_doubles * 8;
        info[3] = plan->build_launches;
        info[4] = plan->last_form;
        info[5] = plan->last_launches;
    }
    return SYMGPU_OK;
}

int symgpu_sample_draw(struct symgpu_sample_s *plan, int64_t n_samples, uint64_t seed, int64_t first_draw, const double *u_dev, int64_t *order_dev,
                       int64_t *idx_dev, int64_t *count_dev, int64_t *n_distinct) {
    SG_REQUIRE(plan, "sample_draw: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    SG_REQUIRE(n_distinct, "sample_draw: null n_distinct");
    *n_distinct = 0;
    SG_REQUIRE(n_samples >= 0 && n_samples <= SP_MAX_SAMPLES, "sample_draw: 0 <= n_samples < 2^31");
    SG_REQUIRE(idx_dev && count_dev, "sample_draw: null idx_dev or count_dev");
    SG_REQUIRE(first_draw >= 0 && first_draw <= INT64_MAX - n_samples, "sample_draw: first_draw >= 0 and first_draw + n_samples < 2^63");
    plan->last_form = 0;
    plan->last_launches = 0;
    if (n_samples == 0) return SYMGPU_OK;
    const int form = sp_count_form(plan->m, n_samples);
    const u64 need = (u64)n_samples * 8 + (form == SYMGPU_SAMPLE_HIST ? (u64)plan->m * 8 : (u64)n_samples * 12) + 8192;
    SG_TRY(matvec_require_memory(need, "the draws and their counting"));
    hipStream_t st = ctx().stream;
    Scratch keys, n_runs;
    SG_TRY(keys.alloc((size_t)n_samples * 8));
    SG_TRY(n_runs.alloc(16));
    int launches = 1;
    hipLaunchKernelGGL(k_sp_draw, dim3(grid_each(n_samples, SP_WG)), dim3(SP_WG), 0, st, sp_tree_of(plan), (i64)n_samples, (u64)seed, (u64)first_draw, u_dev,
                       keys.as<u64>(), (i64 *)order_dev);
    KERNEL_CHECK();
    if (form == SYMGPU_SAMPLE_HIST) SG_TRY(sp_count_hist(plan, keys.as<u64>(), n_samples, (i64 *)idx_dev, (i64 *)count_dev, n_runs.as<u32>(), &launches));
    else SG_TRY(sp_count_sort(plan, keys.as<u64>(), n_samples, (i64 *)idx_dev, (i64 *)count_dev, n_runs.as<u32>(), &launches));
    u32 D = 0;
    SG_TRY(download_any(n_runs.p, &D, 4));
    *n_distinct = (int64_t)D;
    plan->last_form = form;
    plan->last_launches = launches;
    return SYMGPU_OK;
}

int symgpu_counts_signed_sums(symgpu_op_t op, int n_qubits, const int64_t *idx_dev, const int64_t *count_dev, int64_t n_distinct, int64_t *out_host) {
    SG_ENTER(op);
    SG_REQUIRE(op && out_host, "counts_signed_sums: null arguments");
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32, "counts_signed_sums: 1 <= n_qubits <= 32");
    SG_REQUIRE(op->Wq == 1, "counts_signed_sums: the operator's rows have more than one word per half (Wq = 1 wanted)");
    SG_REQUIRE(n_distinct >= 0 && ((idx_dev && count_dev) || n_distinct == 0), "counts_signed_sums: n_distinct >= 0 and the arrays it counts");
    const i64 T = op->T;
    if (T == 0) return SYMGPU_OK;
    SG_REQUIRE(T < ((i64)1 << 31), "counts_signed_sums: T >= 2^31");
    SG_TRY(matvec_require_memory((u64)(T + 1) * 8 + 4096, "the signed sums"));
    hipStream_t st = ctx().stream;
    Scratch out;
    SG_TRY(out.alloc((size_t)(T + 1) * 8));
    HIP_TRY(hipMemsetAsync(out.as<i64>() + T, 0, 8, st));
    hipLaunchKernelGGL(k_sp_signed, dim3((unsigned)T), dim3(SP_WG), 0, st, op->rows, n_qubits, (const i64 *)idx_dev, (const i64 *)count_dev, (i64)n_distinct,
                       out.as<i64>(), T);
    KERNEL_CHECK();
    std::unique_ptr<i64[]> back(new i64[T + 1]);
    SG_TRY(download_any(out.p, back.get(), (size_t)(T + 1) * 8));
    SG_REQUIRE(back[T] == 0, "counts_signed_sums: a row of the operator has an X-part (only I and Z can be read off computational-basis counts)");
    memcpy(out_host, back.get(), (size_t)T * 8);
    return SYMGPU_OK;
}

}  // extern "C"
