// sparse_matrix.hip — PauliwordOp.to_sparse_matrix (reference base.py:1458-1507) of a resident operator of n <= 31 qubits as CSR.
//
// Entry (b, b ^ x_k) += c_k (-i)^{Y_k} (-1)^{|b & z_k|}, qubit 0 the MOST significant bit of b, terms added in operator order; entries
// whose two components are both +-0 are not stored (NaN and inf are).  Plan:
//   1. group the terms by X-part (xgroups.h): per sorted term its z, c' = c (-i)^Y and its flagged group word, per group its x; then,
//      per group and bit level l, the size of the sibling subtree of the binary trie of the sorted x values (sib[d][l]).  Row b lists
//      its groups in the order of x_d ^ b, and the rank of group d in that order is the sum of sib[d][l] over the levels where x_d ^ b
//      has a one bit.
//   2. count pass: one thread per row, the sorted terms staged in LDS a tile at a time (every lane reads the same word: a broadcast),
//      fp64 adds with the sign taken from the parity of b & z; counts[b] = kept entries of row b (4 B per row).
//   3. 64-bit exclusive scan of the counts -> indptr (device).
//   4. fill pass: the same sums for a block of RB rows; each value lands at [row][rank] of a slot array (LDS, or global scratch when
//      RB * D slots do not fit, or SYMGPU_CSR_SCRATCH=1, in several launches once the slots of all rows exceed 512 MiB, or
//      SYMGPU_CSR_SCRATCH_MIB); the slots, read in [row][rank] order, ARE the CSR order, so one block scan per 256 slots compacts them
//      into coalesced writes of data / indices.
#include "xgroups.h"
#include "block_scan.h"
#include <stdlib.h>
#include <string.h>
#include <memory>

namespace symgpu {

constexpr int CSR_WG = 256;                       // threads per workgroup (count pass: one row each)
constexpr int CSR_TILE = 256;                     // sorted terms staged in LDS per round
constexpr int CSR_SLOT_BYTES = 20;                // value (16 B) + column (4 B)
constexpr size_t CSR_SLOT_LDS = 72 * 1024;        // slot array of the LDS path: two workgroups per CU (160 KiB)
constexpr int CSR_MIN_LDS_ROWS = 32;              // fewer rows per workgroup leave too many lanes idle: the scratch form is used
constexpr size_t CSR_SCRATCH_MAX = (size_t)512 << 20;   // global slot scratch per launch of the fallback (raised to 4 workgroups per CU)
constexpr int CSR_SCAN_ITEMS = 4096;              // counts per workgroup of the 64-bit scan
constexpr u64 CSR_MAX_GRID = (u64)1 << 22;       // workgroups per fill launch

// sib[d * n + l] = groups that agree with x_d above bit l and differ from it at bit l
__global__ __launch_bounds__(256) void k_csr_sib(const u32 *__restrict__ gx, u32 D, int n, u32 *__restrict__ sib) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= (i64)D * n) return;
    const u32 d = (u32)(i / n);
    const int l = (int)(i - (i64)d * n);
    const u64 x = gx[d];
    const u64 lo = (((x >> (l + 1)) << 1) | (((x >> l) & 1) ^ 1)) << l;
    sib[i] = lower_bound(gx, D, lo + ((u64)1 << l)) - lower_bound(gx, D, lo);
}

// ---- 2 / 4. the row sums -----------------------------------------------------------------------------------------------------
struct CsrTerms {
    const u32 *tz;
    const f64x2 *tc;
    const u32 *tg;
    const u32 *gx;
    const u32 *sib;
    i64 T;
    u32 D;
    int n;
};

// Walks all sorted terms for row b (active lanes), staged CSR_TILE at a time through LDS by all CSR_WG threads; calls emit(d, value)
// at the last term of every group.  Every thread of the workgroup must call it (barriers).
template <typename Emit>
__device__ __forceinline__ void csr_row_sums(const CsrTerms &P, u64 b, bool active, u32 *s_z, f64x2 *s_c, u32 *s_g, Emit emit) {
    f64x2 acc = {0.0, 0.0};
    for (i64 base = 0; base < P.T; base += CSR_TILE) {
        const int m = (P.T - base) < CSR_TILE ? (int)(P.T - base) : CSR_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += blockDim.x) {
            s_z[j] = P.tz[base + j];
            s_c[j] = P.tc[base + j];
            s_g[j] = P.tg[base + j];
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < m; ++j) {
                const u32 g = s_g[j];
                const f64x2 c = s_c[j];
                const u64 neg = (u64)(__popc((u32)b & s_z[j]) & 1) << 63;
                f64x2 v;
                v.x = __longlong_as_double(__double_as_longlong(c.x) ^ (long long)neg);
                v.y = __longlong_as_double(__double_as_longlong(c.y) ^ (long long)neg);
                acc = (g & CSR_FIRST) ? v : f64x2{acc.x + v.x, acc.y + v.y};
                if (g & CSR_LAST) emit(__builtin_amdgcn_readfirstlane(g & CSR_GID), acc);
            }
        }
    }
}

__device__ __forceinline__ bool csr_kept(f64x2 v) { return !(v.x == 0.0 && v.y == 0.0); }

__global__ __launch_bounds__(CSR_WG) void k_csr_count(CsrTerms P, u32 *__restrict__ counts) {
    __shared__ u32 s_z[CSR_TILE], s_g[CSR_TILE];
    __shared__ f64x2 s_c[CSR_TILE];
    const u64 rows = (u64)1 << P.n;
    const u64 b = (u64)blockIdx.x * CSR_WG + threadIdx.x;
    u32 cnt = 0;
    csr_row_sums(P, b, b < rows, s_z, s_c, s_g, [&](u32, f64x2 v) { cnt += csr_kept(v) ? 1u : 0u; });
    if (b < rows) counts[b] = cnt;
}

// rank of group d in row b's column order
__device__ __forceinline__ u32 csr_rank(const CsrTerms &P, u32 d, u64 b) {
    const u32 y = P.gx[d] ^ (u32)b;
    const u32 *s = P.sib + (size_t)d * P.n;
    u32 r = 0;
    for (int l = 0; l < P.n; ++l) r += ((y >> l) & 1u) ? s[l] : 0u;
    return r;
}

// Block of RB rows from row0: sums into slots [row][rank] (LDS or `gslots` + block * RB * D), then one block scan per 256 slots writes
// the kept ones at indptr[row0] + their position.  IDX: int32 or int64 column indices.
template <bool GLOBAL, typename IDX>
__global__ __launch_bounds__(CSR_WG) void k_csr_fill(CsrTerms P, int RB, u64 block0, const u64 *__restrict__ indptr, u64 nnz, char *__restrict__ gslots,
                                                     f64x2 *__restrict__ data, IDX *__restrict__ indices) {
    extern __shared__ __align__(16) char csr_lds[];
    __shared__ u32 s_z[CSR_TILE], s_g[CSR_TILE];
    __shared__ f64x2 s_c[CSR_TILE];
    __shared__ u32 s_wave[CSR_WG / 64];
    const u64 rows = (u64)1 << P.n;
    const u64 blk = block0 + blockIdx.x;
    const u64 row0 = blk * (u64)RB;
    const u32 D = P.D;
    const size_t S = (size_t)RB * D;
    char *slots = GLOBAL ? gslots + (size_t)blockIdx.x * S * CSR_SLOT_BYTES : csr_lds;
    f64x2 *sv = reinterpret_cast<f64x2 *>(slots);
    u32 *sc = reinterpret_cast<u32 *>(slots + S * sizeof(f64x2));
    const int r = threadIdx.x;
    const u64 b = row0 + r;
    const bool active = r < RB && b < rows;
    csr_row_sums(P, b, active, s_z, s_c, s_g, [&](u32 d, f64x2 v) {
        const u32 k = csr_rank(P, d, b);
        if (k < D) {
            sv[(size_t)r * D + k] = v;
            sc[(size_t)r * D + k] = P.gx[d] ^ (u32)b;
        }
    });
    __syncthreads();
    const u64 rows_here = rows - row0 < (u64)RB ? rows - row0 : (u64)RB;
    const size_t S_valid = (size_t)rows_here * D;
    u64 out = indptr[row0];
    static_assert(CSR_WG == 256, "block_compact_256");
    for (size_t base = 0; base < S_valid; base += CSR_WG) {
        const size_t i = base + threadIdx.x;
        f64x2 v = {0.0, 0.0};
        u32 col = 0;
        bool keep = false;
        if (i < S_valid) {
            v = sv[i];
            col = sc[i];
            keep = csr_kept(v);
        }
        u32 total;
        const u64 pos = out + block_compact_256(keep, s_wave, &total);
        if (keep && pos < nnz) {
            data[pos] = v;
            indices[pos] = (IDX)col;
        }
        out += total;
    }
}

// ---- 3. 64-bit scan of the row counts --------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 csr_block_excl(u64 v, u64 *s_w, u64 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = (u64)__shfl_up((unsigned long long)x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    u64 wb = 0, t = 0;
    for (int w = 0; w < CSR_WG / 64; ++w) {
        wb += w < wave ? s_w[w] : 0;
        t += s_w[w];
    }
    __syncthreads();
    *total = t;
    return wb + x - v;
}

__global__ __launch_bounds__(CSR_WG) void k_csr_scan_sums(const u32 *__restrict__ counts, u64 N, u64 *__restrict__ sums) {
    __shared__ u64 s_w[CSR_WG / 64];
    const u64 base = (u64)blockIdx.x * CSR_SCAN_ITEMS;
    u64 v = 0;
    for (int j = threadIdx.x; j < CSR_SCAN_ITEMS; j += CSR_WG)
        if (base + j < N) v += counts[base + j];
    u64 total;
    csr_block_excl(v, s_w, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[0..nb) -> exclusive, sums[nb] = total
__global__ __launch_bounds__(CSR_WG) void k_csr_scan_top(u64 *__restrict__ sums, u64 nb) {
    __shared__ u64 s_w[CSR_WG / 64];
    u64 carry = 0;
    for (u64 base = 0; base < nb; base += CSR_WG) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < nb ? sums[i] : 0;
        u64 total;
        const u64 e = csr_block_excl(v, s_w, &total);
        if (i < nb) sums[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}

// indptr[i] = sums[block] + counts before i in the block; indptr[N] = total
__global__ __launch_bounds__(CSR_WG) void k_csr_scan_apply(const u32 *__restrict__ counts, u64 N, const u64 *__restrict__ sums, u64 nb, u64 *__restrict__ indptr) {
    __shared__ u64 s_w[CSR_WG / 64];
    constexpr int PER = CSR_SCAN_ITEMS / CSR_WG;
    const u64 base = (u64)blockIdx.x * CSR_SCAN_ITEMS + (u64)threadIdx.x * PER;
    u32 c[PER];
    u64 v = 0;
    for (int j = 0; j < PER; ++j) {
        c[j] = base + j < N ? counts[base + j] : 0u;
        v += c[j];
    }
    u64 total;
    u64 e = sums[blockIdx.x] + csr_block_excl(v, s_w, &total);
    for (int j = 0; j < PER; ++j) {
        if (base + j < N) indptr[base + j] = e;
        e += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) indptr[N] = sums[nb];
}

__global__ __launch_bounds__(256) void k_csr_indptr32(const u64 *__restrict__ in, u64 n, int32_t *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t)in[i];
}

static bool csr_force_scratch() {
    const char *e = getenv("SYMGPU_CSR_SCRATCH");   // read per call: the tests force the global-scratch fill on small inputs
    return e && e[0] == '1';
}

// global slot scratch per launch: CSR_SCRATCH_MAX, or SYMGPU_CSR_SCRATCH_MIB MiB (read per call: the tests make the fill take several
// launches at a small size, as it does by itself when the slots of all rows exceed the limit)
static size_t csr_scratch_max() {
    const char *e = getenv("SYMGPU_CSR_SCRATCH_MIB");
    const long long m = e ? atoll(e) : 0;
    return m > 0 && m <= (1 << 20) ? (size_t)m << 20 : CSR_SCRATCH_MAX;
}

}  // namespace symgpu

using namespace symgpu;

// the state a count call leaves for its fill call: the grouped terms, the trie sizes and the 64-bit indptr, on the operator's device
struct symgpu_csr_s {
    int device = 0;
    XGroups xg;
    u64 nnz = 0;
    Scratch sib, indptr;
};

static CsrTerms csr_terms_of(const symgpu_csr_s *p) {
    const XGroups &g = p->xg;
    return CsrTerms{g.tz.as<u32>(), g.tc.as<f64x2>(), g.tg.as<u32>(), g.gx.as<u32>(), p->sib.as<u32>(), g.T, g.G, g.n};
}

static int csr_count(symgpu_op_t op, int n, symgpu_csr_s *p) {
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << n;
    SG_TRY(xgroups_build(op, n, true, &p->xg));
    SG_TRY(p->indptr.alloc((size_t)(N + 1) * 8));
    if (p->xg.T == 0) {
        HIP_TRY(hipMemsetAsync(p->indptr.p, 0, (size_t)(N + 1) * 8, st));
        p->nnz = 0;
        return SYMGPU_OK;
    }
    const u32 D = p->xg.G;
    SG_TRY(p->sib.alloc((size_t)D * n * 4));
    hipLaunchKernelGGL(k_csr_sib, dim3(grid_each((i64)D * n)), dim3(256), 0, st, p->xg.gx.as<u32>(), D, n, p->sib.as<u32>());
    KERNEL_CHECK();
    Scratch counts, sums;
    const u64 nb = (N + CSR_SCAN_ITEMS - 1) / CSR_SCAN_ITEMS;
    SG_TRY(counts.alloc((size_t)N * 4));
    SG_TRY(sums.alloc((size_t)(nb + 1) * 8));
    hipLaunchKernelGGL(k_csr_count, dim3(grid_each((i64)N, CSR_WG)), dim3(CSR_WG), 0, st, csr_terms_of(p), counts.as<u32>());
    hipLaunchKernelGGL(k_csr_scan_sums, dim3((unsigned)nb), dim3(CSR_WG), 0, st, counts.as<u32>(), N, sums.as<u64>());
    hipLaunchKernelGGL(k_csr_scan_top, dim3(1), dim3(CSR_WG), 0, st, sums.as<u64>(), nb);
    hipLaunchKernelGGL(k_csr_scan_apply, dim3((unsigned)nb), dim3(CSR_WG), 0, st, counts.as<u32>(), N, sums.as<u64>(), nb, p->indptr.as<u64>());
    KERNEL_CHECK();
    u32 w[2] = {0, 0};
    SG_TRY(read_back_words(reinterpret_cast<const u32 *>(p->indptr.as<u64>() + N), 2, nullptr, 0, w));
    p->nnz = (u64)w[0] | ((u64)w[1] << 32);
    return SYMGPU_OK;
}

// The fill's form, decided once from D and the device (the count call reports its scratch size, the fill call runs it): slots in LDS
// when at least CSR_MIN_LDS_ROWS rows fit CSR_SLOT_LDS, else global scratch for 256-row workgroups, launched in chunks.
struct CsrFillForm {
    bool lds = false;
    int RB = CSR_WG;
    u64 nblk = 0, chunk = 0;
    size_t scratch_bytes = 0;
};

static int csr_min_lds_rows() {
    if (const char *e = SG_TUNE("SYMGPU_CSR_MIN_LDS_ROWS")) return atoi(e) > 0 ? atoi(e) : 1;   // tuning: the rows-per-workgroup floor
    return CSR_MIN_LDS_ROWS;
}

static CsrFillForm csr_fill_form(const symgpu_csr_s *p) {
    const bool lds_attr = SG_DEVICE_ONCE(
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_csr_fill<false, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CSR_SLOT_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&k_csr_fill<false, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CSR_SLOT_LDS) == hipSuccess);
    if (!lds_attr) note_degraded("to_sparse_matrix fill (k_csr_fill) in LDS off: the runtime refused its LDS size; every fill takes the global-scratch form");
    const u64 N = (u64)1 << p->xg.n;
    const size_t per_row = (size_t)p->xg.G * CSR_SLOT_BYTES;
    CsrFillForm f;
    if (lds_attr && per_row * csr_min_lds_rows() <= CSR_SLOT_LDS && !csr_force_scratch()) {
        f.lds = true;
        f.RB = (int)(CSR_SLOT_LDS / per_row < (size_t)CSR_WG ? CSR_SLOT_LDS / per_row : CSR_WG);
        f.nblk = (N + f.RB - 1) / f.RB;
        f.chunk = f.nblk < CSR_MAX_GRID ? f.nblk : CSR_MAX_GRID;
        return f;
    }
    const size_t per_blk = (size_t)CSR_WG * per_row;
    f.nblk = (N + CSR_WG - 1) / CSR_WG;
    f.chunk = csr_scratch_max() / per_blk;
    if (f.chunk < (u64)4 * ctx().num_cu) f.chunk = (u64)4 * ctx().num_cu;   // at least four workgroups per CU in every launch
    if (f.chunk > f.nblk) f.chunk = f.nblk;
    f.scratch_bytes = (size_t)f.chunk * per_blk;
    return f;
}

template <typename IDX>
static int csr_fill_launch(const symgpu_csr_s *p, const CsrFillForm &f, f64x2 *data, IDX *indices) {
    hipStream_t st = ctx().stream;
    const CsrTerms P = csr_terms_of(p);
    const size_t per_row = (size_t)p->xg.G * CSR_SLOT_BYTES;
    Scratch slots;
    if (!f.lds) SG_TRY(slots.alloc(f.scratch_bytes));
    for (u64 b0 = 0; b0 < f.nblk; b0 += f.chunk) {
        const u64 nb = f.nblk - b0 < f.chunk ? f.nblk - b0 : f.chunk;
        if (f.lds)
            hipLaunchKernelGGL((k_csr_fill<false, IDX>), dim3((unsigned)nb), dim3(CSR_WG), (size_t)f.RB * per_row, st, P, f.RB, b0,
                               p->indptr.as<u64>(), p->nnz, (char *)nullptr, data, indices);
        else
            hipLaunchKernelGGL((k_csr_fill<true, IDX>), dim3((unsigned)nb), dim3(CSR_WG), 0, st, P, f.RB, b0, p->indptr.as<u64>(), p->nnz,
                               slots.as<char>(), data, indices);
        KERNEL_CHECK();
        bump_counter(f.lds ? SYMGPU_CTR_CSR_FILL_LDS : SYMGPU_CTR_CSR_FILL_SCRATCH);   // launches of the fill by form, here and nowhere else
    }
    return SYMGPU_OK;
}

static int csr_fill(const symgpu_csr_s *p, double *data, void *indices, void *indptr, int index_bytes) {
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << p->xg.n, nnz = p->nnz;
    if (nnz > 0) {
        Scratch d_data, d_idx;
        SG_TRY(d_data.alloc((size_t)nnz * 16));
        SG_TRY(d_idx.alloc((size_t)nnz * index_bytes));
        const CsrFillForm f = csr_fill_form(p);
        if (index_bytes == 4) SG_TRY(csr_fill_launch(p, f, d_data.as<f64x2>(), d_idx.as<int32_t>()));
        else SG_TRY(csr_fill_launch(p, f, d_data.as<f64x2>(), d_idx.as<int64_t>()));
        SG_TRY(symgpu_dev_download(d_data.p, data, (size_t)nnz * 16));
        SG_TRY(symgpu_dev_download(d_idx.p, indices, (size_t)nnz * index_bytes));
    }
    if (index_bytes == 4) {
        Scratch ip32;
        SG_TRY(ip32.alloc((size_t)(N + 1) * 4));
        hipLaunchKernelGGL(k_csr_indptr32, dim3(grid_each((i64)N + 1)), dim3(256), 0, st, p->indptr.as<u64>(), N + 1, ip32.as<int32_t>());
        KERNEL_CHECK();
        SG_TRY(symgpu_dev_download(ip32.p, indptr, (size_t)(N + 1) * 4));
    } else {
        SG_TRY(symgpu_dev_download(p->indptr.p, indptr, (size_t)(N + 1) * 8));
    }
    return SYMGPU_OK;
}

extern "C" {

int symgpu_to_csr_count(symgpu_op_t op, int n_qubits, int64_t *nnz, int64_t *fill_scratch_bytes, symgpu_csr_t *plan) {
    SG_ENTER(op);
    SG_REQUIRE(op && nnz && fill_scratch_bytes && plan, "to_csr_count: arguments");
    *plan = nullptr;
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 31 && op->Wq == 1, "to_csr_count: 1 <= n_qubits <= 31");
    SG_REQUIRE(op->coeff || op->T == 0, "to_csr_count: operator has no coefficients");
    SG_REQUIRE(op->T < ((i64)1 << 30), "to_csr_count: T >= 2^30");
    std::unique_ptr<symgpu_csr_s> p(new symgpu_csr_s());
    p->device = op->device;
    SG_TRY(csr_count(op, n_qubits, p.get()));
    *nnz = (int64_t)p->nnz;
    *fill_scratch_bytes = p->nnz > 0 ? (int64_t)csr_fill_form(p.get()).scratch_bytes : 0;
    *plan = p.release();
    return SYMGPU_OK;
}

int symgpu_to_csr_fill(symgpu_csr_t plan, double *data, void *indices, void *indptr, int index_bytes) {
    SG_REQUIRE(plan, "to_csr_fill: null plan");
    // the plan goes whatever happens, after the scope below has ended (dev_free files a block under its owning device: no context needed)
    const std::unique_ptr<symgpu_csr_s> release(plan);
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    int rc = SYMGPU_OK;
    if (data || indices || indptr) {
        if (!(indptr && (index_bytes == 4 || index_bytes == 8) && (plan->nnz == 0 || (data && indices)))) {
            set_error("invalid argument: to_csr_fill: buffers / index_bytes");
            rc = SYMGPU_E_INVALID;
        } else {
            rc = csr_fill(plan, data, indices, indptr, index_bytes);
        }
    }
    if (rc == SYMGPU_OK) {
        const hipError_t e = hipStreamSynchronize(ctx().stream);
        if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__);
    }
    return rc;
}

}  // extern "C"
