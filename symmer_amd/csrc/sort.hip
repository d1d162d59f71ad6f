// sort.hip — stable LSD radix sort of (u64 key, u32 value) pairs or bare u64 keys: the one request (sort.h), the decision between its two
// forms, and the form of a launch per step.  The one-launch form: sort_coop.hip; the tile body both share: sort_tile.h.
//
// Used by term cleanup (reference: symplectic_cleanup, symmer/operators/utils.py:230-279) to group equal
// rows: keys are 64-bit GF(2)-linear row hashes, values are input indices.  The sort is STABLE, so inside
// a run of equal keys the values stay in ascending input order — which is exactly the order in which the
// reference's `np.add.at` accumulates duplicate coefficients (utils.py:273-274).
//
// HBM-bound: per 8-bit pass each element is read twice (histogram + scatter: 8 B + 12 B) and written once
// (12 B).  Tiles of 4096 elements are ranked with 64-wide wavefront ballots (one match mask per lane from 8
// __ballot calls), staged through LDS in digit order and written out as contiguous per-digit runs.
#include "sort.h"
#include "sort_tile.h"

namespace symgpu {

__global__ __launch_bounds__(256) void k_rs_hist(const u64 *__restrict__ keys, i64 n, int shift, i64 n_tiles, u32 *__restrict__ tile_hist) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * RS_TILE;
    u64 kk[RS_ITEMS];
#pragma unroll
    for (int k = 0; k < RS_ITEMS; ++k) {                               // sixteen loads in flight
        const i64 idx = base + k * 256 + threadIdx.x;
        kk[k] = idx < n ? keys[idx] : 0ULL;
    }
#pragma unroll
    for (int k = 0; k < RS_ITEMS; ++k)
        if (base + k * 256 + threadIdx.x < n) atomicAdd(&h[(kk[k] >> shift) & 255], 1u);
    __syncthreads();
    tile_hist[(i64)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];       // tile-major: one coalesced KB per tile, here and in the scatter
}

// Exclusive scan of the tile histograms over the tiles, per digit, ONE launch per pass.  The histograms are TILE-major (256 counters of a
// tile side by side: every access of k_rs_hist, of this kernel and of the scatter is a coalesced KB; the digit-major layout of rounds 2-3
// made the scatter gather its 256 offsets from 256 different lines).  Workgroup c scans a chunk of `chunk_len` tiles in place (thread d
// walks column d, sixteen rows in flight) and files the chunk's totals write-through; the LAST workgroup to finish (ticket) turns the
// chunk totals into chunk_excl[c][d] and row_total[d].  The scatter adds tile_off[tile][d] + chunk_excl[tile / chunk_len][d].
constexpr int RSC_MAX_CHUNKS = 128;
constexpr int RSC_MIN_LEN = 16;
__global__ __launch_bounds__(256) void k_rs_scan_cols(u32 *__restrict__ tile_hist, i64 n_tiles, i64 chunk_len, u32 *__restrict__ chunk_tot,
                                                       u32 *__restrict__ chunk_excl, u32 *__restrict__ row_total, u32 *__restrict__ ticket) {
    __shared__ u32 s_last;
    const int d = threadIdx.x;
    const i64 t0 = (i64)blockIdx.x * chunk_len, t1 = t0 + chunk_len < n_tiles ? t0 + chunk_len : n_tiles;
    u32 run = 0;
    for (i64 t = t0; t < t1; t += 16) {
        u32 v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = t + k < t1 ? tile_hist[(t + k) * 256 + d] : 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (t + k < t1) tile_hist[(t + k) * 256 + d] = run;
            run += v[k];
        }
    }
    __hip_atomic_store(chunk_tot + (i64)blockIdx.x * 256 + d, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the write-through stores have left before the ticket is taken
    __syncthreads();
    if (d == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    u32 acc = 0;
    for (int c = 0; c < (int)gridDim.x; c += 32) {
        u32 v[32];
#pragma unroll
        for (int k = 0; k < 32; ++k)
            v[k] = c + k < (int)gridDim.x ? __hip_atomic_load(chunk_tot + (i64)(c + k) * 256 + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            if (c + k < (int)gridDim.x) chunk_excl[(i64)(c + k) * 256 + d] = acc;
            acc += v[k];
        }
    }
    row_total[d] = acc;
    if (d == 0) *ticket = 0;                                           // for the next pass (stream order)
}

template <bool HAS_VALS>
__global__ __launch_bounds__(256) void k_rs_scatter(const u64 *__restrict__ keys, const u32 *__restrict__ vals, i64 n, int shift,
                                                     i64 n_tiles, const u32 *__restrict__ tile_off /* [tile][256], scanned inside its chunk */,
                                                     const u32 *__restrict__ chunk_excl /* [chunk][256] */, i64 chunk_len,
                                                     const u32 *__restrict__ row_total /* [256]: keys per digit */,
                                                     u64 *__restrict__ out_keys, u32 *__restrict__ out_vals) {
    __shared__ u64 s_key[RS_TILE];
    __shared__ u32 s_val[HAS_VALS ? RS_TILE : 1];
    __shared__ u32 s_cnt[4][256];      // per-wave running digit counters, then per-wave exclusive offsets.  NOT volatile and not
                                       // through a pointer: both turn every access into a flat, system-scope load / store with a
                                       // wait behind it; wavefront-scope fences order the lanes' reads and writes instead
    __shared__ u32 s_dig_off[256];     // exclusive offset of each digit inside the tile
    __shared__ u32 s_gbase[256];       // global base of each digit for this tile
    __shared__ u32 s_wave[4];

    // XCD-aware tile order: workgroups go round-robin over the 8 XCDs, and consecutive tiles append to the same 256 digit streams — the
    // runs of one tile end in the middle of cache lines that the next tile completes.  Every XCD therefore takes a CONTIGUOUS eighth of
    // the tiles, in order: the partial lines meet in ONE L2 instead of leaving two XCDs as masked partial writes.
    const i64 per_xcd = (n_tiles + 7) / 8;
    const i64 tile = (i64)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (tile >= n_tiles) return;
    const i64 tile_base = tile * RS_TILE;
    const u32 goff = tile_off[tile * 256 + threadIdx.x] + chunk_excl[tile / chunk_len * 256 + threadIdx.x];     // issued first, used behind the key loads
    const u32 gtot = row_total[threadIdx.x];
    u64 key[RS_ITEMS];
    u32 val[HAS_VALS ? RS_ITEMS : 1];
    u32 pos[RS_ITEMS];
    tile_load_items<TileMem::Plain, HAS_VALS>(keys, vals, tile_base, n, key, val);
    if (HAS_VALS) {
        asm volatile("" : "+v"(val[0]), "+v"(val[1]), "+v"(val[2]), "+v"(val[3]), "+v"(val[4]), "+v"(val[5]), "+v"(val[6]), "+v"(val[7]));
        asm volatile("" : "+v"(val[8]), "+v"(val[9]), "+v"(val[10]), "+v"(val[11]), "+v"(val[12]), "+v"(val[13]), "+v"(val[14]), "+v"(val[15]));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cnt[k][threadIdx.x] = 0;
    {   // global base of digit d for this tile = keys of smaller digits + keys of digit d in earlier tiles
        u32 all;
        s_gbase[threadIdx.x] = goff + block_excl_scan_256(gtot, s_wave, &all);
    }
    __syncthreads();
    tile_rank(key, shift, tile_base, n, s_cnt, pos);
    __syncthreads();
    // per-digit: exclusive offsets over waves, tile digit counts, exclusive scan over digits
    (void)tile_digit_offsets(s_cnt, s_dig_off, s_wave);
    __syncthreads();
    tile_stage<HAS_VALS>(key, val, pos, shift, tile_base, n, s_dig_off, s_cnt, s_key, s_val);
    __syncthreads();
    tile_write_runs<TileMem::Plain, HAS_VALS>(s_key, s_val, shift, tile_base, n, s_dig_off, s_gbase, out_keys, out_vals);
}

bool sort_form(i64 n, bool has_vals, bool has_first_hist, SortForm want, bool one_launch_off) {
    if (want == SortForm::Launches || has_first_hist) return false;
    if (n <= 1) return true;
    const i64 n_tiles = (n + RS_TILE - 1) / RS_TILE;
    if (n_tiles > SORT_ONE_LAUNCH_MAX_TILES) return false;
    if (want == SortForm::OneLaunchWherePays && n_tiles > (has_vals ? SORT_ONE_LAUNCH_TILES_PAIRS : SORT_ONE_LAUNCH_TILES_KEYS)) return false;
    if (const char *e = SG_TUNE("SYMGPU_SORT_COOP")) if (e[0] == '0') return false;
    return !one_launch_off;
}

// the form of a launch per step (n > 1): per pass the tile histograms (the first pass: the caller's, if it has them), their column scan
// and the scatter
static_assert(RS_TILE == SORT_TILE, "the tile size callers form their first histogram with");
static int sort_launches(const SortRequest &rq) {
    const i64 n = rq.n;
    if (n >= ((i64)1 << 32)) {
        set_error("radix sort: n = %lld exceeds 2^32 - 1", (long long)n);
        return SYMGPU_E_INVALID;
    }
    hipStream_t st = ctx().stream;
    const i64 n_tiles = (n + RS_TILE - 1) / RS_TILE;
    u32 *ticket;
    SG_TRY(sort_scan_ticket(&ticket));
    const i64 chunk_len = (n_tiles + RSC_MAX_CHUNKS - 1) / RSC_MAX_CHUNKS > RSC_MIN_LEN ? (n_tiles + RSC_MAX_CHUNKS - 1) / RSC_MAX_CHUNKS : RSC_MIN_LEN;
    const unsigned n_chunks = (unsigned)((n_tiles + chunk_len - 1) / chunk_len);
    Scratch hist_own, scan;                                            // scan: row_total[256] | chunk_tot[n_chunks][256] | chunk_excl[n_chunks][256]
    if (!rq.first_hist) SG_TRY(hist_own.alloc((size_t)n_tiles * 256 * sizeof(u32)));
    SG_TRY(scan.alloc((size_t)(1 + 2 * n_chunks) * 256 * sizeof(u32)));
    u32 *row_total = scan.as<u32>(), *chunk_tot = row_total + 256, *chunk_excl = chunk_tot + (size_t)n_chunks * 256;
    u32 *hist_p = rq.first_hist ? rq.first_hist : hist_own.as<u32>();
    u64 *ksrc = rq.keys, *kdst = rq.keys_tmp;
    u32 *vsrc = rq.vals, *vdst = rq.vals_tmp;
    for (int shift = rq.begin_bit; shift < rq.end_bit; shift += 8) {
        if (!(rq.first_hist && shift == rq.begin_bit)) {
            hipLaunchKernelGGL(k_rs_hist, dim3((unsigned)n_tiles), dim3(256), 0, st, ksrc, n, shift, n_tiles, hist_p);
            KERNEL_CHECK();
        }
        hipLaunchKernelGGL(k_rs_scan_cols, dim3(n_chunks), dim3(256), 0, st, hist_p, n_tiles, chunk_len, chunk_tot, chunk_excl, row_total, ticket);
        if (rq.vals)
            hipLaunchKernelGGL(k_rs_scatter<true>, dim3((unsigned)((n_tiles + 7) / 8 * 8)), dim3(256), 0, st, ksrc, vsrc, n, shift, n_tiles, hist_p, chunk_excl,
                               chunk_len, row_total, kdst, vdst);
        else
            hipLaunchKernelGGL(k_rs_scatter<false>, dim3((unsigned)((n_tiles + 7) / 8 * 8)), dim3(256), 0, st, ksrc, (const u32 *)nullptr, n, shift, n_tiles,
                               hist_p, chunk_excl, chunk_len, row_total, kdst, (u32 *)nullptr);
        KERNEL_CHECK();
        u64 *tk = ksrc; ksrc = kdst; kdst = tk;
        u32 *tv = vsrc; vsrc = vdst; vdst = tv;
    }
    return SYMGPU_OK;
}

int radix_sort(const SortRequest &rq, SortResult *res) {
    *res = SortResult{rq.keys, rq.keys_tmp, rq.vals, rq.vals_tmp, false};
    res->one_launch = sort_form(rq.n, rq.vals != nullptr, rq.first_hist != nullptr, rq.want, ctx().sort.coop_disabled);
    if (rq.n <= 1) return SYMGPU_OK;
    SG_TRY(res->one_launch ? sort_one_launch(rq) : sort_launches(rq));
    if (((rq.end_bit - rq.begin_bit + 7) / 8) & 1)                     // an odd number of passes ends in the temporaries
        *res = SortResult{rq.keys_tmp, rq.keys, rq.vals_tmp, rq.vals, res->one_launch};
    return SYMGPU_OK;
}

}  // namespace symgpu

// ------------------------------------------------------------------------------------------------
// debug entry points: the sort and the scans on the caller's device buffers, for tests/test_gpu_sort.py
// ------------------------------------------------------------------------------------------------
using namespace symgpu;

extern "C" {

int symgpu_debug_sort(uint64_t *keys, uint32_t *vals, int64_t n, int begin_bit, int end_bit, int form, int with_first_hist, int *form_ran) {
    SG_ENTER();
    SG_REQUIRE(form_ran && n >= 0 && (keys || n == 0), "debug_sort: null argument or negative n");
    SG_REQUIRE(begin_bit >= 0 && begin_bit < end_bit && end_bit <= 64 && (end_bit - begin_bit) % 8 == 0, "debug_sort: [begin_bit, end_bit) must be a multiple of 8 bits inside [0, 64)");
    SG_REQUIRE(form >= 0 && form <= 2, "debug_sort: form is 0 (a launch per step), 1 (one launch if it fits) or 2 (one launch where the library chooses it)");
    hipStream_t st = ctx().stream;
    Scratch keys_tmp, vals_tmp, hist;
    SG_TRY(keys_tmp.alloc((size_t)n * sizeof(u64)));
    if (vals) SG_TRY(vals_tmp.alloc((size_t)n * sizeof(u32)));
    u32 *first_hist = nullptr;
    if (with_first_hist) {                                               // as a caller does whose own kernel reads the keys anyway
        const i64 n_tiles = (n + RS_TILE - 1) / RS_TILE;
        SG_TRY(hist.alloc((size_t)n_tiles * 256 * sizeof(u32)));
        first_hist = hist.as<u32>();
        if (n_tiles) hipLaunchKernelGGL(k_rs_hist, dim3((unsigned)n_tiles), dim3(256), 0, st, keys, n, begin_bit, n_tiles, first_hist);
        KERNEL_CHECK();
    }
    const SortForm want = form == 0 ? SortForm::Launches : form == 1 ? SortForm::OneLaunchIfFits : SortForm::OneLaunchWherePays;
    SortResult res;
    SG_TRY(radix_sort({keys, keys_tmp.as<u64>(), vals, vals_tmp.as<u32>(), n, begin_bit, end_bit, first_hist, want}, &res));
    if (res.keys != keys) {
        HIP_TRY(hipMemcpyAsync(keys, res.keys, (size_t)n * sizeof(u64), hipMemcpyDeviceToDevice, st));
        if (vals) HIP_TRY(hipMemcpyAsync(vals, res.vals, (size_t)n * sizeof(u32), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *form_ran = res.one_launch ? 1 : 0;
    bool timed_out = false;
    if (res.one_launch) SG_TRY(radix_sort_coop_check(&timed_out));
    if (timed_out) { set_error("debug_sort: the one-launch sort gave up at a barrier; the buffers hold no sorted data"); return SYMGPU_E_HIP; }
    return SYMGPU_OK;
}

int symgpu_debug_scan(const uint32_t *in, uint32_t *out, int64_t n, uint32_t *total) {
    SG_ENTER();
    SG_REQUIRE(n >= 0 && ((in && out) || n == 0), "debug_scan: null argument or negative n");
    SG_TRY(exclusive_scan_u32(in, out, n, total));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

int symgpu_debug_popc_scan(const uint64_t *bits, int64_t n_words, int64_t n32, uint32_t *out, uint32_t *total) {
    SG_ENTER();
    SG_REQUIRE(bits && out && n_words >= 1 && n_words <= POPC_SCAN_SMALL_MAX, "debug_popc_scan: 1 to 8,192 words");
    SG_REQUIRE(n32 < 0 || n32 == 2 * n_words || n32 == 2 * n_words - 1, "debug_popc_scan: n32 is -1, 2 n_words or 2 n_words - 1");
    SG_TRY(popc_scan_small(bits, n_words, n32, out, total));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

}  // extern "C"
