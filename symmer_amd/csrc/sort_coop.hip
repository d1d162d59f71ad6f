// sort_coop.hip — the radix sort of sort.hip as ONE persistent launch, what the scans and the sort keep on a device between calls
// (SortState, common.h), and the protocol by which a launch that could not finish says so.
//
// Up to SORT_ONE_LAUNCH_MAX_TILES tiles: at 10^5 keys a pass of the multi-launch form is four or five launches of a few microseconds
// each — launch bound (26 us per pass); here the passes are separated by two counter barriers each.  Everything that crosses workgroups
// (keys, tile histograms, the barrier counter) moves through agent-scope relaxed loads and stores (write-through / L1-bypassing:
// cdna_hip_programming.md Guideline 16), so the barriers need no fences.  The workgroups must be co-resident: <= SORT_ONE_LAUNCH_MAX_TILES
// blocks of 256 threads and 35 KB of LDS (54 KB with values).
#include "sort.h"
#include "sort_tile.h"

namespace symgpu {

typedef int32_t i32;

// returns false if the other workgroups did not arrive within ~2^22 polls (not co-resident): the caller's kernel gives up, bar[1] says so
__device__ __forceinline__ bool coop_barrier(u32 *bar, u32 target, int G, u32 *s_flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                            // this wavefront's write-through stores have left
    __syncthreads();
    if (G > 1 && threadIdx.x == 0) {
        atomicAdd(bar, 1u);
        u32 ok = 1;
        for (u32 spin = 0; (i32)(__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0; ++spin) {
            if (spin >= (1u << 22) || __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { ok = 0; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!ok) __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_flag = ok;
    }
    __syncthreads();
    return G == 1 || *s_flag != 0;
}

// HAS_VALS: a 32-bit value travels with every key (round 6: the index sort of a plain cleanup — `A + B`, `cleanup()` — of up to 5e5 rows:
// three passes were nine launches, launch bound)
template <bool HAS_VALS>
__global__ __launch_bounds__(256) void k_rs_coop(u64 *__restrict__ buf_a, u64 *__restrict__ buf_b, u32 *__restrict__ val_a, u32 *__restrict__ val_b, i64 n, int begin_bit,
                                                  int n_passes, u32 *__restrict__ tile_hist /* [256][G] */, u32 *__restrict__ bar, u32 bar_base) {
    __shared__ u64 s_key[RS_TILE];
    __shared__ u32 s_val[HAS_VALS ? RS_TILE : 1];
    __shared__ u32 s_cnt[4][256];                           // see k_rs_scatter: plain LDS accesses ordered by wavefront-scope fences
    __shared__ u32 s_dig_off[256];
    __shared__ u32 s_gbase[256];
    __shared__ u32 s_wave[4];
    __shared__ u32 s_ok;
    const int G = gridDim.x, tile = blockIdx.x;
    const i64 tile_base = (i64)tile * RS_TILE;
    u32 n_bar = 0;
    for (int p = 0; p < n_passes; ++p) {
        const int shift = begin_bit + 8 * p;
        const u64 *src = (p & 1) ? buf_b : buf_a;
        u64 *dst = (p & 1) ? buf_a : buf_b;
        const u32 *vsrc = (p & 1) ? val_b : val_a;
        u32 *vdst = (p & 1) ? val_a : val_b;
#pragma unroll
        for (int k = 0; k < 4; ++k) s_cnt[k][threadIdx.x] = 0;
        __syncthreads();
        u64 key[RS_ITEMS];
        u32 pos[RS_ITEMS], val[HAS_VALS ? RS_ITEMS : 1];
        tile_load_items<TileMem::Agent, HAS_VALS>(src, vsrc, tile_base, n, key, val);
        tile_rank(key, shift, tile_base, n, s_cnt, pos);
        __syncthreads();
        // per digit: exclusive offsets over the wavefronts, the tile's count (filed for the other workgroups), exclusive scan over the digits
        const u32 my_count = tile_digit_offsets(s_cnt, s_dig_off, s_wave);
        __hip_atomic_store(&tile_hist[(i64)threadIdx.x * G + tile], my_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!coop_barrier(bar, bar_base + (u32)G * (++n_bar), G, &s_ok)) return;
        {   // global base of every digit for this tile: keys of smaller digits (all tiles) + keys of this digit in earlier tiles
            const int d = threadIdx.x;
            u32 all = 0, before = 0;
            if (G == 1) all = my_count;
            else
                for (int t0 = 0; t0 < G; t0 += 16) {                           // sixteen independent loads per round
                    u32 x[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        x[k] = t0 + k < G ? __hip_atomic_load(&tile_hist[(i64)d * G + t0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                    asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
                    asm volatile("" : "+v"(x[8]), "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15]));
#pragma unroll
                    for (int k = 0; k < 16; ++k) { all += x[k]; if (t0 + k < tile) before += x[k]; }
                }
            u32 total;
            s_gbase[d] = block_excl_scan_256(all, s_wave, &total) + before;
        }
        __syncthreads();
        tile_stage<HAS_VALS>(key, val, pos, shift, tile_base, n, s_dig_off, s_cnt, s_key, s_val);
        __syncthreads();
        tile_write_runs<TileMem::Agent, HAS_VALS>(s_key, s_val, shift, tile_base, n, s_dig_off, s_gbase, dst, vdst);
        if (!coop_barrier(bar, bar_base + (u32)G * (++n_bar), G, &s_ok)) return;
    }
}

// the one-launch form of radix_sort (n > 1, and sort_form has said that it applies): queued on the stream, the result is where the pass
// count puts it
int sort_one_launch(const SortRequest &rq) {
    Context &c = ctx();
    SortState &s = c.sort;
    hipStream_t st = c.stream;
    const i64 n_tiles = (rq.n + RS_TILE - 1) / RS_TILE;
    // s.coop_state: [0] barrier counter (monotonic over the launches; cleared before it can wrap), [1] time-out flag, [64 ..] tile histograms
    if (!s.coop_state) {
        HIP_TRY(hipMalloc((void **)&s.coop_state, (64 + 256 * SORT_ONE_LAUNCH_MAX_TILES) * sizeof(u32)));
        HIP_TRY(hipMemsetAsync(s.coop_state, 0, 64 * sizeof(u32), st));
        s.bar_base = 0;
    }
    const int n_passes = (rq.end_bit - rq.begin_bit + 7) / 8;
    const u32 arrivals = (u32)n_tiles * 2u * (u32)n_passes;
    if (s.bar_base > 0x70000000u - arrivals) {
        HIP_TRY(hipMemsetAsync(s.coop_state, 0, 64 * sizeof(u32), st));
        s.bar_base = 0;
    }
    if (rq.vals)
        hipLaunchKernelGGL((k_rs_coop<true>), dim3((unsigned)n_tiles), dim3(256), 0, st, rq.keys, rq.keys_tmp, rq.vals, rq.vals_tmp, rq.n, rq.begin_bit, n_passes, s.coop_state + 64,
                           s.coop_state, s.bar_base);
    else
        hipLaunchKernelGGL((k_rs_coop<false>), dim3((unsigned)n_tiles), dim3(256), 0, st, rq.keys, rq.keys_tmp, (u32 *)nullptr, (u32 *)nullptr, rq.n, rq.begin_bit, n_passes,
                           s.coop_state + 64, s.coop_state, s.bar_base);
    KERNEL_CHECK();
    s.bar_base += n_tiles > 1 ? arrivals : 0u;
    return SYMGPU_OK;
}

// ---- SortState ---------------------------------------------------------------------------------------------------------------------
int sort_scan_ticket(u32 **ticket) {
    Context &c = ctx();
    if (!c.sort.scan_ticket) {
        HIP_TRY(hipMalloc((void **)&c.sort.scan_ticket, 256));
        HIP_TRY(hipMemsetAsync(c.sort.scan_ticket, 0, 256, c.stream));
    }
    *ticket = c.sort.scan_ticket;
    return SYMGPU_OK;
}
void sort_state_release(SortState &s) {
    if (s.coop_state) (void)hipFree(s.coop_state);
    if (s.scan_ticket) (void)hipFree(s.scan_ticket);
    s = SortState();
}

// ---- the give-up protocol (contracts: sort.h) --------------------------------------------------------------------------------------
const u32 *radix_sort_coop_flag() {
    const SortState &s = ctx().sort;
    return (!s.coop_state || s.coop_disabled) ? nullptr : s.coop_state + 1;
}
void radix_sort_coop_note(u32 flag, bool *timed_out) {
    *timed_out = false;
    if (!flag) return;
    *timed_out = true;
    ctx().sort.coop_disabled = true;
    note_degraded("one-launch radix sort (k_rs_coop) off: an in-kernel barrier timed out (workgroups not co-resident?); sorts take one launch per pass");
}
int radix_sort_coop_check(bool *timed_out) {
    *timed_out = false;
    const u32 *p = radix_sort_coop_flag();
    if (!p) return SYMGPU_OK;
    u32 flag = 0;
    HIP_TRY(hipMemcpy(&flag, p, 4, hipMemcpyDeviceToHost));
    radix_sort_coop_note(flag, timed_out);
    return SYMGPU_OK;
}

}  // namespace symgpu
