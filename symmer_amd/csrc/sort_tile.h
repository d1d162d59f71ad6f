// sort_tile.h — one tile of one radix pass, shared by the scatter kernel of the launches per step (k_rs_scatter, sort.hip) and by the
// one-launch kernel (k_rs_coop, sort_coop.hip): a tile of 4096 elements is ranked with 64-wide wavefront ballots (one match mask per lane
// from 8 __ballot calls), staged through LDS in digit order and written out as contiguous per-digit runs.  Device code; the library is
// built without relocatable device code, so it lives in a header.  The kernels keep what differs between them: where the global base of a
// digit comes from, the tile order, the pass loop and the barriers.  MEM says how the tile's global memory is read and written.
#pragma once
#include "block_scan.h"

namespace symgpu {

constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = 256 * RS_ITEMS;   // 4096
constexpr int RS_WSEG = 64 * RS_ITEMS;    // keys per wave segment

// Plain: ordinary loads and stores (a kernel boundary separates the passes).  Agent: agent-scope relaxed (write-through / L1-bypassing:
// cdna_hip_programming.md Guideline 16) — what crosses workgroups INSIDE a launch, so that its barriers need no fences.
enum class TileMem { Plain, Agent };
template <TileMem MEM, typename T> __device__ __forceinline__ T tile_load(const T *p) {
    if (MEM == TileMem::Agent) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <TileMem MEM, typename T> __device__ __forceinline__ void tile_store(T *p, T v) {
    if (MEM == TileMem::Agent) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// the lanes of the wavefront that hold the same 8-bit digit as this lane (and are valid): per bit one sign-extended field, one
// compare for the ballot and one three-input op per mask half (m & ~(ballot ^ sel)); the plain `m &= bit ? bal : ~bal` compiled to
// 95 VALU instructions per key, this to 45
__device__ __forceinline__ u64 match_digit(u32 d, bool valid) {
    const u64 m0 = __ballot(valid);
    u32 lo = (u32)m0, hi = (u32)(m0 >> 32);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int sel = __builtin_amdgcn_sbfe((int)d, b, 1);                 // 0 or -1
        const u64 bal = __ballot(sel != 0);
        lo = __builtin_amdgcn_bitop3_b32(lo, (u32)bal, (u32)sel, 0x90);       // lo & ~(bal ^ sel)
        hi = __builtin_amdgcn_bitop3_b32(hi, (u32)(bal >> 32), (u32)sel, 0x90);
    }
    return ((u64)hi << 32) | lo;
}

// index of this lane's r-th element: a wavefront owns RS_WSEG consecutive elements of the tile, 64 at a time
__device__ __forceinline__ i64 tile_index(i64 tile_base, int r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return tile_base + (i64)wave * RS_WSEG + r * 64 + lane;
}

// The tile's keys (and values) into registers; invalid lanes hold the key ~0 and the value 0.
// all sixteen loads in flight before the first key is used: the wavefront fences of the ranking loop otherwise pin every load
// behind its own s_waitcnt vmcnt(0) — sixteen dependent round trips per tile (round 3: 331 -> see DESIGN §3.3 per pass at cfg3)
template <TileMem MEM, bool HAS_VALS>
__device__ __forceinline__ void tile_load_items(const u64 *__restrict__ keys, const u32 *__restrict__ vals, i64 tile_base, i64 n, u64 (&key)[RS_ITEMS],
                                                u32 (&val)[HAS_VALS ? RS_ITEMS : 1]) {
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const i64 idx = tile_index(tile_base, r);
        const bool valid = idx < n;
        key[r] = valid ? tile_load<MEM>(keys + idx) : ~0ULL;
        if (HAS_VALS) val[r] = valid ? tile_load<MEM>(vals + idx) : 0u;
    }
    asm volatile("" : "+v"(key[0]), "+v"(key[1]), "+v"(key[2]), "+v"(key[3]), "+v"(key[4]), "+v"(key[5]), "+v"(key[6]), "+v"(key[7]));
    asm volatile("" : "+v"(key[8]), "+v"(key[9]), "+v"(key[10]), "+v"(key[11]), "+v"(key[12]), "+v"(key[13]), "+v"(key[14]), "+v"(key[15]));
    static_assert(RS_ITEMS == 16, "the two statements above name sixteen keys");
}

// pos[r] = rank of this lane's r-th key among the keys of its digit in its wavefront's segment (invalid lanes: unused); on return
// s_cnt[w][d] = keys of digit d in wavefront w's segment.  s_cnt must be zero on entry, for all wavefronts.
__device__ __forceinline__ void tile_rank(const u64 (&key)[RS_ITEMS], int shift, i64 tile_base, i64 n, u32 (&s_cnt)[4][256], u32 (&pos)[RS_ITEMS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 lt_mask = (1ULL << lane) - 1ULL;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const bool valid = tile_index(tile_base, r) < n;
        const u32 d = (u32)(key[r] >> shift) & 255u;
        const u64 m = match_digit(d, valid);
        const u32 rank = __popcll(m & lt_mask);
        const u32 count = __popcll(m);
        u32 base = 0;
        if (valid) base = s_cnt[wave][d];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) s_cnt[wave][d] = base + count;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        pos[r] = base + rank;
    }
}

// per digit (thread d): exclusive offsets over the wavefronts in s_cnt, exclusive scan over the digits in s_dig_off; returns the tile's
// count of digit d.  Between two __syncthreads of the caller's; has two of its own.
__device__ __forceinline__ u32 tile_digit_offsets(u32 (&s_cnt)[4][256], u32 (&s_dig_off)[256], u32 (&s_wave)[4]) {
    const int d = threadIdx.x;
    u32 run = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u32 c = s_cnt[k][d];
        s_cnt[k][d] = run;
        run += c;
    }
    u32 total;
    s_dig_off[d] = block_excl_scan_256(run, s_wave, &total);
    return run;
}

// the tile in digit order in LDS: slot = digit's offset in the tile + wavefront's offset in the digit + rank in the wavefront
template <bool HAS_VALS>
__device__ __forceinline__ void tile_stage(const u64 (&key)[RS_ITEMS], const u32 (&val)[HAS_VALS ? RS_ITEMS : 1], const u32 (&pos)[RS_ITEMS], int shift, i64 tile_base, i64 n,
                                           const u32 (&s_dig_off)[256], const u32 (&s_cnt)[4][256], u64 (&s_key)[RS_TILE], u32 (&s_val)[HAS_VALS ? RS_TILE : 1]) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        if (tile_index(tile_base, r) < n) {
            const u32 d = (u32)(key[r] >> shift) & 255u;
            const u32 slot = s_dig_off[d] + s_cnt[wave][d] + pos[r];
            s_key[slot] = key[r];
            if (HAS_VALS) s_val[slot] = val[r];
        }
    }
}

// the staged tile to its places: digit d's run goes to s_gbase[d] .., consecutive threads write consecutive elements of a run
template <TileMem MEM, bool HAS_VALS>
__device__ __forceinline__ void tile_write_runs(const u64 (&s_key)[RS_TILE], const u32 (&s_val)[HAS_VALS ? RS_TILE : 1], int shift, i64 tile_base, i64 n, const u32 (&s_dig_off)[256],
                                                const u32 (&s_gbase)[256], u64 *__restrict__ out_keys, u32 *__restrict__ out_vals) {
    const i64 n_valid = (n - tile_base < RS_TILE) ? (n - tile_base) : RS_TILE;
#pragma unroll 4
    for (int k = 0; k < RS_ITEMS; ++k) {
        const int s = k * 256 + threadIdx.x;
        if (s < n_valid) {
            const u64 kk = s_key[s];
            const u32 d = (u32)(kk >> shift) & 255u;
            const i64 g = (i64)s_gbase[d] + (s - (int)s_dig_off[d]);
            tile_store<MEM>(out_keys + g, kk);
            if (HAS_VALS) tile_store<MEM>(out_vals + g, s_val[s]);
        }
    }
}

}  // namespace symgpu
