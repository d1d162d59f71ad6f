// block_scan.h — wavefront and workgroup prefix sums of one value per thread, for kernels of 256 threads (device code; the library is built
// without relocatable device code, so shared device functions live in headers).
#pragma once
#include "common.h"

namespace symgpu {

__device__ __forceinline__ u32 wave_incl_scan(u32 v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        u32 n = __shfl_up(v, off);
        if (lane >= off) v += n;
    }
    return v;
}

// block-wide exclusive scan of one value per thread (256 threads); returns exclusive prefix, *total = block sum
__device__ __forceinline__ u32 block_excl_scan_256(u32 v, u32 *s_wave /* [4] */, u32 *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 incl = wave_incl_scan(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u32 s = s_wave[k];
        if (k < wave) off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return off + incl - v;
}

// block-wide compaction of one flag per thread (256 threads): returns the number of kept threads before this one (a kept thread's
// position among the kept), *count = kept threads of the block.  One ballot and its count below the lane per wavefront, four wavefronts
// through LDS.
__device__ __forceinline__ u32 block_compact_256(bool keep, u32 *s_wave /* [4] */, u32 *count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 ballot = __ballot(keep);
    const u32 before = __builtin_amdgcn_mbcnt_hi((u32)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((u32)ballot, 0u));
    if (lane == 0) s_wave[wave] = (u32)__popcll(ballot);
    __syncthreads();
    u32 wbase = 0, all = 0;
    for (int w = 0; w < 4; ++w) {
        const u32 c = s_wave[w];
        wbase += w < wave ? c : 0u;
        all += c;
    }
    __syncthreads();
    *count = all;
    return wbase + before;
}

}  // namespace symgpu
