// scan.hip — device-wide exclusive scan (u32) in two forms, the one-launch population-count scan of a small bitmap, and the ordered sum.
#include "sort.h"
#include "block_scan.h"
#include <stdlib.h>

namespace symgpu {

// ------------------------------------------------------------------------------------------------
// exclusive scan (u32), 2048 elements per block, recursive over block sums
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;

__global__ __launch_bounds__(256) void k_scan_block(const u32 *__restrict__ in, u32 *__restrict__ out, i64 n, u32 *__restrict__ block_sums) {
    __shared__ u32 s_wave[4];
    const i64 base = (i64)blockIdx.x * SCAN_BLOCK + (i64)threadIdx.x * SCAN_ITEMS;
    u32 v[SCAN_ITEMS];
    u32 sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0u;
        sum += v[k];
    }
    u32 total;
    u32 excl = block_excl_scan_256(sum, s_wave, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = excl;
        excl += v[k];
    }
    if (threadIdx.x == 0 && block_sums) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_scan_add(u32 *__restrict__ out, i64 n, const u32 *__restrict__ block_offsets) {
    const i64 base = (i64)blockIdx.x * SCAN_BLOCK + (i64)threadIdx.x * SCAN_ITEMS;
    const u32 off = block_offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < n) out[base + k] += off;
}

__global__ void k_store_total(const u32 *__restrict__ last_in, const u32 *__restrict__ last_out, u32 *__restrict__ total) {
    *total = *last_in + *last_out;
}

// Two launches for up to 2^23 elements (every caller but the very largest): (1) block sums, the LAST workgroup to finish scans them
// (ticket; the sums travel write-through) and files the total, (2) every block scans its 2,048 elements on top of its offset.  The
// recursive form below (block scan, scan of the sums, add, plus a copy and a store for the total) was five or six launches of 4-6 us each
// around a few hundred KB of data.
constexpr int SCAN2_MAX_BLOCKS = 4096;
__global__ __launch_bounds__(256) void k_scan_sums(const u32 *__restrict__ in, i64 n, u32 *__restrict__ block_sums, u32 *__restrict__ total, u32 *__restrict__ ticket) {
    __shared__ u32 s_wave[4];
    __shared__ u32 s_last;
    const i64 base = (i64)blockIdx.x * SCAN_BLOCK + (i64)threadIdx.x * SCAN_ITEMS;
    u32 sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) sum += (base + k < n) ? in[base + k] : 0u;
    u32 tot;
    (void)block_excl_scan_256(sum, s_wave, &tot);
    if (threadIdx.x == 0) {
        __hip_atomic_store(block_sums + blockIdx.x, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    // exclusive scan of the block sums in place: sixteen per thread
    constexpr int PER = SCAN2_MAX_BLOCKS / 256;
    u32 v[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int b = threadIdx.x * PER + k;
        v[k] = b < (int)gridDim.x ? __hip_atomic_load(block_sums + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        mine += v[k];
    }
    u32 all;
    u32 excl = block_excl_scan_256(mine, s_wave, &all);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int b = threadIdx.x * PER + k;
        if (b < (int)gridDim.x) block_sums[b] = excl;
        excl += v[k];
    }
    if (threadIdx.x == 0) { if (total) *total = all; *ticket = 0; }
}
__global__ __launch_bounds__(256) void k_scan_final(const u32 *__restrict__ in, u32 *__restrict__ out, i64 n, const u32 *__restrict__ block_offsets) {
    __shared__ u32 s_wave[4];
    const i64 base = (i64)blockIdx.x * SCAN_BLOCK + (i64)threadIdx.x * SCAN_ITEMS;
    const u32 off = block_offsets[blockIdx.x];
    u32 v[SCAN_ITEMS];
    u32 sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0u;
        sum += v[k];
    }
    u32 total;
    u32 excl = off + block_excl_scan_256(sum, s_wave, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = excl;
        excl += v[k];
    }
}

// Population counts of the 64-bit words of a bitmap and their exclusive prefix in ONE launch, for bitmaps of up to 2^13 words (512K bits):
// the count kernel + the two scan kernels are 5 us each on an idle queue, which is most of a small product's prefix.  One workgroup of
// 1,024 lanes, a lane takes up to eight consecutive words (loaded together).  n32 >= 0: the bitmap was written in 32-bit words, the upper
// half of the last 64-bit word is unwritten when n32 is odd.
__global__ __launch_bounds__(1024) void k_popc_scan_small(const u64 *__restrict__ bits, i64 n, i64 n32, u32 *__restrict__ out, u32 *__restrict__ total) {
    __shared__ u32 s_wave[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 b0 = (i64)threadIdx.x * 8;
    u32 cnt[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const i64 w = b0 + k;
        u64 b = w < n ? bits[w] : 0ULL;
        if (n32 >= 0 && w == n - 1 && (n32 & 1)) b &= 0xFFFFFFFFULL;
        cnt[k] = (u32)__popcll(b);
        sum += cnt[k];
    }
    const u32 incl = wave_incl_scan(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const u32 sv = s_wave[k];
        if (k < wave) off += sv;
        tot += sv;
    }
    u32 run = off + incl - sum;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (b0 + k < n) out[b0 + k] = run;
        run += cnt[k];
    }
    if (threadIdx.x == 0 && total) *total = tot;
}
int popc_scan_small(const u64 *bits, i64 n, i64 n32, u32 *out, u32 *total_dev) {
    hipLaunchKernelGGL(k_popc_scan_small, dim3(1), dim3(1024), 0, ctx().stream, bits, n, n32, out, total_dev);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// out may alias in.  total_dev (optional, device) receives the sum of all n inputs.
int exclusive_scan_u32(const u32 *in, u32 *out, i64 n, u32 *total_dev) {
    hipStream_t st = ctx().stream;
    if (n <= 0) {
        if (total_dev) HIP_TRY(hipMemsetAsync(total_dev, 0, sizeof(u32), st));
        return SYMGPU_OK;
    }
    const i64 nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const bool force_recursive = [] { const char *e = getenv("SYMGPU_SCAN_RECURSIVE"); return e && e[0] == '1'; }();     // tests: the form of the largest inputs
    if (nb <= SCAN2_MAX_BLOCKS && !force_recursive) {
        u32 *ticket;
        SG_TRY(sort_scan_ticket(&ticket));
        Scratch sums;
        SG_TRY(sums.alloc((size_t)nb * sizeof(u32)));
        hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(256), 0, st, in, n, sums.as<u32>(), total_dev, ticket + 1);
        hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(256), 0, st, in, out, n, sums.as<u32>());
        KERNEL_CHECK();
        return SYMGPU_OK;
    }
    Scratch last;   // keep in[n-1] before it is overwritten (aliasing) to form the total
    if (total_dev) {
        SG_TRY(last.alloc(sizeof(u32)));
        HIP_TRY(hipMemcpyAsync(last.p, in + (n - 1), sizeof(u32), hipMemcpyDeviceToDevice, st));
    }
    if (nb == 1) {
        hipLaunchKernelGGL(k_scan_block, dim3(1), dim3(256), 0, st, in, out, n, (u32 *)nullptr);
        KERNEL_CHECK();
    } else {
        Scratch sums;
        SG_TRY(sums.alloc((size_t)nb * sizeof(u32)));
        hipLaunchKernelGGL(k_scan_block, dim3((unsigned)nb), dim3(256), 0, st, in, out, n, sums.as<u32>());
        KERNEL_CHECK();
        SG_TRY(exclusive_scan_u32(sums.as<u32>(), sums.as<u32>(), nb, nullptr));
        hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(256), 0, st, out, n, sums.as<u32>());
        KERNEL_CHECK();
    }
    if (total_dev) {
        hipLaunchKernelGGL(k_store_total, dim3(1), dim3(1), 0, st, last.as<u32>(), out + (n - 1), total_dev);
        KERNEL_CHECK();
    }
    return SYMGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// ordered sum: 0 + v[0] + v[1] + ... in that order (the reference's `inner_product += ...` loops): one wavefront, 64 values per step
// through LDS, lane 0 adds
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ordered_sum(const f64x2 *__restrict__ v, i64 N, f64x2 *__restrict__ out) {
    __shared__ f64x2 s_p[2][64];
    const int lane = threadIdx.x;
    double re = 0.0, im = 0.0;
    int buf = 0;
    for (i64 base = 0; base < N; base += 64, buf ^= 1) {
        if (base + lane < N) s_p[buf][lane] = v[base + lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            const int m = (int)(N - base < 64 ? N - base : 64);
            for (int k = 0; k < m; ++k) { const f64x2 p = s_p[buf][k]; re = __dadd_rn(re, p.x); im = __dadd_rn(im, p.y); }
        }
    }
    if (lane == 0) *out = f64x2{re, im};
}

int ordered_sum_dev(const f64x2 *v, i64 N, f64x2 *out) {
    hipLaunchKernelGGL(k_ordered_sum, dim3(1), dim3(64), 0, ctx().stream, v, N, out);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
