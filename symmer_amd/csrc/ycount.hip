// ycount.hip — Y_count |x & z| of every row (reference: symmer/operators/base.py:604-615): the cached per-operator counts of layout.hip
// (op_ycount: the product's coefficient expansion) and the host entry point.
#include "common.h"
#include <stdlib.h>

namespace symgpu {

// Y_count: one lane group per row on row-major packed rows (tiny, O(T*Wq))
__global__ void k_ycount(const u64 *__restrict__ rows, i64 T, int Wq, int *__restrict__ out) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        const u64 *r = rows + t * 2 * Wq;
        int c = 0;
        for (int w = 0; w < Wq; ++w) c += __popcll(r[w] & r[Wq + w]);
        out[t] = c;
    }
}

// long rows: one block per row, the words spread over its threads (one thread walking 1.5 million words took 0.2 s)
__global__ __launch_bounds__(256) void k_ycount_long(const u64 *__restrict__ rows, i64 t_base, int Wq, int *__restrict__ out) {
    __shared__ int red[4];
    const i64 t = t_base + blockIdx.x;
    const u64 *r = rows + t * 2 * Wq;
    int c = 0;
    for (int w = threadIdx.x; w < Wq; w += 256) c += __popcll(r[w] & r[Wq + w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[t] = red[0] + red[1] + red[2] + red[3];
}

int ycount_dev(const u64 *rows, i64 T, int Wq, int *out) {
    if (T == 0) return SYMGPU_OK;
    if (Wq >= 512) {
        for (i64 t0 = 0; t0 < T; t0 += 0x7fffffff) {
            const i64 nt = T - t0 < 0x7fffffff ? T - t0 : 0x7fffffff;
            hipLaunchKernelGGL(k_ycount_long, dim3((unsigned)nt), dim3(256), 0, ctx().stream, rows, t0, Wq, out);
            KERNEL_CHECK();
        }
        return SYMGPU_OK;
    }
    int grid = (int)((T + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_ycount, dim3(grid), dim3(256), 0, ctx().stream, rows, T, Wq, out);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_ycount(const uint64_t *rows, int64_t T, int Wq, int64_t *out) {
    SG_ENTER();
    SG_REQUIRE(T >= 0 && Wq >= 1 && (T == 0 || (rows && out)), "ycount");
    if (T == 0) return SYMGPU_OK;
    Scratch d, o;
    SG_TRY(d.alloc((size_t)T * 2 * Wq * sizeof(u64)));
    SG_TRY(o.alloc((size_t)T * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(d.p, rows, (size_t)T * 2 * Wq * sizeof(u64), hipMemcpyHostToDevice, ctx().stream));
    count_h2d((size_t)T * 2 * Wq * sizeof(u64)); count_d2h((size_t)T * sizeof(int));
    SG_TRY(ycount_dev(d.as<u64>(), T, Wq, o.as<int>()));
    int *h = (int *)malloc((size_t)T * sizeof(int));
    if (!h) { set_error("host allocation failed"); return SYMGPU_E_NOMEM; }
    hipError_t e = hipMemcpyAsync(h, o.p, (size_t)T * sizeof(int), hipMemcpyDeviceToHost, ctx().stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) { free(h); return hip_fail(e, "ycount download", __FILE__, __LINE__); }
    for (i64 t = 0; t < T; ++t) out[t] = h[t];
    free(h);
    return SYMGPU_OK;
}

}  // extern "C"
