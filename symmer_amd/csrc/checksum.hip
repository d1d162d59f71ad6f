// checksum.hip — sums that tests and benchmarks compare results by: byte sums and popcounts of device buffers, XOR fold and coefficient sum of an operator.
#include "common.h"

namespace symgpu {

constexpr size_t XOR_FOLD_MAX_LDS = 64 << 10;     // dynamic LDS of k_xor_fold: W * 8 bytes
__global__ void k_xor_fold(const u64 *__restrict__ rows, i64 T, int W, u64 *__restrict__ out) {
    // out[w] ^= XOR over rows; one block per grid-stride chunk, lanes over (row, word) pairs
    extern __shared__ u64 s_fold[];
    for (int w = threadIdx.x; w < W; w += blockDim.x) s_fold[w] = 0;
    __syncthreads();
    i64 total = T * (i64)W;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        int w = (int)(idx % W);
        atomicXor((unsigned long long *)&s_fold[w], (unsigned long long)rows[idx]);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < W; w += blockDim.x)
        if (s_fold[w]) atomicXor((unsigned long long *)&out[w], (unsigned long long)s_fold[w]);
}

__global__ void k_sum_f64x2(const double *__restrict__ c, i64 T, double *__restrict__ out) {
    double re = 0, im = 0;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        re += c[2 * t];
        im += c[2 * t + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
        re += __shfl_down(re, off);
        im += __shfl_down(im, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], re);
        atomicAdd(&out[1], im);
    }
}

__global__ void k_sum_u8(const uint8_t *__restrict__ p, i64 n, unsigned long long *__restrict__ out) {
    unsigned long long s = 0;
    i64 n16 = n / 16;
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (i64)gridDim.x * blockDim.x) {
        uint4 v = p4[i];
        // bytes are 0/1: popcount counts them
        s += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (i64 i = n16 * 16; i < n; ++i) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

__global__ void k_popc_u64(const u64 *__restrict__ p, i64 n, unsigned long long *__restrict__ out) {
    unsigned long long s = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) s += __popcll(p[i]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

static int reduce_to_host_u64(void (*launch)(const void *, i64, unsigned long long *, hipStream_t), const void *p, i64 n, uint64_t *sum) {
    Scratch acc;
    SG_TRY(acc.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(acc.p, 0, sizeof(unsigned long long), ctx().stream));
    launch(p, n, acc.as<unsigned long long>(), ctx().stream);
    KERNEL_CHECK();
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, acc.p, sizeof(h), hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    *sum = h;
    return SYMGPU_OK;
}

int symgpu_dev_checksum_u8(const uint8_t *dev, int64_t n, uint64_t *sum) {
    SG_ENTER();
    SG_REQUIRE(dev && sum && n >= 0, "dev_checksum_u8");
    SG_REQUIRE(((uintptr_t)dev & 15) == 0, "dev_checksum_u8: pointer must be 16-byte aligned");
    return reduce_to_host_u64([](const void *p, i64 n_, unsigned long long *o, hipStream_t s) {
        hipLaunchKernelGGL(k_sum_u8, dim3(2048), dim3(256), 0, s, (const uint8_t *)p, n_, o); }, dev, n, sum);
}

int symgpu_dev_popcount_u64(const uint64_t *dev, int64_t n_words, uint64_t *sum) {
    SG_ENTER();
    SG_REQUIRE(dev && sum && n_words >= 0, "dev_popcount_u64");
    return reduce_to_host_u64([](const void *p, i64 n_, unsigned long long *o, hipStream_t s) {
        hipLaunchKernelGGL(k_popc_u64, dim3(2048), dim3(256), 0, s, (const u64 *)p, n_, o); }, dev, n_words, sum);
}

int symgpu_op_popcount(symgpu_op_t op, uint64_t *sum) {
    SG_ENTER(op);
    SG_REQUIRE(op && sum, "op_popcount: null argument");
    if (op->T == 0) { *sum = 0; return SYMGPU_OK; }
    return symgpu_dev_popcount_u64(op->rows, op->T * 2 * op->Wq, sum);
}

int symgpu_op_checksum(symgpu_op_t op, uint64_t *xor_words, double *coeff_sum) {
    SG_ENTER(op);
    SG_REQUIRE(op, "op_checksum: null handle");
    int W = 2 * op->Wq;
    // k_xor_fold keeps one word per column in dynamic LDS: 64 KiB is what a workgroup gets without an attribute
    SG_REQUIRE(!xor_words || (size_t)W * sizeof(u64) <= XOR_FOLD_MAX_LDS, "op_checksum: rows of more than 8,192 words (Wq > 4,096) cannot be folded");
    Scratch acc;
    SG_TRY(acc.alloc((size_t)W * sizeof(u64) + 2 * sizeof(double)));
    HIP_TRY(hipMemsetAsync(acc.p, 0, (size_t)W * sizeof(u64) + 2 * sizeof(double), ctx().stream));
    u64 *dx = acc.as<u64>();
    double *dc = reinterpret_cast<double *>(dx + W);
    if (op->T > 0) {
        if (xor_words) {
            hipLaunchKernelGGL(k_xor_fold, dim3(1024), dim3(256), (size_t)W * sizeof(u64), ctx().stream, op->rows, op->T, W, dx);
            KERNEL_CHECK();
        }
        if (coeff_sum && op->coeff) {
            hipLaunchKernelGGL(k_sum_f64x2, dim3(1024), dim3(256), 0, ctx().stream, op->coeff, op->T, dc);
            KERNEL_CHECK();
        }
    }
    if (xor_words) HIP_TRY(hipMemcpyAsync(xor_words, dx, (size_t)W * sizeof(u64), hipMemcpyDeviceToHost, ctx().stream));
    if (coeff_sum) HIP_TRY(hipMemcpyAsync(coeff_sum, dc, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

}  // extern "C"
