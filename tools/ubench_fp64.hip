// ubench_fp64.hip — the FP64 fused-multiply-add rate the vector units reach: 16 independent chains a thread, nothing but v_fma_f64 in the
// loop.  tools/bench_rdm.py runs the binary and puts the figure beside the TILED form of csrc/rdm.hip.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_fp64.hip -o tools/ubench_fp64
// Prints one line: fp64_fma_tflops <best of 5 launches, 2 flops an fma>
#include <hip/hip_runtime.h>
#include <stdio.h>

#define CHECK(expr)                                                                  \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));               \
            return 1;                                                                \
        }                                                                            \
    } while (0)

constexpr int CHAINS = 16, ITERS = 4096, WG = 256;

__global__ __launch_bounds__(WG) void k_fma(double a, double b, double *out) {
    double v[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) v[c] = (double)(threadIdx.x + c);
    for (int it = 0; it < ITERS; ++it) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c) v[c] = __fma_rn(v[c], a, b);
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) s += v[c];
    if (s == 12345.678) out[0] = s;                  // never true for the arguments below: keeps the chains alive
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount * 8;
    double *out = nullptr;
    CHECK(hipMalloc(&out, 8));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    double best = 0.0;
    for (int rep = 0; rep < 6; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_fma, dim3(grid), dim3(WG), 0, 0, 0.999999, 1e-6, out);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        const double tflops = 2.0 * CHAINS * ITERS * (double)WG * grid / (ms * 1e-3) / 1e12;
        if (rep > 0 && tflops > best) best = tflops;
    }
    CHECK(hipFree(out));
    printf("fp64_fma_tflops %.2f\n", best);
    return 0;
}
