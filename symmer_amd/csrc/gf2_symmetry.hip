// gf2_symmetry.hip — the symmetry-generator kernel (IndependentOp.symmetry_generators, symmer/operators/independent_op.py:124-126):
// build the stacked matrix on the device, reduce it (rref_dev, gf2.hip) and read the generators out.
#include "common.h"
#include "sort.h"

namespace symgpu {

// ---- symmetry-generator matrix build / read-out ----------------------------------------------------
// mat is (2n) x Wc, Wc = Wm + 2*Wq, Wm = ceil(M/64):  row c < n  = [ Z[:,c] | e_c ],  row n+c = [ X[:,c] | e_{n+c} ]
// (the transpose of independent_op.py:124's  vstack([hstack([Z, X]), eye(2n)])  with zero padding columns,
// which can never become pivots).  One wave transposes a 64-term x 64-qubit bit tile with 64 ballots.
__global__ __launch_bounds__(256) void k_build_symmat(const u64 *__restrict__ H, i64 M, int n, int Wq, u64 *__restrict__ mat, i64 Wc) {
    const int lane = threadIdx.x & 63;
    const i64 tile = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);   // 64-term tile index
    const int sw = blockIdx.y;                                   // source word 0..2Wq-1
    const i64 n_tiles = (M + 63) / 64;
    if (tile >= n_tiles) return;
    const i64 t = tile * 64 + lane;
    const u64 word = (t < M) ? H[t * 2 * Wq + sw] : 0ULL;
    u64 mine = 0;
    for (int b = 0; b < 64; ++b) {
        const u64 m = __ballot((word >> b) & 1ULL);
        if (lane == b) mine = m;
    }
    const int q = 64 * (sw % Wq) + lane;
    if (q < n) {
        const i64 c = (sw >= Wq) ? q : (i64)n + q;   // Z words feed rows 0..n-1, X words rows n..2n-1
        mat[c * Wc + tile] = mine;
    }
}

__global__ void k_set_identity(u64 *__restrict__ mat, int n, int Wq, i64 Wc, i64 Wm) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 2 * n) return;
    const int q = c < n ? c : c - n;
    const i64 w = Wm + (c < n ? 0 : Wq) + q / 64;
    mat[(i64)c * Wc + w] |= 1ULL << (q % 64);
}

// flag[c] = 1 iff the first Wm words of row c are all zero (one wave per row)
__global__ __launch_bounds__(256) void k_rowzero_flags(const u64 *__restrict__ mat, i64 R, i64 Wc, i64 Wm, u32 *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    bool nz = false;
    for (i64 w = lane; w < Wm; w += 64) nz |= (mat[r * Wc + w] != 0);
    const u64 any = __ballot(nz);
    if (lane == 0) flag[r] = any ? 0u : 1u;
}

__global__ void k_copy_generators(const u64 *__restrict__ mat, i64 R, i64 Wc, i64 Wm, int W, const u32 *__restrict__ pos, u32 total,
                                  u64 *__restrict__ out) {
    const i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * W) return;
    const i64 r = idx / W;
    const int w = (int)(idx - r * W);
    const u32 p = pos[r];
    const u32 nxt = (r + 1 < R) ? pos[r + 1] : total;
    if (nxt == p + 1) out[(i64)p * W + w] = mat[r * Wc + Wm + w];
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_symmetry_kernel_dev(symgpu_op_t H, int n_qubits, uint64_t *out, int64_t capacity, int64_t *k, int64_t *xor_count) {
    SG_ENTER(H);
    SG_REQUIRE(H && k && n_qubits >= 1, "symmetry_kernel_dev");
    SG_REQUIRE((n_qubits + 63) / 64 == H->Wq, "symmetry_kernel_dev: n_qubits does not match Wq");
    hipStream_t st = ctx().stream;
    const int n = n_qubits, Wq = H->Wq, W = 2 * Wq;
    const i64 M = H->T, Wm = (M + 63) / 64, Wc = Wm + W, R = 2 * (i64)n;
    Scratch mat, flag, total, gens;
    SG_TRY(mat.alloc((size_t)R * Wc * 8));
    HIP_TRY(hipMemsetAsync(mat.p, 0, (size_t)R * Wc * 8, st));
    if (M > 0) {
        dim3 grid((unsigned)((Wm + 3) / 4), (unsigned)W);
        hipLaunchKernelGGL(k_build_symmat, grid, dim3(256), 0, st, H->rows, M, n, Wq, mat.as<u64>(), Wc);
        KERNEL_CHECK();
    }
    hipLaunchKernelGGL(k_set_identity, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, mat.as<u64>(), n, Wq, Wc, Wm);
    KERNEL_CHECK();
    SG_TRY(rref_dev(mat.as<u64>(), R, Wc, xor_count, nullptr));
    SG_TRY(flag.alloc((size_t)R * 4));
    SG_TRY(total.alloc(16));
    hipLaunchKernelGGL(k_rowzero_flags, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, mat.as<u64>(), R, Wc, Wm, flag.as<u32>());
    KERNEL_CHECK();
    SG_TRY(exclusive_scan_u32(flag.as<u32>(), flag.as<u32>(), R, total.as<u32>()));
    u32 kcount = 0;
    SG_TRY(read_back_words(total.as<u32>(), 1, nullptr, 0, &kcount));
    *k = kcount;
    if ((i64)kcount > capacity) {
        set_error("symmetry_kernel: capacity %lld < %u generators", (long long)capacity, kcount);
        return SYMGPU_E_CAPACITY;
    }
    if (kcount == 0) return SYMGPU_OK;
    SG_REQUIRE(out, "symmetry_kernel: null output");
    SG_TRY(gens.alloc((size_t)kcount * W * 8));
    hipLaunchKernelGGL(k_copy_generators, dim3((unsigned)((R * W + 255) / 256)), dim3(256), 0, st, mat.as<u64>(), R, Wc, Wm, W,
                       flag.as<u32>(), kcount, gens.as<u64>());
    KERNEL_CHECK();
    HIP_TRY(hipMemcpyAsync(out, gens.p, (size_t)kcount * W * 8, hipMemcpyDeviceToHost, st));
    count_d2h((size_t)kcount * W * 8);
    HIP_TRY(hipStreamSynchronize(st));
    return SYMGPU_OK;
}

int symgpu_symmetry_kernel(const uint64_t *H, int64_t M, int n_qubits, int Wq, uint64_t *out, int64_t capacity, int64_t *k,
                           int64_t *xor_count) {
    SG_ENTER();
    SG_REQUIRE(M >= 0 && n_qubits >= 1 && Wq == (n_qubits + 63) / 64 && k, "symmetry_kernel: sizes");
    SG_REQUIRE(H || M == 0, "symmetry_kernel: null input");
    OwnedOp op;
    SG_TRY(symgpu_op_upload(H, nullptr, M, Wq, op.slot()));
    return symgpu_symmetry_kernel_dev(op.op, n_qubits, out, capacity, k, xor_count);
}

}  // extern "C"
