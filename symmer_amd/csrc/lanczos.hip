// lanczos.hip — the vector kernels of the matrix-free eigen-iteration (symmer_amd/utils.py exact_gs_energy) on a resident
// basis of complex128 vectors of 2^n elements:
//   symgpu_lanczos_step   w = keep o (H v_j); alpha = Re<v_j, w>; w orthogonalised against v_0 .. v_j by classical Gram-Schmidt done twice;
//                         beta = |w|; v_{j+1} = w / beta
//   symgpu_vec_combine    out = sum_j s_j v_j (the Ritz vector; the restart when out is slot 0)
// Every reduction runs in one fixed two-level order (lz_chunk): the elements are cut into chunks of C = max(256, 2^n / 1024) consecutive
// elements; a workgroup of 256 threads takes one chunk of one inner product: thread t adds the products of elements t, t + 256, ... of the
// chunk to 0 in ascending order, then the 256 thread sums are folded in LDS by halving (s[t] += s[t + 128], then 64, ..., 1); one
// workgroup then adds the chunk sums of every inner product to 0 in ascending chunk order.  No floating-point atomics: the same input
// gives the same bits.  All j + 1 inner products of a Gram-Schmidt pass come from one launch over the basis, all subtractions from one.
#include "matvec.h"
#include <string.h>

namespace symgpu {

constexpr int LZ_WG = 256;

static u64 lz_chunk(u64 N) { return (N >> 10) > LZ_WG ? (N >> 10) : LZ_WG; }
unsigned lz_chunks(u64 N) { return (unsigned)((N + lz_chunk(N) - 1) / lz_chunk(N)); }

// partial[c * nvec + i] = sum over chunk c of conj(basis_i[b]) w[b]; blockIdx.x = chunk, blockIdx.y = i
__global__ __launch_bounds__(LZ_WG) void k_lz_dots(const f64x2 *basis, u64 N, u64 chunk, int nvec, const f64x2 *w, f64x2 *__restrict__ partial) {
    __shared__ f64x2 s[LZ_WG];
    const f64x2 *v = basis + (u64)blockIdx.y * N;
    const u64 b0 = (u64)blockIdx.x * chunk;
    const u64 b1 = b0 + chunk < N ? b0 + chunk : N;
    double re = 0.0, im = 0.0;
    for (u64 b = b0 + threadIdx.x; b < b1; b += LZ_WG) {
        const f64x2 a = v[b], c = w[b];
        re = __dadd_rn(re, __dadd_rn(__dmul_rn(a.x, c.x), __dmul_rn(a.y, c.y)));
        im = __dadd_rn(im, __dsub_rn(__dmul_rn(a.x, c.y), __dmul_rn(a.y, c.x)));
    }
    s[threadIdx.x] = f64x2{re, im};
    __syncthreads();
    for (int h = LZ_WG / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const f64x2 a = s[threadIdx.x], c = s[threadIdx.x + h];
            s[threadIdx.x] = f64x2{__dadd_rn(a.x, c.x), __dadd_rn(a.y, c.y)};
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(u64)blockIdx.x * nvec + blockIdx.y] = s[0];
}

// h[i] = 0 + partial[0][i] + partial[1][i] + ...; then scal[0] = Re h[alpha_of] (alpha_of >= 0), scal[1] = sqrt(Re h[0]) (norm != 0)
__global__ __launch_bounds__(LZ_WG) void k_lz_reduce(const f64x2 *__restrict__ partial, unsigned chunks, int nvec, f64x2 *__restrict__ h, int alpha_of, int norm,
                                                     double *__restrict__ scal) {
    for (int i = threadIdx.x; i < nvec; i += LZ_WG) {
        double re = 0.0, im = 0.0;
        for (unsigned c = 0; c < chunks; ++c) {
            const f64x2 p = partial[(u64)c * nvec + i];
            re = __dadd_rn(re, p.x);
            im = __dadd_rn(im, p.y);
        }
        h[i] = f64x2{re, im};
        if (i == alpha_of) scal[0] = re;
        if (norm && i == 0) scal[1] = __dsqrt_rn(re);
    }
}

// w[b] = ((w[b] - h_0 v_0[b]) - h_1 v_1[b]) - ...: plain IEEE complex products, in basis order
__global__ __launch_bounds__(LZ_WG) void k_lz_subtract(const f64x2 *__restrict__ basis, u64 N, int nvec, const f64x2 *__restrict__ h, f64x2 *__restrict__ w) {
    const u64 b = (u64)blockIdx.x * LZ_WG + threadIdx.x;
    if (b >= N) return;
    f64x2 a = w[b];
    for (int i = 0; i < nvec; ++i) {
        const f64x2 c = h[i], v = basis[(u64)i * N + b];
        a.x = __dsub_rn(a.x, __dsub_rn(__dmul_rn(c.x, v.x), __dmul_rn(c.y, v.y)));
        a.y = __dsub_rn(a.y, __dadd_rn(__dmul_rn(c.x, v.y), __dmul_rn(c.y, v.x)));
    }
    w[b] = a;
}

// out[b] = in[b] / scal[1], nothing if scal[1] is not positive; out may be in
__global__ __launch_bounds__(LZ_WG) void k_lz_scale(const f64x2 *in, u64 N, const double *__restrict__ scal, f64x2 *out) {
    const u64 b = (u64)blockIdx.x * LZ_WG + threadIdx.x;
    const double beta = scal[1];
    if (b >= N || !(beta > 0.0)) return;
    const f64x2 a = in[b];
    out[b] = f64x2{__ddiv_rn(a.x, beta), __ddiv_rn(a.y, beta)};
}

// out[b] = s_0 v_0[b] + s_1 v_1[b] + ... from the first product, in basis order; out may be a basis slot (each thread reads its element
// of every vector before it writes)
__global__ __launch_bounds__(LZ_WG) void k_lz_combine(const f64x2 *basis, u64 N, int m, const double *__restrict__ s, f64x2 *out) {
    const u64 b = (u64)blockIdx.x * LZ_WG + threadIdx.x;
    if (b >= N) return;
    f64x2 a = {0.0, 0.0};
    for (int j = 0; j < m; ++j) {
        const f64x2 v = basis[(u64)j * N + b];
        const f64x2 p = {__dmul_rn(s[j], v.x), __dmul_rn(s[j], v.y)};
        a = j == 0 ? p : f64x2{__dadd_rn(a.x, p.x), __dadd_rn(a.y, p.y)};
    }
    out[b] = a;
}

// the small device state of one call: chunk sums of up to nvec inner products, their totals h, {alpha, beta}
struct LzWork {
    Scratch partial, h, scal;
    int alloc(u64 N, int nvec) {
        SG_TRY(partial.alloc((size_t)lz_chunks(N) * nvec * 16));
        SG_TRY(h.alloc((size_t)nvec * 16));
        SG_TRY(scal.alloc(16));
        HIP_TRY(hipMemsetAsync(scal.p, 0, 16, ctx().stream));
        return SYMGPU_OK;
    }
};

// h[i] = <basis_i, w> for i < nvec, in the fixed order
static int lz_dots(LzWork &k, const f64x2 *basis, u64 N, int nvec, const f64x2 *w, int alpha_of, int norm) {
    hipStream_t st = ctx().stream;
    const unsigned chunks = lz_chunks(N);
    hipLaunchKernelGGL(k_lz_dots, dim3(chunks, (unsigned)nvec), dim3(LZ_WG), 0, st, basis, N, lz_chunk(N), nvec, w, k.partial.as<f64x2>());
    hipLaunchKernelGGL(k_lz_reduce, dim3(1), dim3(LZ_WG), 0, st, k.partial.as<f64x2>(), chunks, nvec, k.h.as<f64x2>(), alpha_of, norm, k.scal.as<double>());
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// *re_out = Re<v, w> in the fixed order (matvec.h): one inner product, the chunk sums in `partial`, the total in *h
int lz_inner(const f64x2 *v, const f64x2 *w, u64 N, f64x2 *partial, f64x2 *h, double *re_out) {
    hipStream_t st = ctx().stream;
    const unsigned chunks = lz_chunks(N);
    hipLaunchKernelGGL(k_lz_dots, dim3(chunks, 1u), dim3(LZ_WG), 0, st, v, N, lz_chunk(N), 1, w, partial);
    hipLaunchKernelGGL(k_lz_reduce, dim3(1), dim3(LZ_WG), 0, st, partial, chunks, 1, h, 0, 0, re_out);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_lanczos_step(struct symgpu_matvec_s *plan, const uint8_t *keep_dev, double *basis_dev, int64_t capacity, int64_t j, double *alpha, double *beta) {
    SG_REQUIRE(plan, "lanczos_step: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    SG_REQUIRE(basis_dev && alpha && beta, "lanczos_step: arguments");
    SG_REQUIRE(capacity >= 1 && capacity < ((i64)1 << 16) && j >= 0 && j < capacity, "lanczos_step: 0 <= j < capacity < 65536");
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << plan->xg.n;
    const int nvec = (int)j + 1;
    SG_TRY(matvec_require_memory(N * 16 + (u64)lz_chunks(N) * nvec * 16 + 4096, "a Lanczos step"));
    Scratch w;
    LzWork k;
    SG_TRY(w.alloc((size_t)N * 16));
    SG_TRY(k.alloc(N, nvec));
    f64x2 *basis = reinterpret_cast<f64x2 *>(basis_dev);
    SG_TRY(matvec_launch(plan, basis + (u64)j * N, w.as<f64x2>(), keep_dev, nullptr));
    const unsigned grid = grid_each((i64)N, LZ_WG);
    for (int pass = 0; pass < 2; ++pass) {                  // classical Gram-Schmidt, twice; alpha is <v_j, w> of the first pass
        SG_TRY(lz_dots(k, basis, N, nvec, w.as<f64x2>(), pass == 0 ? (int)j : -1, 0));
        hipLaunchKernelGGL(k_lz_subtract, dim3(grid), dim3(LZ_WG), 0, st, basis, N, nvec, k.h.as<f64x2>(), w.as<f64x2>());
        KERNEL_CHECK();
    }
    SG_TRY(lz_dots(k, w.as<f64x2>(), N, 1, w.as<f64x2>(), -1, 1));
    if (j + 1 < capacity) {
        hipLaunchKernelGGL(k_lz_scale, dim3(grid), dim3(LZ_WG), 0, st, w.as<f64x2>(), N, k.scal.as<double>(), basis + (u64)(j + 1) * N);
        KERNEL_CHECK();
    }
    u32 words[4] = {0, 0, 0, 0};
    SG_TRY(read_back_words(k.scal.as<u32>(), 4, nullptr, 0, words));
    memcpy(alpha, words, 8);
    memcpy(beta, words + 2, 8);
    return SYMGPU_OK;
}

int symgpu_vec_combine(const double *basis_dev, int64_t m, int n_qubits, const double *s_host, double *out_dev, int normalise) {
    SG_ENTER();
    SG_REQUIRE(basis_dev && s_host && out_dev, "vec_combine: arguments");
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32 && m >= 1 && m < ((i64)1 << 16), "vec_combine: 1 <= n_qubits <= 32, 1 <= m < 65536");
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << n_qubits;
    SG_TRY(matvec_require_memory((u64)m * 8 + (u64)lz_chunks(N) * 16 + 4096, "the Ritz combination"));
    Scratch s;
    LzWork k;
    SG_TRY(s.alloc((size_t)m * 8));
    SG_TRY(k.alloc(N, 1));
    SG_TRY(symgpu_dev_upload(s.p, s_host, m * 8));
    const unsigned grid = grid_each((i64)N, LZ_WG);
    f64x2 *out = reinterpret_cast<f64x2 *>(out_dev);
    hipLaunchKernelGGL(k_lz_combine, dim3(grid), dim3(LZ_WG), 0, st, reinterpret_cast<const f64x2 *>(basis_dev), N, (int)m, s.as<double>(), out);
    KERNEL_CHECK();
    if (normalise) {
        SG_TRY(lz_dots(k, out, N, 1, out, -1, 1));
        hipLaunchKernelGGL(k_lz_scale, dim3(grid), dim3(LZ_WG), 0, st, out, N, k.scal.as<double>(), out);
        KERNEL_CHECK();
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SYMGPU_OK;
}

}  // extern "C"
