// evolve.hip — out = sum_{k=0..K} c_k T_k(H~) psi, H~ = (H - centre) / half_width, T_k the Chebyshev polynomials: a polynomial of a Pauli
// sum H applied to a dense statevector without the matrix (symmer_amd/evolution/time_evolution.py evolve_state; the
// arithmetic of include/symgpu.h f11).  One launch per order k >= 1: the row sum of csrc/matvec.hip (matvec.h: one text) on T_{k-1}, and in
// the epilogue the three-term recurrence T_k = s_k (H T_{k-1} - centre T_{k-1}) - T_{k-2} and out += c_k T_k.  Beyond the gathered reads of
// T_{k-1} a row costs one read of T_{k-2}, one write of T_k, one read and one write of out.  Row b's thread alone touches element b of
// T_{k-2}, T_k and out, so T_k overwrites T_{k-2} in place (two scratch vectors for any K); psi is T_0 and is never written.  No atomics,
// no barrier across workgroups: the order k + 1 is the next launch on the stream.
#include "matvec.h"
#include <math.h>

namespace symgpu {

// the plain IEEE complex product of symgpu_matvec_apply: d the coefficient, v the amplitude
__device__ __forceinline__ f64x2 ch_mul(f64x2 d, f64x2 v) {
    return f64x2{__dsub_rn(__dmul_rn(d.x, v.x), __dmul_rn(d.y, v.y)), __dadd_rn(__dmul_rn(d.x, v.y), __dmul_rn(d.y, v.x))};
}

// K = 0: out = c_0 psi
__global__ __launch_bounds__(MV_TILE) void k_cheb_order0(int n, f64x2 c0, const f64x2 *__restrict__ psi, f64x2 *__restrict__ out) {
    const u64 b64 = (u64)blockIdx.x * MV_TILE + threadIdx.x;
    if (b64 >= ((u64)1 << n)) return;
    out[b64] = ch_mul(c0, psi[b64]);
}

// Order k >= 1.  v = T_{k-1} (gathered), u = T_{k-2} (null at k = 1), w = T_k (may be u; never v), first: k = 1, out starts as c0 v.
__global__ __launch_bounds__(MV_TILE) void k_cheb_step(MvTerms P, double centre, double s, f64x2 c0, f64x2 ck, int first, const f64x2 *__restrict__ v,
                                                       const f64x2 *u, f64x2 *w, f64x2 *__restrict__ out) {
    const u64 rows = (u64)1 << P.n;
    const u64 b64 = (u64)blockIdx.x * MV_TILE + threadIdx.x;
    if (b64 >= rows) return;
    const u32 b = (u32)b64;
    f64x2 acc = {0.0, 0.0};
    if (P.G > 0) {                                            // the row sum of k_mv_apply
        f64x2 xv = v[b ^ P.gx[0]];
        for (u32 g = 0; g < P.G; ++g) {
            const f64x2 x = xv;
            if (g + 1 < P.G) xv = v[b ^ P.gx[g + 1]];
            const f64x2 p = ch_mul(mv_group_sum(P, g, b), x);
            acc = g == 0 ? p : f64x2{__dadd_rn(acc.x, p.x), __dadd_rn(acc.y, p.y)};
        }
    }
    const f64x2 vb = v[b64];
    const f64x2 t = {__dsub_rn(acc.x, __dmul_rn(centre, vb.x)), __dsub_rn(acc.y, __dmul_rn(centre, vb.y))};
    f64x2 tk = {__dmul_rn(s, t.x), __dmul_rn(s, t.y)};
    if (u) {
        const f64x2 ub = u[b64];
        tk = f64x2{__dsub_rn(tk.x, ub.x), __dsub_rn(tk.y, ub.y)};
    }
    w[b64] = tk;
    const f64x2 o = first ? ch_mul(c0, vb) : out[b64];
    const f64x2 p = ch_mul(ck, tk);
    out[b64] = f64x2{__dadd_rn(o.x, p.x), __dadd_rn(o.y, p.y)};
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_cheb_apply(struct symgpu_matvec_s *plan, double centre, double half_width, const double *coef_host, int64_t K, const double *psi_dev,
                      double *out_dev, int *form) {
    SG_REQUIRE(plan, "cheb_apply: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (form) *form = 0;
    SG_REQUIRE(coef_host && psi_dev && out_dev && psi_dev != out_dev, "cheb_apply: coefficients, and psi and out as two device buffers");
    SG_REQUIRE(K >= 0, "cheb_apply: K >= 0");
    SG_REQUIRE(isfinite(half_width) && half_width > 0.0 && isfinite(centre), "cheb_apply: a finite centre and a finite half_width > 0");
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << plan->xg.n;
    SG_TRY(matvec_require_memory(2 * N * 16 + 4096, "the two Chebyshev vectors"));
    Scratch ta, tb;
    SG_TRY(ta.alloc((size_t)N * 16));
    SG_TRY(tb.alloc((size_t)N * 16));
    const f64x2 *psi = reinterpret_cast<const f64x2 *>(psi_dev);
    f64x2 *out = reinterpret_cast<f64x2 *>(out_dev);
    const f64x2 *c = reinterpret_cast<const f64x2 *>(coef_host);
    const dim3 grid(grid_each((i64)N, MV_TILE)), block(MV_TILE);
    const MvTerms P = mv_terms_of(plan);
    const double inv = 1.0 / half_width;
    if (K == 0) {
        hipLaunchKernelGGL(k_cheb_order0, grid, block, 0, st, plan->xg.n, c[0], psi, out);
        KERNEL_CHECK();
    }
    // T_{k-1} and T_{k-2} before order k: (psi, -), (ta, psi), (tb, ta), (ta, tb), ...; T_k goes where T_{k-2} is, once that is not psi
    const f64x2 *v = psi, *u = nullptr;
    for (i64 k = 1; k <= K; ++k) {
        f64x2 *w = k == 1 ? ta.as<f64x2>() : k == 2 ? tb.as<f64x2>() : const_cast<f64x2 *>(u);
        hipLaunchKernelGGL(k_cheb_step, grid, block, 0, st, P, centre, k == 1 ? inv : 2.0 * inv, c[0], c[k], k == 1 ? 1 : 0, v, u, w, out);
        KERNEL_CHECK();
        u = v;
        v = w;
    }
    if (form) *form = SYMGPU_CHEB_DIRECT;
    HIP_TRY(hipStreamSynchronize(st));
    return SYMGPU_OK;
}

}  // extern "C"
