// matvec.hip — y = H x for a Pauli sum H and a dense statevector x, without the matrix (conventions of sparse_matrix.hip):
//   y[b] = sum over the groups g of equal X-part, in ascending x_g, of  D_g(b) x[b ^ x_g],
//   D_g(b) = sum over the terms k of g, in operator order, of  c_k (-i)^{Y_k} (-1)^{|b & z_k|}
// qubit 0 the MOST significant bit of b, x_k, z_k.  Plan: the terms grouped by X-part (xgroups.h), which to_sparse_matrix sums over as
// well: per sorted term z and c', per group x and its first term.  Apply: one thread per row,
// the terms read through wave-uniform addresses (scalar loads, every lane the same term), the sign from the parity of b & z, D_g summed
// from its first term, one gathered read of x per group — the 64 rows of a wavefront read 64 consecutive elements in a permuted order,
// 1 KiB in whole — one plain IEEE complex product, the row's sum started from its first group.  The next group's element is requested
// before the current group's terms are summed.  No atomics: a row belongs to one thread.
#include "matvec.h"
#include <memory>

namespace symgpu {

// ---- y = keep o (H x): MvTerms, mv_signed and mv_group_sum are in matvec.h, shared with evolve.hip -------------------------------------
__global__ __launch_bounds__(MV_TILE) void k_mv_apply(MvTerms P, const f64x2 *__restrict__ x, f64x2 *__restrict__ y, const uint8_t *__restrict__ keep) {
    const u64 rows = (u64)1 << P.n;
    const u64 b64 = (u64)blockIdx.x * MV_TILE + threadIdx.x;
    if (b64 >= rows) return;
    const u32 b = (u32)b64;
    f64x2 acc = {0.0, 0.0};
    if (P.G > 0 && (!keep || keep[b64])) {
        f64x2 xv = x[b ^ P.gx[0]];
        for (u32 g = 0; g < P.G; ++g) {
            const f64x2 v = xv;
            if (g + 1 < P.G) xv = x[b ^ P.gx[g + 1]];
            const f64x2 d = mv_group_sum(P, g, b);
            const f64x2 p = {__dsub_rn(__dmul_rn(d.x, v.x), __dmul_rn(d.y, v.y)), __dadd_rn(__dmul_rn(d.x, v.y), __dmul_rn(d.y, v.x))};
            acc = g == 0 ? p : f64x2{__dadd_rn(acc.x, p.x), __dadd_rn(acc.y, p.y)};
        }
    }
    y[b64] = acc;
}

// keep[b] = the nearest integer to Re D_0(b) equals n_particles; the kept rows counted per workgroup, then one integer atomic each
__global__ __launch_bounds__(256) void k_mv_sector(MvTerms P, long long n_particles, uint8_t *__restrict__ keep, unsigned long long *__restrict__ n_kept) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u64 rows = (u64)1 << P.n;
    const u64 b64 = (u64)blockIdx.x * 256 + threadIdx.x;
    if (b64 < rows) {
        const double d = P.G > 0 ? mv_group_sum(P, 0, (u32)b64).x : 0.0;
        const bool k = rint(d) == (double)n_particles;
        keep[b64] = k ? 1 : 0;
        if (k) atomicAdd(&s_cnt, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(n_kept, (unsigned long long)s_cnt);
}

int matvec_require_memory(u64 bytes, const char *what) {
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (bytes > f) {
        dev_cache_release();
        HIP_TRY(hipMemGetInfo(&f, &t));
    }
    if (bytes > f) {
        set_error("matvec: %s needs %.2f GiB on the device, %.2f GiB free", what, (double)bytes / 1073741824.0, (double)f / 1073741824.0);
        return SYMGPU_E_NOMEM;
    }
    return SYMGPU_OK;
}

int matvec_launch(const symgpu_matvec_s *p, const f64x2 *x, f64x2 *y, const uint8_t *keep, int *form) {
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << p->xg.n;
    if (form) *form = 0;
    if (p->xg.G == 0) {
        HIP_TRY(hipMemsetAsync(y, 0, (size_t)N * 16, st));
        return SYMGPU_OK;
    }
    hipLaunchKernelGGL(k_mv_apply, dim3(grid_each((i64)N, MV_TILE)), dim3(MV_TILE), 0, st, mv_terms_of(p), x, y, keep);
    KERNEL_CHECK();
    if (form) *form = SYMGPU_MATVEC_DIRECT;
    return SYMGPU_OK;
}

static int mv_plan(symgpu_op_t op, int n, symgpu_matvec_s *p) {
    const i64 T = op->T;
    // the sort's buffers (keys, indices, both twice; heads, scan) and the plan's own (z, c', and at most T groups)
    if (T > 0) SG_TRY(matvec_require_memory((u64)T * (8 + 8 + 4 + 4 + 4 + 4 + 4 + 16 + 4 + 4) + 4096, "the plan"));
    SG_TRY(xgroups_build(op, n, false, &p->xg));
    if (T > 0) HIP_TRY(hipStreamSynchronize(ctx().stream));   // the operator and the scratch are not referenced once the call has returned
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_matvec_plan(symgpu_op_t op, int n_qubits, struct symgpu_matvec_s **plan) {
    SG_ENTER(op);
    SG_REQUIRE(op && plan, "matvec_plan: arguments");
    *plan = nullptr;
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32, "matvec_plan: 1 <= n_qubits <= 32");
    SG_REQUIRE(op->Wq == 1, "matvec_plan: the operator's rows have more than one word per half (Wq = 1 wanted)");
    SG_REQUIRE(op->coeff || op->T == 0, "matvec_plan: operator has no coefficients");
    SG_REQUIRE(op->T < ((i64)1 << 31), "matvec_plan: T >= 2^31");
    std::unique_ptr<symgpu_matvec_s> p(new symgpu_matvec_s());
    p->device = op->device;
    SG_TRY(mv_plan(op, n_qubits, p.get()));
    *plan = p.release();
    return SYMGPU_OK;
}

int symgpu_matvec_free(struct symgpu_matvec_s *plan) {
    SG_REQUIRE(plan, "matvec_free: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    delete plan;
    return SYMGPU_OK;
}

int symgpu_matvec_info(struct symgpu_matvec_s *plan, int *n_qubits, int64_t *n_terms, int64_t *n_groups, int64_t *device_bytes) {
    SG_REQUIRE(plan, "matvec_info: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (n_qubits) *n_qubits = plan->xg.n;
    if (n_terms) *n_terms = plan->xg.T;
    if (n_groups) *n_groups = plan->xg.G;
    if (device_bytes) *device_bytes = plan->xg.device_bytes();
    return SYMGPU_OK;
}

int symgpu_matvec_apply(struct symgpu_matvec_s *plan, const double *x_dev, double *y_dev, int *form) {
    SG_REQUIRE(plan, "matvec_apply: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (form) *form = 0;
    SG_REQUIRE(x_dev && y_dev && x_dev != y_dev, "matvec_apply: x and y must be two device buffers");
    SG_TRY(matvec_launch(plan, reinterpret_cast<const f64x2 *>(x_dev), reinterpret_cast<f64x2 *>(y_dev), nullptr, form));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

int symgpu_matvec_sector_mask(struct symgpu_matvec_s *plan_N, int64_t n_particles, uint8_t *keep_dev, int64_t *n_kept) {
    SG_REQUIRE(plan_N, "matvec_sector_mask: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan_N->device);
    SG_ENTER(&scope_op);
    SG_REQUIRE(keep_dev && n_kept, "matvec_sector_mask: arguments");
    *n_kept = 0;
    u32 x0 = 0;
    if (plan_N->xg.G == 1) SG_TRY(read_back_words(plan_N->xg.gx.as<u32>(), 1, nullptr, 0, &x0));
    SG_REQUIRE(plan_N->xg.G <= 1 && x0 == 0, "matvec_sector_mask: the number operator has a term with an X or a Y");
    hipStream_t st = ctx().stream;
    const u64 N = (u64)1 << plan_N->xg.n;
    SG_TRY(matvec_require_memory(4096, "the sector mask"));
    Scratch cnt;
    SG_TRY(cnt.alloc(8));
    HIP_TRY(hipMemsetAsync(cnt.p, 0, 8, st));
    hipLaunchKernelGGL(k_mv_sector, dim3(grid_each((i64)N)), dim3(256), 0, st, mv_terms_of(plan_N), (long long)n_particles, keep_dev,
                       cnt.as<unsigned long long>());
    KERNEL_CHECK();
    u32 w[2] = {0, 0};
    SG_TRY(read_back_words(cnt.as<u32>(), 2, nullptr, 0, w));
    *n_kept = (int64_t)((u64)w[0] | ((u64)w[1] << 32));
    return SYMGPU_OK;
}

}  // extern "C"
