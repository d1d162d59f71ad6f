// xgroups.hip — the terms of an operator grouped by X-part (xgroups.h).
#include "xgroups.h"
#include "sort.h"

namespace symgpu {

// key = x as an n-bit integer, qubit 0 the most significant bit
__global__ __launch_bounds__(256) void k_xg_keys(const u64 *__restrict__ rows, i64 T, int n, u64 *__restrict__ key, u32 *__restrict__ idx) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    key[t] = __brevll(rows[2 * t]) >> (64 - n);
    idx[t] = (u32)t;
}

__global__ __launch_bounds__(256) void k_xg_heads(const u64 *__restrict__ key, i64 T, u32 *__restrict__ head) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= T) return;
    head[s] = (s == 0 || key[s] != key[s - 1]) ? 1u : 0u;
}

// per sorted term s: z, c' and (tg != null) the flagged group word; per group: x and its first term
__global__ __launch_bounds__(256) void k_xg_terms(const u64 *__restrict__ rows, const double *__restrict__ coeff, const u64 *__restrict__ key,
                                                  const u32 *__restrict__ idx, const u32 *__restrict__ gexcl, const u32 *__restrict__ head, i64 T, int n,
                                                  u32 *__restrict__ tz, f64x2 *__restrict__ tc, u32 *__restrict__ gx, u32 *__restrict__ gstart, u32 *__restrict__ tg) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    if (s >= T) return;
    const u32 t = idx[s];
    const u64 x = rows[2 * (i64)t], z = rows[2 * (i64)t + 1];
    const u32 g = gexcl[s] + head[s] - 1;
    const bool last = s == T - 1 || key[s + 1] != key[s];
    const f64x2 c = reinterpret_cast<const f64x2 *>(coeff)[t];
    double re, im;
    apply_phase(c.x, c.y, (3 * __popcll(x & z)) & 3, re, im);       // (-i)^Y = i^{3 Y}
    tz[s] = (u32)(__brevll(z) >> (64 - n));
    tc[s] = f64x2{re, im};
    if (tg) tg[s] = g | (head[s] ? CSR_FIRST : 0u) | (last ? CSR_LAST : 0u);
    if (head[s]) {
        gx[g] = (u32)key[s];
        gstart[g] = (u32)s;
    }
    if (s == T - 1) gstart[g + 1] = (u32)T;
}

int xgroups_build(symgpu_op_t op, int n, bool want_tg, XGroups *out) {
    hipStream_t st = ctx().stream;
    const i64 T = op->T;
    out->T = T;
    out->n = n;
    out->G = 0;
    if (T == 0) return SYMGPU_OK;
    Scratch key, key_tmp, idx, idx_tmp, head, gexcl;
    SG_TRY(key.alloc((size_t)T * 8));
    SG_TRY(key_tmp.alloc((size_t)T * 8));
    SG_TRY(idx.alloc((size_t)T * 4));
    SG_TRY(idx_tmp.alloc((size_t)T * 4));
    SG_TRY(head.alloc((size_t)T * 4));
    SG_TRY(gexcl.alloc((size_t)T * 4 + 4));
    hipLaunchKernelGGL(k_xg_keys, dim3(grid_each(T)), dim3(256), 0, st, op->rows, T, n, key.as<u64>(), idx.as<u32>());
    KERNEL_CHECK();
    SortResult by_x;
    SG_TRY(radix_sort({key.as<u64>(), key_tmp.as<u64>(), idx.as<u32>(), idx_tmp.as<u32>(), T, 0, (n + 7) / 8 * 8, nullptr, SortForm::Launches}, &by_x));
    hipLaunchKernelGGL(k_xg_heads, dim3(grid_each(T)), dim3(256), 0, st, by_x.keys, T, head.as<u32>());
    KERNEL_CHECK();
    u32 *d_total = gexcl.as<u32>() + T;
    SG_TRY(exclusive_scan_u32(head.as<u32>(), gexcl.as<u32>(), T, d_total));
    u32 G = 0;
    SG_TRY(read_back_words(d_total, 1, nullptr, 0, &G));
    out->G = G;
    SG_TRY(out->tz.alloc((size_t)T * 4));
    SG_TRY(out->tc.alloc((size_t)T * 16));
    SG_TRY(out->gx.alloc((size_t)G * 4));
    SG_TRY(out->gstart.alloc((size_t)(G + 1) * 4));
    if (want_tg) SG_TRY(out->tg.alloc((size_t)T * 4));
    hipLaunchKernelGGL(k_xg_terms, dim3(grid_each(T)), dim3(256), 0, st, op->rows, op->coeff, by_x.keys, by_x.vals, gexcl.as<u32>(), head.as<u32>(), T, n,
                       out->tz.as<u32>(), out->tc.as<f64x2>(), out->gx.as<u32>(), out->gstart.as<u32>(), out->tg.as<u32>());
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
