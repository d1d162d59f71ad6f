// rotate_general.hip — the general rotation path (what operators with duplicate rows take, and every rotation under
// SYMGPU_ROTATE_GENERAL): the reference's stacked operator (base.py:1139-1161) built row by row, then the cleanup that merges duplicates.
#include "rotate_common.h"
#include "sort.h"

namespace symgpu {

// Clifford odd-k: product rows whose coefficient is <= thr are dropped by the reference's `*` (cleanup inside
// _multiply_by_operator, base.py:789-793): fold that into the flag that is scanned.
__global__ void k_rot_keepflags(const u32 *__restrict__ anti, const double *__restrict__ coeff, i64 T, double thr, int drop_small,
                                u32 *__restrict__ keep) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        u32 k = anti[t];
        if (k && drop_small && !above_thr(coeff[2 * t], coeff[2 * t + 1], thr)) k = 0;
        keep[t] = k;
    }
}

// coefficients of the stacked operator.  MODE 0: non-Clifford; MODE 1: Clifford.
// apos = exclusive scan of `sel` (anticommuting-and-kept flags); n_sel = its total.
template <int MODE>
__global__ void k_rot_coeff(const double *__restrict__ coeff, const u32 *__restrict__ anti, const u32 *__restrict__ sel,
                            const u32 *__restrict__ apos, const u32 *__restrict__ cpos, const uint8_t *__restrict__ ph, i64 T, i64 n_sel,
                            i64 n_comm, double cos_t, double sin_t, int k, double *__restrict__ out_coeff, u32 *__restrict__ dst_main,
                            u32 *__restrict__ dst_prod) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        const double re = coeff[2 * t], im = coeff[2 * t + 1];
        u32 d_main = 0xffffffffu, d_prod = 0xffffffffu;
        if (MODE == 0) {
            if (!anti[t]) {
                d_main = cpos[t];                                   // commuting rows first, input order
                out_coeff[2 * (i64)d_main] = re; out_coeff[2 * (i64)d_main + 1] = im;
            } else {
                d_main = (u32)(n_comm + apos[t]);                   // cos * P
                out_coeff[2 * (i64)d_main] = __dmul_rn(re, cos_t); out_coeff[2 * (i64)d_main + 1] = __dmul_rn(im, cos_t);
                d_prod = (u32)(n_comm + n_sel + apos[t]);           // (-i sin) * i^e * c   on row P^Q
                double pr, pi;
                phase_mul(re, im, ph[t], pr, pi);
                out_coeff[2 * (i64)d_prod] = __dmul_rn(pi, sin_t); out_coeff[2 * (i64)d_prod + 1] = -__dmul_rn(pr, sin_t);
            }
        } else {
            if (!anti[t]) {
                d_main = (u32)(n_sel + cpos[t]);                    // commuting rows after the rotated ones
                out_coeff[2 * (i64)d_main] = re; out_coeff[2 * (i64)d_main + 1] = im;
            } else if (sel[t]) {
                double pr = re, pi = im;
                if (k & 1) {                                        // c * i^e * (-i)
                    double a, b;
                    phase_mul(re, im, ph[t], a, b);
                    pr = b; pi = -a;
                    d_prod = apos[t];
                } else {
                    d_main = apos[t];
                }
                if (k == 2 || k == 3) { pr = -pr; pi = -pi; }
                const u32 d = (k & 1) ? d_prod : d_main;
                out_coeff[2 * (i64)d] = pr; out_coeff[2 * (i64)d + 1] = pi;
            }
        }
        dst_main[t] = d_main;
        dst_prod[t] = d_prod;
    }
}

// rows of the stacked operator as 16-byte chunks
__global__ void k_rot_rows(const u32x4 *__restrict__ rows, const u32x4 *__restrict__ q, i64 T, int Wq, const u32 *__restrict__ dst_main,
                           const u32 *__restrict__ dst_prod, u32x4 *__restrict__ out) {
    const i64 total = T * Wq;
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        const i64 t = idx / Wq;
        const int c = (int)(idx - t * Wq);
        const u32x4 v = rows[idx];
        const u32 dm = dst_main[t], dp = dst_prod[t];
        if (dm != 0xffffffffu) out[(i64)dm * Wq + c] = v;
        if (dp != 0xffffffffu) out[(i64)dp * Wq + c] = v ^ q[c];
    }
}

__global__ void k_not_flags(const u32 *__restrict__ a, i64 T, u32 *__restrict__ out) {
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) out[t] = a[t] ? 0u : 1u;
}

// Stack [commuting | cos * anticommuting | (-i sin) i^e * (anticommuting ^ Q)] (non-Clifford) or [rotated anticommuting | commuting]
// (Clifford), then the cleanup that merges duplicates.  The rows are analysed (r.anti, r.ph) and Q is on the device.
int rotate_general(RotationRun &r) {
    hipStream_t st = ctx().stream;
    symgpu_op_t in = r.in;
    const i64 T = in->T;
    const int Wq = in->Wq, W = 2 * Wq;
    const bool clifford = r.k >= 0;
    const u32 *anti = r.anti.as<u32>();
    Scratch sel, apos, cpos, totals, dmain, dprod;
    SG_TRY(sel.alloc((size_t)T * 4));
    SG_TRY(apos.alloc((size_t)T * 4));
    SG_TRY(cpos.alloc((size_t)T * 4));
    SG_TRY(totals.alloc(16));
    SG_TRY(dmain.alloc((size_t)T * 4));
    SG_TRY(dprod.alloc((size_t)T * 4));
    // odd-k Clifford: every anticommuting row enters the product; the threshold applies to the merged sums below
    const int drop_small = 0;
    hipLaunchKernelGGL(k_rot_keepflags, dim3(grid_for(T)), dim3(256), 0, st, anti, in->coeff, T, r.thr, drop_small, sel.as<u32>());
    KERNEL_CHECK();
    u32 *tot = totals.as<u32>();
    SG_TRY(exclusive_scan_u32(sel.as<u32>(), apos.as<u32>(), T, tot));            // positions among selected anticommuting rows
    hipLaunchKernelGGL(k_not_flags, dim3(grid_for(T)), dim3(256), 0, st, anti, T, cpos.as<u32>());
    KERNEL_CHECK();
    SG_TRY(exclusive_scan_u32(cpos.as<u32>(), cpos.as<u32>(), T, tot + 1));        // positions among commuting rows
    u32 h[2] = {0, 0};
    SG_TRY(read_back_words(tot, 2, nullptr, 0, h));
    const i64 n_sel = h[0], n_comm = h[1];
    if (n_comm == T) return SYMGPU_OK;        // every term commutes: identity action (base.py:1131-1133)
    *r.all_commute = 0;
    const i64 n_stack = clifford ? (n_sel + n_comm) : (n_comm + 2 * n_sel);
    OwnedOp stack;
    SG_TRY(stack.alloc(rows_or_one(n_stack), n_stack, Wq, true));
    if (clifford)
        hipLaunchKernelGGL(k_rot_coeff<1>, dim3(grid_for(T)), dim3(256), 0, st, in->coeff, anti, sel.as<u32>(), apos.as<u32>(),
                           cpos.as<u32>(), r.ph.as<uint8_t>(), T, n_sel, n_comm, r.cos_t, r.sin_t, r.k, stack->coeff, dmain.as<u32>(), dprod.as<u32>());
    else
        hipLaunchKernelGGL(k_rot_coeff<0>, dim3(grid_for(T)), dim3(256), 0, st, in->coeff, anti, sel.as<u32>(), apos.as<u32>(),
                           cpos.as<u32>(), r.ph.as<uint8_t>(), T, n_sel, n_comm, r.cos_t, r.sin_t, r.k, stack->coeff, dmain.as<u32>(), dprod.as<u32>());
    hipLaunchKernelGGL(k_rot_rows, dim3(grid_for(T * Wq)), dim3(256), 0, st, reinterpret_cast<const u32x4 *>(in->rows),
                       reinterpret_cast<const u32x4 *>(r.q.p), T, Wq, dmain.as<u32>(), dprod.as<u32>(), reinterpret_cast<u32x4 *>(stack->rows));
    KERNEL_CHECK();
    if (clifford && !(r.k & 1)) {
        HIP_TRY(hipStreamSynchronize(st));
        stack->dup_free = in->dup_free;
        stack.hand_out(r.out);
        return SYMGPU_OK;
    }
    OwnedOp res;
    if (clifford) {
        // (anticom_self * Q) of base.py:1143 = cleanup of the rotated rows: duplicates merged in input order, |sum| > thr kept
        // (the exact factors -i / -1 commute with the IEEE sums); then the commuting rows, untouched (base.py:1151-1154)
        OwnedOp merged;
        SG_TRY(cleanup_rows(stack->rows, stack->coeff, n_sel, W, r.thr, 1, merged.slot(), Wq));
        const i64 n_merged = merged->T;
        SG_TRY(res.alloc(rows_or_one(n_merged + n_comm), n_merged + n_comm, Wq, true));
        SG_TRY(symgpu_op_copy_rows(res.op, 0, merged.op, 0, n_merged));
        SG_TRY(symgpu_op_copy_rows(res.op, n_merged, stack.op, n_sel, n_comm));
        HIP_TRY(hipStreamSynchronize(st));
        res->dup_free = in->dup_free;                              // merged rotated rows + the untouched commuting rows
    } else {
        SG_TRY(cleanup_rows(stack->rows, stack->coeff, n_stack, W, r.thr, 1, res.slot(), Wq));
    }
    res.hand_out(r.out);
    return SYMGPU_OK;
}

}  // namespace symgpu
