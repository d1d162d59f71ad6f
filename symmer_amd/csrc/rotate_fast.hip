// rotate_fast.hip — the per-row rotation paths of an operator without duplicate rows (after the analysis, rotate_analyze.hip):
//   non-Clifford: hash join   k_rotf_match2 -> k_rotf_scan3 -> k_rotf_write
//   Clifford:                 k_rotc_classify -> k_rotf_scan3 -> k_rotf_write (also the four-launch form of a Clifford run)
#include "rotate_common.h"

namespace symgpu {

// ---- fast non-Clifford path: hash-table join instead of the sort-based cleanup ---------------------------------------
// For an operator WITHOUT duplicate rows (anything that left cleanup()) the only possible merge is between a product row
// P_k ^ Q and the existing row R_j = P_k ^ Q, which is anticommuting too and whose own product row is P_k: partners come
// in pairs.  So: hash every row (linear hash: h(P^Q) = h(P) ^ h(Q)), insert the rows in an open-addressing table, look
// up h(P_k) ^ h(Q) for every anticommuting row and verify the candidate word by word.  A duplicate row in the input
// (same hash AND same words) raises `dup`; the caller then takes the general sort-based path, which handles it.
// Output order and sums are those of the reference (base.py:1158-1161 + cleanup): kept commuting rows, kept
// anticommuting rows with  cos*c_t + (-i sin) i^{e_p} c_p  (first-occurrence entry first), then the kept unmatched product
// rows; strict |c| > thr everywhere.


// The same join, ONE lane per row, fused with the per-1024-row block counts (k_rotf_count): probe the generation-tagged table for
// h(P) ^ h(Q); only a tag hit reads rows (a lane then compares the two rows word by word).  1024 rows per block.
__global__ __launch_bounds__(1024) void k_rotf_match2(const u64 *__restrict__ rows, const double *__restrict__ coeff, const u64 *__restrict__ h, i64 T,
                                                       int W, const u64 *__restrict__ q, u64 hq, const u32 *__restrict__ anti,
                                                       const uint8_t *__restrict__ ph, JoinTable jt, double cos_t, double sin_t, double thr,
                                                       double *__restrict__ selfc, double *__restrict__ prodc, uint8_t *__restrict__ cls,
                                                       u32 *__restrict__ blk) {
    __shared__ u32 s_c[4];
    if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
    __syncthreads();
    const i64 t = (i64)blockIdx.x * 1024 + threadIdx.x;
    const bool valid = t < T;
    const bool is_anti = valid && anti[t];
    uint8_t c = 0;
    if (valid) {
        i64 partner = -1;
        if (is_anti) {
            const u64 key = h[t] ^ hq;
            u32 pos = (u32)mix64(key) & jt.mask;
            for (;;) {
                const u64 v = jt.slots[pos];
                if (jt_gen(v) != jt.gen) break;
                if ((v >> 32) == (key >> 32)) {
                    const i64 o = jt_row(v);
                    bool same = true;
                    for (int w = 0; w < W; ++w) same &= (rows[o * W + w] == (rows[t * W + w] ^ q[w]));
                    if (same) { partner = o; break; }
                }
                pos = (pos + 1) & jt.mask;
            }
        }
        const double re = coeff[2 * t], im = coeff[2 * t + 1];
        // every coefficient leaves as 0 + c, as the reference's cleanup forms it (a zero component is +0)
        if (!is_anti) {
            selfc[2 * t] = __dadd_rn(0.0, re); selfc[2 * t + 1] = __dadd_rn(0.0, im);
            if (above_thr(re, im, thr)) c = 1;
        } else {
            double sr = __dmul_rn(re, cos_t), si = __dmul_rn(im, cos_t);
            if (partner >= 0) {                                  // merge: (0 + cos*c_t) + (-i sin) i^{e_p} c_p, in that order
                double pr, pi;
                phase_mul(coeff[2 * partner], coeff[2 * partner + 1], ph[partner], pr, pi);
                sr = __dadd_rn(__dadd_rn(0.0, sr), __dmul_rn(pi, sin_t));
                si = __dadd_rn(__dadd_rn(0.0, si), -__dmul_rn(pr, sin_t));
            } else {                                             // its product row is new
                double pr, pi;
                phase_mul(re, im, ph[t], pr, pi);
                const double nr = __dmul_rn(pi, sin_t), ni = -__dmul_rn(pr, sin_t);
                prodc[2 * t] = __dadd_rn(0.0, nr); prodc[2 * t + 1] = __dadd_rn(0.0, ni);
                if (above_thr(nr, ni, thr)) c |= 4;
            }
            selfc[2 * t] = __dadd_rn(0.0, sr); selfc[2 * t + 1] = __dadd_rn(0.0, si);
            if (above_thr(sr, si, thr)) c |= 2;
        }
        cls[t] = c;
    }
    const int lane = threadIdx.x & 63;
    const u64 b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4), b3 = __ballot(is_anti);
    if (lane == 0) {
        atomicAdd(&s_c[0], (u32)__popcll(b0)); atomicAdd(&s_c[1], (u32)__popcll(b1));
        atomicAdd(&s_c[2], (u32)__popcll(b2)); atomicAdd(&s_c[3], (u32)__popcll(b3));
    }
    __syncthreads();
    if (threadIdx.x < 4) blk[blockIdx.x * 4 + threadIdx.x] = s_c[threadIdx.x];
}

// three exclusive scans (kept-commuting, kept-anticommuting, kept-new) + the anticommuting count: the per-1024-row block counts
// come from k_rotf_match2 / k_rotc_classify, every block here adds the counts of the blocks before it (<= 4096) to its local ranks.
__global__ __launch_bounds__(1024) void k_rotf_scan3(const uint8_t *__restrict__ cls, i64 T, const u32 *__restrict__ blk, int n_blk,
                                                      u32 *__restrict__ pos_self, u32 *__restrict__ pos_new, RotCounts *__restrict__ cnt,
                                                      const u32 *__restrict__ jt_flags, u32 jt_gen_now, RotCounts *__restrict__ host_cnt = nullptr) {
    __shared__ u32 s_w[3][16];
    __shared__ u32 s_base[4], s_all[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 4) { s_base[threadIdx.x] = 0; s_all[threadIdx.x] = 0; }
    __syncthreads();
    {   // counts of the blocks before this one (and, for the last block, of all blocks)
        u32 before[4] = {0, 0, 0, 0}, all[4] = {0, 0, 0, 0};
        for (int b = threadIdx.x; b < n_blk; b += 1024)
#pragma unroll
            for (int k = 0; k < 4; ++k) { const u32 x = blk[b * 4 + k]; all[k] += x; if (b < (int)blockIdx.x) before[k] += x; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            for (int off = 32; off > 0; off >>= 1) { before[k] += __shfl_down(before[k], off); all[k] += __shfl_down(all[k], off); }
            if (lane == 0) { if (before[k]) atomicAdd(&s_base[k], before[k]); if (all[k]) atomicAdd(&s_all[k], all[k]); }
        }
    }
    const i64 t = (i64)blockIdx.x * 1024 + threadIdx.x;
    const uint8_t c = (t < T) ? cls[t] : 0;
    u32 ex[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u64 b = __ballot((c >> k) & 1);
        ex[k] = __popcll(b & ((1ULL << lane) - 1ULL));
        if (lane == 0) s_w[k][wave] = __popcll(b);
    }
    __syncthreads();
    u32 off[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int w2 = 0; w2 < wave; ++w2) off[k] += s_w[k][w2];
    if (t < T) {
        pos_self[t] = (c & 1) ? s_base[0] + off[0] + ex[0] : s_base[1] + off[1] + ex[1];
        pos_new[t] = s_base[2] + off[2] + ex[2];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        cnt->nC = s_all[0]; cnt->nA = s_all[1]; cnt->nN = s_all[2]; cnt->nAnti = s_all[3];
        cnt->dup = (jt_flags && jt_flags[0] == jt_gen_now) ? 1u : 0u;        // one read-back for the counts and the duplicate flag
        // the same five words straight into pinned host memory: the host reads them after the stream synchronisation that ends the
        // rotation, without a device-to-host copy in between
        if (host_cnt) { host_cnt->nC = s_all[0]; host_cnt->nA = s_all[1]; host_cnt->nN = s_all[2]; host_cnt->nAnti = s_all[3]; host_cnt->dup = cnt->dup; }
    }
}

__global__ void k_rotf_write(const u32x4 *__restrict__ rows, const u32x4 *__restrict__ q, i64 T, int Wq, const uint8_t *__restrict__ cls,
                             const u32 *__restrict__ pos_self, const u32 *__restrict__ pos_new, const RotCounts *__restrict__ cnt,
                             const double *__restrict__ selfc, const double *__restrict__ prodc, u32x4 *__restrict__ out_rows,
                             double *__restrict__ out_coeff, int clifford, const u64 *__restrict__ hin, u64 hq, u64 *__restrict__ hout) {
    // hin / hout (may be null): row hashes of the input and of the result — h is linear, so h(P ^ Q) = h(P) ^ h(Q)
    const i64 total = T * Wq;
    // output order: non-Clifford [commuting | cos * anticommuting | new rows]; Clifford [rotated anticommuting | commuting]
    const i64 baseC = clifford ? (i64)cnt->nA + cnt->nN : 0;
    const i64 baseA = clifford ? 0 : (i64)cnt->nC;
    const i64 baseN = clifford ? 0 : (i64)cnt->nC + cnt->nA;
    // The first ceil(T / 256) blocks move the 16-byte coefficients and the 8-byte hashes, ONE LANE PER ROW (consecutive rows of a class
    // go to consecutive slots: near-coalesced); the remaining blocks move the rows, one 16-byte chunk per lane.  Done by the chunk-0
    // lane of every row inside the row stream, the small stores — one lane of 16, scattered between the 256-byte row stores —
    // are what the product's row stream showed to be expensive (product.hip, tools/ubench_fused.hip).
    const i64 n_cf = (T + blockDim.x - 1) / blockDim.x;
    if ((i64)blockIdx.x < n_cf) {
        const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= T) return;
        const uint8_t k = cls[t];
        if (k & 3) {
            const i64 d = (k & 1) ? baseC + pos_self[t] : baseA + pos_self[t];
            reinterpret_cast<f64x2 *>(out_coeff)[d] = reinterpret_cast<const f64x2 *>(selfc)[t];
            if (hout) hout[d] = hin[t];
        }
        if (k & 4) {
            const i64 d = baseN + pos_new[t];
            reinterpret_cast<f64x2 *>(out_coeff)[d] = reinterpret_cast<const f64x2 *>(prodc)[t];
            if (hout) hout[d] = hin[t] ^ hq;
        }
        return;
    }
    const int wsh = (Wq & (Wq - 1)) == 0 ? __builtin_ctz((unsigned)Wq) : -1;      // chunks per row a power of two: shift instead of a 64-bit divide
    const i64 n_row_blocks = (i64)gridDim.x - n_cf;
    // four chunks per lane and step, every load of a step issued before the first store: class byte, both slot words and the
    // chunk itself do not depend on each other (the one-chunk loop chained class -> branch -> loads: 3.8 TB/s at 10^6 terms)
    constexpr int WU = 4;
    const i64 stride = n_row_blocks * blockDim.x;
    for (i64 idx0 = ((i64)blockIdx.x - n_cf) * blockDim.x + threadIdx.x; idx0 < total; idx0 += stride * WU) {
        i64 t[WU];
        int c[WU];
        uint8_t k[WU];
        u32 ps[WU], pn[WU];
        u32x4 v[WU];
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            const i64 idx = idx0 + u * stride < total ? idx0 + u * stride : idx0;
            t[u] = wsh >= 0 ? idx >> wsh : idx / Wq;
            c[u] = (int)(idx - t[u] * Wq);
            k[u] = cls[t[u]];
            ps[u] = pos_self[t[u]];
            pn[u] = pos_new[t[u]];
            v[u] = rows[idx];
        }
#pragma unroll
        for (int u = 0; u < WU; ++u) {
            if (idx0 + u * stride >= total) break;
            if (k[u] & 3) {
                const i64 d = (k[u] & 1) ? baseC + ps[u] : baseA + ps[u];
                __builtin_nontemporal_store(v[u], &out_rows[d * Wq + c[u]]);
            }
            if (k[u] & 4) {
                const i64 d = baseN + pn[u];
                __builtin_nontemporal_store(v[u] ^ q[c[u]], &out_rows[d * Wq + c[u]]);
            }
        }
    }
}

// Clifford rotation (angle = k * pi/2), classes + per-1024-row block counts in one launch:
//   commuting row            -> class 1, coefficient unchanged
//   anticommuting, even k    -> class 2 (the row itself), coefficient c (k = 0) or -c (k = 2)
//   anticommuting, odd k     -> class 4 (row ^ Q), coefficient c * i^e * (-i), negated for k = 3; rows with |c| <= thr are
//                               dropped as the reference's `*` does (cleanup inside _multiply_by_operator, base.py:789-793)
// `k` arrives already mapped by rotation_args (negative multiples are not reduced mod 4, base.py:1148).
__global__ __launch_bounds__(1024) void k_rotc_classify(const u32 *__restrict__ anti, const uint8_t *__restrict__ ph, const double *__restrict__ coeff,
                                                         i64 T, int k, double thr, uint8_t *__restrict__ cls, double *__restrict__ selfc,
                                                         double *__restrict__ prodc, u32 *__restrict__ blk) {
    __shared__ u32 s_c[4];
    if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
    __syncthreads();
    const i64 t = (i64)blockIdx.x * 1024 + threadIdx.x;
    uint8_t c = 0;
    bool a = false;
    if (t < T) {
        const double re = coeff[2 * t], im = coeff[2 * t + 1];
        a = anti[t] != 0;
        if (!a) {
            c = 1;
            selfc[2 * t] = re; selfc[2 * t + 1] = im;
        } else if (k & 1) {
            if (above_thr(re, im, thr)) {
                double x, y;
                phase_mul(re, im, ph[t], x, y);
                double pr = y, pi = -x;
                if (k == 3) { pr = -pr; pi = -pi; }
                prodc[2 * t] = pr; prodc[2 * t + 1] = pi;
                c = 4;
            }
        } else {
            const bool neg = (k == 2);
            selfc[2 * t] = neg ? -re : re; selfc[2 * t + 1] = neg ? -im : im;
            c = 2;
        }
        cls[t] = c;
    }
    const int lane = threadIdx.x & 63;
    const u64 b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4), b3 = __ballot(a);
    if (lane == 0) {
        atomicAdd(&s_c[0], (u32)__popcll(b0)); atomicAdd(&s_c[1], (u32)__popcll(b1));
        atomicAdd(&s_c[2], (u32)__popcll(b2)); atomicAdd(&s_c[3], (u32)__popcll(b3));
    }
    __syncthreads();
    if (threadIdx.x < 4) blk[blockIdx.x * 4 + threadIdx.x] = s_c[threadIdx.x];
}

int RotScratch::alloc(i64 T) {
    n_blk = (int)((T + 1023) / 1024);
    SG_TRY(blk.alloc((size_t)n_blk * 16));
    SG_TRY(selfc.alloc((size_t)T * 16));
    SG_TRY(prodc.alloc((size_t)T * 16));
    SG_TRY(cls.alloc((size_t)T));
    SG_TRY(pself.alloc((size_t)T * 4));
    SG_TRY(pnew.alloc((size_t)T * 4));
    SG_TRY(cnt.alloc(sizeof(RotCounts)));
    return SYMGPU_OK;
}

void launch_rotf_write(const u64 *rows, const u64 *q, i64 T, int Wq, const RotScratch &s, u64 *out_rows, double *out_coeff, int clifford,
                       const u64 *hin, u64 hq, u64 *hout) {
    hipLaunchKernelGGL(k_rotf_write, dim3(grid_for((T * Wq + 3) / 4) + (unsigned)((T + 255) / 256)), dim3(256), 0, ctx().stream, reinterpret_cast<const u32x4 *>(rows),
                       reinterpret_cast<const u32x4 *>(q), T, Wq, s.cls.as<uint8_t>(), s.pself.as<u32>(), s.pnew.as<u32>(), s.cnt.as<RotCounts>(),
                       s.selfc.as<double>(), s.prodc.as<double>(), reinterpret_cast<u32x4 *>(out_rows), out_coeff, clifford, hin, hq, hout);
}

// one Clifford rotation of analysed rows: classify + count -> scan -> write (errors: hipGetLastError of the caller)
void clifford_classify_scan_write(const u64 *rows, const double *coeff, const u64 *q, const u32 *anti, const uint8_t *ph, i64 T, int Wq, int k,
                                  double thr, const RotScratch &s, RotCounts *host_cnt, u64 *out_rows, double *out_coeff, const u64 *hin, u64 hq,
                                  u64 *hout) {
    hipStream_t st = ctx().stream;
    hipLaunchKernelGGL(k_rotc_classify, dim3(s.n_blk), dim3(1024), 0, st, anti, ph, coeff, T, k, thr, s.cls.as<uint8_t>(), s.selfc.as<double>(),
                       s.prodc.as<double>(), s.blk.as<u32>());
    hipLaunchKernelGGL(k_rotf_scan3, dim3(s.n_blk), dim3(1024), 0, st, s.cls.as<uint8_t>(), T, s.blk.as<u32>(), s.n_blk, s.pself.as<u32>(), s.pnew.as<u32>(),
                       s.cnt.as<RotCounts>(), (const u32 *)nullptr, 0u, host_cnt);
    launch_rotf_write(rows, q, T, Wq, s, out_rows, out_coeff, 1, hin, hq, hout);
}

// Non-Clifford rotation as a hash join, four launches and no clearing pass:
//   k_rot_analyze<.., INSERT>  flags + phase exponents (+ row hashes unless the handle carries them) + insert into the join table
//   k_rotf_match2              probe h(P) ^ h(Q), verify, classify, coefficients, per-block counts
//   k_rotf_scan3, k_rotf_write output slots, rows + coefficients + hashes of the result
// *done = 1: result in *out / *all_commute; *done = 0: duplicate rows (the rows are analysed: on to the general path)
int rotate_join(RotationRun &r, int *done) {
    hipStream_t st = ctx().stream;
    symgpu_op_t in = r.in;
    const i64 T = in->T;
    const int Wq = in->Wq, W = 2 * Wq;
    *done = 0;
    SG_TRY(ensure_hash_tables(ctx().hash_tab ? ctx().hash_seed : 1));
    const u64 seed = ctx().hash_seed;
    const u64 hq = host_row_hash(r.q_host, W);
    JoinTable jt;
    SG_TRY(join_table_for(T, &jt));
    RotScratch s;
    SG_TRY(s.alloc(T));
    SG_TRY(analyze_rows(in, r.q.as<u64>(), r.anti.as<u32>(), r.ph.as<uint8_t>(), &jt, r.sw, r.q_host));    // Q reaches the device with this launch
    hipLaunchKernelGGL(k_rotf_match2, dim3(s.n_blk), dim3(1024), 0, st, in->rows, in->coeff, in->hash, T, W, r.q.as<u64>(), hq, r.anti.as<u32>(),
                       r.ph.as<uint8_t>(), jt, r.cos_t, r.sin_t, r.thr, s.selfc.as<double>(), s.prodc.as<double>(), s.cls.as<uint8_t>(), s.blk.as<u32>());
    RotCounts *hcnt = nullptr, *hcnt_dev = nullptr;
    SG_TRY(host_counts(&hcnt, &hcnt_dev));
    hipLaunchKernelGGL(k_rotf_scan3, dim3(s.n_blk), dim3(1024), 0, st, s.cls.as<uint8_t>(), T, s.blk.as<u32>(), s.n_blk, s.pself.as<u32>(), s.pnew.as<u32>(),
                       s.cnt.as<RotCounts>(), jt.flags, jt.gen, hcnt_dev);
    KERNEL_CHECK();
    OwnedOp res;
    SG_TRY(res.alloc(2 * T, 0, Wq, true));                     // upper bound: no host round trip before the write kernel
    SG_TRY(res.attach_hash());
    res->hash_seed = seed;
    launch_rotf_write(in->rows, r.q.as<u64>(), T, Wq, s, res->rows, res->coeff, 0, in->hash, hq, res->hash);
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    const RotCounts hc = *hcnt;
    if (hc.nAnti == 0) { if (!hc.dup) in->dup_free = 1; *r.all_commute = 1; *done = 1; return SYMGPU_OK; }   // identity action (base.py:1131-1133): the result is dropped
    if (hc.dup) return SYMGPU_OK;                              // duplicates in the input: the result is dropped, general path
    res->T = (i64)hc.nC + hc.nA + hc.nN;
    res->dup_free = 1;                 // the input had no duplicates (checked above) and every P^Q that met a row was merged into it
    in->dup_free = 1;
    res.hand_out(r.out);
    *r.all_commute = 0;
    *done = 1;
    return SYMGPU_OK;
}

// Clifford fast path: analyze (done before) -> classify+count -> scan -> write, one host round trip at the very end.
int rotate_clifford_fast(RotationRun &r) {
    hipStream_t st = ctx().stream;
    symgpu_op_t in = r.in;
    const i64 T = in->T;
    const int Wq = in->Wq;
    RotScratch s;
    SG_TRY(s.alloc(T));
    RotCounts *hcnt = nullptr, *hcnt_dev = nullptr;
    SG_TRY(host_counts(&hcnt, &hcnt_dev));
    OwnedOp res;
    SG_TRY(res.alloc(T, 0, Wq, true));                         // a Clifford rotation never adds rows
    // row hashes, if the operand carries them, are handed on (rotated rows: h ^ h(Q)) so that a later non-Clifford rotation or
    // duplicate check of the chain does not hash again
    const u64 *in_hash = (in->hash && ctx().hash_tab && in->hash_seed == ctx().hash_seed) ? in->hash : nullptr;
    u64 hq = 0;
    if (in_hash) {
        hq = host_row_hash(r.q_host, 2 * Wq);
        SG_TRY(res.attach_hash());
        res->hash_seed = in->hash_seed;
    }
    clifford_classify_scan_write(in->rows, in->coeff, r.q.as<u64>(), r.anti.as<u32>(), r.ph.as<uint8_t>(), T, Wq, r.k, r.thr, s, hcnt_dev, res->rows,
                                 res->coeff, in_hash, hq, res->hash);
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(st));
    const RotCounts hc = *hcnt;
    if (hc.nAnti == 0) { *r.all_commute = 1; return SYMGPU_OK; }   // identity action (base.py:1131-1133): the result is dropped
    res->T = (i64)hc.nC + hc.nA + hc.nN;
    res->dup_free = in->dup_free;      // distinct rows stay distinct: P^Q anticommutes with Q, so it never meets a commuting row
    res.hand_out(r.out);
    *r.all_commute = 0;
    return SYMGPU_OK;
}

}  // namespace symgpu
