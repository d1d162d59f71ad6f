// rotate_chain_forms.hip — a run of Clifford rotations of a clean operator (symgpu_rotate_clifford_chain_dev) in the forms other than
// the register chain (rotate_chain.hip): LDS-resident and single-workgroup kernels for small operators, two launches per rotation, and
// the Clifford fast path's four launches per rotation.  Every form returns with the stream synchronised.
#include "rotate_common.h"
#include "block_scan.h"

namespace symgpu {

// ---- a whole chain of Clifford rotations in ONE launch (small operators) ------------------------------------------------------
// perform_rotations / CircuitSymmerlator apply thousands of pi/2-multiples to an operator of a few (hundred) terms: per rotation the
// launches and the count read-back of the general path cost 60 us, the data movement nothing.  For an operator that is CLEAN —
// no duplicate rows and every |c| > 1e-15, i.e. it has been through cleanup(), which is what perform_rotations guarantees after
// its first step — a Clifford rotation drops nothing and merges nothing (base.py:1139-1154 followed by cleanup(), :1185): it is
// a stable partition [anticommuting | commuting] with row ^= Q and c *= i^e (-i) (odd k), c = -c (k in {2,3}) on the anticommuting
// part, or nothing at all if every term commutes.  One workgroup keeps flags, phase exponents and slots in LDS and ping-pongs
// the rows between two global buffers (L2 resident), one block barrier per phase.

__global__ __launch_bounds__(1024) void k_clifford_chain(u64 *__restrict__ rowsA, double *__restrict__ coeffA, u64 *__restrict__ rowsB,
                                                          double *__restrict__ coeffB, int T, int Wq, int G, const u64 *__restrict__ qs,
                                                          const int *__restrict__ ks, int K, int *__restrict__ result_in_b) {
    __shared__ uint8_t s_anti[CHAIN_TMAX], s_ph[CHAIN_TMAX];
    __shared__ u32 s_pos[CHAIN_TMAX];
    __shared__ u32 s_wsum[16], s_total;
    const int W = 2 * Wq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = threadIdx.x % G, rsub = threadIdx.x / G, rows_per_pass = 1024 / G;
    u64 *cur_r = rowsA, *nxt_r = rowsB;
    double *cur_c = coeffA, *nxt_c = coeffB;
    int in_b = 0;
    for (int r = 0; r < K; ++r) {
        const u64 *q = qs + (i64)r * W;
        const int k = ks[r];
        // ---- phase 1: anticommutation flag and phase exponent of every row (G lanes per row, as k_rot_analyze) ----
        int yq = 0;
        for (int w = 0; w < Wq; ++w) yq += __popcll(q[w] & q[Wq + w]);
        for (int t0 = 0; t0 < T; t0 += rows_per_pass) {
            const int t = t0 + rsub;
            u64 par = 0, flip = 0;
            int yp = 0, yout = 0;
            if (t < T) {
                const u64 *row = cur_r + (i64)t * W;
                for (int w = g; w < Wq; w += G) {
                    const u64 x = row[w], z = row[Wq + w], xq = q[w], zq = q[Wq + w];
                    par ^= (x & zq) ^ (z & xq);
                    flip ^= x & zq;
                    yp += __popcll(x & z);
                    yout += __popcll((x ^ xq) & (z ^ zq));
                }
            }
            int pp = __popcll(par) & 1, fp = __popcll(flip) & 1;
            for (int off = G >> 1; off > 0; off >>= 1) {
                pp ^= __shfl_xor(pp, off);
                fp ^= __shfl_xor(fp, off);
                yp += __shfl_xor(yp, off);
                yout += __shfl_xor(yout, off);
            }
            if (g == 0 && t < T) {
                s_anti[t] = (uint8_t)pp;
                s_ph[t] = (uint8_t)((3 * (yp + yq) + yout + 2 * fp) & 3);
            }
        }
        __syncthreads();
        // ---- phase 2: slots of the stable partition [anticommuting | commuting]: thread i owns rows 8i .. 8i+7 ----
        u32 mine = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int t = 8 * (int)threadIdx.x + j; if (t < T) mine += s_anti[t]; }
        const u32 incl = wave_incl_scan(mine, lane);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) { u32 acc = 0; for (int w2 = 0; w2 < 16; ++w2) { const u32 v = s_wsum[w2]; s_wsum[w2] = acc; acc += v; } s_total = acc; }
        __syncthreads();
        const u32 n_anti = s_total;
        if (n_anti == 0) { __syncthreads(); continue; }              // every term commutes with Q: identity (base.py:1131-1133)
        {
            u32 a_before = s_wsum[wave] + incl - mine;                // anticommuting rows before row 8i
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = 8 * (int)threadIdx.x + j;
                if (t < T) {
                    const bool a = s_anti[t];
                    s_pos[t] = a ? a_before : n_anti + ((u32)t - a_before);
                    a_before += a;
                }
            }
        }
        __syncthreads();
        // ---- phase 3: rows and coefficients to their slots in the other buffer ----
        for (int t0 = 0; t0 < T; t0 += rows_per_pass) {
            const int t = t0 + rsub;
            if (t < T) {
                const bool a = s_anti[t];
                const bool flipq = a && (k & 1);
                const u64 *row = cur_r + (i64)t * W;
                u64 *dst = nxt_r + (i64)s_pos[t] * W;
                for (int w = g; w < W; w += G) dst[w] = row[w] ^ (flipq ? q[w] : 0ULL);
                if (g == 0) {
                    double re = cur_c[2 * t], im = cur_c[2 * t + 1];
                    if (a) {
                        if (k & 1) { double x, y; phase_mul(re, im, s_ph[t], x, y); re = y; im = -x; }     // c * i^e * (-i)
                        if (k == 2 || k == 3) { re = -re; im = -im; }
                    }
                    nxt_c[2 * s_pos[t]] = re; nxt_c[2 * s_pos[t] + 1] = im;
                }
            }
        }
        __threadfence_block();
        __syncthreads();
        { u64 *tr = cur_r; cur_r = nxt_r; nxt_r = tr; double *tc = cur_c; cur_c = nxt_c; nxt_c = tc; in_b ^= 1; }
    }
    if (threadIdx.x == 0) *result_in_b = in_b;
}

// The same run with the operator resident in LDS (<= 128 rows and <= 64 KiB of rows: the circuit simulator's observables).  The
// global version above goes through L2 twice per rotation (rows written by the previous rotation are read back by other waves of
// the workgroup: 4.9 us per rotation at 64 rows of 256 bytes); here rows and coefficients ping-pong between two LDS buffers, Q of
// the NEXT rotation is fetched into registers while the current one runs, and a rotation is three barriers.
__global__ __launch_bounds__(1024) void k_clifford_chain_lds(u64 *__restrict__ rows, double *__restrict__ coeff, int T, int Wq, int G,
                                                              const u64 *__restrict__ qs, const int *__restrict__ ks, int K) {
    extern __shared__ __attribute__((aligned(16))) u64 lds_dyn[];    // [2][T * W] rows
    __shared__ double s_c[2][2 * CHAIN_LDS_T];
    __shared__ u64 s_q2[2][128];                                     // Q of this rotation / of the next one (written before the barrier
                                                                      // that ends the previous rotation's row move, which still reads its Q)
    __shared__ uint8_t s_anti[CHAIN_LDS_T], s_ph[CHAIN_LDS_T];
    __shared__ u32 s_pos[CHAIN_LDS_T];
    __shared__ u32 s_cnt[2];
    const int W = 2 * Wq, n_words = T * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = threadIdx.x % G, rsub = threadIdx.x / G, rows_per_pass = 1024 / G;
    u64 *buf0 = lds_dyn, *buf1 = lds_dyn + n_words;
    for (int i = threadIdx.x; i < n_words; i += 1024) buf0[i] = rows[i];
    for (int i = threadIdx.x; i < 2 * T; i += 1024) s_c[0][i] = coeff[i];
    int cur = 0;
    u64 q_next = (K > 0 && (int)threadIdx.x < W) ? qs[threadIdx.x] : 0ULL;
    for (int r = 0; r < K; ++r) {
        const int k = ks[r];
        u64 *s_q = s_q2[r & 1];
        if ((int)threadIdx.x < W) s_q[threadIdx.x] = q_next;
        __syncthreads();                                              // Q in place; the previous rotation's buffers complete
        if (r + 1 < K && (int)threadIdx.x < W) q_next = qs[(i64)(r + 1) * W + threadIdx.x];   // in flight during this rotation
        u64 *cr = cur ? buf1 : buf0, *nr = cur ? buf0 : buf1;
        double *cc = s_c[cur], *ncf = s_c[cur ^ 1];
        // ---- flags + phase exponents (G lanes per row; the Y count of Q is formed along the way by the same lanes) ----
        for (int t0 = 0; t0 < T; t0 += rows_per_pass) {
            const int t = t0 + rsub;
            u64 par = 0, flip = 0;
            int yp = 0, yout = 0, yq = 0;
            if (t < T) {
                const u64 *row = cr + t * W;
                for (int w = g; w < Wq; w += G) {
                    const u64 x = row[w], z = row[Wq + w], xq = s_q[w], zq = s_q[Wq + w];
                    par ^= (x & zq) ^ (z & xq);
                    flip ^= x & zq;
                    yp += __popcll(x & z);
                    yout += __popcll((x ^ xq) & (z ^ zq));
                    yq += __popcll(xq & zq);
                }
            }
            int pp = __popcll(par) & 1, fp = __popcll(flip) & 1;
            for (int off = G >> 1; off > 0; off >>= 1) {
                pp ^= __shfl_xor(pp, off);
                fp ^= __shfl_xor(fp, off);
                yp += __shfl_xor(yp, off);
                yout += __shfl_xor(yout, off);
                yq += __shfl_xor(yq, off);
            }
            if (g == 0 && t < T) {
                s_anti[t] = (uint8_t)pp;
                s_ph[t] = (uint8_t)((3 * (yp + yq) + yout + 2 * fp) & 3);
            }
        }
        __syncthreads();
        // ---- slots of the stable partition [anticommuting | commuting]: waves 0 and 1, one row per lane ----
        if (wave < 2) {
            const int t = wave * 64 + lane;
            const bool a = t < T && s_anti[t];
            const u64 bal = __ballot(a);
            if (lane == 0) s_cnt[wave] = (u32)__popcll(bal);
            s_pos[t < CHAIN_LDS_T ? t : 0] = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));      // rank inside the wave, completed below
        }
        __syncthreads();
        const u32 n0 = s_cnt[0], n_anti = n0 + s_cnt[1];
        if (n_anti == 0) continue;                                    // every term commutes with Q: identity (base.py:1131-1133)
        // ---- rows and coefficients to their slots in the other buffer ----
        for (int t0 = 0; t0 < T; t0 += rows_per_pass) {
            const int t = t0 + rsub;
            if (t < T) {
                const bool a = s_anti[t];
                const u32 a_before = s_pos[t] + (t >= 64 ? n0 : 0u);
                const u32 pos = a ? a_before : n_anti + ((u32)t - a_before);
                const bool flipq = a && (k & 1);
                const u64 *row = cr + t * W;
                u64 *dst = nr + pos * W;
                for (int w = g; w < W; w += G) dst[w] = row[w] ^ (flipq ? s_q[w] : 0ULL);
                if (g == 0) {
                    double re = cc[2 * t], im = cc[2 * t + 1];
                    if (a) {
                        if (k & 1) { double x, y; phase_mul(re, im, s_ph[t], x, y); re = y; im = -x; }     // c * i^e * (-i)
                        if (k == 2 || k == 3) { re = -re; im = -im; }
                    }
                    ncf[2 * pos] = re; ncf[2 * pos + 1] = im;
                }
            }
        }
        cur ^= 1;                                                     // the barrier at the top of the next rotation completes the move
    }
    __syncthreads();
    const u64 *fr = cur ? buf1 : buf0;
    for (int i = threadIdx.x; i < n_words; i += 1024) rows[i] = fr[i];
    for (int i = threadIdx.x; i < 2 * T; i += 1024) coeff[i] = s_c[cur][i];
}


// ---- a run of Clifford rotations of a CLEAN operator, two launches per rotation -----------------------------------------------------
// Back-to-back launches are launch-rate bound (3.9 us per launch, four per rotation: 15.6 us at any size up to 8,000 rows).  For a
// clean operator a Clifford rotation is just a stable partition [anticommuting | commuting] with new coefficients, so two launches
// do: (A) flags, phase exponents, the new coefficient of every row and the anticommuting count of every 1024-row group, one 16-byte
// chunk per lane as in k_rot_analyze_chunks; (B) every block derives the output slots of its own rows — groups before it from the
// <= 256 group counts, rows before it inside its group from their byte flags — and moves rows and coefficients.  The group counts
// ping-pong between two arrays (B of rotation r clears the array A of rotation r+1 adds to).  Rows of a power-of-two number of chunks,
// <= CHAIN_TWO_T rows; everything else keeps the four-launch form.
template <int WQ, int CCH_ROWS>
__global__ __launch_bounds__(256) void k_cchain_flags(const u32x4 *__restrict__ rows, const double *__restrict__ coeff, i64 T, const u64 *__restrict__ q_dev,
                                                       int k, uint8_t *__restrict__ af, double *__restrict__ nc, u32 *__restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) u64 sq[2 * WQ];
    __shared__ int s_yq;
    __shared__ u32 s_n;
    if ((int)threadIdx.x < 2 * WQ) sq[threadIdx.x] = q_dev[threadIdx.x];
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (threadIdx.x < 64) {                                          // Y count of Q: one wavefront
        int y = 0;
        for (int w = threadIdx.x; w < WQ; w += 64) y += __popcll(sq[w] & sq[WQ + w]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) y += __shfl_xor(y, off);
        if (threadIdx.x == 0) s_yq = y;
    }
    __syncthreads();
    constexpr int R = 256 / WQ, ITER = CCH_ROWS / R;                 // CCH_ROWS rows per block: the block's fixed costs are paid once
    const int c = threadIdx.x & (WQ - 1);
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const i64 t = (i64)blockIdx.x * CCH_ROWS + it * R + threadIdx.x / WQ;
        const bool valid = t < T;
        const u32x4 v = valid ? rows[t * WQ + c] : (u32x4)(0u);
        u32 par, ye;
        if constexpr (WQ == 1) {
            const u32x4 qv = *reinterpret_cast<const u32x4 *>(sq);
            const u32 f = __popc(v.x & qv.z) + __popc(v.y & qv.w);
            par = f + __popc(v.z & qv.x) + __popc(v.w & qv.y) + (f << 16);
            ye = (__popc(v.x & v.z) + __popc(v.y & v.w)) | ((__popc((v.x ^ qv.x) & (v.z ^ qv.z)) + __popc((v.y ^ qv.y) & (v.w ^ qv.w))) << 16);
        } else {
            const u32x4 qs = reinterpret_cast<const u32x4 *>(sq)[c], qo = reinterpret_cast<const u32x4 *>(sq)[c ^ (WQ / 2)];
            const bool xhalf = c < WQ / 2;
            const u32 p = __popc(v.x & qo.x) + __popc(v.y & qo.y) + __popc(v.z & qo.z) + __popc(v.w & qo.w);
            const u32x4 o = {rot_other_half<WQ>(v.x), rot_other_half<WQ>(v.y), rot_other_half<WQ>(v.z), rot_other_half<WQ>(v.w)};
            const u32 yp = __popc(v.x & o.x) + __popc(v.y & o.y) + __popc(v.z & o.z) + __popc(v.w & o.w);
            const u32 yo = __popc((v.x ^ qs.x) & (o.x ^ qo.x)) + __popc((v.y ^ qs.y) & (o.y ^ qo.y)) + __popc((v.z ^ qs.z) & (o.z ^ qo.z)) +
                           __popc((v.w ^ qs.w) & (o.w ^ qo.w));
            par = rot_row_sum<WQ>(p + (xhalf ? (p << 16) : 0u));
            ye = rot_row_sum<WQ>(xhalf ? (yp | (yo << 16)) : 0u);
        }
        if (c == 0 && valid) {
            const bool anti = par & 1u;
            const int e = (int)((3u * ((ye & 0xFFFFu) + (u32)s_yq) + (ye >> 16) + 2u * ((par >> 16) & 1u)) & 3u);
            double re = coeff[2 * t], im = coeff[2 * t + 1];
            if (anti) {
                if (k & 1) {                                          // c * i^e * (-i), negated for k = 3 (k_rotc_classify)
                    double x, y;
                    phase_mul(re, im, e, x, y);
                    re = y; im = -x;
                    if (k == 3) { re = -re; im = -im; }
                } else if (k == 2) { re = -re; im = -im; }
                atomicAdd(&s_n, 1u);
            }
            af[t] = anti ? 1 : 0;
            nc[2 * t] = re; nc[2 * t + 1] = im;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(&cnt[((i64)blockIdx.x * CCH_ROWS) >> 10], s_n);   // CCH_ROWS divides 1024: a block lies inside one group
}

template <int WQ, int CCH_ROWS>
__global__ __launch_bounds__(256) void k_cchain_move(const u32x4 *__restrict__ rows, i64 T, const u64 *__restrict__ q_dev, int k,
                                                      const uint8_t *__restrict__ af, const double *__restrict__ nc, const u32 *__restrict__ cnt,
                                                      int n_cnt, u32 *__restrict__ cnt_next, u32x4 *__restrict__ out_rows, double *__restrict__ out_coeff) {
    constexpr int R = 256 / WQ, ITER = CCH_ROWS / R;
    __shared__ u32 s_sum[3];                                          // anticommuting rows: in the groups before, in all groups, before the block inside its group
    __shared__ uint8_t s_flag[CCH_ROWS];
    __shared__ u32 s_pos[CCH_ROWS];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const i64 t0 = (i64)blockIdx.x * CCH_ROWS;
    const int g = (int)(t0 >> 10);
    const i64 g0 = (i64)g << 10;
    u32 before = 0, all = 0, inside = 0;
    if ((int)threadIdx.x < n_cnt) {
        const u32 x = cnt[threadIdx.x];
        all = x;
        if ((int)threadIdx.x < g) before = x;
    }
    {   // byte flags of the rows [g0, t0): at most 1020 bytes, one u32 per thread (t0 - g0 is a multiple of CCH_ROWS >= 4)
        const i64 w = g0 + 4 * (i64)threadIdx.x;
        if (w < t0) inside = (*reinterpret_cast<const u32 *>(af + w) * 0x01010101u) >> 24;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        before += (u32)__shfl_xor((int)before, off); all += (u32)__shfl_xor((int)all, off); inside += (u32)__shfl_xor((int)inside, off);
    }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_sum[0], before); atomicAdd(&s_sum[1], all); atomicAdd(&s_sum[2], inside); }
    if (blockIdx.x == 0 && (int)threadIdx.x < n_cnt) cnt_next[threadIdx.x] = 0;      // the array the next rotation's flags kernel adds to
    if ((int)threadIdx.x < CCH_ROWS) s_flag[threadIdx.x] = (t0 + threadIdx.x < T) ? af[t0 + threadIdx.x] : 0;
    __syncthreads();
    if ((int)threadIdx.x < CCH_ROWS && t0 + threadIdx.x < T) {
        // rank among the block's rows: the flags of the same wavefront's lower lanes (CCH_ROWS <= 256: up to 4 wavefronts)
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const u64 bal = __ballot(s_flag[threadIdx.x] != 0);
        u32 rank = (u32)__popcll(bal & ((1ULL << lane) - 1ULL));
        for (int w2 = 0; w2 < wv; ++w2)
            for (int r = 0; r < 64; ++r) rank += s_flag[w2 * 64 + r];
        const u32 a_before = s_sum[0] + s_sum[2] + rank;              // anticommuting rows before this one
        const i64 t = t0 + threadIdx.x;
        const u32 pos = s_flag[threadIdx.x] ? a_before : s_sum[1] + (u32)(t - a_before);
        s_pos[threadIdx.x] = pos;
        reinterpret_cast<f64x2 *>(out_coeff)[pos] = reinterpret_cast<const f64x2 *>(nc)[t];
    }
    __syncthreads();
    const int c = threadIdx.x & (WQ - 1);
    const u32x4 qc = reinterpret_cast<const u32x4 *>(q_dev)[c];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int rl = it * R + threadIdx.x / WQ;
        const i64 t = t0 + rl;
        if (t < T) {
            u32x4 v = rows[t * WQ + c];
            if (s_flag[rl] && (k & 1)) v ^= qc;
            out_rows[(i64)s_pos[rl] * WQ + c] = v;
        }
    }
}

bool chain_lds_attr_ok() {
    return SG_DEVICE_ONCE(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_clifford_chain_lds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              128 * 1024) == hipSuccess);
}

// small operator, resident in LDS for the whole run: the result is back in `a`
int chain_lds(const ChainRun &c, int *in_b) {
    hipLaunchKernelGGL(k_clifford_chain_lds, dim3(1), dim3(1024), (size_t)2 * c.T * 2 * c.Wq * 8, ctx().stream, c.a->rows, c.a->coeff, (int)c.T, c.Wq,
                       row_lanes(c.Wq), c.qs, c.ks, (int)c.K);
    *in_b = 0;
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

// small operator: the whole run in one single-workgroup launch
int chain_single_workgroup(const ChainRun &c, int *in_b) {
    hipStream_t st = ctx().stream;
    Scratch which;
    SG_TRY(which.alloc(16));
    hipLaunchKernelGGL(k_clifford_chain, dim3(1), dim3(1024), 0, st, c.a->rows, c.a->coeff, c.b->rows, c.b->coeff, (int)c.T, c.Wq, row_lanes(c.Wq), c.qs,
                       c.ks, (int)c.K, which.as<int>());
    KERNEL_CHECK();
    HIP_TRY(hipMemcpyAsync(in_b, which.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                                  // `which` goes back to the allocator on return
    return SYMGPU_OK;
}

// two launches per rotation (k_cchain_flags / k_cchain_move): rows of a power-of-two number of chunks <= 64
int chain_two_launch(const ChainRun &c, int *in_b) {
    hipStream_t st = ctx().stream;
    const i64 T = c.T;
    const int W = 2 * c.Wq;
    Scratch af, nc, cnts;
    const int n_cnt = (int)((T + 1023) / 1024);
    SG_TRY(af.alloc((size_t)T + 1024));
    SG_TRY(nc.alloc((size_t)T * 16));
    SG_TRY(cnts.alloc(2 * 256 * sizeof(u32)));
    HIP_TRY(hipMemsetAsync(cnts.p, 0, 2 * 256 * sizeof(u32), st));
    symgpu_op_t cur = c.a, nxt = c.b;
    // rows per block: 256 / WQ (one pass: lowest latency, 6.7-7.1 us per rotation up to 1,000 rows) or 64 (the block's fixed
    // costs — Q, group counts, flag prefix — paid once per four passes: 10.4 / 13.4 / 20.8 / 26.7 us at 8,000 / 16,384 /
    // 65,536 / 131,072 rows against 12.9 / 20.7 / 40.2 / 59.3 us)
    const bool big = T > 4096;
    auto rotate = [&](i64 r, auto wq, auto rows_per_block) {
        constexpr int WQ = decltype(wq)::value, ROWS = decltype(rows_per_block)::value;
        const u64 *q = c.qs + r * W;
        u32 *c_now = cnts.as<u32>() + (r & 1) * 256, *c_next = cnts.as<u32>() + ((r + 1) & 1) * 256;
        const u32x4 *src = reinterpret_cast<const u32x4 *>(cur->rows);
        const i64 gb = (T + ROWS - 1) / ROWS;
        hipLaunchKernelGGL((k_cchain_flags<WQ, ROWS>), dim3((unsigned)gb), dim3(256), 0, st, src, cur->coeff, T, q, c.ks_host[r], af.as<uint8_t>(), nc.as<double>(), c_now);
        hipLaunchKernelGGL((k_cchain_move<WQ, ROWS>), dim3((unsigned)gb), dim3(256), 0, st, src, T, q, c.ks_host[r], af.as<uint8_t>(), nc.as<double>(), c_now, n_cnt,
                           c_next, reinterpret_cast<u32x4 *>(nxt->rows), nxt->coeff);
    };
    wq_dispatch<64, 1, 2, 4, 8, 16, 32>(c.Wq, [&](auto wq) {
        constexpr int ONE_PASS = 256 / decltype(wq)::value;
        for (i64 r = 0; r < c.K; ++r) {
            if (big && ONE_PASS < 64) rotate(r, wq, std::integral_constant<int, 64>{});
            else rotate(r, wq, std::integral_constant<int, ONE_PASS>{});
            symgpu_op_t t2 = cur; cur = nxt; nxt = t2;
        }
    });
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(st));                                  // the scratch buffers go back to the allocator on return
    *in_b = (cur == c.b) ? 1 : 0;
    return SYMGPU_OK;
}

// large operator: the per-rotation kernels of the Clifford fast path (rotate_fast.hip), enqueued back to back — T is constant for a
// clean operator (nothing is dropped: thr = -1), so no count has to come back to the host between the rotations
int chain_four_launch(const ChainRun &c, int *in_b) {
    hipStream_t st = ctx().stream;
    const i64 T = c.T;
    const int W = 2 * c.Wq;
    Scratch anti, ph;
    RotScratch s;
    SG_TRY(anti.alloc((size_t)T * 4));
    SG_TRY(ph.alloc((size_t)T));
    SG_TRY(s.alloc(T));
    symgpu_op_t cur = c.a, nxt = c.b;
    for (i64 r = 0; r < c.K; ++r) {
        u64 *q = c.qs + r * W;
        cur->T = T;
        SG_TRY(analyze_rows(cur, q, anti.as<u32>(), ph.as<uint8_t>(), nullptr, c.sw));   // flags + phase exponents (chunk-per-lane kernel where the row length allows it)
        clifford_classify_scan_write(cur->rows, cur->coeff, q, anti.as<u32>(), ph.as<uint8_t>(), T, c.Wq, c.ks_host[r], -1.0, s, nullptr, nxt->rows,
                                     nxt->coeff, nullptr, 0, nullptr);
        symgpu_op_t t2 = cur; cur = nxt; nxt = t2;
    }
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(st));                                  // the scratch buffers go back to the allocator on return
    *in_b = (cur == c.b) ? 1 : 0;
    return SYMGPU_OK;
}

}  // namespace symgpu
