// rotate_resident_kernel.hip — a single-Pauli rotation (reference: PauliwordOp._rotate_by_single_Pword, symmer/operators/base.py:1090-1161)
// as ONE persistent launch: the kernel, phase by phase, and the function that launches a planned call.
//
// The multi-launch paths (rotate_analyze.hip, rotate_fast.hip: analyze | match | scan | write) are bound by their three kernel boundaries, by the second
// pass over the rows and by the host round trips between them, not by bytes: 40 us of kernels for 8.5 us of traffic at 10^5 terms of
// 1,000 qubits.  Here the operator is spread over the chip instead: one workgroup per CU, each owning a contiguous block of
// ceil(T / G) rows that it reads from HBM ONCE into its LDS (256 CUs x <= 150 KiB = 38 MB of operator; BASELINE cfg2 is 25.6 MB),
// and everything that the kernel boundaries used to order is ordered inside the launch by two all-gathers of 8-byte granules
// {tag, counts} (cdna_hip_programming.md Guideline 16, form R2: the data is the flag, agent-scope relaxed stores and loads, no fence
// because no plain-stored payload crosses workgroups):
//
//   A   rows -> LDS, with the flags and phase exponents of every row formed on the way in registers (one 16-byte chunk per lane, DPP
//       lane exchange as in product.hip's row stream; rows that are not a power-of-two number of chunks: from LDS afterwards);
//       non-Clifford: every anticommuting row enters the join table with ONE compare-and-swap under its CANONICAL key
//       min(h, h ^ h(Q)) — a row P_k and the row P_k ^ Q it would merge with share that key, so whoever of the two comes second
//       finds the other in the slot, notes it in LDS and tells the first through partner[] (agent-scope store).  Table and notes
//       are all-zero between launches: every claimed slot and every note read is zeroed again by its owner after all-gather #1
//   g1  all-gather #1: kept commuting rows per workgroup (and: every partner note is in place)
//   B   final coefficients (cos c_t + (-i sin) i^e' c_partner, or the new row's (-i sin) i^e c_t), classes, ranks inside the block
//   g2  all-gather #2: kept anticommuting / new rows per workgroup; the commuting rows are written while it is in flight
//   C   rows (LDS -> HBM, 16 bytes per lane), coefficients and handed-on hashes to their final slots; counts to pinned host memory
//
// Output order, sums and thresholds are those of the hash-join path (rotate_fast.hip) (commuting | cos * anticommuting (+ partner) | new rows,
// strict |c| > thr; Clifford: rotated anticommuting | commuting), bit for bit — tests/test_gpu_parity.py runs both.
// Exactness does not rest on the hash: the second row of every pair is compared with its partner chunk by chunk (row ^ Q against
// the partner's row in HBM); a mismatch, a third row under one canonical key, or an all-gather that does not complete (workgroups
// not co-resident) makes the call report failure and the caller takes the multi-launch path.
#include "rotate_resident.h"

namespace symgpu {

enum { M_OK = 1, M_FAIL = 2, M_NC = 3, M_NA = 4, M_NN = 5, M_NANTI = 6, M_PREF_C = 8, M_TOT_C = 9, M_PREF_A = 10, M_TOT_A = 11, M_PREF_N = 12,
       M_TOT_N = 13, M_TOT_ANTI = 14 };

// What the phases of one workgroup share: its LDS (res_layout), its block of rows, and the two row chunks per lane that the Registers
// form keeps out of LDS.
struct ResBlock {
    u32x4 *s_rows; f64x2 *s_coef;
    u32 *s_ps;                                    // join state, later: rank of the row in its class
    u32 *s_posn;                                  // (high word of a pending row's occupant), later: rank of the new row
    uint8_t *s_info, *s_cls; u64 *s_q, *s_wtot; u32 *s_misc;
    const u32x4 *sq4, *rows_blk;                  // s_q as chunks; the block's rows in memory
    i64 row0; int Rw, nchunk, Wq;                 // first row, rows and chunks of the block, chunks per row
    int nreg, reg_chunks;                         // chunks [0, reg_chunks) of the block live in keep0 / keep1
    bool hbm;                                     // (block-uniform) rows read again from memory where they are needed
    int tid, lane, wave, G, w;
    u32x4 &keep0, &keep1;
};

__device__ __forceinline__ u64 ag_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ag_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 ag_load32(const u32 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ag_store32(u32 *p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One wavefront re-reads all G granules until every tag is `tag`; on success the three count fields (16, 16 and 15 bits) are summed
// over the workgroups before `w` (pref) and over all of them (tot); `flagged`: some workgroup set RES_GRAN_FAIL.  Returns false
// after RES_SPIN_LIMIT sweeps.
__device__ __forceinline__ bool ag_sweep(const u64 *gran, int G, u32 tag, int w, int lane, u32 (&pref)[3], u32 (&tot)[3], bool &flagged) {
    u64 v[4];
    for (u32 spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = lane + 64 * j;
            v[j] = idx < G ? ag_load(gran + idx) : ((u64)tag << 48);
            ok &= (u32)(v[j] >> 48) == tag;
        }
        if (__ballot(ok) == ~0ULL) break;
        if (spins >= RES_SPIN_LIMIT) return false;
        __builtin_amdgcn_s_sleep(2);
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) { pref[f] = 0; tot[f] = 0; }
    bool fl = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = lane + 64 * j;
        if (idx < G) {
            fl |= (v[j] & RES_GRAN_FAIL) != 0;
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                const u32 x = (u32)(v[j] >> (16 * f)) & (f == 2 ? 0x7FFFu : 0xFFFFu);
                tot[f] += x;
                if (idx < w) pref[f] += x;
            }
        }
    }
#pragma unroll
    for (int f = 0; f < 3; ++f)
        for (int off = 32; off > 0; off >>= 1) { pref[f] += (u32)__shfl_xor((int)pref[f], off); tot[f] += (u32)__shfl_xor((int)tot[f], off); }
    flagged = __ballot(fl) != 0ULL;
    return true;
}

// The counts of a launch in pinned host memory: two 8-byte words that carry the call's tag — the data is the flag, the host waits
// until both show it.  [tag 16 | nC 22 | nA 22], [tag 16 | code 4 | nN 22 | nAnti 22]
__device__ __forceinline__ void res_report(const ResArgs &a, u32 code, u32 nC, u32 nA, u32 nN, u32 nAnti) {
    __hip_atomic_store(&a.host_words[0], ((u64)a.host_tag << 48) | ((u64)nC << 22) | nA, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&a.host_words[1], ((u64)a.host_tag << 48) | ((u64)code << 44) | ((u64)nN << 22) | nAnti, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A workgroup leaves (done or timed out).  Success is reported EARLY, by one workgroup as soon as the second all-gather has told it
// the counts (res_early_report): the host prepares and enqueues whatever comes next while the rows are still on their way out.  Failures
// are reported by the LAST workgroup to leave — it sees every failure word written before the others' arrivals; should one appear
// after success has been reported (a time-out behind a completed all-gather: not reachable by construction) it goes to the `late`
// word, which fails the next call loudly.
__device__ __forceinline__ void res_leave(const ResArgs &a) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const u32 prev = atomicAdd(a.finished, 1u);
    if (prev + 1u == a.finish_target) {
        u32 code = 0;
        if (ag_load32(&a.fail[0]) == a.epoch) code = 2;
        if (ag_load32(&a.fail[1]) == a.epoch) code = 3;
        if (code) {
            if (ag_load32(a.published) == a.epoch) __hip_atomic_store(a.host_late, ((u32)a.epoch << 4) | code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else res_report(a, code, 0, 0, 0, 1);
        }
    }
}
// 0 + c, as the reference's cleanup forms every coefficient of a non-Clifford rotation (a zero component leaves as +0)
__device__ __forceinline__ f64x2 plus_zero(f64x2 c) { return f64x2{__dadd_rn(0.0, c.x), __dadd_rn(0.0, c.y)}; }
// rows leave with non-temporal stores; write-through (sc0 sc1) stores measured the same kernel duration (27.5 us)
__device__ __forceinline__ void row_store(u32x4 v, u32x4 *p) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void res_stamp(const ResArgs &a, const ResBlock &b, int i) {
    if (a.trace && b.tid == 0) a.trace[(size_t)b.w * 16 + i] = wall_clock64();
}
// flag and the two phase exponents of a row from its counts (k_rot_analyze, rotate_analyze.hip): bit 0 = anticommutes with Q, bits 1-2 = the
// exponent e of P * Q, bits 3-4 = the exponent e' of (P ^ Q) * Q, i.e. the e of the row's partner
__device__ __forceinline__ uint8_t res_info(u32 anti, u32 fp, u32 yp, u32 yout, u32 yq) {
    const u32 e = (3u * (yp + yq) + yout + 2u * fp) & 3u;
    const u32 ep = (3u * (yout + yq) + yp + 2u * (fp ^ (yq & 1u))) & 3u;
    return (uint8_t)((anti & 1u) | (e << 1) | (ep << 3));
}
// chunk `it * 1024 + tid` of the block, from memory, from the registers or from LDS
__device__ __forceinline__ u32x4 res_chunk(const ResBlock &b, int it, int i) {
    return b.hbm ? b.rows_blk[i] : ((it < b.nreg) ? (it == 0 ? b.keep0 : b.keep1) : b.s_rows[i - b.reg_chunks]);
}
// f(it, i, r, c) for every chunk i = it * 1024 + tid of the block that this thread holds: chunk c of row r
template <class F> __device__ __forceinline__ void res_for_chunks(const ResBlock &b, F f) {
    const int Wq = b.Wq;
    int r = b.tid / Wq, c = b.tid - r * Wq;
    const int dr = RES_THREADS / Wq, dc = RES_THREADS - dr * Wq;
    for (int it = 0, i = b.tid; i < b.nchunk; ++it, i += RES_THREADS) {
        f(it, i, r, c);
        r += dr; c += dc;
        if (c >= Wq) { c -= Wq; ++r; }
    }
}

// The workgroup's views of its LDS and of its block.  WQ: see k_rot_resident
template <int WQ> __device__ __forceinline__ ResBlock res_block(const ResArgs &a, unsigned char *smem, u32x4 &keep0, u32x4 &keep1) {
    const int nreg = WQ > 0 ? a.nreg : 0;                                      // (rows of a generic length are analysed from LDS: all of them live there)
    const bool hbm = a.hbm != 0;
    const ResLayout L = res_layout(a.R, a.Wq, nreg, hbm ? 1 : 0);
    const int tid = threadIdx.x, Wq = WQ > 0 ? WQ : a.Wq, w = blockIdx.x;
    const i64 row0 = (i64)w * a.R;
    const int Rw = (int)(a.T - row0 < (i64)a.R ? a.T - row0 : (i64)a.R);
    u64 *s_q = reinterpret_cast<u64 *>(smem + L.q);
    return ResBlock{reinterpret_cast<u32x4 *>(smem + L.rows), reinterpret_cast<f64x2 *>(smem + L.coef), reinterpret_cast<u32 *>(smem + L.ps),
                    reinterpret_cast<u32 *>(smem + L.posn), smem + L.info, smem + L.cls, s_q, reinterpret_cast<u64 *>(smem + L.wtot),
                    reinterpret_cast<u32 *>(smem + L.misc), reinterpret_cast<const u32x4 *>(s_q), a.rows + row0 * Wq, row0, Rw, Rw * Wq, Wq,
                    nreg, nreg * RES_THREADS, hbm, tid, tid & 63, tid >> 6, (int)gridDim.x, w, keep0, keep1};
}

// The counts of chunk x, held by lane c of its row's WQ lanes, summed over the row: par = |x & zq| + |z & xq| (+ |x & zq| << 16),
// ye = Y_P | Y_out << 16.  A row is an aligned group of WQ lanes (RES_THREADS is a multiple of WQ): X words in its lower, Z words in its upper half
template <int WQ> __device__ __forceinline__ void res_chunk_counts(u32x4 x, const u32x4 *sq4, int c, u32 &par, u32 &ye) {
    if constexpr (WQ == 1) {
        const u32x4 qv = sq4[0];
        const u32 f = __popc(x.x & qv.z) + __popc(x.y & qv.w);
        par = f + __popc(x.z & qv.x) + __popc(x.w & qv.y) + (f << 16);
        ye = (__popc(x.x & x.z) + __popc(x.y & x.w)) | ((__popc((x.x ^ qv.x) & (x.z ^ qv.z)) + __popc((x.y ^ qv.y) & (x.w ^ qv.w))) << 16);
    } else {
        const u32x4 qs = sq4[c], qo = sq4[c ^ (WQ / 2)];
        const bool xhalf = c < WQ / 2;
        const u32 p = __popc(x.x & qo.x) + __popc(x.y & qo.y) + __popc(x.z & qo.z) + __popc(x.w & qo.w);
        const u32x4 o = {rot_other_half<WQ>(x.x), rot_other_half<WQ>(x.y), rot_other_half<WQ>(x.z), rot_other_half<WQ>(x.w)};
        const u32 yp = __popc(x.x & o.x) + __popc(x.y & o.y) + __popc(x.z & o.z) + __popc(x.w & o.w);
        const u32 yo = __popc((x.x ^ qs.x) & (o.x ^ qo.x)) + __popc((x.y ^ qs.y) & (o.y ^ qo.y)) + __popc((x.z ^ qs.z) & (o.z ^ qo.z)) +
                       __popc((x.w ^ qs.w) & (o.w ^ qo.w));
        par = rot_row_sum<WQ>(p + (xhalf ? (p << 16) : 0u));
        ye = rot_row_sum<WQ>(xhalf ? (yp | (yo << 16)) : 0u);
    }
}

// ---- A1: the block's rows and coefficients: HBM -> registers / LDS, read once; flags and phase exponents on the way ---------------
template <int MODE, int WQ> __device__ __forceinline__ void res_A1(const ResArgs &a, const ResBlock &b) {
    const int tid = b.tid, nchunk = b.nchunk, Rw = b.Rw;
    const bool hbm = b.hbm;
    const i64 row0 = b.row0;
    const f64x2 *coeff2 = reinterpret_cast<const f64x2 *>(a.coeff);
    const u32x4 *src = a.rows + row0 * b.Wq;
    if (WQ == 0 && hbm)                                                        // (nothing to do with the rows here: A2 analyses them from memory)
        for (int r = tid; r < Rw; r += RES_THREADS) b.s_coef[r] = coeff2[row0 + r];
    for (int i0 = 0; i0 < ((WQ == 0 && hbm) ? 0 : nchunk); i0 += RES_LD_UNROLL * RES_THREADS) {
        u32x4 v[RES_LD_UNROLL];
#pragma unroll
        for (int j = 0; j < RES_LD_UNROLL; ++j) {
            const int i = i0 + j * RES_THREADS + tid;
            v[j] = i < nchunk ? (hbm ? src[i] : __builtin_nontemporal_load(src + i)) : (u32x4)(0u);   // (hbm: the rows are read again: no streaming hint)
        }
        if (i0 == 0)
            for (int r = tid; r < Rw; r += RES_THREADS) b.s_coef[r] = coeff2[row0 + r];
        // hashes, probed slots and answers of this round's rows.  (One struct on purpose: arrays of their own are turned into 16-register
        // vectors before the loops over j are unrolled — the kernel then needs more than its 128 registers and spills.)
        struct { u64 hrow[RES_LD_UNROLL], casold[RES_LD_UNROLL]; u32 caspos[RES_LD_UNROLL]; } p;
        if constexpr (WQ > 0) {
            const int c = tid & (WQ - 1);
            // non-Clifford: the chunk-0 lane of an anticommuting row issues the row's compare-and-swap on the join table as soon as
            // the flag is known; the answers (~2 us each) come back while the remaining chunks are analysed and stored
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < RES_LD_UNROLL; ++j) {
                    const int i = i0 + j * RES_THREADS + tid;
                    p.hrow[j] = (c == 0 && i < nchunk) ? a.hin[row0 + i / WQ] : 0ULL;
                    p.casold[j] = 0; p.caspos[j] = RES_NO_SLOT;
                }
            }
#pragma unroll
            for (int j = 0; j < RES_LD_UNROLL; ++j) {
                const int i = i0 + j * RES_THREADS + tid;
                u32 par, ye;
                res_chunk_counts<WQ>(v[j], b.sq4, c, par, ye);
                if (c == 0 && i < nchunk) {
                    b.s_info[i / WQ] = res_info(par & 1u, (par >> 16) & 1u, ye & 0xFFFFu, ye >> 16, a.yq);
                    if (MODE == 0 && (par & 1u)) {
                        const u64 h = p.hrow[j], hp = h ^ a.hq, ck = h < hp ? h : hp;
                        p.caspos[j] = (u32)mix64(ck) & a.mask;
                        p.casold[j] = atomicCAS(reinterpret_cast<unsigned long long *>(&a.slots[p.caspos[j]]), 0ULL,
                                              (unsigned long long)((ck & 0xFFFFFFFF00000000ULL) | (u64)(row0 + i / WQ + 1)));
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RES_LD_UNROLL; ++j) {
            const int i = i0 + j * RES_THREADS + tid;
            if (i0 == 0 && j < 2 && j < b.nreg) { if (j == 0) b.keep0 = v[j]; else b.keep1 = v[j]; }
            else if (i < nchunk && !hbm) b.s_rows[i - b.reg_chunks] = v[j];
        }
        if constexpr (WQ > 0 && MODE == 0) {
            // What the first probes found (only now: the empty statement keeps the compiler from testing each answer right behind
            // its compare-and-swap, which would serialise the eight round trips): 0 = the slot is this row's; an occupant is
            // left in {s_posn : s_ps} for A3, which continues the walk from there.
            asm volatile("" : "+v"(p.casold[0]), "+v"(p.casold[1]), "+v"(p.casold[2]), "+v"(p.casold[3]), "+v"(p.casold[4]), "+v"(p.casold[5]), "+v"(p.casold[6]), "+v"(p.casold[7]));
            static_assert(RES_LD_UNROLL == 8, "the statement above names eight answers");
            const int c = tid & (WQ - 1);
#pragma unroll
            for (int j = 0; j < RES_LD_UNROLL; ++j) {
                const int i = i0 + j * RES_THREADS + tid;
                if (c == 0 && i < nchunk) {
                    const bool anti = p.caspos[j] != RES_NO_SLOT, pending = anti && p.casold[j] != 0;
                    b.s_ps[i / WQ] = pending ? (u32)p.casold[j] : p.caspos[j];
                    b.s_posn[i / WQ] = (u32)(p.casold[j] >> 32);
                    b.s_cls[i / WQ] = (uint8_t)(pending ? CL_PENDING : (anti ? CL_CLAIMED : 0));
                }
            }
        }
    }
}

// ---- A2: flags and phase exponents from LDS, GA lanes per row (row lengths that are not a power-of-two number of chunks) ----------
__device__ __forceinline__ void res_A2(const ResArgs &a, const ResBlock &b) {
    const int Wq = b.Wq, W = 2 * Wq, Rw = b.Rw;
    const int GA = a.GA, g = b.tid & (GA - 1), rsub = b.tid / GA, rpp = RES_THREADS / GA;
    const u64 *rows64 = b.hbm ? reinterpret_cast<const u64 *>(b.rows_blk) : reinterpret_cast<const u64 *>(b.s_rows);
    for (int r0 = 0; r0 < Rw; r0 += rpp) {
        const int r = r0 + rsub;
        u32 pf = 0, yy = 0;                     // pf: parity of |x & zq| + |z & xq| (bit 0) and of |x & zq| (bit 1); yy: Y_P | Y_out << 16
        if (r < Rw) {
            const u64 *row = rows64 + (size_t)r * W;
            u64 par = 0, flip = 0;
            for (int ww = g; ww < Wq; ww += GA) {
                const u64 x = row[ww], z = row[Wq + ww], xq = b.s_q[ww], zq = b.s_q[Wq + ww];
                par ^= (x & zq) ^ (z & xq);
                flip ^= x & zq;
                yy += (u32)__popcll(x & z) + ((u32)__popcll((x ^ xq) & (z ^ zq)) << 16);
            }
            pf = ((u32)__popcll(par) & 1u) | (((u32)__popcll(flip) & 1u) << 1);
        }
        for (int off = GA >> 1; off > 0; off >>= 1) { pf ^= (u32)__shfl_xor((int)pf, off); yy += (u32)__shfl_xor((int)yy, off); }
        if (g == 0 && r < Rw) b.s_info[r] = res_info(pf & 1u, (pf >> 1) & 1u, yy & 0xFFFFu, yy >> 16, a.yq);
    }
    __syncthreads();
}

// ---- A3: commuting rows are classified; every anticommuting row meets its partner, if it has one, in the join table; the block's
//      granule of all-gather #1 leaves ---------------------------------------------------------------------------------------------
template <int WQ> __device__ __forceinline__ void res_A3(const ResArgs &a, const ResBlock &b) {
    u32 nC = 0;
    bool bad = false;
    for (int r = b.tid; r < b.Rw; r += RES_THREADS) {
        const uint8_t info = b.s_info[r];
        uint8_t cls = 0;
        u32 ps = 0;
        if (!(info & 1)) {
            const f64x2 c = b.s_coef[r];
            if (above_thr(c.x, c.y, a.thr)) { cls = CL_C; ++nC; }
        } else if (WQ > 0 && (b.s_cls[r] & CL_CLAIMED)) {
            cls = CL_CLAIMED; ps = b.s_ps[r];                                  // claimed by the probe issued from the load loop
        } else {
            // generic row lengths: the whole walk; otherwise: the first probe met the occupant left in {s_posn : s_ps} — the walk goes on there
            const i64 t = b.row0 + r;
            const u64 h = a.hin[t], hp = h ^ a.hq, ck = h < hp ? h : hp;
            const u64 entry = (ck & 0xFFFFFFFF00000000ULL) | (u64)(t + 1);
            u32 pos = (u32)mix64(ck) & a.mask;
            bool have_old = WQ > 0;
            for (;;) {
                const u64 old = have_old ? (((u64)b.s_posn[r] << 32) | b.s_ps[r])
                                         : atomicCAS(reinterpret_cast<unsigned long long *>(&a.slots[pos]), 0ULL, (unsigned long long)entry);
                have_old = false;
                if (old == 0) { cls = CL_CLAIMED; ps = pos; break; }           // first of its key: a partner, if any, will leave a note
                if ((old >> 32) == (ck >> 32)) {
                    const i64 o = (i64)(old & 0xFFFFFFFFULL) - 1;
                    const u64 ho = a.hin[o];
                    if (ho == hp) {                                            // the row this one merges with (verified below)
                        cls = CL_SECOND; ps = (u32)o;
                        ag_store32(&a.partner[o], (u32)(t + 1));
                        break;
                    }
                    if (ho == h) { bad = true; break; }                        // two rows with one hash: not for this path
                }
                pos = (pos + 1) & a.mask;
            }
        }
        b.s_ps[r] = ps;
        b.s_cls[r] = cls;
    }
    for (int off = 32; off > 0; off >>= 1) nC += (u32)__shfl_xor((int)nC, off);
    if (b.lane == 0 && nC) atomicAdd(&b.s_misc[M_NC], nC);
    if (bad) b.s_misc[M_FAIL] = 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                           // every partner note has left this wavefront
    __syncthreads();
    if (b.tid == 0) ag_store(&a.gran1[b.w], ((u64)(2 * a.epoch) << 48) | b.s_misc[M_NC]);
    res_stamp(a, b, 2);
}

// ---- verification of the pairs found from THIS block (while all-gather #1 is in flight): row ^ Q against the partner's row ----------
__device__ __forceinline__ void res_verify_pairs(const ResArgs &a, const ResBlock &b) {
    bool mism = false;
    res_for_chunks(b, [&](int it, int i, int r, int c) {
        if (b.s_cls[r] & CL_SECOND) {
            const u32x4 mine = res_chunk(b, it, i) ^ b.sq4[c], theirs = a.rows[(i64)b.s_ps[r] * b.Wq + c];
            mism |= (mine.x != theirs.x) | (mine.y != theirs.y) | (mine.z != theirs.z) | (mine.w != theirs.w);
        }
    });
    if (mism) b.s_misc[M_FAIL] = 1;
}

// ---- g1: all-gather #1.  false: it timed out — the others are released and this workgroup has left ----------------------------------
__device__ __forceinline__ bool res_g1(const ResArgs &a, const ResBlock &b, u32 &prefC, u32 &totC) {
    if (b.wave == 0) {
        u32 pref[3], tot[3];
        bool flagged;
        const bool ok = ag_sweep(a.gran1, b.G, 2 * a.epoch, b.w, b.lane, pref, tot, flagged);
        if (b.lane == 0) { b.s_misc[M_OK] = ok ? 1u : 0u; b.s_misc[M_PREF_C] = pref[0]; b.s_misc[M_TOT_C] = tot[0]; }
    }
    __syncthreads();
    res_stamp(a, b, 3);
    if (b.s_misc[M_FAIL] && b.tid == 0) ag_store32(&a.fail[0], a.epoch);
    if (!b.s_misc[M_OK]) {                                                     // time-out: release the others and leave
        if (b.tid == 0) {
            ag_store32(&a.fail[1], a.epoch);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            ag_store(&a.gran2[b.w], ((u64)(2 * a.epoch + 1) << 48) | RES_GRAN_FAIL);
            res_leave(a);
        }
        return false;
    }
    prefC = b.s_misc[M_PREF_C]; totC = b.s_misc[M_TOT_C];
    return true;
}

// ---- B: classes of the anticommuting rows and the final coefficient of those that merge; slots and notes go back to zero -----------
__device__ __forceinline__ void res_B(const ResArgs &a, const ResBlock &b) {
    const f64x2 *coeff2 = reinterpret_cast<const f64x2 *>(a.coeff);
    for (int r = b.tid; r < b.Rw; r += RES_THREADS) {
        const uint8_t info = b.s_info[r];
        if (!(info & 1)) continue;
        const uint8_t st = b.s_cls[r];
        int part = (st & CL_SECOND) ? (int)b.s_ps[r] : -1;
        if (st & CL_CLAIMED) {
            const u32 pv = ag_load32(&a.partner[b.row0 + r]);
            if (pv) { part = (int)pv - 1; ag_store32(&a.partner[b.row0 + r], 0u); }
            ag_store(&a.slots[b.s_ps[r]], 0ULL);
        }
        const f64x2 c = b.s_coef[r];
        double sr = __dmul_rn(c.x, a.cos_t), si = __dmul_rn(c.y, a.cos_t);
        uint8_t cls = 0;
        double pr, pi;
        if (part >= 0) {                                                       // (0 + cos c_t) + (-i sin) i^{e'} c_p, in that order
            const f64x2 cp = coeff2[part];
            phase_mul(cp.x, cp.y, (info >> 3) & 3, pr, pi);
            sr = __dadd_rn(__dadd_rn(0.0, sr), __dmul_rn(pi, a.sin_t));
            si = __dadd_rn(__dadd_rn(0.0, si), -__dmul_rn(pr, a.sin_t));
            b.s_coef[r] = f64x2{sr, si};                                       // final; an unmatched row keeps c: cos c and the new row's
            cls |= CL_MATCHED;                                                 // coefficient are formed from it when they are written
        } else {                                                               // its product row is new
            phase_mul(c.x, c.y, (info >> 1) & 3, pr, pi);
            if (above_thr(__dmul_rn(pi, a.sin_t), -__dmul_rn(pr, a.sin_t), a.thr)) cls |= CL_N;
        }
        if (above_thr(sr, si, a.thr)) cls |= CL_A;
        b.s_cls[r] = cls;
    }
}

// ---- Clifford: class and rotated coefficient per row (k_rotc_classify, rotate_fast.hip) ---------------------------------------------
__device__ __forceinline__ void res_classify_clifford(const ResArgs &a, const ResBlock &b) {
    const int k = a.k;
    for (int r = b.tid; r < b.Rw; r += RES_THREADS) {
        const uint8_t info = b.s_info[r];
        uint8_t cls = 0;
        if (!(info & 1)) {
            cls = CL_C;
        } else {
            const f64x2 c = b.s_coef[r];
            if (k & 1) {
                if (above_thr(c.x, c.y, a.thr)) {
                    double x, y;
                    phase_mul(c.x, c.y, (info >> 1) & 3, x, y);
                    double pr = y, pi = -x;                                    // c * i^e * (-i)
                    if (k == 3) { pr = -pr; pi = -pi; }
                    b.s_coef[r] = f64x2{pr, pi};
                    cls = CL_N | CL_MATCHED;                                   // (MATCHED: the coefficient in LDS is the one to write)
                }
            } else {
                if (k == 2) b.s_coef[r] = f64x2{-c.x, -c.y};
                cls = CL_A | CL_MATCHED;
            }
        }
        b.s_cls[r] = cls;
    }
}

// ---- ranks of the rows inside the block: ballots per pass of 1,024 rows give the rank inside the wavefront and the counts per
//      (pass, wavefront); wavefront 0 adds them up and publishes the block's granule of all-gather #2 at once (it is in flight while
//      everybody turns the ranks into block-wide ones) ---------------------------------------------------------------------------
template <int MODE> __device__ __forceinline__ void res_ranks(const ResArgs &a, const ResBlock &b) {
    const int tid = b.tid, lane = b.lane, wave = b.wave, Rw = b.Rw;
    u32 *s_pos = b.s_ps;                                                       // the join state is dead: the word now holds the row's rank
    const int K = (Rw + RES_THREADS - 1) / RES_THREADS;                        // <= 16
    const u64 lt = (1ULL << lane) - 1ULL;
    for (int j = 0; j < K; ++j) {
        const int r = j * RES_THREADS + tid;
        const uint8_t cl = r < Rw ? b.s_cls[r] : 0;
        const bool an = r < Rw && (b.s_info[r] & 1);
        const u64 b0 = __ballot(cl & CL_C), b1 = __ballot(cl & CL_A), b2 = __ballot(cl & CL_N), b3 = __ballot(an);
        if (r < Rw) {
            s_pos[r] = (u32)__popcll(((cl & CL_C) ? b0 : b1) & lt);
            b.s_posn[r] = (u32)__popcll(b2 & lt);
        }
        if (lane == 0) b.s_wtot[j * 16 + wave] = (u64)__popcll(b0) | ((u64)__popcll(b1) << 16) | ((u64)__popcll(b2) << 32) | ((u64)__popcll(b3) << 48);
    }
    __syncthreads();
    if (wave == 0) {
        const int ne = K * 16;                                                 // <= 256 entries, four per lane
        u64 sum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int e = lane + 64 * i; if (e < ne) sum += b.s_wtot[e]; }
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) {
            const u64 tag2 = (u64)(2 * a.epoch + 1) << 48;
            const u64 nC = sum & 0xFFFFu, nA = (sum >> 16) & 0xFFFFu, nN = (sum >> 32) & 0xFFFFu, nAnti = (sum >> 48) & 0xFFFFu;
            // Clifford: ONE all-gather carries {rotated rows (class A or N: only one of them occurs per k), commuting rows, all anticommuting}
            if (MODE == 1) ag_store(&a.gran2[b.w], tag2 | (nA + nN) | (nC << 16) | (nAnti << 32));
            else ag_store(&a.gran2[b.w], tag2 | nA | (nN << 16) | (nAnti << 32) | (b.s_misc[M_FAIL] ? RES_GRAN_FAIL : 0ULL));
        }
    }
    for (int j = 0; j < K; ++j) {
        const int r = j * RES_THREADS + tid;
        u64 base = 0;
        for (int e = 0; e < j * 16 + wave; ++e) base += b.s_wtot[e];
        if (r < Rw) {
            s_pos[r] += (b.s_cls[r] & CL_C) ? (u32)base & 0xFFFFu : (u32)(base >> 16) & 0xFFFFu;
            b.s_posn[r] += (u32)(base >> 32) & 0xFFFFu;
        }
    }
}

// ---- the report: the last wavefront of the last workgroup (the one with the shortest block) follows all-gather #2 before it
//      turns to its share of the rows, and tells the host the counts the moment they are final and nobody has failed -------------
template <int MODE> __device__ __forceinline__ void res_early_report(const ResArgs &a, const ResBlock &b, u32 totC) {
    if (b.w == b.G - 1 && b.wave == RES_THREADS / 64 - 1) {
        u32 pref[3], tot[3];
        bool flagged;
        const bool ok = ag_sweep(a.gran2, b.G, 2 * a.epoch + 1, b.w, b.lane, pref, tot, flagged);
        if (b.lane == 0 && ok && !flagged) {
            ag_store32(a.published, a.epoch);
            if (MODE == 1) res_report(a, 0, tot[1], (a.k & 1) ? 0 : tot[0], (a.k & 1) ? tot[0] : 0, tot[2]);
            else res_report(a, 0, totC, tot[0], tot[1], tot[2]);
        }
    }
}

// ---- C1: the commuting rows go out while the second all-gather is in flight (non-Clifford) -------------------------------------------
__device__ __forceinline__ void res_C1(const ResArgs &a, const ResBlock &b, u32 prefC) {
    const u32 *s_pos = b.s_ps;
    f64x2 *out_coeff2 = reinterpret_cast<f64x2 *>(a.out_coeff);
    res_for_chunks(b, [&](int it, int i, int r, int c) {
        if (b.s_cls[r] & CL_C) row_store(res_chunk(b, it, i), &a.out_rows[(i64)(prefC + s_pos[r]) * b.Wq + c]);
    });
    for (int r2 = b.tid; r2 < b.Rw; r2 += RES_THREADS)
        if (b.s_cls[r2] & CL_C) {
            const i64 d = (i64)prefC + s_pos[r2];
            out_coeff2[d] = plus_zero(b.s_coef[r2]);                           // 0 + c: the reference's cleanup sums into zeros (-0 -> +0)
            if (a.out_hash) a.out_hash[d] = a.hin[b.row0 + r2];
        }
}

// ---- g2: all-gather #2.  false: it timed out and this workgroup has left ------------------------------------------------------------
template <int MODE> __device__ __forceinline__ bool res_g2(const ResArgs &a, const ResBlock &b) {
    u32 *s_misc = b.s_misc;
    if (b.wave == 0) {
        u32 pref[3], tot[3];
        bool flagged;
        const bool ok = ag_sweep(a.gran2, b.G, 2 * a.epoch + 1, b.w, b.lane, pref, tot, flagged);
        if (b.lane == 0) {
            s_misc[M_OK] = ok ? 1u : 0u;
            if (MODE == 1) {      // rotated rows first (filed under A or N, whichever this k produces), then the commuting ones
                s_misc[M_PREF_A] = pref[0]; s_misc[M_TOT_A] = (a.k & 1) ? 0 : tot[0]; s_misc[M_PREF_N] = pref[0]; s_misc[M_TOT_N] = (a.k & 1) ? tot[0] : 0;
                s_misc[M_PREF_C] = pref[1]; s_misc[M_TOT_C] = tot[1];
            } else {
                s_misc[M_PREF_A] = pref[0]; s_misc[M_TOT_A] = tot[0]; s_misc[M_PREF_N] = pref[1]; s_misc[M_TOT_N] = tot[1];
            }
            s_misc[M_TOT_ANTI] = tot[2];
        }
    }
    __syncthreads();
    res_stamp(a, b, 6);
    if (!s_misc[M_OK]) {
        if (b.tid == 0) {
            ag_store32(&a.fail[1], a.epoch);
            res_leave(a);
        }
        return false;
    }
    return true;
}

// ---- C2: the remaining rows, coefficients and hashes.  Output order: non-Clifford [commuting | cos * anticommuting | new rows];
//      Clifford [rotated anticommuting | commuting] ------------------------------------------------------------------------------
template <int MODE> __device__ __forceinline__ void res_C2(const ResArgs &a, const ResBlock &b, u32 prefC, u32 totC) {
    const u32 *s_pos = b.s_ps, *s_posn = b.s_posn;
    f64x2 *out_coeff2 = reinterpret_cast<f64x2 *>(a.out_coeff);
    if (MODE == 1) { prefC = b.s_misc[M_PREF_C]; totC = b.s_misc[M_TOT_C]; }
    const u32 prefA = b.s_misc[M_PREF_A], totA = b.s_misc[M_TOT_A], prefN = b.s_misc[M_PREF_N], totN = b.s_misc[M_TOT_N];
    const i64 baseC = (MODE == 1 ? (i64)totA + totN : 0) + prefC;
    const i64 baseA = (MODE == 1 ? 0 : (i64)totC) + prefA;
    const i64 baseN = (MODE == 1 ? 0 : (i64)totC + totA) + prefN;
    const int Wq = b.Wq;
    res_for_chunks(b, [&](int it, int i, int r, int c) {
        const uint8_t cl = b.s_cls[r];
        if (cl & ((MODE == 1 ? CL_C : 0) | CL_A | CL_N)) {
            const u32x4 x = res_chunk(b, it, i);
            if (MODE == 1 && (cl & CL_C)) row_store(x, &a.out_rows[(baseC + s_pos[r]) * Wq + c]);
            if (cl & CL_A) row_store(x, &a.out_rows[(baseA + s_pos[r]) * Wq + c]);
            if (cl & CL_N) row_store(x ^ b.sq4[c], &a.out_rows[(baseN + s_posn[r]) * Wq + c]);
        }
    });
    for (int r2 = b.tid; r2 < b.Rw; r2 += RES_THREADS) {
        const uint8_t cl = b.s_cls[r2];
        if (!(cl & ((MODE == 1 ? CL_C : 0) | CL_A | CL_N))) continue;
        const f64x2 c = b.s_coef[r2];
        const u64 h = a.out_hash ? a.hin[b.row0 + r2] : 0ULL;
        if (MODE == 1 && (cl & CL_C)) {
            const i64 d = baseC + s_pos[r2];
            out_coeff2[d] = c;
            if (a.out_hash) a.out_hash[d] = h;
        }
        if (cl & CL_A) {
            const i64 d = baseA + s_pos[r2];
            const f64x2 ca = (cl & CL_MATCHED) ? c : f64x2{__dmul_rn(c.x, a.cos_t), __dmul_rn(c.y, a.cos_t)};
            out_coeff2[d] = MODE == 0 ? plus_zero(ca) : ca;
            if (a.out_hash) a.out_hash[d] = h;
        }
        if (cl & CL_N) {
            const i64 d = baseN + s_posn[r2];
            f64x2 cn = c;
            if (MODE == 0) {                                                   // (-i sin) i^e c, from the row's own coefficient
                double pr, pi;
                phase_mul(c.x, c.y, (b.s_info[r2] >> 1) & 3, pr, pi);
                cn = plus_zero(f64x2{__dmul_rn(pi, a.sin_t), -__dmul_rn(pr, a.sin_t)});
            }
            out_coeff2[d] = cn;
            if (a.out_hash) a.out_hash[d] = h ^ a.hq;
        }
    }
}

// MODE 0: non-Clifford (hash join); MODE 1: Clifford (k = clifford_k of rotation_args, 0..3)
// WQ: 16-byte chunks per row if that is a power of two <= 32 (analysis in registers while the rows stream in), else 0 (from LDS)
// A (A1, A2, A3, pair verification) -> g1 -> B -> ranks -> report -> C1 -> g2 -> C2 -> leave; Clifford: A1, A2, classify in place of A3 .. B
template <int MODE, int WQ>
__global__ __launch_bounds__(RES_THREADS) void k_rot_resident(const ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (a.inject && blockIdx.x == gridDim.x - 1) return;
    u32x4 keep0 = (u32x4)(0u), keep1 = (u32x4)(0u);
    const ResBlock b = res_block<WQ>(a, smem, keep0, keep1);
    res_stamp(a, b, 0);
    if (b.tid < 2 * b.Wq) b.s_q[b.tid] = a.q.w[b.tid];
    if (b.tid < 32) b.s_misc[b.tid] = 0;
    __syncthreads();
    res_A1<MODE, WQ>(a, b);
    __syncthreads();
    if constexpr (WQ == 0) res_A2(a, b);
    res_stamp(a, b, 1);
    u32 prefC = 0, totC = 0;
    if (MODE == 0) {
        res_A3<WQ>(a, b);
        res_verify_pairs(a, b);
        if (!res_g1(a, b, prefC, totC)) return;
        res_B(a, b);
    } else {
        res_classify_clifford(a, b);
    }
    __syncthreads();
    res_stamp(a, b, 4);
    res_ranks<MODE>(a, b);
    __syncthreads();
    res_early_report<MODE>(a, b, totC);
    if (MODE == 0) res_C1(a, b, prefC);
    res_stamp(a, b, 5);
    if (!res_g2<MODE>(a, b)) return;
    res_C2<MODE>(a, b, prefC, totC);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                               // every wavefront's rows have left ...
    __syncthreads();
    res_stamp(a, b, 7);
    if (b.tid == 0) res_leave(a);            // ... before the block counts as gone
}

typedef void (*ResKernel)(const ResArgs);
static ResKernel res_kernel(bool clifford, int Wq) {
    if (clifford) return wq_dispatch<0, 1, 2, 4, 8, 16, 32>(Wq, [](auto wq) -> ResKernel { return k_rot_resident<1, decltype(wq)::value>; });
    return wq_dispatch<0, 1, 2, 4, 8, 16, 32>(Wq, [](auto wq) -> ResKernel { return k_rot_resident<0, decltype(wq)::value>; });
}

bool resident_lds_attr_ok() {
    return SG_DEVICE_ONCE(([] {
        for (int m = 0; m < 2; ++m)
            for (int wq : {1, 2, 4, 8, 16, 32, 3})
                if (hipFuncSetAttribute(reinterpret_cast<const void *>(res_kernel(m == 1, wq)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RES_LDS_MAX) != hipSuccess) return false;
        return true;
    }()));
}

hipError_t launch_resident(const ResidentPlan &p, bool clifford, hipStream_t st, const ResArgs &a) {
    bump_counter(counter_of(p.form));
    {
        ProfScope prof(4);
        hipLaunchKernelGGL(res_kernel(clifford, a.Wq), dim3((unsigned)p.G), dim3(RES_THREADS), (size_t)p.lds_bytes, st, a);
    }
    return hipGetLastError();
}

}  // namespace symgpu
