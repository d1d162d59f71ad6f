// rotate_analyze.hip — first stage of every multi-launch rotation: anticommutation flag and phase exponent of every row against Q, and
// (hash join, duplicate check) the insert of every row into the persistent join table.
#include "rotate_common.h"

namespace symgpu {

// flags[t] = 1 iff row t anticommutes with q;  ph[t] = phase exponent e of (row_t * q).
// HASH: also the linear row hash h1 of cleanup_hash.hip (same tables, same per-lane Horner) for the hash-join fast path.
__device__ __forceinline__ u64 rot_rotl64(u64 x, int r) { r &= 63; return r ? ((x << r) | (x >> (64 - r))) : x; }

// insert row t (hash h) — duplicates (same tag AND same words) raise the flag; one lane per row
__device__ __forceinline__ void jt_insert(const JoinTable jt, const u64 *__restrict__ rows, int W, i64 t, u64 h) {
    const u64 entry = (h & 0xFFFFFFFF00000000ULL) | ((u64)jt.gen << 22) | (u64)(t + 1);
    u32 pos = (u32)mix64(h) & jt.mask;
    for (;;) {
        u64 v = __hip_atomic_load(&jt.slots[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (jt_gen(v) != jt.gen) {                                   // empty (or left over from an earlier rotation): claim it
            const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&jt.slots[pos]), (unsigned long long)v, (unsigned long long)entry);
            if (old == v) return;
            v = old;
            if (jt_gen(v) != jt.gen) continue;                       // lost the race to a stale writer?  cannot happen, but retry the slot
        }
        if ((v >> 32) == (h >> 32)) {                                // same 32-bit tag: duplicate row, or a tag collision
            const i64 o = jt_row(v);
            bool same = true;
            for (int w = 0; w < W; ++w) same &= (rows[o * W + w] == rows[t * W + w]);
            if (same) { jt.flags[0] = jt.gen; return; }
        }
        pos = (pos + 1) & jt.mask;
    }
}

// HASH: compute the row hashes (-> hout); otherwise INSERT reads them from hin.  INSERT: put every row into the join table.
// QARG: the rotation's Pauli row Q arrives BY VALUE in the kernel arguments (rows of <= 64 words) instead of in `q_dev`, which
// block 0 then fills for the kernels that follow on the stream — no host-to-device copy in front of the first kernel of a rotation.
template <bool HASH, bool INSERT, bool QARG = false>
__global__ __launch_bounds__(256) void k_rot_analyze(const u64 *__restrict__ rows, i64 T, int Wq, int G, u64 *__restrict__ q_dev,
                                                      u32 *__restrict__ flags, uint8_t *__restrict__ ph, const u64 *__restrict__ tab_g,
                                                      u64 *__restrict__ hout, const u64 *__restrict__ hin, JoinTable jt, QArg qa = QArg()) {
    __shared__ u64 tab[HASH ? 8 * 256 : 1];
    __shared__ u64 sq[QARG ? 64 : 1];
    if (QARG) {
        if ((int)threadIdx.x < 2 * Wq) {
            const u64 v = qa.w[threadIdx.x];
            sq[threadIdx.x] = v;
            if (blockIdx.x == 0) q_dev[threadIdx.x] = v;
        }
    }
    if (HASH) {
        for (int k = threadIdx.x; k < 8 * 256; k += 256) tab[k] = tab_g[2 * k];      // h1 entries only
    }
    if (HASH || QARG) __syncthreads();
    const u64 *q = QARG ? sq : q_dev;
    const int rows_per_block = 256 / G;
    const int g = threadIdx.x % G, rsub = threadIdx.x / G;
    // Y count of q (every lane redundantly; Wq is small)
    int yq = 0;
    for (int w = 0; w < Wq; ++w) yq += __popcll(q[w] & q[Wq + w]);
    const int W = 2 * Wq;
    for (i64 t0 = (i64)blockIdx.x * rows_per_block; t0 < T; t0 += (i64)gridDim.x * rows_per_block) {
        const i64 t = t0 + rsub;
        u64 par = 0, flip = 0;
        int yp = 0, yout = 0;
        u64 h1 = 0;
        if (t < T) {
            const u64 *r = rows + t * 2 * Wq;
            for (int w = g; w < Wq; w += G) {
                const u64 x = r[w], z = r[Wq + w], xq = q[w], zq = q[Wq + w];
                par ^= (x & zq) ^ (z & xq);
                flip ^= x & zq;
                yp += __popcll(x & z);
                yout += __popcll((x ^ xq) & (z ^ zq));
            }
            if (HASH) {
                // lane g of a 64-lane virtual row owns words g, g+64, ...; here G <= 64 lanes cover the row, so every
                // lane loops over the virtual lanes vg = g, g+G, ... < 64 it stands for
                const int n_blk = (W + 63) / 64;
                for (int vg = g; vg < 64; vg += G) {
                    u64 hv = 0;
                    for (int b = 0; b < n_blk; ++b) {
                        const int w = b * 64 + vg;
                        u64 a1 = 0;
                        if (w < W) {
                            const u64 x = r[w];
#pragma unroll
                            for (int k = 0; k < 8; ++k) a1 ^= tab[k * 256 + (int)((x >> (8 * k)) & 255)];
                        }
                        hv ^= hv << 13; hv ^= hv >> 7; hv ^= hv << 17;
                        hv ^= rot_rotl64(a1, vg);
                    }
                    h1 ^= hv;
                }
            }
        }
        int pp = __popcll(par) & 1, fp = __popcll(flip) & 1;
        for (int off = G >> 1; off > 0; off >>= 1) {
            pp ^= __shfl_xor(pp, off);
            fp ^= __shfl_xor(fp, off);
            yp += __shfl_xor(yp, off);
            yout += __shfl_xor(yout, off);
            if (HASH) h1 ^= __shfl_xor(h1, off);
        }
        if (g == 0 && t < T) {
            flags[t] = (u32)pp;
            ph[t] = (uint8_t)((3 * (yp + yq) + yout + 2 * fp) & 3);
            if (HASH) hout[t] = h1;
            if (INSERT) jt_insert(jt, rows, W, t, HASH ? h1 : hin[t]);
        }
    }
}


// The same analysis with ONE 16-byte chunk of a row per lane (rows whose 16-byte chunk count WQ = words per X block is a power
// of two <= 64 and whose hashes are cached): a row is an aligned group of WQ lanes, X words in its lower and Z words in its upper
// half, loads are 1 KiB per wave instruction (k_rot_analyze reads 8 bytes per lane and walks six dependent chains per block at
// 1e5 rows: 22 us; this: 9 us).  Lane exchange as in product.hip's row stream: x & z and (x ^ xq) & (z ^ zq) need the other half
// of the row (DPP / ds_bpermute), x & zq and z & xq only the other half of Q, which every lane reads from LDS.
template <int WQ, bool INSERT, bool QARG>
__global__ __launch_bounds__(256) void k_rot_analyze_chunks(const u32x4 *__restrict__ rows, i64 T, u64 *__restrict__ q_dev, u32 *__restrict__ flags,
                                                             uint8_t *__restrict__ ph, const u64 *__restrict__ hin, JoinTable jt, QArg qa) {
    __shared__ __attribute__((aligned(16))) u64 sq[2 * WQ];
    __shared__ int s_yq;
    if (INSERT) {
        // The join-table insert needs nothing from the analysis (row index + cached hash), and done by the one lane per row group
        // that ends the analysis it was a chain load -> atomic load -> CAS with 4 lanes of 64 busy: 10 of the kernel's 18 us.  The
        // FIRST ceil(T / 256) blocks of the grid are insert blocks, ONE LANE PER ROW (dispatched first: their latency chain runs
        // while the analysis blocks stream the rows behind them).
        const i64 n_ins = (T + 255) / 256;
        if ((i64)blockIdx.x < n_ins) {
            const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
            if (t < T) jt_insert(jt, reinterpret_cast<const u64 *>(rows), 2 * WQ, t, hin[t]);
            return;
        }
    }
    const i64 bx = (i64)blockIdx.x - (INSERT ? (T + 255) / 256 : 0);     // analysis block index
    if ((int)threadIdx.x < 2 * WQ) {
        const u64 v = QARG ? qa.w[threadIdx.x] : q_dev[threadIdx.x];
        sq[threadIdx.x] = v;
        if (QARG && bx == 0) q_dev[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int y = 0;
        for (int w = 0; w < WQ; ++w) y += __popcll(sq[w] & sq[WQ + w]);
        s_yq = y;
    }
    __syncthreads();
    constexpr int R = 256 / WQ;                                       // rows per block
    const int c = threadIdx.x & (WQ - 1);                            // chunk of the row: c < WQ/2 holds X words (WQ == 1: x and z word)
    const i64 t = bx * R + threadIdx.x / WQ;
    const bool valid = t < T;
    const u32x4 v = valid ? rows[t * WQ + c] : (u32x4)(0u);
    u32 par, ye;                                                      // par: |x & zq| + |z & xq| (+ |x & zq| << 16);  ye: Y_P | Y_out << 16
    if constexpr (WQ == 1) {
        const u32x4 qv = *reinterpret_cast<const u32x4 *>(sq);
        const u32 f = __popc(v.x & qv.z) + __popc(v.y & qv.w);
        par = f + __popc(v.z & qv.x) + __popc(v.w & qv.y) + (f << 16);
        ye = (__popc(v.x & v.z) + __popc(v.y & v.w)) | ((__popc((v.x ^ qv.x) & (v.z ^ qv.z)) + __popc((v.y ^ qv.y) & (v.w ^ qv.w))) << 16);
    } else {
        const u32x4 qs = reinterpret_cast<const u32x4 *>(sq)[c], qo = reinterpret_cast<const u32x4 *>(sq)[c ^ (WQ / 2)];
        const bool xhalf = c < WQ / 2;
        const u32 p = __popc(v.x & qo.x) + __popc(v.y & qo.y) + __popc(v.z & qo.z) + __popc(v.w & qo.w);    // x & zq (X half), z & xq (Z half)
        const u32x4 o = {rot_other_half<WQ>(v.x), rot_other_half<WQ>(v.y), rot_other_half<WQ>(v.z), rot_other_half<WQ>(v.w)};
        const u32 yp = __popc(v.x & o.x) + __popc(v.y & o.y) + __popc(v.z & o.z) + __popc(v.w & o.w);
        const u32 yo = __popc((v.x ^ qs.x) & (o.x ^ qo.x)) + __popc((v.y ^ qs.y) & (o.y ^ qo.y)) + __popc((v.z ^ qs.z) & (o.z ^ qo.z)) +
                       __popc((v.w ^ qs.w) & (o.w ^ qo.w));
        par = rot_row_sum<WQ>(p + (xhalf ? (p << 16) : 0u));
        ye = rot_row_sum<WQ>(xhalf ? (yp | (yo << 16)) : 0u);          // both halves form the same x & z words: count them once
    }
    if (c == 0 && valid) {
        flags[t] = par & 1u;
        ph[t] = (uint8_t)((3u * ((ye & 0xFFFFu) + (u32)s_yq) + (ye >> 16) + 2u * ((par >> 16) & 1u)) & 3u);
    }
}

// pinned, device-mapped host copy of the counts (one per context): written by k_rotf_scan3, read after the final synchronisation
int host_counts(RotCounts **host, RotCounts **dev) {
    Context &c = ctx();
    if (!c.rot_host_cnt) {
        HIP_TRY(hipHostMalloc(&c.rot_host_cnt, 64, hipHostMallocMapped));
        for (int i = 0; i < 8; ++i) reinterpret_cast<volatile u64 *>(c.rot_host_cnt)[i] = 0;
        HIP_TRY(hipHostGetDevicePointer(&c.rot_host_cnt_dev, c.rot_host_cnt, 0));
    }
    *host = reinterpret_cast<RotCounts *>(c.rot_host_cnt);
    *dev = reinterpret_cast<RotCounts *>(c.rot_host_cnt_dev);
    return SYMGPU_OK;
}

// The persistent join table: at least 4 slots per row, a fresh generation per call (cleared when the 10-bit generation wraps).
int join_table_for(i64 T, JoinTable *jt) {
    Context &c = ctx();
    size_t cap = 1024;
    while ((i64)cap < 4 * T) cap <<= 1;
    if (!c.rot_flags) {
        HIP_TRY(hipMalloc((void **)&c.rot_flags, 16));
        HIP_TRY(hipMemsetAsync(c.rot_flags, 0, 16, c.stream));
    }
    if (cap > c.rot_table_cap) {
        // from the library's allocator (arena): an operator that grows from rotation to rotation outgrows the table several times, and
        // a hipFree + hipMalloc pair costs 0.3 ms each time; everything that touches the table is on the one library stream
        if (c.rot_table) { dev_free(c.rot_table); c.rot_table = nullptr; c.rot_table_cap = 0; }
        SG_TRY(dev_alloc(cap * 8, (void **)&c.rot_table));
        c.rot_table_cap = cap;
        c.rot_gen = 0;
    }
    if (c.rot_gen == 0 || c.rot_gen >= 1023) {                 // new table, or the generation field wraps: every slot empty again
        HIP_TRY(hipMemsetAsync(c.rot_table, 0, c.rot_table_cap * 8, c.stream));
        HIP_TRY(hipMemsetAsync(c.rot_flags, 0, 16, c.stream));
        c.rot_gen = 0;
    }
    ++c.rot_gen;
    jt->slots = c.rot_table;
    jt->mask = (u32)(cap - 1);                                 // a call uses the first `cap` slots of a possibly larger table
    jt->gen = c.rot_gen;
    jt->flags = c.rot_flags;
    return SYMGPU_OK;
}

int analyze_rows(symgpu_op_t in, u64 *q_dev, u32 *anti, uint8_t *ph, const JoinTable *jt, const RotateSwitches &sw, const u64 *q_host_arg) {
    hipStream_t st = ctx().stream;
    const i64 T = in->T;
    const int Wq = in->Wq;
    const int G = row_lanes(Wq);
    const int rpb = 256 / G;
    // word kernel: grid-stride over <= 1024 blocks (uncapped measured 20.6 / 14.2 us against 22.4 / 10.8 us with / without the insert)
    i64 g = (T + rpb - 1) / rpb;
    if (g > sw.analyze_cap) g = sw.analyze_cap;
    const JoinTable none = {nullptr, 0, 0, nullptr};
    QArg qa;
    const bool by_arg = q_host_arg != nullptr && 2 * Wq <= 64;           // Q travels in the kernel arguments (see k_rot_analyze)
    if (by_arg) for (int w = 0; w < 2 * Wq; ++w) qa.w[w] = q_host_arg[w];
    else if (q_host_arg) HIP_TRY(hipMemcpyAsync(q_dev, q_host_arg, (size_t)2 * Wq * 8, hipMemcpyHostToDevice, st));
    const bool have_hash = jt && in->hash && in->hash_seed == ctx().hash_seed;
    if (sw.chunks && (!jt || have_hash) && Wq <= 64 && (Wq & (Wq - 1)) == 0) {
        // one 16-byte chunk per lane (k_rot_analyze_chunks); rows of other lengths and the launch that also hashes keep the word kernel
        const u32x4 *pr = reinterpret_cast<const u32x4 *>(in->rows);
        const i64 gb = (T + 256 / Wq - 1) / (256 / Wq), gi = (T + 255) / 256;     // analysis blocks, then (with a join table) insert blocks
        wq_dispatch<64, 1, 2, 4, 8, 16, 32>(Wq, [&](auto wq) {
            constexpr int WQ = decltype(wq)::value;
            if (jt) {
                if (by_arg) hipLaunchKernelGGL((k_rot_analyze_chunks<WQ, true, true>), dim3((unsigned)(gb + gi)), dim3(256), 0, st, pr, T, q_dev, anti, ph, in->hash, *jt, qa);
                else hipLaunchKernelGGL((k_rot_analyze_chunks<WQ, true, false>), dim3((unsigned)(gb + gi)), dim3(256), 0, st, pr, T, q_dev, anti, ph, in->hash, *jt, qa);
            } else {
                if (by_arg) hipLaunchKernelGGL((k_rot_analyze_chunks<WQ, false, true>), dim3((unsigned)gb), dim3(256), 0, st, pr, T, q_dev, anti, ph, (const u64 *)nullptr, none, qa);
                else hipLaunchKernelGGL((k_rot_analyze_chunks<WQ, false, false>), dim3((unsigned)gb), dim3(256), 0, st, pr, T, q_dev, anti, ph, (const u64 *)nullptr, none, qa);
            }
        });
        KERNEL_CHECK();
        return SYMGPU_OK;
    }
    // word kernel: HASH (compute the row hashes into hout) and INSERT as compile-time flags
    auto words = [&](auto hash, auto insert, const u64 *tab, u64 *hout, const u64 *hin, const JoinTable &j) {
        constexpr bool H = decltype(hash)::value, I = decltype(insert)::value;
        if (by_arg) hipLaunchKernelGGL((k_rot_analyze<H, I, true>), dim3((unsigned)g), dim3(256), 0, st, in->rows, T, Wq, G, q_dev, anti, ph, tab, hout, hin, j, qa);
        else hipLaunchKernelGGL((k_rot_analyze<H, I, false>), dim3((unsigned)g), dim3(256), 0, st, in->rows, T, Wq, G, q_dev, anti, ph, tab, hout, hin, j, qa);
    };
    if (!jt) {
        words(std::false_type{}, std::false_type{}, nullptr, nullptr, nullptr, none);
    } else if (have_hash) {
        words(std::false_type{}, std::true_type{}, nullptr, nullptr, in->hash, *jt);
    } else {
        if (in->hash) { dev_free(in->hash); in->hash = nullptr; }
        SG_TRY(dev_alloc((size_t)in->capacity * 8 + 16, (void **)&in->hash));      // cached on the operand: its next rotation skips the hashing
        in->hash_seed = ctx().hash_seed;
        bump_counter(SYMGPU_CTR_OP_ROW_HASH_BUILDS);
        words(std::true_type{}, std::true_type{}, ctx().hash_tab, in->hash, nullptr, *jt);
    }
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// odd multiples of pi/2 multiply by Q through the reference's __mul__ (merge + threshold on sums): the Clifford fast path is only the
// same thing for an operator without duplicate rows.  Flags + the same join-table insert as the hash join: does the operator hold two
// equal rows?
int rotate_dup_check(RotationRun &r) {
    const i64 T = r.in->T;
    SG_TRY(ensure_hash_tables(ctx().hash_tab ? ctx().hash_seed : 1));
    JoinTable jt;
    SG_TRY(join_table_for(T, &jt));
    SG_TRY(analyze_rows(r.in, r.q.as<u64>(), r.anti.as<u32>(), r.ph.as<uint8_t>(), &jt, r.sw, r.q_host));
    u32 hflag = 0;
    SG_TRY(read_back_words(jt.flags, 1, nullptr, 0, &hflag));
    r.has_dup = hflag == jt.gen;
    if (!r.has_dup) r.in->dup_free = 1;
    return SYMGPU_OK;
}

}  // namespace symgpu
