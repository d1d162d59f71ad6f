// cleanup_segments.hip — the segment stages of a cleanup attempt (cleanup_driver.hip): the fix-up of the runs the truncated sort left
// unordered, the identity segment of a squared operator, and the segment sums with their exact row-against-row verification.
#include "cleanup_common.h"
#include "block_scan.h"

namespace symgpu {

// lazy mode, after the sort: which 64-position chunks of the sorted keys hold a member of a segment with more than one element?
// A position that equals its predecessor (the test k_heads_sums makes: prefix, then P * P twins, then the full keys rebuilt from the
// operand hash tables) marks its own chunk and its predecessor's.  Four chunks per wavefront and step, all loads of a step in flight.
template <bool PACKED>
__global__ __launch_bounds__(256) void k_find_merges(const u64 *__restrict__ keys, i64 T, const u32 *__restrict__ zero_len, PackedLayout L,
                                                      const u64 *__restrict__ hI, const u64 *__restrict__ hO, int same_operand, u32 *__restrict__ dirtybits) {
    const i64 ZL = zero_len ? (i64)*zero_len : 0;
    const int lane = threadIdx.x & 63;
    const i64 n_steps = (T + 255) / 256;
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_steps; g += (i64)gridDim.x * 4) {
        const i64 base = g * 256;
        u64 k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const i64 sp = base + 64 * j + lane; k[j] = sp < T ? keys[sp] : 0ULL; }
        const u64 prev = base > 0 ? keys[base - 1] : 0ULL;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i64 sp = base + 64 * j + lane;
            u64 k0 = __shfl_up(k[j], 1);
            const u64 carry_in = j > 0 ? __shfl(k[j > 0 ? j - 1 : 0], 63) : prev;
            if (lane == 0) k0 = carry_in;
            const bool valid = sp < T && sp >= ZL;
            bool eq;
            if (PACKED) {
                eq = valid && sp > 0 && (k[j] >> L.F()) == (k0 >> L.F());
                if (eq && !(same_operand && L.i(k[j]) == L.o(k0) && L.o(k[j]) == L.i(k0))) eq = L.full_key(hI, hO, k[j]) == L.full_key(hI, hO, k0);
            } else eq = valid && sp > 0 && k[j] == k0;
            const u64 b = __ballot(eq);
            if (b != 0ULL && lane == 0) {
                const i64 chunk = base / 64 + j;
                atomicOr(&dirtybits[chunk >> 5], 1u << (chunk & 31));
                if ((b & 1ULL) && chunk > 0) atomicOr(&dirtybits[(chunk - 1) >> 5], 1u << ((chunk - 1) & 31));
            }
        }
    }
}

// ---- the identity segment of a squared operator -------------------------------------------------------------------------------
// P * P has N diagonal pairs (i, i), and every one of them is the identity row: N equal keys — with FULL KEY ZERO, because the row
// hash is linear (h(0) = 0) — i.e. one segment of >= N elements at the very start of the sorted array.  k_heads_sums sums a
// segment sequentially, one wavefront walking chunk after chunk: 157 dependent chunk steps for N = 10,000, 0.8 of the kernel's
// 1.64 ms at cfg3, 40 of 44 us at cfg1.  The squared path already associates its sums differently from the reference (twin first:
// exact for dyadic coefficients, rounding-level otherwise), so the zero-key segment is reduced in parallel here, in a FIXED order
// (per-thread ascending positions, then threads, then blocks in order: deterministic), and k_heads_sums starts behind it.
// Members that are not diagonal pairs (duplicate rows in P, or a 64-bit collision) are verified row against row like everywhere.
constexpr int ZB = 1024;                                              // sorted positions per block
__global__ __launch_bounds__(256) void k_zero_partial(const u64 *__restrict__ keys, i64 Tk, const u64 *__restrict__ hI, const u64 *__restrict__ hO,
                                                       PackedLayout L, const u64 *__restrict__ rows, int W, const double *__restrict__ cf,
                                                       double *__restrict__ part, u32 *__restrict__ part_n, u32 *__restrict__ collision,
                                                       u32 Ni, u32 *__restrict__ lazy_markbits) {
    __shared__ double s_re[256], s_im[256];
    __shared__ u32 s_n[256];
    const i64 base = (i64)blockIdx.x * ZB;
    if (L.full_key(hI, hO, keys[base]) != 0ULL) {                     // uniform: the zero keys are a prefix of the sorted array
        if (threadIdx.x == 0) { part[2 * blockIdx.x] = 0.0; part[2 * blockIdx.x + 1] = 0.0; part_n[blockIdx.x] = 0u; }
        return;
    }
    double re = 0.0, im = 0.0;
    u32 n = 0;
    bool mism = false, offdiag = false;
    for (int j = 0; j < ZB / 256; ++j) {
        const i64 p = base + threadIdx.x + 256 * j;
        if (p >= Tk) break;
        const u64 k = keys[p];
        if (L.full_key(hI, hO, k) != 0ULL) break;                     // behind the segment: so is everything this thread has left
        const u32 i = L.i(k), o = L.o(k);
        const int e = L.e(k);
        double cr, cim;
        pair_coefficient(cf[2 * i], cf[2 * i + 1], cf[2 * o], cf[2 * o + 1], e, cr, cim);
        if (i != o) {
            if (e & 1) { cr = 0.0; cim = 0.0; } else { cr = __dadd_rn(cr, cr); cim = __dadd_rn(cim, cim); }
            for (int w = 0; w < W; ++w) mism |= rows[(i64)i * W + w] != rows[(i64)o * W + w];      // identity row <=> equal factors
            offdiag = true;
        }
        re = __dadd_rn(re, cr);
        im = __dadd_rn(im, cim);
        ++n;
        if (lazy_markbits) {                                          // not a single: whatever k_mark_singles decided is void (k_zero_close files the head)
            const u32 slot = tri_slot(o, i, Ni);
            atomicAnd(&lazy_markbits[slot >> 5], ~(1u << (slot & 31u)));
        }
    }
    s_re[threadIdx.x] = re; s_im[threadIdx.x] = im; s_n[threadIdx.x] = n;
    if (mism) atomicOr(collision, 1u);
    if (offdiag) atomicOr(collision + 2, 1u);                          // a member that is not a diagonal pair: P holds duplicate rows
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0, q = 0.0;
        u32 c = 0;
        for (int t = 0; t < 256; ++t) { r = __dadd_rn(r, s_re[t]); q = __dadd_rn(q, s_im[t]); c += s_n[t]; }
        part[2 * blockIdx.x] = r; part[2 * blockIdx.x + 1] = q; part_n[blockIdx.x] = c;
    }
}
// The identity coefficient of P * P exactly as the reference forms it when P has no duplicate rows: the N diagonal pairs are then the
// only members of the identity segment, and np.add.at adds their coefficients c_i * c_i (the phase exponent of P_i * P_i is 0) to
// 0.0 one after the other in index order (utils.py:273-274).  A sequential sum is sequential: ONE wavefront, 64 products per step
// staged in LDS, lane 0 adds them in order (two independent chains, re and im).  ~12 cycles per term: 50 us at N = 10,000 — on the
// side stream next to the key generation and the sort of the same call, which take milliseconds.
__global__ __launch_bounds__(64) void k_diag_seq_sum(const double *__restrict__ cf, u32 N, double *__restrict__ out) {
    __shared__ f64x2 s_p[2][64];
    const int lane = threadIdx.x;
    double re = 0.0, im = 0.0;
    int buf = 0;
    for (u32 base = 0; base < N; base += 64, buf ^= 1) {
        const u32 i = base + lane;
        if (i < N) {
            const f64x2 c = reinterpret_cast<const f64x2 *>(cf)[i];
            double pr, pi;
            pair_coefficient(c.x, c.y, c.x, c.y, 0, pr, pi);
            s_p[buf][lane] = f64x2{pr, pi};
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            const u32 m = N - base < 64u ? N - base : 64u;
            if (m == 64u) {
#pragma unroll
                for (int k = 0; k < 64; ++k) { const f64x2 p = s_p[buf][k]; re = __dadd_rn(re, p.x); im = __dadd_rn(im, p.y); }
            } else {
                for (u32 k = 0; k < m; ++k) { const f64x2 p = s_p[buf][k]; re = __dadd_rn(re, p.x); im = __dadd_rn(im, p.y); }
            }
        }
    }
    if (lane == 0) { out[0] = re; out[1] = im; }
}

// blocks in order; files the identity term under the slot of the segment's first element and tells k_heads_sums where to start
__global__ void k_zero_close(const u64 *__restrict__ keys, const double *__restrict__ part, const u32 *__restrict__ part_n, i64 n_blocks,
                             PackedLayout L, u32 Ni, double thr, int use_thr, u32 *__restrict__ markbits, double *__restrict__ sum_of,
                             u32 *__restrict__ zero_len, u32 *__restrict__ patchbits, const double *__restrict__ diag_seq,
                             const u32 *__restrict__ offdiag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double re = 0.0, im = 0.0;
    u64 len = 0;
    for (i64 b = 0; b < n_blocks; ++b) {
        const u32 c = part_n[b];
        if (c == 0) break;
        re = __dadd_rn(re, part[2 * b]); im = __dadd_rn(im, part[2 * b + 1]);
        len += c;
        if (c < (u32)ZB) break;
    }
    // exactly the N diagonal pairs: the reference's sequential sum (k_diag_seq_sum) instead of the blocked one
    if (diag_seq && len == (u64)Ni && *offdiag == 0u) { re = diag_seq[0]; im = diag_seq[1]; }
    *zero_len = (u32)len;
    if (len == 0) return;
    if (use_thr && !above_thr(re, im, thr)) return;
    const u64 k0 = keys[0];                                           // stable sort: the segment's smallest pair index
    const u32 first = tri_slot(L.o(k0), L.i(k0), Ni);
    atomicOr(&markbits[first >> 5], 1u << (first & 31u));
    if (patchbits) atomicOr(&patchbits[first >> 5], 1u << (first & 31u));
    sum_of[2 * (i64)first] = re; sum_of[2 * (i64)first + 1] = im;
}

// head flags + exact verification of equal-key neighbours + coefficient gather into sorted order.
// PAIR: row(t) = inner[t % Ni] ^ outer[t / Ni].  One wavefront owns 64 consecutive sorted positions; the positions whose
// key equals their predecessor's are verified COOPERATIVELY with 16-byte loads: G = pow2 >= W/2 lanes (<= 64) cover the
// 16-byte chunks of the two rows, the 64/G lane groups each walk the candidates of their own lane range, so 64/G
// comparisons (4 row reads each in PAIR mode) are in flight per step.  A mismatch (two different rows with one 64-bit
// hash) only raises the collision flag: the caller reseeds the hash and redoes the pass, so exactness never rests on the
// hash.  cg[s] = coeff[idx[s]] turns the segment sums into sequential reads.
__device__ __forceinline__ bool differs(u32x4 a, u32x4 b) {
    const u32x4 d = a ^ b;
    return (d.x | d.y | d.z | d.w) != 0u;
}
// PACKED (implies PAIR): keys are packed pair keys; idx and coeff are unused: the input index, the full key and the pair
// coefficient c_i * c_o * i^e come from the key's fields and the operand tables hI / hO / ci / co.
//
// The SAME kernel forms the segment sums, so that neither the head flags nor the coefficients in sorted order are ever
// written to memory: every wavefront owns a contiguous range of 64-position chunks; head lanes add the coefficients of the
// non-head lanes that follow them one shuffle at a time — SEQUENTIALLY in ascending input order (the sort is stable), exactly
// np.add.at's order (utils.py:273-274) — and a segment that runs past the end of a chunk is carried (wave-uniform
// accumulator) into the next chunks, past the end of the wave's own range if necessary (those chunks are only decoded, their
// owner verifies them); the leading non-head positions of a range therefore belong to the previous wave and are skipped.
// A term that survives the strict |c| > thr test sets the bit of its first input index in `markbits` (T bits: 12.5 MB for
// 1e8 terms, cache resident) and files its sum under that index in `sum_of` for the output stage.
template <bool PAIR, bool PACKED>
__global__ __launch_bounds__(256) void k_heads_sums(const u64 *__restrict__ keys, const u32 *__restrict__ idx, i64 T, const u64 *__restrict__ rows, int W,
                                                     const u64 *__restrict__ inner, u32 Ni, const u64 *__restrict__ outer, int G,
                                                     const double *__restrict__ coeff, u32 *__restrict__ collision,
                                                     const u64 *__restrict__ hI, const u64 *__restrict__ hO, PackedLayout L,
                                                     const double *__restrict__ ci, const double *__restrict__ co,
                                                     double thr, int use_thr, u32 *__restrict__ markbits, double *__restrict__ sum_of,
                                                     i64 chunks_per_wave, int squared, const u32 *__restrict__ zero_len = nullptr,
                                                     u32 *__restrict__ patchbits = nullptr, const u32 *__restrict__ dirtybits = nullptr) {
    // patchbits != null ("lazy" mode, see k_mark_singles): one-element segments are not touched at all, and wavefront w only works on
    // the chunks whose bit is set in dirtybits[w] (k_find_merges: the chunks that hold a member of a segment of more than one element)
    // zero_len (squared operators): the first *zero_len sorted positions are the identity segment, already reduced by k_zero_partial /
    // k_zero_close — they are treated like positions past the end (they end every run and contribute nothing)
    const i64 ZL = zero_len ? (i64)*zero_len : 0;
    // squared (PACKED only, P * P): the keys are the pairs with i >= o; an off-diagonal pair stands for itself and its twin
    // (o, i), whose coefficient is bit-identical in magnitude (IEEE products and sums commute): it counts twice if the two terms
    // commute (e even) and not at all if they anticommute (e odd) — it then only marks the first occurrence of its row.
    const int lane = threadIdx.x & 63;
    const int gi = lane / G, gl = lane % G;
    const int C = W / 2;                                             // 16-byte chunks per row
    const u64 gmask = G == 64 ? ~0ULL : (((1ULL << G) - 1ULL) << (gi * G));
    const i64 n_chunks = (T + 63) / 64;
    const i64 gw = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    u32 dirty = 0;
    if (dirtybits) {                                                // eight chunks per wavefront: a quarter of a bitmap word
        if (gw * 8 >= n_chunks) return;
        dirty = (__builtin_amdgcn_readfirstlane(dirtybits[gw >> 2]) >> (8 * (int)(gw & 3))) & 0xFFu;
        if (dirty == 0) return;
    }

    const bool lazy = patchbits != nullptr;
    auto close = [&](u32 first, double re, double im, bool multi) {   // strict threshold, bitmap, sum filed under the first index
        if (lazy && !multi) return;                                   // a single: decided by k_mark_singles, rebuilt by k_emit_meta
        if (use_thr && !above_thr(re, im, thr)) {
            if (lazy) atomicAnd(&markbits[first >> 5], ~(1u << (first & 31u)));
            return;
        }
        atomicOr(&markbits[first >> 5], 1u << (first & 31u));
        if (lazy) atomicOr(&patchbits[first >> 5], 1u << (first & 31u));
        double2 o; o.x = re; o.y = im;
        reinterpret_cast<double2 *>(sum_of)[first] = o;
    };

    bool open = false;                  // wave-uniform: a segment is carried across chunk boundaries
    double are = 0.0, aim = 0.0;        // its running sum
    u32 afirst = 0;                     // input index of its first (head) element
    bool amulti = false;                // it has more than one element so far
    bool mism = false;
    for (;;) {                          // the wavefront's chunk ranges: one, or — dirtybits — one per set bit
    i64 c0, c1;
    if (dirtybits) {
        if (dirty == 0) break;
        c0 = gw * 8 + __builtin_ctz(dirty);
        dirty &= dirty - 1;
        c1 = c0 + 1;
        open = false;
    } else {
        c0 = gw * chunks_per_wave;
        if (c0 >= n_chunks) break;
        c1 = c0 + chunks_per_wave < n_chunks ? c0 + chunks_per_wave : n_chunks;
    }
    for (i64 chunk = c0;; ++chunk) {
        if (chunk >= c1 && !open) break;
        if (chunk >= n_chunks) {        // the carried segment ends with the data
            if (lane == 0) close(afirst, are, aim, amulti);
            break;
        }
        const bool own = chunk < c1;    // beyond the own range: decode only, to finish the carried segment
        if (!own) {
            // Peek before decoding a foreign chunk: the carried segment only continues if the chunk's FIRST key equals the key before
            // it — almost never (an operator without duplicate rows merges nothing).  Two wave-uniform loads instead of 64 keys,
            // 128 coefficient-table gathers and the sum loop: with one chunk per wavefront this second pass was half of the kernel.
            const i64 s0 = chunk * 64;                                // 0 < s0 < T
            const u64 kb = keys[s0], ka = keys[s0 - 1];
            bool eq0;
            if (PACKED) {
                eq0 = (kb >> L.F()) == (ka >> L.F());
                if (eq0 && !(inner == outer && L.i(kb) == L.o(ka) && L.o(kb) == L.i(ka))) eq0 = (hI[L.i(kb)] ^ hO[L.o(kb)]) == (hI[L.i(ka)] ^ hO[L.o(ka)]);
            } else eq0 = kb == ka;
            if (!eq0) {
                if (lane == 0) close(afirst, are, aim, amulti);
                break;
            }
        }
        const i64 s = chunk * 64 + lane;
        const bool valid = s < T && s >= ZL;
        // this position: key k1, input index t1 (PAIR: as (i1, o1)); predecessor k0 / t0 / (i0, o0) from the neighbour lane
        // (lane 0 reads position s-1 itself)
        u64 k1 = valid ? keys[s] : 0ULL;
        u64 k0 = __shfl_up(k1, 1);
        if (lane == 0 && valid && s > 0) k0 = keys[s - 1];
        u32 t1 = 0, i1 = 0, o1 = 0, t0 = 0, i0 = 0, o0 = 0;
        bool eq;
        if (PACKED) {
            i1 = L.i(k1); o1 = L.o(k1); i0 = L.i(k0); o0 = L.o(k0);
            // index under which the term is filed: the pair index, or — squared mode — its slot in the compacted key order (the
            // same order, half the index space: bitmap and sums stay dense)
            t1 = squared ? tri_slot(o1, i1, Ni) : o1 * Ni + i1;
            // equal 64-bit keys?  Different hash prefixes: no.  P * P twins (i, o) / (o, i): yes, the two hash tables are the
            // same.  Otherwise (about 1 % of the positions) the full keys are rebuilt from the operand hash tables.
            eq = valid && s > 0 && (k1 >> L.F()) == (k0 >> L.F());
            if (eq && !(inner == outer && i1 == o0 && o1 == i0)) eq = (hI[i1] ^ hO[o1]) == (hI[i0] ^ hO[o0]);
        } else {
            if (valid) t1 = idx[s];
            t0 = __shfl_up(t1, 1);
            if (lane == 0 && valid && s > 0) t0 = idx[s - 1];
            if (PAIR) { o1 = t1 / Ni; i1 = t1 - o1 * Ni; o0 = t0 / Ni; i0 = t0 - o0 * Ni; }
            eq = valid && s > 0 && k1 == k0;
        }
        double2 c; c.x = 0.0; c.y = 0.0;
        // lazy: only members of segments with more than one element need their coefficient — a position that equals its predecessor,
        // one whose successor equals it, and lane 63 (its successor is in the next chunk)
        bool need = valid;
        if (lazy) {
            const int eq_next = __shfl_down((int)eq, 1);
            need = valid && (eq || eq_next || lane == 63);
            if (valid && eq) atomicAnd(&markbits[t1 >> 5], ~(1u << (t1 & 31u)));      // a follower is never the first occurrence
        }
        if (need) {
            if (PACKED) {
                pair_coefficient(ci[2 * i1], ci[2 * i1 + 1], co[2 * o1], co[2 * o1 + 1], L.e(k1), c.x, c.y);
                if (squared && i1 != o1) {
                    if (L.e(k1) & 1) { c.x = 0.0; c.y = 0.0; }
                    else { c.x = __dadd_rn(c.x, c.x); c.y = __dadd_rn(c.y, c.y); }
                }
            } else c = reinterpret_cast<const double2 *>(coeff)[t1];
        }
        if (own) {
            // exact verification of the equal-key neighbours.  P * P: row(i, o) == row(o, i) by commutativity of XOR when both
            // operands are the same array — nothing to read
            const bool trivially_equal = PAIR && inner == outer && i1 == o0 && o1 == i0;
            u64 sub = __ballot(eq && !trivially_equal) & gmask;      // this group's candidates
            while (__ballot(sub != 0ULL)) {                          // wave-uniform
                const bool act = sub != 0ULL;
                const int p = act ? __builtin_ctzll(sub) : 0;
                sub &= sub - 1;
                if (PAIR) {
                    const i64 ci1 = __shfl(i1, p), co1 = __shfl(o1, p), ci0 = __shfl(i0, p), co0 = __shfl(o0, p);
                    if (act) {
                        const u32x4 *r1 = reinterpret_cast<const u32x4 *>(inner + ci1 * W), *q1 = reinterpret_cast<const u32x4 *>(outer + co1 * W);
                        const u32x4 *r0 = reinterpret_cast<const u32x4 *>(inner + ci0 * W), *q0 = reinterpret_cast<const u32x4 *>(outer + co0 * W);
                        for (int cc = gl; cc < C; cc += G) mism |= differs(r1[cc] ^ q1[cc], r0[cc] ^ q0[cc]);
                    }
                } else {
                    const i64 a1 = __shfl(t1, p), a0 = __shfl(t0, p);
                    if (act) {
                        const u32x4 *r1 = reinterpret_cast<const u32x4 *>(rows + a1 * W), *r0 = reinterpret_cast<const u32x4 *>(rows + a0 * W);
                        for (int cc = gl; cc < C; cc += G) mism |= differs(r1[cc], r0[cc]);
                    }
                }
            }
        }
        // ---- segment sums on the head flags (positions past the end act as heads: they end every run) ----
        const u64 m = __ballot(!valid || !eq);
        const int lead = m ? __builtin_ctzll(m) : 64;             // leading non-head lanes continue the carried segment
        if (open) {
            for (int k = 0; k < lead; ++k) {
                are = __dadd_rn(are, __shfl(c.x, k));
                aim = __dadd_rn(aim, __shfl(c.y, k));
            }
            if (lead > 0) amulti = true;
        }
        if (m == 0ULL) continue;                                  // no head in this chunk
        if (open) {
            if (lane == 0) close(afirst, are, aim, amulti);
            open = false;
        }
        if (!own) break;                                          // beyond the own range only the carry had to be closed
        const bool is_head = valid && !eq;
        const u64 above = lane == 63 ? 0ULL : (m >> (lane + 1));
        const int run = above ? __builtin_ctzll(above) : 63 - lane;   // non-head lanes that follow this lane in the chunk
        double re = __dadd_rn(0.0, c.x), im = __dadd_rn(0.0, c.y);
        for (int k = 1; __ballot(is_head && k <= run); ++k) {
            const double vx = __shfl_down(c.x, k), vy = __shfl_down(c.y, k);
            if (is_head && k <= run) {
                re = __dadd_rn(re, vx);
                im = __dadd_rn(im, vy);
            }
        }
        // the last head of a full chunk may continue in the next chunk: carry it; everything else closes here
        const int last = 63 - __builtin_clzll(m);
        // a full chunk whose last head is a real position: its run reaches lane 63 and may continue in the next chunk
        const bool carry = chunk * 64 + 64 <= T && ((__ballot(valid) >> last) & 1ULL);
        if (is_head && !(carry && lane == last)) close(t1, re, im, run > 0);
        if (carry) {
            open = true;
            are = __shfl(re, last);
            aim = __shfl(im, last);
            afirst = __shfl(t1, last);
            amulti = __shfl(run, last) > 0;
        }
    }
    if (!dirtybits) break;
    }
    if (__ballot(mism) && lane == 0) atomicOr(collision, 1u);
}

// Truncated sort fix-up.  The radix sort only orders the top `nb` key bits (random hash bits: ~log2(T)+5..12 of them already
// separate almost all distinct keys).  Inside a run of equal prefixes the elements are still in input order; if such a
// run holds more than one distinct key it is re-ordered here by (full key, input order) with a stable insertion sort.
// Runs longer than FIX_MAX that are not uniform raise `fallback`: the caller then redoes a full 64-bit sort.
constexpr int FIX_MAX = 48;
// Round 3: the keys that need a look at all — a key inside a run that differs from its predecessor (round 6: no longer every run's first
// key as well: an input full of repeated rows has a run start at every third position, and walking all those uniform runs was a quarter of a
// plain cleanup, 60 of 237 us at 10^5 rows) — are flagged by a streaming pass (k_fixup_find: four chunks per wavefront and step,
// one 64-bit word of flags per chunk, plain stores: appending to ONE list counter instead serialises 4e5 returning atomics on one
// address, 2.8 ms) and worked off by wavefronts that expand the flags of 4,096 positions into a dense list (k_fixup_work): the thread
// of a flagged key measures its run by the prefixes, raises `fallback` if it is longer than FIX_MAX (a long UNIFORM run — the identity
// segment of a squared operator — has no flagged key and costs nothing) and, if no earlier member of the run is flagged, sorts it.
// Threads of one run may read keys while its first flagged member reorders them: all of them share the prefix, which is all the others
// look at (who is first is read from the flags, which nobody writes here).  (The two launches this replaces walked the runs from inside the streaming pass: 0.33 ms at cfg3, now 0.11.)
// PACKED: keys are packed pair keys (full key recomputed from the (i, o) fields), there is no separate idx array.
template <bool PACKED>
__device__ __forceinline__ bool fixup_differ(u64 k, u64 kp, const u64 *__restrict__ hI, const u64 *__restrict__ hO, const PackedLayout &L, bool same_operand) {
    if (PACKED) {
        if (same_operand && L.i(k) == L.o(kp) && L.o(k) == L.i(kp)) return false;         // P * P twins: equal keys by construction
        return L.full_key(hI, hO, k) != L.full_key(hI, hO, kp);
    }
    return k != kp;
}
template <bool PACKED>
__global__ __launch_bounds__(256) void k_fixup_find(const u64 *__restrict__ keys, i64 T, int shift, const u64 *__restrict__ hI, const u64 *__restrict__ hO,
                                                     PackedLayout L, bool same_operand, u64 *__restrict__ rarebits, u32 *__restrict__ dirtybits) {
    // dirtybits (lazy cleanup): a key that EQUALS its predecessor is a merged term — its chunk and its predecessor's are the ones
    // k_heads_sums has to visit (k_find_merges' job, done here in the same pass; a run that k_fixup_work reorders is marked again there)
    const int lane = threadIdx.x & 63;
    const i64 n_steps = (T + 255) / 256;
    for (i64 g = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_steps; g += (i64)gridDim.x * 4) {
        const i64 base = g * 256;
        u64 k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const i64 sp = base + 64 * j + lane; k[j] = sp < T ? keys[sp] : 0ULL; }
        const u64 prev = base > 0 ? keys[base - 1] : 0ULL;
        const u64 next = base + 256 < T ? keys[base + 256] : 0ULL;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const i64 sp = base + 64 * j + lane;
            u64 kp = __shfl_up(k[j], 1), kn = __shfl_down(k[j], 1);
            const u64 in_lo = j > 0 ? __shfl(k[j > 0 ? j - 1 : 0], 63) : prev;
            const u64 in_hi = j < 3 ? __shfl(k[j < 3 ? j + 1 : 3], 0) : next;
            if (lane == 0) kp = in_lo;
            if (lane == 63) kn = in_hi;
            const bool valid = sp < T;
            const bool with_prev = valid && sp > 0 && (kp >> shift) == (k[j] >> shift);
            const bool with_next = valid && sp + 1 < T && (kn >> shift) == (k[j] >> shift);
            (void)with_next;
            const bool rare = with_prev && fixup_differ<PACKED>(k[j], kp, hI, hO, L, same_operand);
            const u64 b = __ballot(rare);
            if (lane == 0 && base + 64 * j < T) rarebits[base / 64 + j] = b;
            if (dirtybits) {
                const u64 m = __ballot(with_prev && !rare);
                if (m != 0ULL && lane == 0) {
                    const i64 chunk = base / 64 + j;
                    atomicOr(&dirtybits[chunk >> 5], 1u << (chunk & 31));
                    if ((m & 1ULL) && chunk > 0) atomicOr(&dirtybits[(chunk - 1) >> 5], 1u << ((chunk - 1) & 31));
                }
            }
        }
    }
}
template <bool PACKED>
__global__ __launch_bounds__(256) void k_fixup_work(u64 *__restrict__ keys, u32 *__restrict__ idx, i64 T, int shift, const u64 *__restrict__ rarebits,
                                                     u32 *__restrict__ fallback, const u64 *__restrict__ hI,
                                                     const u64 *__restrict__ hO, PackedLayout L, bool same_operand, u32 *__restrict__ dirtybits) {
    __shared__ unsigned short s_list[4][4096];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned short *list = s_list[wave];
    const i64 n_chunks = (T + 63) / 64;
    const i64 cw = ((i64)blockIdx.x * 4 + wave) * 64 + lane;                  // this lane's chunk: 64 chunks = 4,096 positions per wavefront
    u64 bits = cw < n_chunks ? rarebits[cw] : 0ULL;
    const u32 cnt = (u32)__popcll(bits);
    const u32 incl = wave_incl_scan(cnt, lane);
    const u32 n = __shfl(incl, 63);
    if (n == 0) return;                                                       // wave-uniform
    {
        u32 at = incl - cnt;
        while (bits) { list[at++] = (unsigned short)(lane * 64 + __builtin_ctzll(bits)); bits &= bits - 1; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const i64 wbase = ((i64)blockIdx.x * 4 + wave) * 4096;
    for (u32 it = lane; it < n; it += 64) {
        const i64 sp = wbase + list[it];
        const u64 k = keys[sp];                                               // (only its prefix is used: the run's first flagged member may be moving keys)
        // the run's start and end (prefixes do not change under the reordering)
        i64 b = sp, e = sp + 1;
        while (b > 0 && sp - b <= FIX_MAX && (keys[b - 1] >> shift) == (k >> shift)) --b;
        while (e < T && e - b <= FIX_MAX && (keys[e] >> shift) == (k >> shift)) ++e;
        if (e - b > FIX_MAX) { atomicOr(fallback, 1u); continue; }           // a long run that is not uniform: the caller sorts completely
        bool first = true;                                                    // the run's FIRST flagged member reorders it (the flags are not written here)
        for (i64 j = b + 1; j < sp; ++j)
            if ((rarebits[j >> 6] >> (j & 63)) & 1ULL) { first = false; break; }
        if (!first) continue;
        for (i64 a = b + 1; a < e; ++a) {                                     // stable insertion sort by full key
            const u64 ka = keys[a];
            if (PACKED) {
                const u64 fa = L.full_key(hI, hO, ka);
                i64 c = a - 1;
                while (c >= b && L.full_key(hI, hO, keys[c]) > fa) { keys[c + 1] = keys[c]; --c; }
                keys[c + 1] = ka;
            } else {
                const u32 ia = idx[a];
                i64 c = a - 1;
                while (c >= b && keys[c] > ka) { keys[c + 1] = keys[c]; idx[c + 1] = idx[c]; --c; }
                keys[c + 1] = ka;
                idx[c + 1] = ia;
            }
        }
        if (dirtybits)                                                        // the merged terms of the reordered run, where they are now
            for (i64 a = b + 1; a < e; ++a)
                if (!fixup_differ<PACKED>(keys[a], keys[a - 1], hI, hO, L, same_operand)) {
                    const i64 ca = a / 64, cb = (a - 1) / 64;
                    atomicOr(&dirtybits[ca >> 5], 1u << (ca & 31));
                    if (cb != ca) atomicOr(&dirtybits[cb >> 5], 1u << (cb & 31));
                }
    }
}

__global__ __launch_bounds__(256) void k_count_bits(const u32 *__restrict__ bits, i64 n_words, u32 *__restrict__ total) {
    u32 c = 0;
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (i64)gridDim.x * blockDim.x) c += (u32)__popc(bits[w]);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, c);
}

// zeroes of up to three buffers in ONE launch (byte counts multiples of 4): hipMemsetAsync is a launch per buffer, two when the size is not a
// multiple of its fill kernel's granule, 5 us each on an otherwise idle queue
__global__ __launch_bounds__(256) void k_zero_two(u32 *__restrict__ a, i64 na, u32 *__restrict__ b, i64 nb, u32 *__restrict__ c, i64 nc) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < na; i += (i64)gridDim.x * 256) a[i] = 0u;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nb; i += (i64)gridDim.x * 256) b[i] = 0u;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nc; i += (i64)gridDim.x * 256) c[i] = 0u;
}
int zero_two(void *a, size_t bytes_a, void *b, size_t bytes_b, void *c, size_t bytes_c) {
    const i64 na = (i64)(bytes_a / 4), nb = b ? (i64)(bytes_b / 4) : 0, nc = c ? (i64)(bytes_c / 4) : 0;
    if (na + nb + nc == 0) return SYMGPU_OK;
    i64 nmax = na > nb ? na : nb;
    nmax = nmax > nc ? nmax : nc;
    hipLaunchKernelGGL(k_zero_two, dim3(grid_for(nmax, 256, 4096)), dim3(256), 0, ctx().stream, static_cast<u32 *>(a), na, static_cast<u32 *>(b), nb,
                       static_cast<u32 *>(c), nc);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// P * P: the identity coefficient in the reference's own (sequential) order, see k_diag_seq_sum.  Large operators: on the side stream,
// joined just before k_zero_close reads it; small ones inline (two event operations cost more than the kernel).
int cleanup_diag_begin(CleanupRun &r) {
    Context &c = ctx(); const i64 Ni = r.rq.p.Ni;
    SG_TRY(r.diag_seq.alloc(16));
    r.diag_side = Ni > 2048;
    if (r.diag_side) { HIP_TRY(hipEventRecord(c.ev_fork, r.st)); HIP_TRY(hipStreamWaitEvent(c.stream2, c.ev_fork, 0)); }
    hipLaunchKernelGGL(k_diag_seq_sum, dim3(1), dim3(64), 0, r.diag_side ? c.stream2 : r.st, r.rq.p.ci, (u32)Ni, r.diag_seq.as<double>());
    KERNEL_CHECK();
    if (r.diag_side) HIP_TRY(hipEventRecord(c.ev_join, c.stream2));
    return SYMGPU_OK;
}

// the status words zeroed (and the bitmaps the later stages expect zeroed); the runs of equal prefixes that hold more than one key put in order
int cleanup_fixups(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; const PairOperands &p = r.rq.p; CleanupRun::Attempt &a = r.a; hipStream_t st = r.st; const i64 Tsort = a.Tsort;
    // (no key has a partner — Tsort == 0 —: every term is a single, decided by k_mark_singles; the patch bitmap is zeroed in the same launch)
    // (and without the lazy flow the kept-term bitmap, which the segment sums then fill: one launch for both)
    a.mark_zeroed = !pl.lazy && Tsort > 0;
    if (!(a.fix_bits < 64 && Tsort > 0 && pl.lazy))
        SG_TRY(zero_two(r.collision.p, 16, Tsort == 0 ? r.patchbits.p : nullptr, (size_t)(pl.Tk + 63) / 64 * 8, a.mark_zeroed ? r.markbits.p : nullptr,
                        (size_t)(pl.Tk + 31) / 32 * 4));
    if (!(a.fix_bits < 64 && Tsort > 0)) return SYMGPU_OK;
    const i64 n_ch = (Tsort + 63) / 64;
    SG_TRY(r.fixlist.alloc((size_t)n_ch * 8 + 16));                         // one word of flags per 64 positions
    u32 *dirty_fx = nullptr;
    if (pl.lazy) {                                                          // the chunks with merged terms are found in the same pass
        const i64 n_dw = (n_ch + 31) / 32;
        SG_TRY(r.dirtybits.alloc((size_t)n_dw * 4 + 16));
        // (with the flagged keys alone in the sorted array the lazy flow is never given up below: its patch bitmap is zeroed here too)
        a.patch_zeroed = a.sus_active && r.patchbits.p != nullptr;
        SG_TRY(zero_two(r.collision.p, 16, r.dirtybits.p, (size_t)n_dw * 4 + 16, a.patch_zeroed ? r.patchbits.p : nullptr, (size_t)((pl.Tk + 63) / 64) * 8));
        dirty_fx = r.dirtybits.as<u32>();
        a.merges_found = true;
    }
    const dim3 gff((unsigned)grid_for((Tsort + 255) / 256, 4, 8192));
    const dim3 gfw((unsigned)((n_ch + 255) / 256));
    const int shift = 64 - a.fix_bits;
    if (pl.packed) {
        hipLaunchKernelGGL(k_fixup_find<true>, gff, dim3(256), 0, st, a.ks, Tsort, shift, r.hI.as<u64>(), r.hO_p, pl.L, p.inner == p.outer, r.fixlist.as<u64>(), dirty_fx);
        hipLaunchKernelGGL(k_fixup_work<true>, gfw, dim3(256), 0, st, a.ks, (u32 *)nullptr, Tsort, shift, r.fixlist.as<u64>(), r.collision.as<u32>() + 1,
                           r.hI.as<u64>(), r.hO_p, pl.L, p.inner == p.outer, dirty_fx);
    } else {
        hipLaunchKernelGGL(k_fixup_find<false>, gff, dim3(256), 0, st, a.ks, Tsort, shift, (const u64 *)nullptr, (const u64 *)nullptr, pl.L, false, r.fixlist.as<u64>(), dirty_fx);
        hipLaunchKernelGGL(k_fixup_work<false>, gfw, dim3(256), 0, st, a.ks, a.is, Tsort, shift, r.fixlist.as<u64>(), r.collision.as<u32>() + 1,
                           (const u64 *)nullptr, (const u64 *)nullptr, pl.L, false, dirty_fx);
    }
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// the sums of the segments of more than one key (all segments without the lazy flow), filed under their first input index
int cleanup_segment_sums(CleanupRun &r) {
    const CleanupPlan &pl = r.pl; const CleanupRequest &rq = r.rq; const PairOperands &p = rq.p; CleanupRun::Attempt &a = r.a;
    hipStream_t st = r.st; const i64 Tsort = a.Tsort; const int W = rq.W; const u64 *ks = a.ks;
    if (Tsort == 0) return SYMGPU_OK;    // nothing can merge (no key has a partner): every term is a single, decided by k_mark_singles
    int G = 1;                                   // lanes per verified candidate: one 16-byte chunk each
    while (G < W / 2 && G < 64) G <<= 1;
    const i64 n_chunks = (Tsort + 63) / 64;
    // The kernel is latency bound (dependent key load -> operand table gathers -> store per 64-position chunk; rocprofv3: 6 % of
    // the wave cycles issue, 53 % wait on memory), so it wants many short waves rather than few long ones: cfg3 6.39 / 6.16 /
    // 6.10 / 6.04 ms at 2^15 / 2^17 / 2^19 / 2^21 wavefronts (a wave also decodes the chunk after its range to close the
    // segment it carries, so one chunk per wave reads the keys twice — still the fastest).
    const i64 HS_WAVES = r.sw.hs_waves;
    const i64 cpw = (n_chunks + HS_WAVES - 1) / HS_WAVES;     // <= HS_WAVES wavefronts, each on a contiguous range of chunks
    const i64 n_waves = (n_chunks + cpw - 1) / cpw;
    const dim3 gs((unsigned)((n_waves + 3) / 4));
    const u64 *nul = nullptr; const double *nud = nullptr;
    // Adaptive: when many chunks hold merged terms — an input full of repeated rows: the followers' bitmap atomics of the lazy
    // flow then cost more than the heads' scatter it saves (10^8 pairs with ~5 copies of every row: 6.2 ms lazy against 4.5 ms
    // filed) — every term is filed from the sorted order after all; k_mark_singles' pass was wasted (one count read-back).
    if (a.lazy && a.merges_found && r.sw.lazy != 1 && !a.sus_active) {       // (sus_active: the sorted keys ARE the merged terms)
        u32 *dcount = r.collision.as<u32>() + 3;
        hipLaunchKernelGGL(k_count_bits, dim3(grid_for((n_chunks + 31) / 32)), dim3(256), 0, st, r.dirtybits.as<u32>(), (n_chunks + 31) / 32, dcount);
        KERNEL_CHECK();
        u32 h_dirty = 0;
        SG_TRY(read_back_words(dcount, 1, nullptr, 0, &h_dirty));
        if ((i64)h_dirty * 8 > n_chunks) a.lazy = false;
    }
    if (a.lazy) { if (!a.patch_zeroed) SG_TRY(zero_two(r.patchbits.p, (size_t)((pl.Tk + 63) / 64) * 8, nullptr, 0)); }
    else if (!a.mark_zeroed) SG_TRY(zero_two(r.markbits.p, (size_t)((pl.Tk + 31) / 32) * 4, nullptr, 0));
    u32 *patch_p = a.lazy ? r.patchbits.as<u32>() : nullptr;
    const u32 *zero_len_p = nullptr;
    if (pl.squared && r.sw.zero_seg) {
        // the identity segment (the N diagonal pairs and whatever else multiplies to the identity) in parallel, see k_zero_partial
        const i64 n_zb = (Tsort + ZB - 1) / ZB;
        SG_TRY(r.zpart.alloc((size_t)n_zb * 16));
        SG_TRY(r.zcount.alloc((size_t)n_zb * 4 + 16));
        u32 *zl = r.zcount.as<u32>() + n_zb;
        hipLaunchKernelGGL(k_zero_partial, dim3((unsigned)n_zb), dim3(256), 0, st, ks, Tsort, r.hI.as<u64>(), r.hO_p, pl.L, p.inner, W, p.ci,
                           r.zpart.as<double>(), r.zcount.as<u32>(), r.collision.as<u32>(), (u32)p.Ni, a.lazy ? r.markbits.as<u32>() : (u32 *)nullptr);
        if (r.diag_side) { HIP_TRY(hipStreamWaitEvent(st, ctx().ev_join, 0)); r.diag_side = false; }
        hipLaunchKernelGGL(k_zero_close, dim3(1), dim3(64), 0, st, ks, r.zpart.as<double>(), r.zcount.as<u32>(), n_zb, pl.L, (u32)p.Ni, rq.thr, rq.use_thr,
                           r.markbits.as<u32>(), r.sum_of.as<double>(), zl, patch_p, r.diag_seq.as<double>(), r.collision.as<u32>() + 2);
        zero_len_p = zl;
    }
    const u32 *dirty_p = nullptr;
    dim3 gsl = gs;
    if (a.lazy) {
        // the chunks that hold a member of a segment of more than one element; k_heads_sums then works on those only
        const i64 n_dw = (n_chunks + 31) / 32;
        if (!a.merges_found) {
            SG_TRY(r.dirtybits.alloc((size_t)n_dw * 4 + 16));
            HIP_TRY(hipMemsetAsync(r.dirtybits.p, 0, (size_t)n_dw * 4 + 16, st));
            const dim3 gf((unsigned)grid_for((Tsort + 255) / 256, 4, 8192));
            if (pl.packed) hipLaunchKernelGGL(k_find_merges<true>, gf, dim3(256), 0, st, ks, Tsort, zero_len_p, pl.L, r.hI.as<u64>(), r.hO_p, p.inner == p.outer ? 1 : 0, r.dirtybits.as<u32>());
            else hipLaunchKernelGGL(k_find_merges<false>, gf, dim3(256), 0, st, ks, Tsort, zero_len_p, pl.L, nul, nul, 0, r.dirtybits.as<u32>());
            KERNEL_CHECK();
        }
        dirty_p = r.dirtybits.as<u32>();
        gsl = dim3((unsigned)(((n_chunks + 7) / 8 + 3) / 4));
    }
    const int sq = pl.squared ? 1 : 0;
    if (pl.packed)
        hipLaunchKernelGGL((k_heads_sums<true, true>), gsl, dim3(256), 0, st, ks, (const u32 *)nullptr, Tsort, nul, W, p.inner, (u32)p.Ni, p.outer, G, nud,
                           r.collision.as<u32>(), r.hI.as<u64>(), r.hO_p, pl.L, p.ci, p.co, rq.thr, rq.use_thr, r.markbits.as<u32>(), r.sum_of.as<double>(), cpw, sq,
                           zero_len_p, patch_p, dirty_p);
    else if (rq.pair)
        hipLaunchKernelGGL((k_heads_sums<true, false>), gsl, dim3(256), 0, st, ks, a.is, Tsort, nul, W, p.inner, (u32)p.Ni, p.outer, G, r.coeff,
                           r.collision.as<u32>(), nul, nul, pl.L, nud, nud, rq.thr, rq.use_thr, r.markbits.as<u32>(), r.sum_of.as<double>(), cpw, sq,
                           (const u32 *)nullptr, patch_p, dirty_p);
    else
        hipLaunchKernelGGL((k_heads_sums<false, false>), gsl, dim3(256), 0, st, ks, a.is, Tsort, rq.rows, W, nul, 1u, nul, G, r.coeff,
                           r.collision.as<u32>(), nul, nul, pl.L, nud, nud, rq.thr, rq.use_thr, r.markbits.as<u32>(), r.sum_of.as<double>(), cpw, sq,
                           (const u32 *)nullptr, patch_p, dirty_p);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
