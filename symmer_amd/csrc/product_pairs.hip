// product_pairs.hip — the word-major pair kernel of the all-pairs product: phase exponent of every pair on the VALU.
//
//   coeff  =  c_i * c_o * i^e ,  e = (3(Y_i+Y_o) + Y_out + 2|x_left & z_right|) mod 4
//
// k_mul_coeff: 8 instructions per pair per 64-bit word (xor, bitop3, bcnt, bitop3 per 32-bit half).  Word-major operands: 8 outer terms per
// wave arrive in SGPRs via s_load_dwordx16, 4 inner terms per lane via coalesced 512-byte loads.  Writes 16 B/pair (coefficients), 8 B/pair
// (cleanup keys) or 1 B/pair (phase exponents), coalesced along the inner index.  VALU-bound: 0.158 ms per 2.56e7 pairs of 1,000 qubits.
// The product uses it for rows that are not a power-of-two number of 16-byte chunks (product_driver.hip); the fused product + cleanup
// always (mul_keys_dev, mul_coeff_dev).  product_common.h lists the files.
#include "product_common.h"

namespace symgpu {

__device__ __forceinline__ u32 xor_and(u32 acc, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(acc, b, c, 0x78); }   // a ^ (b & c)
__device__ __forceinline__ u32 to_vgpr(u32 s) { u32 v; asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s)); return v; }
__device__ __forceinline__ u32 and_xor(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x60); }     // a & (b ^ c)
__device__ __forceinline__ u32 bcnt_acc(u32 x, u32 acc) { u32 r; asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc)); return r; }   // popc(x) + acc

// phase exponent of a pair: (3 (Y_i + Y_o) + Y_out + 2 |x_left & z_right|) mod 4, the last term as the parity of the accumulated flip word
__device__ __forceinline__ u32 pair_exponent(u32 yi, int yo, u32 cnt, u32 flip) { return (3u * (yi + (u32)yo) + cnt + 2u * (__popc(flip) & 1u)) & 3u; }
// packed cleanup key [hash][e: 2][o: bo][i: bi] (cleanup_common.h); hmask clears the hash bits the three fields take
__device__ __forceinline__ u64 pack_pair_key(u64 hi, u64 ho, u64 hmask, u64 e, i64 o, i64 i, const PairKeyArgs &ka) {
    return ((hi ^ ho) & hmask) | (e << (ka.bi + ka.bo)) | ((u64)o << ka.bi) | (u64)i;
}
__device__ __forceinline__ u64 pair_hash_mask(const PairKeyArgs &ka) { return ~((1ULL << (ka.bi + ka.bo + 2)) - 1ULL); }

// KM = 0: coefficients.  KM = 1 (keys): instead of the coefficient the kernel emits the packed cleanup key of every pair
// (hash | phase exponent e | o | i): the 16-byte coefficient is never materialised, the cleanup rebuilds c_i * c_o * i^e from
// e and the two operand tables.  KM = 2 (keys of a squared operator, both operands the same array): the twins (i, o) / (o, i)
// of P * P are the same row with the same coefficient magnitude — equal if the two terms commute (e even), opposite if they
// anticommute (e odd) — and the twin with i > o comes first in pair-index order.  Only the pairs with i >= o get a key, half
// of them, written compacted in index order (slot = o*Ni - o(o-1)/2 + i - o); the cleanup weights them 1 (i == o), 2
// (commuting) or 0 (anticommuting: the pair still fixes the first-occurrence position of its row).
template <bool INNER_LEFT, int KM>
__global__ __launch_bounds__(256) void k_mul_coeff(const u64 *__restrict__ It, i64 Ipad, i64 Ni, const double *__restrict__ ci,
                                                    const u64 *__restrict__ Ot, i64 Opad, i64 No, const double *__restrict__ co,
                                                    int Wq, double *__restrict__ out /* [(o)*Ni + i][2], o relative to slab */,
                                                    PairKeyArgs ka) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr bool KEYS = KM != 0;
    const i64 o0 = ((i64)blockIdx.y * PW + wave) * PO;   // wave-uniform, relative to the slab
    const i64 ibase = (i64)blockIdx.x * (64 * PJ);
    if (ibase >= Ipad) return;                                         // surplus block of the grid padded to a multiple of 8 (below)
    if (KM == 2 && ibase + 64 * PJ - 1 < o0 + ka.o_base) return;       // tile strictly below the diagonal: no pair with i >= o

    u32 cnt[PO][PJ], flip[PO][PJ];
    u32 yi[PJ];
    int yo[PO];
#pragma unroll
    for (int a = 0; a < PO; ++a) {
        yo[a] = 0;
#pragma unroll
        for (int b = 0; b < PJ; ++b) cnt[a][b] = flip[a][b] = 0;
    }
#pragma unroll
    for (int b = 0; b < PJ; ++b) yi[b] = 0;

    const u64 *pox = Ot + o0, *poz = Ot + (i64)Wq * Opad + o0;
    const u64 *pix = It + ibase + lane, *piz = It + (i64)Wq * Ipad + ibase + lane;

    // The words of step w + 1 are fetched before the arithmetic of step w; one parity accumulator for both halves of a word frees the
    // registers the second set of operand words needs.
    // Two register sets used in turn (no copies between them): the loads of step w + 1 are issued at the top of step w and first used a
    // whole step later — the scalar loads of the outer words too, which the single-set form waited for right where it issued them.
    struct Words { u64 xi[PJ], zi[PJ], xo[PO], zo[PO]; };
    Words A, B;
    auto fetch = [&](Words &d, int w) {
#pragma unroll
        for (int b = 0; b < PJ; ++b) {
            d.xi[b] = pix[(i64)w * Ipad + 64 * b];
            d.zi[b] = piz[(i64)w * Ipad + 64 * b];
        }
#pragma unroll
        for (int a = 0; a < PO; ++a) {
            d.xo[a] = pox[(i64)w * Opad + a];      // wave-uniform -> s_load
            d.zo[a] = poz[(i64)w * Opad + a];
        }
    };
    auto step = [&](const Words &c) {
#pragma unroll
        for (int b = 0; b < PJ; ++b) yi[b] += __popcll(c.xi[b] & c.zi[b]);
#pragma unroll
        for (int a = 0; a < PO; ++a) yo[a] += __popcll(c.xo[a] & c.zo[a]);
#pragma unroll
        for (int a = 0; a < PO; ++a) {
            // SGPR sources cost ~40 % VALU issue rate on gfx950 (tools/ubench_bitop.hip): copy the uniform words to VGPRs once
            // (the words that only feed a two-operand v_xor stay scalar: an SGPR source is free there)
            const u32 xol = INNER_LEFT ? (u32)c.xo[a] : to_vgpr((u32)c.xo[a]), xoh = INNER_LEFT ? (u32)(c.xo[a] >> 32) : to_vgpr((u32)(c.xo[a] >> 32));
            const u32 zol = to_vgpr((u32)c.zo[a]), zoh = to_vgpr((u32)(c.zo[a] >> 32));
#pragma unroll
            for (int b = 0; b < PJ; ++b) {
                const u32 xil = (u32)c.xi[b], xih = (u32)(c.xi[b] >> 32), zil = (u32)c.zi[b], zih = (u32)(c.zi[b] >> 32);
                // Y_out += |(xi^xo) & (zi^zo)|   (v_bcnt with its accumulator operand: the compiler adds two counts with a third instruction)
                cnt[a][b] = bcnt_acc(and_xor(xil ^ xol, zil, zol), cnt[a][b]);
                cnt[a][b] = bcnt_acc(and_xor(xih ^ xoh, zih, zoh), cnt[a][b]);
                // flip ^= x_left & z_right
                if (INNER_LEFT) {
                    flip[a][b] = xor_and(flip[a][b], xil, zol);
                    flip[a][b] = xor_and(flip[a][b], xih, zoh);
                } else {
                    flip[a][b] = xor_and(flip[a][b], zil, xol);
                    flip[a][b] = xor_and(flip[a][b], zih, xoh);
                }
            }
        }
    };
    fetch(A, 0);
    int w = 0;
    for (; w + 1 < Wq; w += 2) {
        fetch(B, w + 1);
        step(A);
        fetch(A, w + 2 < Wq ? w + 2 : w + 1);
        step(B);
    }
    if (w < Wq) step(A);

    // Epilogue.  The stores of a full 8-outer-term tile are issued unconditionally back to back: a conditional store per
    // pair made the compiler drain the memory counter (s_waitcnt vmcnt(0)) before every single store.
    const bool full_o = o0 + PO <= No;                                   // wave-uniform
    u64 ho[PO];
    double cor[PO], coi[PO];
#pragma unroll
    for (int a = 0; a < PO; ++a) {
        const i64 o = (o0 + a < No) ? o0 + a : (No > 0 ? No - 1 : 0);    // clamped: rows past the end are computed, never stored
        if (KEYS) ho[a] = ka.hO[o];
        else { cor[a] = co[2 * o]; coi[a] = co[2 * o + 1]; }
    }
    const u64 hmask = KEYS ? pair_hash_mask(ka) : 0;
    if (KM == 2) {
#pragma unroll
        for (int a = 0; a < PO; ++a) {
            const i64 o = o0 + a + ka.o_base;                               // absolute outer index
            if (o0 + a >= No) break;                                        // wave-uniform
            u64 *dst = ka.keys + (o * Ni - o * (o - 1) / 2 - o);            // + i
#pragma unroll
            for (int b = 0; b < PJ; ++b) {
                const i64 i = ibase + 64 * b + lane;
                const u64 e = pair_exponent(yi[b], yo[a], cnt[a][b], flip[a][b]);
                if (i < Ni && i >= o) {
                    if (ka.ebytes) ka.ebytes[(o * Ni - o * (o - 1) / 2 - o) + i] = (unsigned char)(e | (i == o ? 4u : 0u));      // (uniform choice)
                    else dst[i] = pack_pair_key(ka.hI[i], ho[a], hmask, e, o, i, ka);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < PJ; ++b) {
        const i64 i = ibase + 64 * b + lane;
        if (i >= Ni) continue;
        if (KEYS) {
            const u64 hi = ka.hI[i];
            u64 key[PO];
#pragma unroll
            for (int a = 0; a < PO; ++a)
                key[a] = pack_pair_key(hi, ho[a], hmask, pair_exponent(yi[b], yo[a], cnt[a][b], flip[a][b]), o0 + a + ka.o_base, i, ka);
            if (ka.ebytes) {                                                // (uniform) one byte per pair: the phase exponent
                unsigned char *db = ka.ebytes + o0 * Ni + i;
                if (full_o) {
#pragma unroll
                    for (int a = 0; a < PO; ++a) db[(i64)a * Ni] = (unsigned char)((key[a] >> (ka.bi + ka.bo)) & 3u);
                } else {
#pragma unroll
                    for (int a = 0; a < PO; ++a)
                        if (o0 + a < No) db[(i64)a * Ni] = (unsigned char)((key[a] >> (ka.bi + ka.bo)) & 3u);
                }
                continue;
            }
            u64 *dst = ka.keys + o0 * Ni + i;
            if (full_o) {
#pragma unroll
                for (int a = 0; a < PO; ++a) dst[(i64)a * Ni] = key[a];
            } else {
#pragma unroll
                for (int a = 0; a < PO; ++a)
                    if (o0 + a < No) dst[(i64)a * Ni] = key[a];
            }
            continue;
        }
        const double ar = ci[2 * i], ai = ci[2 * i + 1];
        double2 v[PO];
#pragma unroll
        for (int a = 0; a < PO; ++a)
            pair_coefficient(ar, ai, cor[a], coi[a], (int)pair_exponent(yi[b], yo[a], cnt[a][b], flip[a][b]), v[a].x, v[a].y);
        double2 *dst = reinterpret_cast<double2 *>(out) + o0 * Ni + i;
        if (full_o) {
#pragma unroll
            for (int a = 0; a < PO; ++a) {
                const f64x2 w = {v[a].x, v[a].y};
                __builtin_nontemporal_store(w, reinterpret_cast<f64x2 *>(dst + (i64)a * Ni));   // streamed out: keep the operands in L2
            }
        } else {
#pragma unroll
            for (int a = 0; a < PO; ++a)
                if (o0 + a < No) dst[(i64)a * Ni] = v[a];
        }
    }
}

// the instantiation for a mode: km = 0 coefficients, 1 keys, 2 keys of a squared operator (left and right are the same operand)
static void launch_pairs(int inner_is_left, int km, dim3 grid, hipStream_t st, const u64 *It, i64 Ipad, i64 Ni, const double *ci, const u64 *Ot,
                         i64 Opad, i64 No, const double *co, int Wq, double *out, const PairKeyArgs &ka) {
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, It, Ipad, Ni, ci, Ot, Opad, No, co, Wq, out, ka); };
    if (km == 2) go(k_mul_coeff<true, 2>);
    else if (km == 1) inner_is_left ? go(k_mul_coeff<true, 1>) : go(k_mul_coeff<false, 1>);
    else inner_is_left ? go(k_mul_coeff<true, 0>) : go(k_mul_coeff<false, 0>);
}

int mul_coeff_launch(const u64 *It, i64 Ipad, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end, int Wq,
                     int inner_is_left, double *out_coeff, hipStream_t st, Scratch &ot, const PairKeyArgs *keys) {
    const i64 No = o_end - o_begin;
    const int W = 2 * Wq;
    // P * P in key mode: the word-major copy of the inner operand IS the outer one (its padding is the wider of the two)
    const bool same_operand = keys && keys->squared && o_begin == 0 && No == Ni;
    const i64 Opad = same_operand ? Ipad : round_up(No, PO * PW);
    const u64 *Ot = It;
    if (!same_operand) {
        SG_TRY(ot.alloc((size_t)Opad * W * sizeof(u64)));
        SG_TRY(to_wordmajor(outer + o_begin * W, No, W, ot.as<u64>(), Opad, st));
        Ot = ot.as<u64>();
    }
    // grid.x a multiple of 8: inner tile bx is then always read by XCD bx % 8, whose L2 keeps its eighth of the word-major inner
    // operand across the outer row blocks (same reasoning as for the row streams, product.hip)
    const i64 gx = ((Ni + 64 * PJ - 1) / (64 * PJ) + 7) / 8 * 8;
    return for_each_y_batch(round_up(No, PO * PW) / (PO * PW), [&](i64 y0, i64 ny) {
        const i64 ooff = y0 * PO * PW;
        const dim3 grid((unsigned)gx, (unsigned)ny);
        if (keys) {
            // key mode runs over the whole outer operand (o_begin == 0); the o field stays absolute through o_base
            PairKeyArgs ka = *keys;
            ka.hO += ooff;
            if (!ka.squared) ka.keys += ooff * Ni;                          // dense keys: slot o*Ni + i; squared: compacted, absolute slots
            ka.o_base = ooff;
            launch_pairs(inner_is_left, ka.squared ? 2 : 1, grid, st, It, Ipad, Ni, nullptr, Ot + ooff, Opad, No - ooff, nullptr, Wq, nullptr, ka);
        } else {
            launch_pairs(inner_is_left, 0, grid, st, It, Ipad, Ni, ci, Ot + ooff, Opad, No - ooff, co + 2 * (o_begin + ooff), Wq,
                         out_coeff + 2 * ooff * Ni, PairKeyArgs());
        }
        KERNEL_CHECK();
        return (int)SYMGPU_OK;
    });
}

// mul_coeff_dev and mul_keys_dev: nothing to do / few pairs of very long rows, parallel over the words (wide.hip) / the pair kernel on a
// word-major copy of the inner operand
static int mul_pairs(const u64 *inner, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end, int Wq,
                     int inner_is_left, double *out_coeff, const PairKeyArgs *keys) {
    if (Ni == 0 || o_end - o_begin <= 0) return SYMGPU_OK;
    if (wide_pairs_worthwhile(Ni, o_end - o_begin, Wq))
        return wide_mul_coeff_dev(inner, ci, Ni, outer, co, o_begin, o_end, Wq, inner_is_left, out_coeff, keys);
    const i64 Ipad = round_up(Ni, 64 * PJ);
    Scratch it, ot;
    SG_TRY(it.alloc((size_t)Ipad * 2 * Wq * sizeof(u64)));
    SG_TRY(to_wordmajor(inner, Ni, 2 * Wq, it.as<u64>(), Ipad));
    return mul_coeff_launch(it.as<u64>(), Ipad, ci, Ni, outer, co, o_begin, o_end, Wq, inner_is_left, out_coeff, ctx().stream, ot, keys);
}

int mul_coeff_dev(const u64 *inner, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end,
                  int Wq, int inner_is_left, double *out_coeff) {
    return mul_pairs(inner, ci, Ni, outer, co, o_begin, o_end, Wq, inner_is_left, out_coeff, nullptr);
}

int mul_keys_dev(const u64 *inner, i64 Ni, const u64 *outer, i64 No, int Wq, int inner_is_left, PairKeyArgs ka) {
    return mul_pairs(inner, nullptr, Ni, outer, nullptr, 0, No, Wq, inner_is_left, nullptr, &ka);
}

}  // namespace symgpu
