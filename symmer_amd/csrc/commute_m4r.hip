// commute_m4r.hip — termwise commutation as a GF(2) matrix product by the Method of Four Russians, tables in LDS: preparation of the right
// operand and expansion of bit-packed output.  The kernel itself is commute_m4r7.hip, the choice of kernel and tile plan_commutes (commute_driver.hip).
// (reference: symmer/operators/base.py:938-971 -> matmul_GF2 / numba_dot_matmal_GF2, utils.py:9-78: f64 dgemm, then % 2)
//
//   C = NOT( A . Omega . B^T  mod 2 ),  A: N x 2n bits, B: M x 2n bits       (True = commute)
//
// The register-tile kernel of commute.hip spends 4 VALU instructions per pair and 64-bit word (256 lane-ops per pair at n = 2000) and is
// VALU-issue bound.  Here the contraction axis is cut into groups of bits; for a group and a tile of 2048 columns a workgroup tabulates all
// XOR-combinations of the group's bit-rows of the (bit-transposed, X/Z-swapped) right operand in LDS, and a row of A then needs ONE
// ds_read_b128 per lane and group (a wave instruction serves 4 rows x 2048 columns) — 1/13 of the VALU work per pair.
// Rounds 2-4 used one 256-entry table (8 bits, 64 KiB) per step: 40.1 ms for the 200,000^2 adjacency matrix of cfg5, its look-up stream
// VALU bound at 5 instructions per read.  Round 5 (commute_m4r7.hip): two 128-entry tables per step folded with v_bitop3, 36.1 ms; round 6:
// persistent workgroups over the (tile, step) space, 31.2 ms.
//
//   BT[c][jw]   bit c of B rows 64jw..64jw+63 (bit-major copy, cached on the operator); row c of the contraction pairs A bit c with B bit
//               c +- 64Wq (x with z', z with x'), which is just a row offset into BT.
#include "commute_common.h"

namespace symgpu {

// bit-major copy of B: BT[c][jw], c = 64*sw + bit.  One wave transposes eight 64 x 64 bit blocks of one source word and
// writes 64 contiguous bytes per bit-row.
__global__ __launch_bounds__(256) void k_m4r_bt(const u64 *__restrict__ rows, i64 M, int W, u64 *__restrict__ BT, i64 Mw_pad) {
    const int lane = threadIdx.x & 63;
    const i64 group = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);       // group of 8 column words
    const int sw = blockIdx.y;
    if (group * 8 >= Mw_pad) return;
    u64 mine[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const i64 t = (group * 8 + g) * 64 + lane;
        const u64 word = (t < M) ? rows[t * W + sw] : 0ULL;
        u64 m = 0;
        for (int b = 0; b < 64; ++b) {
            const u64 bal = __ballot((word >> b) & 1ULL);
            if (lane == b) m = bal;
        }
        mine[g] = m;
    }
    u64 *dst = BT + ((i64)64 * sw + lane) * Mw_pad + group * 8;
#pragma unroll
    for (int g = 0; g < 8; ++g) dst[g] = mine[g];
}

// bit-packed rows -> np.bool_ bytes for ANY row length and base alignment: the output [N][M] is treated as one flat run of N * M bytes and
// written in aligned 16-byte chunks (non-temporal), a chunk taking its 16 bits from one row or — across a row boundary — from two or
// more.  (Rounds 2-5 wrote rows whose length is not a multiple of 16 byte by byte: 13 ms for a 100,008^2 table against 2.6 ms for
// 100,000^2 — and 15 of 16 term counts are not multiples of 16.)  A block owns a contiguous span; row and column of its first byte
// come from one 64-bit division, the chunks inside from 32-bit ones.
constexpr int B2B_CHUNKS_PER_THREAD = 8;
__device__ __forceinline__ u32 b2b_bits16(const u64 *__restrict__ row, i64 j) {          // bits [j, j + 16) of a bit-packed row
    const i64 w = j >> 6;
    const int sh = (int)(j & 63);
    u64 v = row[w] >> sh;
    if (sh > 48) v |= row[w + 1] << (64 - sh);
    return (u32)v & 0xFFFFu;
}
__global__ __launch_bounds__(256) void k_bits_to_bytes_flat(const u64 *__restrict__ bits, i64 stride_words, i64 N, i64 M, uint8_t *__restrict__ out) {
    const i64 total = N * M;
    const i64 head = (i64)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) < total ? (i64)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) : total;
    const i64 n_chunks = (total - head) >> 4;
    const i64 span = (i64)256 * B2B_CHUNKS_PER_THREAD;                 // chunks per block
    const i64 c_block = (i64)blockIdx.x * span;
    auto bit_at = [&](i64 f) -> u32 { const i64 i = f / M, j = f - i * M; return (u32)(bits[i * stride_words + (j >> 6)] >> (j & 63)) & 1u; };
    if (blockIdx.x == 0) {                                             // the unaligned head and tail: a few bytes, one at a time
        for (i64 f = threadIdx.x; f < head; f += 256) out[f] = (uint8_t)bit_at(f);
        for (i64 f = head + (n_chunks << 4) + threadIdx.x; f < total; f += 256) out[f] = (uint8_t)bit_at(f);
    }
    if (c_block >= n_chunks) return;
    const i64 f_block = head + (c_block << 4);
    const i64 i_block = f_block / M, j_block = f_block - i_block * M;  // uniform
    u32x4 *dst = reinterpret_cast<u32x4 *>(out + head) + c_block;
#pragma unroll
    for (int k = 0; k < B2B_CHUNKS_PER_THREAD; ++k) {
        const i64 c = (i64)k * 256 + threadIdx.x;                      // chunk inside the span: consecutive lanes, consecutive chunks
        if (c_block + c >= n_chunks) break;
        const i64 d = j_block + (c << 4);                              // column of the chunk's first byte, counted from row i_block
        i64 i, j;
        if (d < ((i64)1 << 31) && M < ((i64)1 << 31)) { const u32 q = (u32)d / (u32)M; i = i_block + q; j = d - (i64)q * M; }
        else { const i64 q = d / M; i = i_block + q; j = d - q * M; }
        u32 b16;
        if (j + 16 <= M) {
            b16 = b2b_bits16(bits + i * stride_words, j);
        } else {                                                       // the chunk runs over the end of row i (rows shorter than 16: of several rows)
            b16 = 0;
            i64 ii = i, jj = j;
            for (int t = 0; t < 16; ++t) {
                if (ii < N) b16 |= ((u32)(bits[ii * stride_words + (jj >> 6)] >> (jj & 63)) & 1u) << t;
                if (++jj == M) { jj = 0; ++ii; }
            }
        }
        __builtin_nontemporal_store(bits16_to_bytes(b16), dst + c);
    }
}

int bits_to_bytes_dev(const u64 *bits, i64 stride_words, i64 N, i64 M, uint8_t *out) {
    if (N <= 0 || M <= 0) return SYMGPU_OK;
    const i64 n_chunks = (N * M) / 16 + 1;
    const i64 span = (i64)256 * B2B_CHUNKS_PER_THREAD;
    const i64 g = (n_chunks + span - 1) / span;
    SG_REQUIRE(g < ((i64)1 << 31), "bits_to_bytes: table too large for one launch");
    hipLaunchKernelGGL(k_bits_to_bytes_flat, dim3((unsigned)g), dim3(256), 0, ctx().stream, bits, stride_words, N, M, out);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

// the bit-major copy of B is cached on its operator (an adjacency matrix computed slab by slab transposes B once)
int m4r_bit_major(const CommutePlan &pl, const u64 *B, i64 M, int W, symgpu_op_s *b_owner, Scratch &scratch, const u64 **bt) {
    symgpu_op_s *const cache = (b_owner && b_owner->rows == B && b_owner->T == M) ? b_owner : nullptr;
    u64 *build = nullptr;                                              // where a copy has to be built; null: the cached one is valid
    if (!cache) {
        SG_TRY(scratch.alloc(pl.bt_bytes));
        build = scratch.as<u64>();
    } else if (!cache->bt || cache->bt_T != M || cache->bt_pad != pl.Mw_pad) {
        if (cache->bt) { dev_free(cache->bt); cache->bt = nullptr; }
        SG_TRY(dev_alloc(pl.bt_bytes, (void **)&cache->bt));
        build = cache->bt;
    }
    if (build) {
        hipLaunchKernelGGL(k_m4r_bt, dim3((unsigned)((pl.Mw_pad / 8 + 3) / 4), (unsigned)W), dim3(256), 0, ctx().stream, B, M, W, build, pl.Mw_pad);
        KERNEL_CHECK();
        if (cache) { cache->bt_pad = pl.Mw_pad; cache->bt_T = M; bump_counter(SYMGPU_CTR_OP_BIT_MAJOR_BUILDS); }
    }
    *bt = cache ? cache->bt : scratch.as<u64>();
    return SYMGPU_OK;
}

}  // namespace symgpu
