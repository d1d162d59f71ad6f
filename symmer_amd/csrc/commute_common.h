// commute_common.h — what the files of the termwise commutation share; private to them:
//   commute_driver.hip   switches, plan, one stage per path, commutes_dev, symgpu_commutes / symgpu_commutes_dev / symgpu_commutes_bits_dev
//   commute.hip          the register-tile kernel k_commutes and its launch wrapper
//   commute_m4r.hip      Four Russians: the bit-major copy of the right operand (k_m4r_bt) and the byte expansion (k_bits_to_bytes_flat)
//   commute_m4r7.hip     Four Russians: k_m7_a7, k_m7_klist, k_commutes_m4r7s, k_m7_fixup and their launch wrapper
// The wide-row path is wide.hip (wide_commutes_dev, wide_pairs_worthwhile: common.h — the product and the cleanup use them too).
#pragma once
#include "common.h"

namespace symgpu {

constexpr int M7_TILE_W = 32;             // Four Russians: 64-bit words per column tile, 2048 columns
constexpr int M7_WAVES = 8;               // ... waves per workgroup; a wave holds 4 slots of R rows: 32 R rows per tile
constexpr int RT_BLOCK_ROWS = 32;         // register tile: rows of A / columns of B per workgroup (commute.hip: CI * WAVES, 64 * DJ)
constexpr int RT_BLOCK_COLS = 512;

// Every switch of the commutation ("Environment switches"), read once at the top of a call — on every call, the tests flip them
// between calls of one process.  Each forces a path the library also takes by itself.
struct CommuteSwitches {
    bool wide_worthwhile = false;         // SYMGPU_WIDE and the size rule, as wide_pairs_worthwhile (wide.hip) answers them for this call's shape
    int force_m4r = -1;                   // SYMGPU_COMMUTE_M4R=1 / 0: the Four-Russians kernel / never it; -1: the measured threshold
    int force_R = 0;                      // SYMGPU_M4R_R=16 / 24 / 48: the tile height; 0: the measured rule
    bool unfused = false;                 // SYMGPU_M4R_UNFUSED (set): bytes through bit-packed scratch rows + k_bits_to_bytes_flat
    int stream = -1;                      // SYMGPU_M4R_STREAM=0 / non-zero: one tile per workgroup / stream-K where it is possible; -1: the measured rule
    bool force_fixup = false;             // SYMGPU_M4R_FIXUP (set): every split tile of a stream-K launch goes to k_m7_fixup
};

enum class CommutePath {
    FourRussians,                         // LDS tables: 1/13 of the VALU work per pair, a fixed price per workgroup (commute_m4r.hip, commute_m4r7.hip)
    WideRows,                             // few pairs of very long rows: the word axis is the parallel one (wide.hip)
    RegisterTile,                         // everything else (commute.hip)
};

// What a call decides before it launches anything (plan_commutes, commute_driver.hip).  Only the fields of the chosen path are set.
struct CommutePlan {
    CommutePath path;
    i64 Npad;                             // rows of the left operand's padded copy: register tile — the word-major copy; Four Russians — A7
    // ---- register tile
    i64 Mpad;                             // columns of the word-major copy of B
    bool shared_copy;                     // adjacency (B is A): one word-major copy serves both sides
    i64 gx, gy_total;                     // workgroups along i / along j (launched in batches of at most 65535)
    // ---- Four Russians
    int R;                                // rows per 16-lane slot: 16, 24 or 48
    int num_cu;                           // workgroups of a stream-K launch
    i64 Mw, Mw_pad;                       // 64-bit words of a bit-packed result row / padded to whole column tiles
    int ng7, max_pairs;                   // 7-bit groups of a packed row / steps of a tile at most (pairs of groups)
    i64 n_rt, n_tiles;                    // row tiles / tiles
    bool fused_bytes;                     // np.bool_ output from the kernel's own epilogue
    bool stream;                          // stream-K launch (else one tile per workgroup)
    bool force_fixup;
    size_t bt_bytes, a7_bytes, flag_bytes, klist_bytes, steptab_bytes, part_bytes, bits_bytes;   // scratch (part: stream-K only; bits: unfused bytes only)
    i64 tile_rows() const { return (i64)4 * M7_WAVES * R; }
};

static inline i64 round_up(i64 x, i64 m) { return (x + m - 1) / m * m; }

// 16 result bits -> 16 np.bool_ bytes (bit k -> byte k)
__device__ __forceinline__ u32x4 bits16_to_bytes(u32 b16) {
    u32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32 x = (b16 >> (4 * q)) & 0xFu;
        v[q] = (x | (x << 7) | (x << 14) | (x << 21)) & 0x01010101u;
    }
    return v;
}

// The launch wrappers (SG_HIDDEN: private to these files, kept out of the library's dynamic symbols).
// commute.hip: At / Bt = word-major copies padded to pl.Npad / pl.Mpad terms; exactly one of out / out_bits is non-null
SG_HIDDEN int launch_register_tile(const CommutePlan &pl, const u64 *At, i64 N, const u64 *Bt, i64 M, int Wq, uint8_t *out, u64 *out_bits);

// commute_m4r.hip
// *bt = the bit-major copy of B (pl.Mw_pad words per bit-row): the one cached on b_owner when B is all of that operator's rows (built
// on the first call), else built into `scratch`
SG_HIDDEN int m4r_bit_major(const CommutePlan &pl, const u64 *B, i64 M, int W, symgpu_op_s *b_owner, Scratch &scratch, const u64 **bt);
SG_HIDDEN int bits_to_bytes_dev(const u64 *bits, i64 stride_words, i64 N, i64 M, uint8_t *out);   // bit-packed rows -> np.bool_ [N][M], any M, any alignment

// commute_m4r7.hip: the left operand's layouts (A7, klist, step table), the kernel the plan names and, after a stream-K launch, the fix-up.
// dst / stride: pl.fused_bytes — np.bool_ [N][stride]; else bit-packed rows of `stride` words
SG_HIDDEN int launch_four_russians(const CommutePlan &pl, const u64 *A, i64 N, i64 M, int Wq, const u64 *bt, void *dst, i64 stride);

}  // namespace symgpu
