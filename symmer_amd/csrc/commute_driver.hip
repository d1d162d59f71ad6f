// commute_driver.hip — termwise commutation / adjacency (reference: symmer/operators/base.py:938-971 via matmul_GF2, utils.py:9-78) and
// its C entry points: reads the switches, plans a call and runs it as one stage.  The kernels and their launch wrappers are in commute.hip
// (register tile), commute_m4r.hip / commute_m4r7.hip (Four Russians) and wide.hip (wide rows); commute_common.h lists the files.
#include "commute_common.h"
#include <stdlib.h>

namespace symgpu {

// wide_pairs_worthwhile (wide.hip) reads SYMGPU_WIDE, for the product and the cleanup as well; its answer for this call's shape travels with the switches
static CommuteSwitches read_commute_switches(i64 N, i64 M, int Wq) {
    CommuteSwitches sw;
    sw.wide_worthwhile = wide_pairs_worthwhile(N, M, Wq);
    const char *e = nullptr;
    if ((e = getenv("SYMGPU_COMMUTE_M4R"))) sw.force_m4r = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1);
    if ((e = getenv("SYMGPU_M4R_R"))) {
        const int r = atoi(e);
        if (r == 16 || r == 24 || r == 48) sw.force_R = r;
    }
    sw.unfused = getenv("SYMGPU_M4R_UNFUSED") != nullptr;
    if ((e = getenv("SYMGPU_M4R_STREAM"))) sw.stream = atoi(e) != 0;
    sw.force_fixup = getenv("SYMGPU_M4R_FIXUP") != nullptr;
    return sw;
}

// ---- thresholds of the Four-Russians path ----------------------------------------------------------------------------------
constexpr int M7_STREAM_MIN_WORK = 125;                // tile-steps per persistent workgroup from which it pays
constexpr int M7_STREAM_MIN_STEPS = 32;                // steps a tile (pairs of 7-bit groups of the padded row: 28 at n <= 192, 37 above) from which the stream-K launch pays

static i64 m4r_workgroups(i64 N, i64 M, int R) {
    const i64 Mw = (M + 63) / 64;
    return ((N + 32 * R - 1) / (32 * R)) * ((Mw + M7_TILE_W - 1) / M7_TILE_W);
}
// Which kernel: the Four-Russians kernel does 1/13 of the VALU work per pair but pays a fixed price per workgroup (operand transposes,
// 64 KiB of tables per step shared by >= 512 rows), so it needs enough rows and columns to fill the chip with its 512..1536 x 2048 tiles; the
// register-tile kernel serves everything smaller.  The threshold asks for enough 512 x 2048 tiles to occupy most of the chip (below that
// the register-tile kernel wins: 1024 x 16384 at n = 2000 takes 0.10 ms there and 0.6 ms here; 4096 x 65536: 1.03 ms against 0.66 ms) and
// for tiles that are at least half full in both directions: a 512 x 2048 tile costs the same whether it holds 1 row or 512 (100,000 x 1
// at n = 1000: 0.14 ms on the register-tile kernel, 0.34 ms here).
static bool m4r_worthwhile(i64 N, i64 M, int num_cu) { return N >= 256 && M >= 1024 && m4r_workgroups(N, M, 16) >= (3 * num_cu) / 4; }
// tile heights: R rows per 16-lane slot -> 32 R rows per workgroup.  Taller tiles amortise the tables over more rows (round 5, 200,000^2
// terms at n = 2000: R = 16 / 24 / 48 -> 60.0 / 50.8 / 36.1 ms), but a workgroup finishes a tile with a store phase no other work on its CU
// hides, so a launch wants several tiles per CU for the stores of one workgroup to fall under the lookups of the others — the more, the
// shorter the tile's lookup phase is.  Measured (round 6, profiles/r06_m4r_pick.txt, n in 20..2000 x N in 20,000..100,000): the tallest
// height with  tiles x steps-per-tile >= 200 x CUs  is within 5 % of the best of the three everywhere; below 32 steps (n <= 192: rows of at
// most three words a half) the table is bound by its own bytes and R = 16 is never beaten.  SYMGPU_M4R_R forces one (tests).
static int m4r_pick(i64 N, i64 M, i64 steps, int forced, int num_cu) {
    if (forced) return forced;
    if (steps < 32) return 16;
    const int cand[2] = {48, 24};
    for (int R : cand)
        if (m4r_workgroups(N, M, R) * steps >= (i64)200 * num_cu) return R;
    return 16;
}

// Pure host code: no HIP call, no context, no environment.  SYMGPU_COMMUTE_M4R=1 / 0 comes first (the tests run both kernels on every
// case; forcing Four Russians beats the wide path), then the measured threshold, and only a call that Four Russians does not take goes to
// the wide-row kernel where that is worthwhile (sw.wide_worthwhile: wide_pairs_worthwhile's answer for this shape).
static CommutePlan plan_commutes(i64 N, i64 M, int Wq, bool same_operand, bool wants_bytes, const CommuteSwitches &sw, int num_cu) {
    CommutePlan pl{};
    if (sw.force_m4r >= 0 ? sw.force_m4r == 1 : m4r_worthwhile(N, M, num_cu)) pl.path = CommutePath::FourRussians;
    else if (sw.wide_worthwhile) pl.path = CommutePath::WideRows;                   // few pairs of very long rows
    else pl.path = CommutePath::RegisterTile;

    if (pl.path == CommutePath::RegisterTile) {
        pl.shared_copy = same_operand;                 // adjacency: one word-major copy serves both sides
        pl.Mpad = round_up(M, RT_BLOCK_COLS);
        pl.Npad = same_operand ? pl.Mpad : round_up(N, RT_BLOCK_ROWS);
        pl.gx = pl.Npad / RT_BLOCK_ROWS;
        pl.gy_total = pl.Mpad / RT_BLOCK_COLS;
    } else if (pl.path == CommutePath::FourRussians) {
        pl.num_cu = num_cu;
        pl.ng7 = (128 * Wq + 6) / 7;
        pl.max_pairs = (pl.ng7 + 1) / 2;
        pl.R = m4r_pick(N, M, pl.max_pairs, sw.force_R, num_cu);
        pl.Mw = (M + 63) / 64;
        pl.Mw_pad = round_up(pl.Mw, M7_TILE_W);
        pl.Npad = round_up(N, pl.tile_rows());         // multiples of 256
        pl.n_rt = pl.Npad / pl.tile_rows();
        pl.n_tiles = pl.n_rt * (pl.Mw_pad / M7_TILE_W);
        // np.bool_ output: expanded by the kernel's own epilogue, rows of any length at any base (unaligned 16-byte stores where they have to be).
        // SYMGPU_M4R_UNFUSED=1: bit-packed rows to scratch + the flat expansion kernel (a second pass: 2.8 against 2.3 ms at 100,000^2 terms of 20
        // qubits, but 0.30 against 0.36 ms at 30,000^2) — kept as the tested alternative.
        pl.fused_bytes = wants_bytes && !sw.unfused;
        // one tile per workgroup where the persistent launch's published parts only cost: short operators (below M7_STREAM_MIN_STEPS steps a
        // tile the table is bound by its own bytes — 30,000^2 terms of 20 / 100 / 150 qubits, R = 16: 0.339 / 0.370 / 0.372 ms streamed against
        // 0.284 / 0.307 / 0.339 ms tile by tile), launches of little work (20,000^2 terms of 200 / 300 / 400 qubits: 0.220 / 0.238 / 0.259 against
        // 0.189 / 0.219 / 0.254 ms; the streamed launch wins from about 125 tile-steps per workgroup) and fewer tiles than compute units
        // (profiles/r06_m4r_pick.txt).  Runtime switches ("Environment switches"): both force a path the kernel takes by itself —
        // SYMGPU_M4R_STREAM=1 still needs a tile per compute unit, =0 always wins.
        const bool enough_tiles = pl.n_tiles >= num_cu;
        pl.stream = enough_tiles && (sw.stream >= 0 ? sw.stream == 1
                                                    : pl.max_pairs >= M7_STREAM_MIN_STEPS && pl.n_tiles * pl.max_pairs >= (i64)M7_STREAM_MIN_WORK * num_cu);
        pl.force_fixup = sw.force_fixup;
        pl.bt_bytes = (size_t)64 * 2 * Wq * pl.Mw_pad * 8;
        pl.a7_bytes = (size_t)(pl.ng7 + 1) * pl.Npad;
        pl.flag_bytes = ((size_t)(pl.ng7 + 1) * 4 + 255) / 256 * 256;   // (a whole number of 256-byte pieces: one fill kernel, not a body and a tail)
        pl.klist_bytes = (size_t)(pl.ng7 + 2) * 4;
        pl.steptab_bytes = (size_t)(pl.max_pairs + 2) * 16 * 8;
        pl.part_bytes = pl.stream ? (size_t)num_cu * 2 * pl.tile_rows() * M7_TILE_W * 8 : 0;
        pl.bits_bytes = wants_bytes && !pl.fused_bytes ? (size_t)N * pl.Mw * 8 : 0;
    }
    return pl;
}

// ---- stages: A: N rows, B: M rows, row-major packed device pointers; exactly one of out / out_bits is non-null ---------------------
// which kernel served the call is counted here: register tile, wide rows, Four Russians (by launch)
static int run_register_tile(const CommutePlan &pl, const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits) {
    bump_counter(SYMGPU_CTR_COMMUTE_REGISTER_TILE);
    const int W = 2 * Wq;
    Scratch at, bt;
    SG_TRY(at.alloc((size_t)pl.Npad * W * sizeof(u64)));
    SG_TRY(to_wordmajor(A, N, W, at.as<u64>(), pl.Npad));
    if (!pl.shared_copy) {
        SG_TRY(bt.alloc((size_t)pl.Mpad * W * sizeof(u64)));
        SG_TRY(to_wordmajor(B, M, W, bt.as<u64>(), pl.Mpad));
    }
    return launch_register_tile(pl, at.as<u64>(), N, pl.shared_copy ? at.as<u64>() : bt.as<u64>(), M, Wq, out, out_bits);
}

static int run_wide_rows(const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits) {
    bump_counter(SYMGPU_CTR_COMMUTE_WIDE_ROWS);
    return wide_commutes_dev(A, N, B, M, Wq, out, out_bits);
}

static int run_four_russians(const CommutePlan &pl, const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits, symgpu_op_s *b_owner) {
    if (pl.stream) bump_counter(SYMGPU_CTR_COMMUTE_M4R_STREAMK);
    else bump_counter(SYMGPU_CTR_COMMUTE_M4R_TILE);
    Scratch bt_scratch, bits;
    const u64 *bt = nullptr;
    SG_TRY(m4r_bit_major(pl, B, M, 2 * Wq, b_owner, bt_scratch, &bt));
    if (pl.fused_bytes) return launch_four_russians(pl, A, N, M, Wq, bt, out, M);
    const bool expand = out != nullptr;                                // bytes wanted, not fused: bit-packed rows to scratch, then the flat expansion
    if (expand) SG_TRY(bits.alloc(pl.bits_bytes));
    SG_TRY(launch_four_russians(pl, A, N, M, Wq, bt, expand ? bits.p : out_bits, pl.Mw));
    return expand ? bits_to_bytes_dev(bits.as<u64>(), pl.Mw, N, M, out) : SYMGPU_OK;
}

int commutes_dev(const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits, symgpu_op_s *b_owner) {
    int rc = SYMGPU_OK;
    if (N != 0 && M != 0) {
        const CommuteSwitches sw = read_commute_switches(N, M, Wq);
        const CommutePlan pl = plan_commutes(N, M, Wq, B == A && M == N, out != nullptr, sw, ctx().num_cu);
        switch (pl.path) {
            case CommutePath::FourRussians: rc = run_four_russians(pl, A, N, B, M, Wq, out, out_bits, b_owner); break;
            case CommutePath::WideRows: rc = run_wide_rows(A, N, B, M, Wq, out, out_bits); break;
            case CommutePath::RegisterTile: rc = run_register_tile(pl, A, N, B, M, Wq, out, out_bits); break;
        }
    }
    return rc;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_commutes_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint8_t *out_dev) {
    SG_ENTER(A, B);
    SG_REQUIRE(A && B && A->Wq == B->Wq, "commutes_dev: operands must share Wq");
    SG_REQUIRE(0 <= a_begin && a_begin <= a_end && a_end <= A->T, "commutes_dev: bad row range");
    SG_REQUIRE(out_dev || a_end == a_begin || B->T == 0, "commutes_dev: null output");
    return commutes_dev(A->rows + a_begin * 2 * A->Wq, a_end - a_begin, B->rows, B->T, A->Wq, out_dev, nullptr, B);
}

int symgpu_commutes_bits_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint64_t *out_bits_dev) {
    SG_ENTER(A, B);
    SG_REQUIRE(A && B && A->Wq == B->Wq, "commutes_bits_dev: operands must share Wq");
    SG_REQUIRE(0 <= a_begin && a_begin <= a_end && a_end <= A->T, "commutes_bits_dev: bad row range");
    SG_REQUIRE(out_bits_dev || a_end == a_begin || B->T == 0, "commutes_bits_dev: null output");
    return commutes_dev(A->rows + a_begin * 2 * A->Wq, a_end - a_begin, B->rows, B->T, A->Wq, nullptr, out_bits_dev, B);
}

int symgpu_commutes(const uint64_t *A, int64_t N, const uint64_t *B, int64_t M, int Wq, uint8_t *out) {
    SG_ENTER();
    SG_REQUIRE(N >= 0 && M >= 0 && Wq >= 1, "commutes: sizes");
    if (N == 0 || M == 0) return SYMGPU_OK;
    SG_REQUIRE(A && B && out, "commutes: null pointer");
    const size_t rb = (size_t)2 * Wq * sizeof(u64);
    Scratch da, db, dout;
    SG_TRY(da.alloc((size_t)N * rb));
    HIP_TRY(hipMemcpyAsync(da.p, A, (size_t)N * rb, hipMemcpyHostToDevice, ctx().stream));
    count_h2d((size_t)N * rb); count_d2h((size_t)N * (size_t)M);
    const u64 *pb = da.as<u64>();
    if (!(B == A && M == N)) {
        SG_TRY(db.alloc((size_t)M * rb));
        HIP_TRY(hipMemcpyAsync(db.p, B, (size_t)M * rb, hipMemcpyHostToDevice, ctx().stream));
        count_h2d((size_t)M * rb);
        pb = db.as<u64>();
    }
    SG_TRY(dout.alloc((size_t)N * (size_t)M));
    SG_TRY(commutes_dev(da.as<u64>(), N, pb, M, Wq, dout.as<uint8_t>(), nullptr));
    prefault_host(out, (size_t)N * (size_t)M);
    HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)N * (size_t)M, hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

}  // extern "C"
