// gf2_driver.hip — in-place GF(2) row reduction of a device matrix (rref_dev) and its C entry points: reads the switches, plans a call and
// runs it as stages.  The kernels, their launch wrappers and the description of the blocked form are in gf2.hip; gf2_common.h lists the files.
#include "gf2_common.h"
#include <stdlib.h>
#include <stdio.h>

namespace symgpu {

// Every switch of the elimination, read once at the top of a call: the tests flip them between calls of one process.
struct Gf2Switches {
    bool small = true;               // SYMGPU_GF2_SMALL=0: small matrices through the blocked schedule
    bool m4r = true;                 // SYMGPU_GF2_M4R=0: flag-per-block-row sweep (what a refused LDS attribute leaves)
    bool fused_select = true;        // SYMGPU_GF2_FUSED_SELECT=0: the selector launch on its own in front of phase 0 (three launches per block)
    bool inject_time_out = false;    // SYMGPU_GF2_FUSED_SELECT=2 (tests): the fused attempt is treated as timed out
    // tuning knobs (SG_TUNE: compiled out of the default build)
    bool lookahead = true;           // SYMGPU_GF2_LOOKAHEAD=0: lead -> panel -> select -> sweep, one block after the other
    bool full_panel = true;          // SYMGPU_GF2_FULL_PANEL=0: never panel on the full rows in LDS
    bool lean_panel = true;          // SYMGPU_GF2_LEAN_PANEL=0: two-word windows run the generic loop
    bool debug = false;              // SYMGPU_GF2_DEBUG (set): one line per blocked reduction on stderr
};

static Gf2Switches read_gf2_switches() {
    Gf2Switches sw;
    const char *e = nullptr;
    if ((e = getenv("SYMGPU_GF2_SMALL"))) sw.small = e[0] != '0';
    if ((e = getenv("SYMGPU_GF2_M4R"))) sw.m4r = e[0] != '0';
    if ((e = getenv("SYMGPU_GF2_FUSED_SELECT"))) { sw.fused_select = e[0] != '0'; sw.inject_time_out = e[0] == '2'; }
    if ((e = SG_TUNE("SYMGPU_GF2_LOOKAHEAD"))) sw.lookahead = e[0] != '0';
    if ((e = SG_TUNE("SYMGPU_GF2_FULL_PANEL"))) sw.full_panel = e[0] != '0';
    if ((e = SG_TUNE("SYMGPU_GF2_LEAN_PANEL"))) sw.lean_panel = e[0] != '0';
    sw.debug = SG_TUNE("SYMGPU_GF2_DEBUG") != nullptr;
    return sw;
}

static bool g_gf2_fused_off = false;         // a launch-A wait timed out once: the process keeps to the separate-launch schedule

// What a call decides before it launches anything.
enum class Gf2Path { Small, Blocked };       // the whole reduction in one workgroup / 64-row blocks
enum class Gf2Schedule {                     // of the blocked path
    LookaheadFused,                          // two launches per block: selectors + rows of the next block in one grid, panel inside the main sweep
    LookaheadSeparate,                       // three: the selector launch on its own (what a time-out of the fused form falls back to)
    PlainM4r,                                // no lookahead: lead -> panel -> select -> Four-Russians sweep
    PlainFlags,                              // ... -> flag-per-block-row sweep
};
struct Gf2Plan {
    Gf2Path path;
    Gf2Schedule schedule;
    int m4_tiles, m4_chunks;
    bool full_panel, lean_panel;
    // The fused schedule waits inside a launch for flags of other workgroups (bounded, ~1 s).  Should that wait ever give up, the matrix is half
    // updated in place — so a copy of the input is kept (2 x 27 MB at 5 TB/s = 11 us of a 2 ms call at cfg4) and the reduction is redone from it.
    bool safety_copy() const { return path == Gf2Path::Blocked && schedule == Gf2Schedule::LookaheadFused; }
};

static Gf2Plan plan_rref(i64 R, i64 Wc, const Gf2Switches &sw) {
    Gf2Plan pl{};
    pl.full_panel = sw.full_panel;
    pl.lean_panel = sw.lean_panel;
    const bool small_attr = gf2_small_attr_ok();
    pl.path = (R <= SMALL_R && Wc <= SMALL_WC && small_attr && sw.small) ? Gf2Path::Small : Gf2Path::Blocked;
    if (pl.path == Gf2Path::Small) return pl;
    // Four-Russians sweep (128 KiB of LDS per workgroup) unless disabled or refused by the runtime
    const bool m4r = gf2_m4r_attr_ok() && sw.m4r;
    pl.m4_tiles = (int)((Wc + M4_TW - 1) / M4_TW);
    pl.m4_chunks = 256 / pl.m4_tiles;                            // one workgroup per CU: about one round of workgroups
    if ((i64)pl.m4_chunks > (R + 127) / 128) pl.m4_chunks = (int)((R + 127) / 128);   // the table costs about 100 rows of work
    if (pl.m4_chunks < 1) pl.m4_chunks = 1;
    if (sw.lookahead && m4r && (i64)pl.m4_tiles * pl.m4_chunks + 1 < ((i64)1 << 31))
        pl.schedule = sw.fused_select && !g_gf2_fused_off ? Gf2Schedule::LookaheadFused : Gf2Schedule::LookaheadSeparate;
    else
        pl.schedule = m4r ? Gf2Schedule::PlainM4r : Gf2Schedule::PlainFlags;
    return pl;
}

// ---- stages ------------------------------------------------------------------------------------------------------------
// one-workgroup path: its own two buffers, one launch, one wait
static int run_small(u64 *rows, i64 R, i64 Wc, i64 *xor_count, i64 *pivots_host) {
    hipStream_t st = ctx().stream;
    Scratch piv, count;
    SG_TRY(piv.alloc((size_t)R * 8));
    SG_TRY(count.alloc(16));
    HIP_TRY(hipMemsetAsync(count.p, 0, 16, st));
    SG_TRY(launch_rref_small(rows, R, Wc, piv.as<i64>(), count.as<unsigned long long>()));
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, count.p, 8, hipMemcpyDeviceToHost, st));
    if (pivots_host) HIP_TRY(hipMemcpyAsync(pivots_host, piv.p, (size_t)R * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (xor_count) *xor_count = (i64)h;
    return SYMGPU_OK;
}

static int alloc_run(Gf2Run &g) {
    hipStream_t st = ctx().stream;
    const i64 R = g.R, Wc = g.Wc;
    SG_TRY(g.info.alloc(2 * sizeof(BlockInfo)));
    SG_TRY(g.state.alloc(sizeof(SweepState)));
    SG_TRY(g.lead.alloc(WK * sizeof(int)));
    SG_TRY(g.sel.alloc((size_t)R * 8));
    SG_TRY(g.snap.alloc((size_t)WK * Wc * 8));
    SG_TRY(g.counters.alloc(sizeof(Gf2Counters)));
    SG_TRY(g.piv.alloc((size_t)R * 8));
    SG_TRY(g.rowcnt.alloc((size_t)R * 4));
    HIP_TRY(hipMemsetAsync(g.rowcnt.p, 0, (size_t)R * 4, st));
    HIP_TRY(hipMemsetAsync(g.counters.p, 0, sizeof(Gf2Counters), st));
    SG_TRY(g.ready.alloc(2 * WK * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(g.ready.p, 0, 2 * WK * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(g.state.p, 0, sizeof(SweepState), st));
    HIP_TRY(hipMemsetAsync(g.info.p, 0, 2 * sizeof(BlockInfo), st));   // {i0 = 0, kk = 0}: "nothing swept yet, next block starts at row 0"
    return SYMGPU_OK;
}

// progress read-back: the first 64-bit word at `dev` (BlockInfo::i0, SweepState::next_i0) and, if asked for, the int behind it (BlockInfo::kk)
static int read_progress(const void *dev, i64 *row, int *kk = nullptr) {
    u32 w[3] = {0, 0, 0};
    SG_TRY(read_back_words(static_cast<const u32 *>(dev), kk ? 3 : 2, nullptr, 0, w));
    *row = (i64)(((u64)w[1] << 32) | w[0]);
    if (kk) *kk = (int)w[2];
    return SYMGPU_OK;
}

// Pipeline, two or three launches per block: select(b) -> phase 0: sweep of the rows of block b+1 + their leading words -> phase 1: panel of
// block b+1 (-> the other info buffer) inside the sweep of all remaining rows.  The very first iteration has nothing to sweep (zeroed info): it
// only collects the leading words of rows 0..63 and panels block 0.  `it` keeps counting across batches.
static int run_lookahead(const Gf2Run &g, bool fused) {
    launch_fill_nolead(g);
    i64 it = 0, done = 0, prev = -1;
    for (bool finished = false; !finished;) {
        i64 n_iter = (g.R - done + WK - 1) / WK + 1;
        if (n_iter > 4096) n_iter = 4096;
        for (i64 k = 0; k < n_iter; ++k, ++it) SG_TRY(launch_lookahead_step(g, it, fused));
        // the block that has been panelled but not swept yet: kk == 0 means the matrix is exhausted
        i64 i0 = 0;
        int kk = 0;
        SG_TRY(read_progress(g.info.as<BlockInfo>() + ((it + 1) & 1), &i0, &kk));
        if (kk == 0) finished = true;
        else if (i0 <= prev) { set_error("rref: no progress (internal error)"); return SYMGPU_E_INVALID; }
        prev = done = i0;
    }
    return SYMGPU_OK;
}

static int run_plain(const Gf2Run &g, bool m4r) {
    i64 done = 0;
    while (done < g.R) {
        // optimistic batch: every block consumes up to 64 rows; blocks that end early are caught by the read-back
        i64 n_iter = (g.R - done + WK - 1) / WK;
        if (n_iter > 4096) n_iter = 4096;
        for (i64 it = 0; it < n_iter; ++it) SG_TRY(launch_plain_step(g, m4r));
        i64 next_i0 = 0;
        SG_TRY(read_progress(g.state.p, &next_i0));
        if (next_i0 <= done) { set_error("rref: no progress (internal error)"); return SYMGPU_E_INVALID; }
        done = next_i0;
    }
    return SYMGPU_OK;
}

// the counters of the run (and the pivots): *timed_out = a tile workgroup gave up waiting, the matrix is then partly updated
static int read_counters(const Gf2Run &g, const Gf2Switches &sw, i64 *xor_count, i64 *pivots_host, bool *timed_out) {
    hipStream_t st = ctx().stream;
    SG_TRY(launch_row_xor_sum(g));
    Gf2Counters h{};
    static_assert(sizeof(Gf2Counters) == 32 && sizeof(Gf2Counters) % 4 == 0, "read back as words");
    if (pivots_host) {
        HIP_TRY(hipMemcpyAsync(&h, g.counters.p, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(pivots_host, g.piv.p, (size_t)g.R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        SG_TRY(read_back_words(g.counters.as<u32>(), 6, nullptr, 0, reinterpret_cast<u32 *>(&h)));
    }
    // which panel the blocks of this run took (SYMGPU_CTR_GF2_*; a run that is redone after a time-out counts twice)
    bump_counter(SYMGPU_CTR_GF2_BLOCKS_PANELLED, (i64)(u32)h.blocks);
    bump_counter(SYMGPU_CTR_GF2_PANEL_FULL_ROWS, (i64)h.full_panels);
    bump_counter(SYMGPU_CTR_GF2_PANEL_WINDOW, (i64)(u32)(h.blocks >> 32));
    if (sw.debug) fprintf(stderr, "rref %lld x %lld words: full-row panels %u\n", (long long)g.R, (long long)g.Wc, h.full_panels);
    *timed_out = h.timed_out != 0;
    if (!*timed_out && xor_count) *xor_count = (i64)h.xors;
    return SYMGPU_OK;
}

static int run_blocked(u64 *rows, i64 R, i64 Wc, const Gf2Plan &pl, const Gf2Switches &sw, i64 *xor_count, i64 *pivots_host, bool *timed_out) {
    Gf2Run g{rows, R, Wc, pl.m4_tiles, pl.m4_chunks, pl.full_panel ? 1 : 0, pl.lean_panel ? 1 : 0};
    SG_TRY(alloc_run(g));
    switch (pl.schedule) {
        case Gf2Schedule::LookaheadFused: SG_TRY(run_lookahead(g, true)); break;
        case Gf2Schedule::LookaheadSeparate: SG_TRY(run_lookahead(g, false)); break;
        case Gf2Schedule::PlainM4r: SG_TRY(run_plain(g, true)); break;
        case Gf2Schedule::PlainFlags: SG_TRY(run_plain(g, false)); break;
    }
    return read_counters(g, sw, xor_count, pivots_host, timed_out);
}

int rref_dev(u64 *rows, i64 R, i64 Wc, i64 *xor_count, i64 *pivots_host) {
    hipStream_t st = ctx().stream;
    if (xor_count) *xor_count = 0;
    if (R <= 0 || Wc <= 0) return SYMGPU_OK;
    if (Wc >= ((i64)1 << 31) - 64) { set_error("rref: Wc too large"); return SYMGPU_E_INVALID; }
    const Gf2Switches sw = read_gf2_switches();
    Gf2Plan pl = plan_rref(R, Wc, sw);
    if (pl.path == Gf2Path::Small) return run_small(rows, R, Wc, xor_count, pivots_host);
    Scratch orig;
    if (pl.safety_copy()) {
        if (orig.alloc((size_t)R * Wc * 8) != SYMGPU_OK) {
            // no room for the safety copy (a matrix near the memory limit): the separate-launch schedule needs none and has no wait to time out
            orig.p = nullptr;
            set_error("");
            pl.schedule = Gf2Schedule::LookaheadSeparate;
        } else {
            HIP_TRY(hipMemcpyAsync(orig.p, rows, (size_t)R * Wc * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    bool timed_out = false;
    SG_TRY(run_blocked(rows, R, Wc, pl, sw, xor_count, pivots_host, &timed_out));
    if (sw.inject_time_out && pl.safety_copy()) timed_out = true;
    if (!timed_out) return SYMGPU_OK;
    if (!orig.p) { set_error("rref: an in-launch wait timed out on a schedule that has none (internal error)"); return SYMGPU_E_HIP; }
    // restore the matrix and redo it with separate launches; a real time-out keeps the fused form off for the rest of the process
    g_gf2_fused_off = !sw.inject_time_out;
    if (!sw.inject_time_out) note_degraded("GF(2) fused selector launch off: an in-kernel wait timed out (workgroups not co-resident?); the elimination takes three launches per block");
    HIP_TRY(hipMemcpyAsync(rows, orig.p, (size_t)R * Wc * 8, hipMemcpyDeviceToDevice, st));
    if (xor_count) *xor_count = 0;
    pl.schedule = Gf2Schedule::LookaheadSeparate;
    SG_TRY(run_blocked(rows, R, Wc, pl, sw, xor_count, pivots_host, &timed_out));
    if (timed_out) { set_error("rref: time-out on the separate-launch schedule (internal error)"); return SYMGPU_E_HIP; }
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_rref_dev(uint64_t *rows_dev, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots_host) {
    SG_ENTER();
    SG_REQUIRE(R >= 0 && Wc >= 0 && (rows_dev || R * Wc == 0), "rref_dev");
    return rref_dev(rows_dev, R, Wc, xor_count, pivots_host);
}

int symgpu_rref(uint64_t *rows, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots) {
    SG_ENTER();
    SG_REQUIRE(R >= 0 && Wc >= 0 && (rows || R * Wc == 0), "rref");
    if (xor_count) *xor_count = 0;
    if (R == 0 || Wc == 0) {
        if (pivots) for (i64 r = 0; r < R; ++r) pivots[r] = -1;
        return SYMGPU_OK;
    }
    Scratch d;
    SG_TRY(d.alloc((size_t)R * Wc * 8));
    HIP_TRY(hipMemcpyAsync(d.p, rows, (size_t)R * Wc * 8, hipMemcpyHostToDevice, ctx().stream));
    count_h2d((size_t)R * Wc * 8); count_d2h((size_t)R * Wc * 8);
    SG_TRY(rref_dev(d.as<u64>(), R, Wc, xor_count, pivots));
    HIP_TRY(hipMemcpyAsync(rows, d.p, (size_t)R * Wc * 8, hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

}  // extern "C"
