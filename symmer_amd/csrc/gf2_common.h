// gf2_common.h — what the files of the GF(2) elimination share; private to them:
//   gf2.hip            the kernels of the blocked path (lead, panel, select, sweep), the one-workgroup kernel and their launch wrappers
//   gf2_panel.h        the panel device code (included by gf2.hip only: device functions live in their kernel's translation unit)
//   gf2_driver.hip     switches, plan, stages, rref_dev, symgpu_rref / symgpu_rref_dev
//   gf2_symmetry.hip   symmetry-generator matrix build and read-out around rref_dev (includes common.h only)
#pragma once
#include "common.h"

namespace symgpu {

constexpr int WK = 64;        // max rows per block = lanes of the panel wave
constexpr int WN = 4;         // window width in 64-bit words
constexpr int NOLEAD = 0x7fffffff;

struct BlockInfo {
    i64 i0;                   // first row of the block
    int kk;                   // rows in the block (0: nothing left)
    int pivw[WK];             // absolute pivot word per block row, -1 = no pivot (zero row)
    int pivb[WK];
    u64 mask[WK];             // block rows (bit r < kk, r != j) holding pivot j's column at time j
    u64 T[WK];                // new_row_r = XOR_{i in T[r]} old_row_i
    int w_next;               // the largest pivot word of the block: where the NEXT block's window most likely starts (-1: no guess)
};

struct SweepState {
    i64 next_i0;              // first row not yet processed
};

// What a blocked reduction counts, zeroed in front of it.  `blocks` takes ONE packed add per block from the panel.
struct Gf2Counters {
    unsigned long long xors;                    // row-XORs as the reference performs them (the panels' share; k_sum_u32 adds the rows')
    u32 timed_out;                              // a tile workgroup of k_sweep_m4r<M4_SELECT_NEXT> gave up waiting for the selectors
    u32 full_panels;                            // blocks panelled on the full rows in LDS
    unsigned long long blocks;                  // blocks panelled | of these on the two-word window << 32
    unsigned long long unused;
};

// k_sweep_m4r<PHASE>: what one launch of the Four-Russians sweep does (plain integers: they are part of the kernels' names)
constexpr int M4_NEXT = 0;                      // sweeps only the rows of the next block and collects their leading words
constexpr int M4_PANEL_REST = 1;                // workgroup 0 panels the next block, the others sweep all remaining rows
constexpr int M4_ALL = 2;                       // plain sweep of all rows, no lookahead
constexpr int M4_SELECT_NEXT = 3;               // M4_NEXT and the selector launch in one grid

constexpr int M4_TW = 64;                       // words per column tile = lanes
constexpr int M4_NT = 1024;                     // threads per workgroup (16 waves; one workgroup per CU because of the table)
constexpr int M4_U = 4;                         // rows in flight per wave
constexpr size_t M4_LDS = (size_t)16 * 16 * M4_TW * sizeof(u64);
constexpr int SEL_PRI = 4;                      // priority blocks: 16 rows (wavefronts) each = the next block's 64 rows
struct FusedSelect {
    u64 *sel;                                   // writable view of the selectors
    u64 *snap;
    u32 *rowcnt;
    u64 *ready;                                 // [64][2] granules {epoch 32 | half of the row's selector 32}: the data is the flag
    u32 epoch;
    Gf2Counters *counters;                      // where a tile workgroup that gave up waiting, and the full-row choice, are recorded
    int full_panel;                             // 1: the panel may switch to the full rows in LDS (panel_full)
    int lean_panel;                             // 1: two-word windows run panel_loop_narrow (0: the generic loop; tests)
};

constexpr int SMALL_R = 64, SMALL_WC = 64;     // wider dense matrices are faster on the blocked path (measured)

// One blocked reduction: the matrix, the buffers its launches share (allocated once by the driver) and what the plan fixed for them.
struct Gf2Run {
    u64 *rows;
    i64 R, Wc;
    int m4_tiles, m4_chunks;                    // column tiles of 64 words; row chunks of the main sweep (about one workgroup per CU)
    int full_panel, lean_panel;                 // FusedSelect
    Scratch info, state, lead;                  // 2 BlockInfo (swept / panelled, alternating), SweepState, [64] leading words of the next block
    Scratch sel, snap, rowcnt;                  // [R] selectors, [64][Wc] old block rows, [R] row-XORs of every row
    Scratch counters, piv, ready;               // Gf2Counters, [R] pivot columns, [64][2] selector flags of the fused launch
};

// gf2.hip: launches (the grid arithmetic lives there) and the once-per-device LDS attributes of the kernels
bool gf2_small_attr_ok();                       // k_rref_small may use 32 KiB of dynamic LDS
bool gf2_m4r_attr_ok();                         // k_sweep_m4r<0..3> may use 128 KiB
int launch_rref_small(u64 *rows, i64 R, i64 Wc, i64 *pivots, unsigned long long *xor_count);
void launch_fill_nolead(const Gf2Run &g);
// iteration `it` of the lookahead schedule: selectors of block it-1 and the sweep of block it's rows (one grid if `fused`), then the panel of
// block it inside the sweep of all other rows
int launch_lookahead_step(const Gf2Run &g, i64 it, bool fused);
int launch_plain_step(const Gf2Run &g, bool m4r);   // lead -> panel -> select -> sweep (Four Russians or flag per block row) of the next block
int launch_row_xor_sum(const Gf2Run &g);        // counters.xors += sum of rowcnt

}  // namespace symgpu
