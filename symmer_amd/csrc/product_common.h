// product_common.h — what the files of the all-pairs product share; private to them:
//   product.hip          the row streams (k_mul_rows, k_mul_rows_e, k_mul_coeff_expand), the inner-operand tiling and their launch wrappers
//   product_pairs.hip    the word-major pair kernel k_mul_coeff (coefficients or cleanup keys), mul_coeff_dev / mul_keys_dev
//   product_driver.hip   switches, plan, stages, symgpu_mul_allpairs_dev / symgpu_mul_allpairs
// PairKeyArgs and the declarations of mul_coeff_dev / mul_keys_dev are in common.h: the cleanup and wide.hip use them.
#pragma once
#include "common.h"

namespace symgpu {

// tile of the pair kernel
constexpr int PO = 8;   // outer terms per wave (SGPR operand)
constexpr int PJ = 4;   // inner terms per lane: i = ibase + 64*b + lane
constexpr int PW = 4;   // waves per block, stacked along o

constexpr i64 MAX_GRID_Y = 65535;

// The plain row stream's tuning knobs (defaults are the measured best on MI355X; SYMGPU_ROWS_VARIANT="rc,rto,nt[,threads[,pad8]]" overrides
// for experiments): 16-byte chunks per lane, outer rows per block, non-temporal stores, block size, grid.x padded to a multiple of 8
struct RowsVariant { int rc = 1, rto = 1, nt = 1, threads = 256, pad8 = 1; };

// Every switch of the product, read once at the top of a call: the tests flip the first two between calls of one process.
// SYMGPU_WIDE is not here: wide_pairs_worthwhile reads it, for the commutation and the cleanup as well.
struct ProductSwitches {
    bool fused = true;               // SYMGPU_PRODUCT_FUSED=0: coefficients from the pair kernel instead of the phase-byte row stream
    double tile_mb = 0;              // SYMGPU_PRODUCT_TILE_MB (tests): MiB of inner operand per tile of a row stream; <= 0: the measured sizes
    // tuning knobs (SG_TUNE: compiled out of the default build)
    bool overlap = false;            // SYMGPU_PRODUCT_OVERLAP=1: the pair kernel on the side stream beside the row stream
    RowsVariant rv;                  // SYMGPU_ROWS_VARIANT
};

// What a call with coefficients runs, with the measurements behind the choice (per 256-row slab of 10^5 inner terms of 1,000 qubits).
enum class ProductPath {
    RowsOnly,                        // the output has no coefficients: the plain row stream
    // The row stream forms the phase sums on the way (its VALU is idle) and a streaming kernel expands them to coefficients: 0.075 ms of
    // streaming in place of the pair kernel's 0.158 ms of VALU work.  Needs a row of a power-of-two number of 16-byte chunks, <= 64.
    PhaseStream,
    WideCoeffThenRows,               // few pairs of very long rows: coefficients parallel over the words (wide.hip), then the plain row stream
    // Pair kernel (VALU-bound, 16 B/pair), then the plain row stream (HBM-bound, 16*Wq B/pair), ONE AFTER THE OTHER on the main stream.  The
    // one-row-per-block row stream lives on the inner operand staying in each XCD's L2 (product.hip), and the pair kernel's 436 MB of traffic
    // per slab running beside it evicts that: in turn 0.95 + 0.15 = 1.10 ms, overlapped 1.34 ms.  ONE launch doing both was slower still
    // (1.86e10 pairs/s): the long VALU prologue of every block delays its stores.
    WordMajorThenRows,
    WordMajorBesideRows,             // the same on two streams (SYMGPU_PRODUCT_OVERLAP=1, for experiments): it paid while the row stream
                                     // wrote 12 rows per block (6.1 TB/s either way)
};
// the counter of the calls a path served (product_driver.hip bumps it at the switch)
constexpr symgpu_counter counter_of(ProductPath p) { return (symgpu_counter)(SYMGPU_CTR_PRODUCT_ROWS_ONLY + (int)p); }
static_assert(counter_of(ProductPath::RowsOnly) == SYMGPU_CTR_PRODUCT_ROWS_ONLY && counter_of(ProductPath::PhaseStream) == SYMGPU_CTR_PRODUCT_PHASE_STREAM &&
              counter_of(ProductPath::WideCoeffThenRows) == SYMGPU_CTR_PRODUCT_WIDE_COEFF_THEN_ROWS &&
              counter_of(ProductPath::WordMajorThenRows) == SYMGPU_CTR_PRODUCT_WORD_MAJOR_THEN_ROWS &&
              counter_of(ProductPath::WordMajorBesideRows) == SYMGPU_CTR_PRODUCT_WORD_MAJOR_BESIDE_ROWS, "ProductPath and its counters are in one order");

// What a call decides before it launches anything.  A row stream (plain or phase-byte) covers the inner operand tile by tile and the outer rows
// in batches of at most MAX_GRID_Y grid.y indices: for_each_piece.
struct ProductPlan {
    ProductPath path;
    // shape of the row stream: the plain one's variant or, for the phase-byte kernel, what that kernel is built for (one chunk per lane, one
    // outer row per workgroup, 256 threads, grid.x padded to a multiple of 8: the surplus workgroups exit, tile bx is always on XCD bx % 8)
    RowsVariant rv;
    i64 n_chunks, tile;              // 16-byte chunks of the inner operand / of one tile of it (inner_tile_chunks)
    i64 gy_total;                    // grid.y indices that cover the slab, rv.rto outer rows each
    int rshift;                      // phase-byte stream: log2 of the R = 256 / Wq rows of a workgroup
    size_t eb_bytes;                 // ... its scratch of 2-bit phase sums: R/4 bytes per row block of one batch
    static i64 pad_to_8(i64 g) { return (g + 7) / 8 * 8; }
    i64 grid_x(i64 nc) const {       // workgroups along x of a tile of nc chunks
        const i64 per = (i64)rv.threads * rv.rc, gx = (nc + per - 1) / per;
        return rv.pad8 ? pad_to_8(gx) : gx;
    }
    i64 expand_grid_x(i64 ni) const { return pad_to_8((ni + 255) / 256); }   // coefficient expansion: one 256-term piece of one outer row per workgroup
};

// the batches of at most MAX_GRID_Y that cover gy_total grid.y indices: f(y0, ny) -> SYMGPU_OK or the error that ends the walk
template <typename F> int for_each_y_batch(i64 gy_total, F &&f) {
    for (i64 y0 = 0; y0 < gy_total; y0 += MAX_GRID_Y) SG_TRY(f(y0, gy_total - y0 < MAX_GRID_Y ? gy_total - y0 : MAX_GRID_Y));
    return SYMGPU_OK;
}
// the launches of a row stream, tile by tile and in every tile batch by batch: f(c_lo, nc, y0, ny), chunks [c_lo, c_lo + nc) of the inner operand
template <typename F> int for_each_piece(const ProductPlan &pl, F &&f) {
    for (i64 c_lo = 0; c_lo < pl.n_chunks; c_lo += pl.tile) {
        const i64 nc = pl.n_chunks - c_lo < pl.tile ? pl.n_chunks - c_lo : pl.tile;
        SG_TRY(for_each_y_batch(pl.gy_total, [&](i64 y0, i64 ny) { return f(c_lo, nc, y0, ny); }));
    }
    return SYMGPU_OK;
}

static inline i64 round_up(i64 x, i64 m) { return (x + m - 1) / m * m; }

// product.hip: launches on the main stream, each with its error check (the row kernels inside a ProfScope of class 0)
i64 inner_tile_chunks(i64 n_chunks, int Wq, double tile_mb);
int launch_rows(const RowsVariant &rv, dim3 grid, const u32x4 *inner, i64 n_chunks, const u32x4 *outer, int Wq, i64 o_count, u32x4 *out, i64 out_stride);
int launch_rows_e(int Wq, int inner_is_left, dim3 grid, const u32x4 *inner, i64 n_chunks, const u32x4 *outer, u32x4 *out, unsigned char *eb,
                  i64 out_stride);
int launch_coeff_expand(dim3 grid, const unsigned char *eb, i64 egx, int rshift, const int *yi, const int *yo, const double *ci, const double *co,
                        i64 Ni, double *out, i64 out_stride);

// product_pairs.hip: coefficients of the slab of outer rows [o_begin, o_end): out_coeff[(o-o_begin)*Ni + i], or (keys) the cleanup keys of all
// pairs.  It = word-major inner operand (padded to Ipad, a multiple of 64*PJ); the kernels go to stream `st`, the word-major outer slab to `ot`.
int mul_coeff_launch(const u64 *It, i64 Ipad, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end, int Wq,
                     int inner_is_left, double *out_coeff, hipStream_t st, Scratch &ot, const PairKeyArgs *keys = nullptr);

}  // namespace symgpu
