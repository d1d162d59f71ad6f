// product_driver.hip — the all-pairs product of two device operators and its C entry points: reads the switches, plans a call and runs it
// as stages.  The row-stream kernels and their launch wrappers are in product.hip, the pair kernel in product_pairs.hip; product_common.h
// lists the files.
#include "product_common.h"
#include <stdlib.h>
#include <stdio.h>

namespace symgpu {

static ProductSwitches read_product_switches() {
    ProductSwitches sw;
    const char *e = nullptr;
    if ((e = getenv("SYMGPU_PRODUCT_FUSED"))) sw.fused = e[0] != '0';
    if ((e = getenv("SYMGPU_PRODUCT_TILE_MB"))) sw.tile_mb = atof(e);
    if ((e = SG_TUNE("SYMGPU_PRODUCT_OVERLAP"))) sw.overlap = e[0] == '1';
    if ((e = SG_TUNE("SYMGPU_ROWS_VARIANT"))) {
        RowsVariant &rv = sw.rv;
        int a = 0, b2 = 0, c = 0, d = 256, p8 = 1;
        const int got = sscanf(e, "%d,%d,%d,%d,%d", &a, &b2, &c, &d, &p8);
        if (got >= 3 && (a == 1 || a == 2 || a == 4 || a == 8) && b2 >= 1) { rv.rc = a; rv.rto = b2; rv.nt = c != 0; }
        if (got >= 4 && (d == 64 || d == 128 || d == 256 || d == 512 || d == 1024)) rv.threads = d;
        if (got >= 5) rv.pad8 = p8 != 0;
    }
    return sw;
}

static bool phase_stream_supported(int Wq) { return Wq >= 1 && Wq <= 64 && (Wq & (Wq - 1)) == 0; }

// Pure host code.  The order of the tests matters: the phase-byte stream is asked first and serves every row length it can, whatever the
// pair count — it costs no more than the rows alone do — and the wide kernel only competes with the pair kernel for what is left (rows that
// are not a power-of-two number of chunks, or SYMGPU_PRODUCT_FUSED=0).
static ProductPlan plan_product(i64 Ni, i64 No, int Wq, bool with_coeff, const ProductSwitches &sw) {
    ProductPlan pl{};
    if (!with_coeff) pl.path = ProductPath::RowsOnly;
    else if (sw.fused && phase_stream_supported(Wq)) pl.path = ProductPath::PhaseStream;
    else if (wide_pairs_worthwhile(Ni, No, Wq)) pl.path = ProductPath::WideCoeffThenRows;
    else pl.path = sw.overlap ? ProductPath::WordMajorBesideRows : ProductPath::WordMajorThenRows;
    const bool phase = pl.path == ProductPath::PhaseStream;
    pl.rv = phase ? RowsVariant{1, 1, 1, 256, 1} : sw.rv;
    pl.n_chunks = Ni * Wq;
    pl.tile = inner_tile_chunks(pl.n_chunks, Wq, sw.tile_mb);
    pl.gy_total = (No + pl.rv.rto - 1) / pl.rv.rto;
    if (phase) {
        const i64 R = 256 / Wq;
        while (((i64)1 << pl.rshift) < R) ++pl.rshift;
        pl.eb_bytes = (size_t)(No < MAX_GRID_Y ? No : MAX_GRID_Y) * pl.grid_x(pl.tile < pl.n_chunks ? pl.tile : pl.n_chunks) * (R / 4);
    }
    return pl;
}

// ---- stages ------------------------------------------------------------------------------------------------------------
struct ProductCall {
    symgpu_op_s *inner, *outer, *out;
    i64 o_begin, o_end;                                                     // the slab of outer rows
    int inner_is_left;
};

// rows of the slab: out->rows[((o-o_begin)*Ni + i)*W + w]
static int stream_rows(const ProductPlan &pl, const ProductCall &p) {
    const int Wq = p.inner->Wq;
    return for_each_piece(pl, [&](i64 c_lo, i64 nc, i64 y0, i64 ny) {
        const i64 ooff = y0 * pl.rv.rto;
        return launch_rows(pl.rv, dim3((unsigned)pl.grid_x(nc), (unsigned)ny), reinterpret_cast<const u32x4 *>(p.inner->rows) + c_lo, nc,
                           reinterpret_cast<const u32x4 *>(p.outer->rows + (p.o_begin + ooff) * 2 * Wq), Wq, p.o_end - p.o_begin - ooff,
                           reinterpret_cast<u32x4 *>(p.out->rows) + ooff * pl.n_chunks + c_lo, pl.n_chunks);
    });
}

// rows AND coefficients through the phase-byte row stream: per piece k_mul_rows_e, then k_mul_coeff_expand on the bytes it left
static int stream_rows_and_phase_bytes(const ProductPlan &pl, const ProductCall &p) {
    const i64 Ni = p.inner->T;
    const int Wq = p.inner->Wq;
    const int *yi = nullptr, *yo = nullptr;
    SG_TRY(op_ycount(p.inner, &yi));
    SG_TRY(op_ycount(p.outer, &yo));
    Scratch eb;
    SG_TRY(eb.alloc(pl.eb_bytes));
    return for_each_piece(pl, [&](i64 c_lo, i64 nc, i64 y0, i64 ny) {
        const i64 i_lo = c_lo / Wq, ni = nc / Wq, o_lo = p.o_begin + y0;
        const i64 gx = pl.grid_x(nc);
        SG_TRY(launch_rows_e(Wq, p.inner_is_left, dim3((unsigned)gx, (unsigned)ny), reinterpret_cast<const u32x4 *>(p.inner->rows) + c_lo, nc,
                             reinterpret_cast<const u32x4 *>(p.outer->rows + o_lo * 2 * Wq),
                             reinterpret_cast<u32x4 *>(p.out->rows) + y0 * pl.n_chunks + c_lo, eb.as<unsigned char>(), pl.n_chunks));
        return launch_coeff_expand(dim3((unsigned)pl.expand_grid_x(ni), (unsigned)ny), eb.as<unsigned char>(), gx, pl.rshift, yi + i_lo, yo + o_lo, p.inner->coeff + 2 * i_lo,
                                   p.outer->coeff + 2 * o_lo, ni, p.out->coeff + 2 * (y0 * Ni + i_lo), Ni);
    });
}

static int wide_coeff_then_rows(const ProductPlan &pl, const ProductCall &p) {
    SG_TRY(wide_mul_coeff_dev(p.inner->rows, p.inner->coeff, p.inner->T, p.outer->rows, p.outer->coeff, p.o_begin, p.o_end, p.inner->Wq,
                              p.inner_is_left, p.out->coeff, nullptr));
    return stream_rows(pl, p);
}

// coefficients from the pair kernel on stream `st`; It = the inner operand's word-major copy (op_wordmajor: built on the main stream, cached
// across the slabs of one inner operand)
static int pair_coeff(const ProductCall &p, const u64 *It, i64 Ipad, hipStream_t st, Scratch &ot) {
    return mul_coeff_launch(It, Ipad, p.inner->coeff, p.inner->T, p.outer->rows, p.outer->coeff, p.o_begin, p.o_end, p.inner->Wq, p.inner_is_left,
                            p.out->coeff, st, ot);
}

static int wordmajor_coeff_then_rows(const ProductPlan &pl, const ProductCall &p) {
    const u64 *It = nullptr;
    i64 Ipad = 0;
    SG_TRY(op_wordmajor(p.inner, 64 * PJ, &It, &Ipad));
    Scratch ot;
    SG_TRY(pair_coeff(p, It, Ipad, ctx().stream, ot));
    return stream_rows(pl, p);
}

// Two-stream form.  Both launches are issued, the join event is recorded and waited on, and only then is the first error returned: the main
// stream must never run ahead of work queued on the side stream.
static int wordmajor_coeff_beside_rows(const ProductPlan &pl, const ProductCall &p) {
    Context &c = ctx();
    const u64 *It = nullptr;
    i64 Ipad = 0;
    SG_TRY(op_wordmajor(p.inner, 64 * PJ, &It, &Ipad));
    Scratch ot;
    HIP_TRY(hipEventRecord(c.ev_fork, c.stream));
    HIP_TRY(hipStreamWaitEvent(c.stream2, c.ev_fork, 0));
    const int rc = pair_coeff(p, It, Ipad, c.stream2, ot);
    const hipError_t e1 = hipEventRecord(c.ev_join, c.stream2);
    const int rc2 = stream_rows(pl, p);
    const hipError_t e2 = hipStreamWaitEvent(c.stream, c.ev_join, 0);
    if (rc != SYMGPU_OK) return rc;
    if (rc2 != SYMGPU_OK) return rc2;
    if (e1 != hipSuccess) return hip_fail(e1, "event record (join)", __FILE__, __LINE__);
    if (e2 != hipSuccess) return hip_fail(e2, "stream wait (join)", __FILE__, __LINE__);
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_mul_allpairs_dev(symgpu_op_t inner, symgpu_op_t outer, int64_t o_begin, int64_t o_end, int inner_is_left,
                            symgpu_op_t out) {
    SG_ENTER(inner, outer, out);
    SG_REQUIRE(inner && outer && out, "mul_allpairs_dev: null handle");
    SG_REQUIRE(out != inner && out != outer, "mul_allpairs_dev: out must not be one of the operands");
    SG_REQUIRE(inner->Wq == outer->Wq && out->Wq == inner->Wq, "mul_allpairs_dev: operands must share Wq");
    SG_REQUIRE(0 <= o_begin && o_begin <= o_end && o_end <= outer->T, "mul_allpairs_dev: bad outer range");
    const i64 rows = (o_end - o_begin) * inner->T;
    if (rows > out->capacity) {
        set_error("mul_allpairs_dev: output capacity %lld < %lld rows", (long long)out->capacity, (long long)rows);
        return SYMGPU_E_CAPACITY;
    }
    op_invalidate(out);
    if (rows > 0) {
        if (out->coeff) SG_REQUIRE(inner->coeff && outer->coeff, "mul_allpairs_dev: operands have no coefficients");
        const ProductSwitches sw = read_product_switches();
        const ProductPlan pl = plan_product(inner->T, o_end - o_begin, inner->Wq, out->coeff != nullptr, sw);
        const ProductCall p{inner, outer, out, o_begin, o_end, inner_is_left};
        bump_counter(counter_of(pl.path));                // which path served the call
        switch (pl.path) {
            case ProductPath::RowsOnly: SG_TRY(stream_rows(pl, p)); break;
            case ProductPath::PhaseStream: SG_TRY(stream_rows_and_phase_bytes(pl, p)); break;
            case ProductPath::WideCoeffThenRows: SG_TRY(wide_coeff_then_rows(pl, p)); break;
            case ProductPath::WordMajorThenRows: SG_TRY(wordmajor_coeff_then_rows(pl, p)); break;
            case ProductPath::WordMajorBesideRows: SG_TRY(wordmajor_coeff_beside_rows(pl, p)); break;
        }
    }
    out->T = rows;
    return SYMGPU_OK;
}

int symgpu_mul_allpairs(const uint64_t *inner, const double *ci, int64_t Ni, const uint64_t *outer, const double *co,
                        int64_t No, int Wq, int inner_is_left, uint64_t *out_rows, double *out_coeff) {
    SG_ENTER();
    SG_REQUIRE(Ni >= 0 && No >= 0 && Wq >= 1, "mul_allpairs: sizes");
    if (Ni == 0 || No == 0) return SYMGPU_OK;
    SG_REQUIRE(inner && outer && ci && co && out_rows && out_coeff, "mul_allpairs: null pointer");
    OwnedOp a, b, o;
    SG_TRY(symgpu_op_upload(inner, ci, Ni, Wq, a.slot()));
    SG_TRY(symgpu_op_upload(outer, co, No, Wq, b.slot()));
    SG_TRY(o.alloc(Ni * No, 0, Wq, true));
    SG_TRY(symgpu_mul_allpairs_dev(a.op, b.op, 0, No, inner_is_left, o.op));
    return symgpu_op_download(o.op, out_rows, out_coeff, Ni * No);
}

}  // extern "C"
