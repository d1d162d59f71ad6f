// cleanup_driver.hip — duplicate-term cleanup (reference: symplectic_cleanup, symmer/operators/utils.py:230-279;
// PauliwordOp.cleanup base.py:617-638) and the fused product+cleanup (base.py:764-794).
//
// The reference keys a hash map with the full row.  Here rows are grouped by sorting a 64-bit GF(2)-LINEAR
// row hash  h(r) = XOR over set bits of a random 64-bit vector per bit position, evaluated as 8 byte-table
// lookups per word (LDS), a per-word rotation and a per-64-word-block xorshift step.  Linearity gives
// h(a ^ b) = h(a) ^ h(b): the key of product row (i, o) is hI[i] ^ hO[o], so the fused path never
// materialises the N*M product rows — only the surviving unique rows are written.
// Exactness does not rest on the hash: after the stable sort every adjacent equal-key pair is compared
// word by word; any mismatch reseeds the tables and retries (SYMGPU_E_COLLISION if it survives 4 seeds).
//
// Pipeline: hash -> stable LSD radix sort (key, input index) -> head flags + verify -> scan (segment ids)
//           -> per-segment SEQUENTIAL coefficient sum in input order (== np.add.at, utils.py:273-274)
//           -> threshold |c| > thr (strict, utils.py:275-278) -> first-occurrence order via mark+scan over
//           input positions (qiskit `unordered_unique` order, utils.py:271) -> gather surviving rows.
#include "cleanup_common.h"
#include <stdlib.h>
#include <stdio.h>

namespace symgpu {

static CleanupSwitches read_cleanup_switches() {
    CleanupSwitches sw;
    const char *e = nullptr;
    if ((e = getenv("SYMGPU_CLEANUP_UNPACKED"))) sw.unpacked = e[0] == '1';
    if ((e = getenv("SYMGPU_CLEANUP_NOSQUARE"))) sw.nosquare = e[0] == '1';
    if ((e = getenv("SYMGPU_CLEANUP_LAZY"))) sw.lazy = e[0] == '0' ? 0 : 1;
    if ((e = getenv("SYMGPU_CLEANUP_SUSPECTS"))) sw.suspects = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    if ((e = getenv("SYMGPU_CLEANUP_KEYBYTES"))) sw.key_bytes = e[0] != '0';
    sw.nofloor = getenv("SYMGPU_CLEANUP_NOFLOOR") != nullptr;
    if ((e = getenv("SYMGPU_EMIT_FUSED"))) sw.emit_fused = e[0] != '0';
    if ((e = SG_TUNE("SYMGPU_HS_WAVES"))) sw.hs_waves = atoll(e);
    if ((e = SG_TUNE("SYMGPU_CLEANUP_ZEROSEG"))) sw.zero_seg = e[0] != '0';
    if ((e = SG_TUNE("SYMGPU_EMIT_TOUCH"))) sw.emit_touch = e[0] != '0';
    sw.emit_no_one_outer = SG_TUNE("SYMGPU_EMIT_NO_ONE_OUTER") != nullptr;
    if ((e = SG_TUNE("SYMGPU_EMIT_SHAPE"))) { int nw = 2, u = 4; sscanf(e, "%d,%d", &nw, &u); sw.emit_shape = nw * 16 + u; }
    if ((e = SG_TUNE("SYMGPU_EMIT_RC"))) sw.emit_rc = atoi(e);
    return sw;
}

// full_sort: a long mixed prefix run in an earlier attempt — 64-bit keys of all T terms, sorted on all 64 bits (pair coefficients materialised)
static CleanupPlan plan_cleanup(const CleanupRequest &rq, const CleanupSwitches &sw, bool full_sort = false) {
    CleanupPlan pl;
    const PairOperands &p = rq.p;
    // pair mode sorts PACKED keys (hash | e | o | i) unless the index fields need more than 32 bits (SYMGPU_CLEANUP_UNPACKED=1: tests)
    while (rq.pair && ((i64)1 << pl.L.bi) < p.Ni) ++pl.L.bi;
    while (rq.pair && ((i64)1 << pl.L.bo) < p.No) ++pl.L.bo;
    pl.packed = rq.pair && pl.L.bi + pl.L.bo <= 32 && pl.L.bi < 32 && !sw.unpacked && !full_sort;
    // P * P with one device operand for both factors: keys only for the pairs with i >= o (product.hip, KM = 2), weighted 1 / 2 / 0
    // — valid when exact zeros are dropped anyway (strict |c| > thr with thr >= 0): without a threshold the reference keeps the
    // rows of anticommuting pairs with coefficient 0, and the sum x + y - x of a row shared with other pairs need not equal y
    // (and thr > 0: the twin-first sums differ from the reference's sequential ones by rounding for coefficients that are not dyadic, and
    // against thr = 0 a residue of 1e-33 instead of an exact 0 keeps or drops a ROW — tools/stress_cleanup.py, tiny planted coefficients)
    pl.squared = pl.packed && p.inner == p.outer && p.Ni == p.No && p.ci == p.co && rq.use_thr && rq.thr > 0.0 && !sw.nosquare;
    pl.Tk = pl.squared ? p.Ni * (p.Ni + 1) / 2 : rq.T;                  // the pairs with i >= o
    const int hash_bits = pl.packed ? 64 - pl.L.F() : 64;                // a packed key carries 64 - F >= 30 hash bits
    pl.nbits = full_sort ? 64 : sorted_bits(pl.Tk, hash_bits);
    // singles decided in index order, only merged terms filed from the sorted order (k_mark_singles); SYMGPU_CLEANUP_LAZY=0: every term filed
    // Default: products only.  A plain cleanup is what follows `A + B` or a rotation — inputs full of repeated rows, where every chunk
    // holds merged terms and the extra passes buy nothing (10^6 terms of 1,000 qubits, 2.7 copies of every row: 0.89 ms lazy against
    // 0.55 ms filed); SYMGPU_CLEANUP_LAZY=1 forces the lazy flow for plain cleanups too (tests), 0 switches it off everywhere.
    pl.lazy_call = sw.lazy == 1 || (sw.lazy == -1 && rq.pair);
    // the lazy flow pays off on big key sets (its passes are fixed costs, the scatter it avoids only hurts at scale): from 2^18 keys for
    // general products (2.5e5 keys: 0.178 -> 0.164 ms, 1.5e6: 0.32 -> 0.25, 4e6: 0.60 -> 0.42), from 2^20 for squared operators (5e5 keys:
    // 0.222 against 0.231 lazy; 1.1e6: 0.31 -> 0.30, 3.1e6: 0.42 -> 0.37) — round 4's gate was 2^22 for both
    pl.lazy = pl.lazy_call && (sw.lazy == 1 || pl.Tk >= ((i64)1 << (pl.squared ? 20 : 18)));
    // products whose keys mostly merge with nothing: stop the sort early and sort only the keys that have a partner
    // (k_find_suspects).  Applies when a run of the partial order is short (<= 2,048 keys on average) and the operands are not
    // one array used twice without the squared-operator compaction (then EVERY key has its twin).
    pl.sus_try = pl.packed && pl.lazy && sw.suspects != 0 && pl.nbits == 32 && (pl.Tk >> SUS_RUN_BITS) <= 2048 && !(p.inner == p.outer && !pl.squared);
    // round 6: where the flag pass works from the operand hash tables (pair_dups.hip) nobody reads the keys but the marking of
    // the single terms, and all it reads of them is the phase exponent and "is the diagonal": the key kernel then writes ONE BYTE
    // per pair (into the key buffer) and k_mark_bytes marks from those; the few flagged keys are rebuilt at their compaction.
    // Should the flag pass give up, the keys are generated after all.
    pl.key_bytes = pl.sus_try && pair_dups_fits(p.Ni, p.No, pl.squared, pl.Tk, nullptr) && !wide_pairs_worthwhile(p.Ni, p.No, rq.W / 2) && sw.key_bytes;
    return pl;
}

static LazyEmit lazy_emit(const CleanupRun &r) {
    LazyEmit lz; lz.no_one_outer = r.sw.emit_no_one_outer ? 1 : 0;
    if (r.a.lazy) {
        lz.mode = r.pl.packed ? 1 : 2; lz.squared = r.pl.squared ? 1 : 0;
        lz.patchbits = r.patchbits.as<u32>(); lz.e_lo = r.e_lo.as<u32>(); lz.e_hi = r.e_hi.as<u32>();
        lz.ci = r.rq.p.ci; lz.co = r.rq.p.co; lz.coeff = r.coeff;
    }
    return lz;
}

// The output stage's prefix over the kept-term bitmap is formed BEFORE the attempt's status words are read: the count of kept terms comes
// back with them (an attempt that has to be repeated throws the prefix away).  hback: [0] the count, [1] a collision, [2] a long mixed prefix
// run, [3] the one-launch sort's flag
static int cleanup_status(CleanupRun &r, u32 hback[4]) {
    EmitPrefix &pre = r.pre;
    pre.wide = r.sw.fused(r.rq.W / 2);
    SG_TRY(emit_prefix(r.markbits.as<u32>(), r.pl.Tk, pre.wordprefix, pre.total, pre.wide));
    pre.touched = false;
    if (pre.wide && r.sw.emit_touch == -1)      // (the output stage's bitmaps back into the cache: queued ahead of the read-back, not behind it)
        SG_TRY(emit_touch(r.markbits.as<u32>(), r.pl.Tk, lazy_emit(r), pre));
    // (ONE trip to the host for the count and the status words.  Measured and dropped, round 6: small results allocated for every index
    // and the output stage queued before the count is in — same-box A/B 3 - 14 us SLOWER per call, 72 -> 75 us at 10^3 rows.)
    SG_TRY(read_back_words(pre.total.as<u32>(), 1, r.collision.as<u32>(), 2, hback, r.a.sus_coop ? radix_sort_coop_flag() : nullptr));
    pre.n_out = hback[0];
    return SYMGPU_OK;
}

static int cleanup_run(const CleanupRequest &rq, symgpu_op_t *out) {
    if (rq.T >= ((i64)1 << 32) - 1) {
        set_error("cleanup: %lld terms exceed the 2^32-2 limit of the 32-bit index sort", (long long)rq.T);
        return SYMGPU_E_INVALID;
    }
    if (rq.T == 0) {
        OwnedOp res;
        SG_TRY(res.alloc(1, 0, rq.Wq_out, true));
        res->dup_free = 1;
        res.hand_out(out);
        return SYMGPU_OK;
    }
    CleanupRun r;
    r.rq = rq; r.sw = read_cleanup_switches(); r.pl = plan_cleanup(rq, r.sw);
    r.st = ctx().stream; r.coeff = rq.coeff;
    r.same_rows = rq.pair && rq.p.outer == rq.p.inner && rq.p.No == rq.p.Ni;
    const i64 T = rq.T;
    const size_t bitmap_bytes = (size_t)((T + 63) / 64) * 8;         // whole 64-bit words: k_mark_singles stores one per wavefront
    SG_TRY(r.keys.alloc((size_t)T * 8));
    SG_TRY(r.keys2.alloc((size_t)T * 8));
    SG_TRY(r.markbits.alloc(bitmap_bytes));                          // kept terms by first input index (one bit each)
    if (r.pl.lazy_call) {
        SG_TRY(r.patchbits.alloc(bitmap_bytes));                     // ... whose coefficient is a filed sum
        if (rq.pair) { SG_TRY(r.e_lo.alloc(bitmap_bytes)); SG_TRY(r.e_hi.alloc(bitmap_bytes)); }   // phase exponents of the pairs, by index
    }
    SG_TRY(r.sum_of.alloc((size_t)T * 16));                         // their summed coefficients, indexed the same way
    SG_TRY(r.collision.alloc(16));
    if (rq.pair) {
        SG_TRY(r.hI.alloc((size_t)rq.p.Ni * 8));
        if (!r.same_rows) SG_TRY(r.hO.alloc((size_t)rq.p.No * 8));
        r.hO_p = r.same_rows ? r.hI.as<u64>() : r.hO.as<u64>();
    } else {
        SG_TRY(r.idx.alloc((size_t)T * 4));
        SG_TRY(r.idx2.alloc((size_t)T * 4));
    }
    r.seed = ctx().hash_tab ? ctx().hash_seed : 1;
    struct JoinSide {                                                  // whatever way the function is left: the main stream is ordered behind the side
        bool &pending;                                                 // stream's kernel before its 16-byte result buffer goes back to the allocator
        ~JoinSide() { if (pending) (void)hipStreamWaitEvent(ctx().stream, ctx().ev_join, 0); }
    } join_side{r.diag_side};
    if (r.pl.squared) SG_TRY(cleanup_diag_begin(r));
    bool ok = false;
    for (int attempt = 0; attempt < 6 && !ok; ++attempt) {
        r.a = CleanupRun::Attempt(r.pl);
        SG_TRY(ensure_hash_tables(r.seed));
        SG_TRY(cleanup_hash_keys(r));
        SG_TRY(cleanup_order(r));
        SG_TRY(cleanup_fixups(r));
        SG_TRY(cleanup_segment_sums(r));
        u32 hback[4] = {0, 0, 0, 0};
        SG_TRY(cleanup_status(r, hback));
        if (r.a.sus_coop) {                                        // the one-launch sort of the flagged keys gave up at a barrier (GPU shared): its
            bool timed_out = false;                                // output is garbage; the form is off now, the next attempt sorts with launches
            radix_sort_coop_note(hback[3], &timed_out);
            if (timed_out) continue;
        }
        if (hback[2]) { bump_counter(SYMGPU_CTR_FLOW_FULL_SORT_REPEAT); r.pl = plan_cleanup(rq, r.sw, true); continue; }   // a long mixed prefix run: redo with a full 64-bit sort over all pairs, same seed
        ok = (hback[1] == 0);
        if (!ok) { ++r.seed; bump_counter(SYMGPU_CTR_HASH_RESEEDS); }   // genuine 64-bit hash collision: reseed and retry
    }
    if (!ok) { set_error("cleanup: 64-bit row-hash collision survived 4 reseeds"); return SYMGPU_E_COLLISION; }
    const PairOperands &p = rq.p;
    return cleanup_finish(r.markbits.as<u32>(), r.sum_of.as<double>(), r.pl.Tk, rq.pair, rq.rows, rq.W, p.inner, p.Ni, p.outer, out, rq.Wq_out,
                          r.pl.squared, lazy_emit(r), rq.want_first, r.sw, r.pre);
}

// plain mode: rows/coeff of T terms
int cleanup_rows(const u64 *rows, const double *coeff, i64 T, int W, double thr, int use_thr, symgpu_op_t *out, int Wq_out, bool want_first) {
    CleanupRequest rq;
    rq.rows = rows; rq.coeff = coeff; rq.T = T; rq.W = W; rq.Wq_out = Wq_out; rq.thr = thr; rq.use_thr = use_thr; rq.want_first = want_first;
    return cleanup_run(rq, out);
}

// pair mode: the Ni * No pairs of a product; there is no materialised input
int cleanup_pairs(const PairOperands &p, double thr, int use_thr, symgpu_op_t *out, bool want_first) {
    CleanupRequest rq;
    rq.pair = true; rq.p = p; rq.T = p.Ni * p.No; rq.W = p.W; rq.Wq_out = p.Wq_out; rq.thr = thr; rq.use_thr = use_thr; rq.want_first = want_first;
    return cleanup_run(rq, out);
}

// the tail of the calls that take and return host arrays: *n_out, the capacity check (`what`: the call's words for it), the download
int finish_to_host(OwnedOp &res, const char *what, uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out) {
    if (n_out) *n_out = res->T;
    if (res->T > capacity) {
        set_error("%s %lld < %lld rows", what, (long long)capacity, (long long)res->T);
        return SYMGPU_E_CAPACITY;
    }
    if (res->T > 0) SG_TRY(symgpu_op_download(res.op, out_rows, out_coeff, capacity));
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

static PairOperands product_operands(symgpu_op_t inner, symgpu_op_t outer, int inner_is_left) {
    PairOperands p;
    p.inner = inner->rows; p.outer = outer->rows; p.ci = inner->coeff; p.co = outer->coeff;
    p.Ni = inner->T; p.No = outer->T; p.W = 2 * inner->Wq; p.Wq_out = inner->Wq; p.inner_is_left = inner_is_left;
    return p;
}

extern "C" {

int symgpu_cleanup_dev(symgpu_op_t in, double thr, int use_thr, symgpu_op_t *out) {
    SG_ENTER(in);
    SG_REQUIRE(in && out, "cleanup_dev: null handle");
    SG_REQUIRE(in->coeff || in->T == 0, "cleanup_dev: operator has no coefficients");
    return cleanup_rows(in->rows, in->coeff, in->T, 2 * in->Wq, thr, use_thr, out, in->Wq);
}

int symgpu_mul_cleanup_dev(symgpu_op_t inner, symgpu_op_t outer, int inner_is_left, double thr, int use_thr, symgpu_op_t *out) {
    SG_ENTER(inner, outer);
    SG_REQUIRE(inner && outer && out, "mul_cleanup_dev: null handle");
    SG_REQUIRE(inner->Wq == outer->Wq, "mul_cleanup_dev: operands must share Wq");
    const i64 Ni = inner->T, No = outer->T;
    if (Ni * No == 0) return cleanup_rows(nullptr, nullptr, 0, 2 * inner->Wq, thr, use_thr, out, inner->Wq);
    SG_REQUIRE(inner->coeff && outer->coeff, "mul_cleanup_dev: operands have no coefficients");
    SG_REQUIRE(No == 0 || Ni < ((i64)1 << 32) / No, "mul_cleanup_dev: Ni*No must stay below 2^32 (tile the outer operand)");
    return cleanup_pairs(product_operands(inner, outer, inner_is_left), thr, use_thr, out);
}

// The same two calls, with the first-occurrence index of every output term kept on the result (symgpu_op_first_index): what a caller needs
// to merge cleaned partial results of ONE product in the reference's order (symmer_amd/parallel.py: hash-partitioned multi-GPU cleanup).
int symgpu_cleanup_indexed_dev(symgpu_op_t in, double thr, int use_thr, symgpu_op_t *out) {
    SG_ENTER(in);
    SG_REQUIRE(in && out, "cleanup_indexed_dev: null handle");
    SG_REQUIRE(in->coeff || in->T == 0, "cleanup_indexed_dev: operator has no coefficients");
    return cleanup_rows(in->rows, in->coeff, in->T, 2 * in->Wq, thr, use_thr, out, in->Wq, true);
}

int symgpu_mul_cleanup_indexed_dev(symgpu_op_t inner, symgpu_op_t outer, int inner_is_left, double thr, int use_thr, symgpu_op_t *out) {
    SG_ENTER(inner, outer);
    SG_REQUIRE(inner && outer && out, "mul_cleanup_indexed_dev: null handle");
    SG_REQUIRE(inner->Wq == outer->Wq, "mul_cleanup_indexed_dev: operands must share Wq");
    const i64 Ni = inner->T, No = outer->T;
    if (Ni * No == 0) return cleanup_rows(nullptr, nullptr, 0, 2 * inner->Wq, thr, use_thr, out, inner->Wq, true);
    SG_REQUIRE(inner->coeff && outer->coeff, "mul_cleanup_indexed_dev: operands have no coefficients");
    SG_REQUIRE(Ni < ((i64)1 << 32) / No, "mul_cleanup_indexed_dev: Ni*No must stay below 2^32 (tile the outer operand)");
    return cleanup_pairs(product_operands(inner, outer, inner_is_left), thr, use_thr, out, true);
}

int symgpu_op_first_index(symgpu_op_t op, uint64_t *first_host, int64_t capacity) {
    SG_ENTER(op);
    SG_REQUIRE(op && (first_host || op->T == 0), "op_first_index: null argument");
    SG_REQUIRE(op->first || op->T == 0, "op_first_index: the operator does not come from an *_indexed cleanup");
    if (capacity < op->T) { set_error("op_first_index: capacity %lld < %lld rows", (long long)capacity, (long long)op->T); return SYMGPU_E_CAPACITY; }
    if (op->T > 0) {
        HIP_TRY(hipMemcpyAsync(first_host, op->first, (size_t)op->T * 8, hipMemcpyDeviceToHost, ctx().stream));
        count_d2h((size_t)op->T * 8);
        HIP_TRY(hipStreamSynchronize(ctx().stream));
    }
    return SYMGPU_OK;
}

int symgpu_cleanup(const uint64_t *rows, const double *coeff, int64_t T, int W, double thr, int use_thr, uint64_t *out_rows,
                   double *out_coeff, int64_t capacity, int64_t *n_out) {
    SG_ENTER();
    SG_REQUIRE(T >= 0 && W >= 2 && (W % 2) == 0 && capacity >= 0, "cleanup: sizes (W must be 2*Wq)");
    SG_REQUIRE(T == 0 || (rows && coeff), "cleanup: null input");
    OwnedOp in, res;
    SG_TRY(symgpu_op_upload(rows, coeff, T, W / 2, in.slot()));
    SG_TRY(cleanup_rows(in->rows, in->coeff, T, W, thr, use_thr, res.slot(), W / 2));
    in.reset();
    return finish_to_host(res, "output capacity", out_rows, out_coeff, capacity, n_out);
}

int symgpu_mul_cleanup(const uint64_t *inner, const double *ci, int64_t Ni, const uint64_t *outer, const double *co, int64_t No,
                       int Wq, int inner_is_left, double thr, int use_thr, uint64_t *out_rows, double *out_coeff, int64_t capacity,
                       int64_t *n_out) {
    SG_ENTER();
    SG_REQUIRE(Ni >= 0 && No >= 0 && Wq >= 1 && capacity >= 0, "mul_cleanup: sizes");
    if (Ni == 0 || No == 0) { if (n_out) *n_out = 0; return SYMGPU_OK; }
    SG_REQUIRE(inner && outer && ci && co, "mul_cleanup: null input");
    OwnedOp a, b, res;
    SG_TRY(symgpu_op_upload(inner, ci, Ni, Wq, a.slot()));
    SG_TRY(symgpu_op_upload(outer, co, No, Wq, b.slot()));
    SG_TRY(symgpu_mul_cleanup_dev(a.op, b.op, inner_is_left, thr, use_thr, res.slot()));
    a.reset(); b.reset();
    return finish_to_host(res, "output capacity", out_rows, out_coeff, capacity, n_out);
}

}  // extern "C"
