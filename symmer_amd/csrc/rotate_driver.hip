// rotate_driver.hip — single-Pauli rotation (reference: PauliwordOp._rotate_by_single_Pword,
// symmer/operators/base.py:1090-1161) as ONE fused device pass over a device-resident operator.
//
//   R(t) P R(t)^+ = P                        if [P, Q] = 0
//                 = cos(t) P + sin(t)(-i P Q) if {P, Q} = 0
//
// analyze : per row, anticommutation parity with Q and the phase exponent e of P*Q
//           (e = (3(Y_P+Y_Q) + Y_out + 2|x_P & z_Q|) mod 4), G lanes per row, xor/popcount + shuffles.
// scan    : positions of anticommuting rows (exclusive scan of flags).
// build   : non-Clifford: stack [commuting | cos * anticommuting | (-i sin) i^e * (anticommuting ^ Q)] in the
//           reference's order (base.py:1158-1161), then first-occurrence cleanup (cleanup_driver.hip) merges P^Q
//           partners; Clifford (angle = k*pi/2): [rotated anticommuting | commuting], no merge (base.py:1139-1154);
//           odd k: row ^ Q with c * i^e * (-i), k in {2,3}: negated (k is NOT reduced mod 4, base.py:1148).
// Equivalent to the reference's three intermediate cleanups when the input has no duplicate rows
// (every operator that left cleanup() qualifies).  Inputs WITH duplicate rows: the non-Clifford path
// detects them in its hash insert and falls back to stack + cleanup; the odd-k Clifford path forms anticom_self * Q
// through __mul__ in the reference (base.py:1143), which merges duplicate product rows and thresholds the SUMS — so an
// operator not known to be duplicate-free (symgpu_op_s::dup_free) is checked once with the same hash insert, and if
// duplicates exist the rotated anticommuting part goes through cleanup before the commuting rows are appended.
//
// This file reads the switches, plans a call and runs its stages: rotate_common.h lists the files that hold them.
#include "rotate_common.h"
#include <stdlib.h>

namespace symgpu {

// chain: the switches of a run of Clifford rotations, else those of a single rotation (the other half keeps its defaults) — every getenv
// scans the whole environment, and the one-launch rotation is short enough for that to show
static RotateSwitches read_rotate_switches(bool chain) {
    RotateSwitches sw;
    const char *e = nullptr;
    if (!chain) {
        sw.general = getenv("SYMGPU_ROTATE_GENERAL") != nullptr;
        if ((e = getenv("SYMGPU_ROT_RESIDENT"))) sw.resident = e[0] == '0' ? 0 : e[0] == '2' ? 2 : e[0] == '3' ? 3 : 1;
        if ((e = getenv("SYMGPU_ROT_HBM"))) sw.hbm = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    } else {
        if ((e = getenv("SYMGPU_CHAIN_REG"))) sw.chain_reg = e[0] != '0';
        if ((e = getenv("SYMGPU_CHAIN_LOCAL_T"))) {
            sw.local_t_set = true;
            sw.local_t = atoll(e);
            if (sw.local_t > CHAIN_TMAX) sw.local_t = CHAIN_TMAX;
        }
        if ((e = SG_TUNE("SYMGPU_CHAIN_LDS"))) sw.chain_lds = e[0] != '0';
        if ((e = SG_TUNE("SYMGPU_CHAIN_TWO"))) sw.chain_two = e[0] != '0';
        if ((e = SG_TUNE("SYMGPU_CHAIN_TWO_T"))) sw.chain_two_t = atoll(e);
    }
    if ((e = SG_TUNE("SYMGPU_ROT_CHUNKS"))) sw.chunks = e[0] != '0';
    if ((e = SG_TUNE("SYMGPU_ROT_ANALYZE_CAP"))) sw.analyze_cap = atoll(e);
    return sw;
}

// The stages of one single rotation, in this order.  A stage that runs either completes the call or hands on to the next; what sends a
// call on is found at run time (a failed verification of the one-launch kernel, duplicate rows found by the join or the check).
struct RotationPlan {
    bool fits_join;          // the 22-bit row index of a join-table entry holds every row
    ResidentPlan resident;   // one persistent launch, if the operator qualifies: geometry and residency form
    bool join;               // non-Clifford: hash join
    bool dup_check;          // odd-k Clifford of an operator not known to be duplicate-free: join-table insert and read-back first
    bool clifford_fast;      // Clifford: classify, scan, write (unless the check found duplicate rows)
    // every other call: analysis, then the general stack + cleanup
};

static RotationPlan plan_rotation(symgpu_op_t in, int clifford_k, const RotateSwitches &sw) {
    RotationPlan pl;
    const bool clifford = clifford_k >= 0;
    // odd multiples of pi/2 multiply by Q through the reference's __mul__ (merge + threshold on sums): the per-row fast path is
    // only the same thing for an operator without duplicate rows
    const bool may_merge = clifford && (clifford_k & 1) && !in->dup_free;
    pl.fits_join = in->T < JOIN_MAX_T;
    if (!sw.general) pl.resident = plan_resident(in->T, in->Wq, in->dup_free != 0, clifford_k, ctx().num_cu, sw);
    pl.join = !clifford && !sw.general && pl.fits_join;
    pl.dup_check = may_merge && !sw.general && pl.fits_join;
    pl.clifford_fast = clifford && !sw.general && in->T <= SCAN_MAX_T && (!may_merge || pl.fits_join);   // too large to check: merging path
    return pl;
}

// The form of a run of Clifford rotations (T > 0 rows, K > 0 rotations).
enum class ChainForm { Registers, Lds, SingleWorkgroup, TwoLaunch, FourLaunch };
constexpr symgpu_counter counter_of(ChainForm f) { return (symgpu_counter)(SYMGPU_CTR_CHAIN_REGISTERS + (int)f); }   // runs by form
static_assert(counter_of(ChainForm::Registers) == SYMGPU_CTR_CHAIN_REGISTERS && counter_of(ChainForm::Lds) == SYMGPU_CTR_CHAIN_LDS &&
              counter_of(ChainForm::SingleWorkgroup) == SYMGPU_CTR_CHAIN_SINGLE_WORKGROUP && counter_of(ChainForm::TwoLaunch) == SYMGPU_CTR_CHAIN_TWO_LAUNCHES &&
              counter_of(ChainForm::FourLaunch) == SYMGPU_CTR_CHAIN_FOUR_LAUNCHES, "ChainForm and its counters are in one order");

static ChainForm plan_chain(i64 T, int Wq, const RotateSwitches &sw) {
    const int W = 2 * Wq;
    const bool regs = clifford_chain_registers_applicable(T, Wq, sw.chain_reg);
    // the whole run with the rows in registers and ONE sort of the accumulated partition bits per 40 rotations (rotate_chain.hip):
    // faster than every other form at every size (1 term: 0.5 us per rotation against 1.6 of the LDS-resident kernel, 128 terms:
    // 1.2 against 3.7, 10^5 terms: 5.3 against 22.9 of the two-launch form)
    if (regs && !sw.local_t_set) return ChainForm::Registers;
    if (sw.chain_lds && T <= sw.local_t && T <= CHAIN_LDS_T && W <= 128 && (size_t)2 * T * W * 8 <= 128 * 1024 && chain_lds_attr_ok())
        return ChainForm::Lds;
    if (T <= sw.local_t) return ChainForm::SingleWorkgroup;
    if (regs) return ChainForm::Registers;        // SYMGPU_CHAIN_LOCAL_T set and T above it: the tests' way to the register chain
    if (sw.chain_two && Wq <= 64 && (Wq & (Wq - 1)) == 0 && T <= sw.chain_two_t) return ChainForm::TwoLaunch;
    return ChainForm::FourLaunch;
}

// which form served the run is counted here and nowhere else
static int run_chain(ChainForm form, const ChainRun &c, int *in_b) {
    bump_counter(counter_of(form));
    switch (form) {
        case ChainForm::Registers: return chain_registers(c, in_b);
        case ChainForm::Lds: return chain_lds(c, in_b);
        case ChainForm::SingleWorkgroup: return chain_single_workgroup(c, in_b);
        case ChainForm::TwoLaunch: return chain_two_launch(c, in_b);
        default: return chain_four_launch(c, in_b);
    }
}

// The operator 0 * I (one identity row, coefficient 0): what the reference's cleanup() makes of an operator without terms (base.py:631-632)
static int zero_identity_op(int Wq, symgpu_op_t *out) {
    OwnedOp z;
    SG_TRY(z.alloc(1, 1, Wq, true));
    hipStream_t st = ctx().stream;
    HIP_TRY(hipMemsetAsync(z->rows, 0, (size_t)2 * Wq * 8, st));
    HIP_TRY(hipMemsetAsync(z->coeff, 0, 16, st));
    HIP_TRY(hipStreamSynchronize(st));
    z.hand_out(out);
    return SYMGPU_OK;
}

// does any row of `op` commute with the row q (host)?  Only asked when a non-Clifford rotation has left no term at all.
static int any_row_commutes(symgpu_op_t op, const u64 *q_host, bool *any) {
    OwnedOp q;
    SG_TRY(symgpu_op_upload(q_host, nullptr, 1, op->Wq, q.slot()));
    Scratch flags;
    SG_TRY(flags.alloc((size_t)op->T));
    SG_TRY(symgpu_commutes_dev(op, 0, op->T, q.op, flags.as<uint8_t>()));
    uint64_t sum = 0;
    SG_TRY(symgpu_dev_checksum_u8(flags.as<uint8_t>(), op->T, &sum));
    *any = sum != 0;
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_rotate_single_dev_n(symgpu_op_t in, const uint64_t *q_row_host, double cos_t, double sin_t, int clifford_k, double thr,
                               symgpu_op_t *out, int *all_commute, int64_t *n_out) {
    SG_ENTER(in);
    SG_REQUIRE(n_out, "rotate_single_dev_n: null argument");
    *n_out = 0;
    SG_TRY(symgpu_rotate_single_dev(in, q_row_host, cos_t, sin_t, clifford_k, thr, out, all_commute));
    if (*out) *n_out = (*out)->T;
    return SYMGPU_OK;
}

int symgpu_rotate_single_dev(symgpu_op_t in, const uint64_t *q_row_host, double cos_t, double sin_t, int clifford_k, double thr,
                             symgpu_op_t *out, int *all_commute) {
    SG_ENTER(in);
    SG_REQUIRE(in && q_row_host && out && all_commute, "rotate_single_dev: null argument");
    SG_REQUIRE(in->coeff || in->T == 0, "rotate_single_dev: operator has no coefficients");
    const i64 T = in->T;
    *out = nullptr;                                                  // stages that do not complete the call leave both as they are
    *all_commute = 1;
    if (T == 0) return SYMGPU_OK;
    SG_REQUIRE(T < ((i64)1 << 31), "rotate_single_dev: too many rows");
    const RotateSwitches sw = read_rotate_switches(false);
    const RotationPlan pl = plan_rotation(in, clifford_k, sw);
    int done = 0;
    if (pl.resident.applicable) {
        SG_TRY(rotate_resident_try(in, q_row_host, cos_t, sin_t, clifford_k, thr, sw, pl.resident, out, all_commute, &done));
        if (done) return SYMGPU_OK;
    }
    RotationRun r{in, q_row_host, cos_t, sin_t, thr, clifford_k, sw, out, all_commute};
    SG_TRY(r.q.alloc((size_t)2 * in->Wq * 8));
    SG_TRY(r.anti.alloc((size_t)T * 4));
    SG_TRY(r.ph.alloc((size_t)T));
    // exactly one analysis launch; Q reaches the device with it (in its kernel arguments when the row has <= 64 words)
    if (pl.join) {
        SG_TRY(rotate_join(r, &done));
        if (done) { bump_counter(SYMGPU_CTR_ROTATE_HASH_JOIN); return SYMGPU_OK; }            // else duplicate rows: the general stage
    } else if (pl.dup_check) {
        SG_TRY(rotate_dup_check(r));
    } else {
        SG_TRY(analyze_rows(in, r.q.as<u64>(), r.anti.as<u32>(), r.ph.as<uint8_t>(), nullptr, sw, q_row_host));
    }
    // the stage that completed the rotation is counted: the hash join above, the Clifford fast path, the general path, and of the last
    // the rotations whose duplicate check found two equal rows (the one-launch kernel counts its own: SYMGPU_CTR_RESIDENT_DONE)
    if (pl.clifford_fast && !r.has_dup) {
        SG_TRY(rotate_clifford_fast(r));
        bump_counter(SYMGPU_CTR_ROTATE_CLIFFORD_FAST);
        return SYMGPU_OK;
    }
    SG_TRY(rotate_general(r));
    bump_counter(SYMGPU_CTR_ROTATE_GENERAL);
    if (pl.dup_check && r.has_dup) bump_counter(SYMGPU_CTR_ROTATE_GENERAL_BY_DUP_CHECK);
    return SYMGPU_OK;
}

int symgpu_perform_rotations_dev(symgpu_op_t in, const uint64_t *q_rows_host, const double *cos_t, const double *sin_t, const int *ks_host, int64_t K,
                                 double thr, int clean, symgpu_op_t *out, uint8_t *acted, int64_t *n_done, int *clean_out) {
    SG_ENTER(in);
    SG_REQUIRE(in && out && n_done && clean_out && K >= 0 && (K == 0 || (q_rows_host && cos_t && sin_t && ks_host)), "perform_rotations_dev: null argument");
    const int W = 2 * in->Wq;
    OwnedOp mine;                                                    // the operator after the steps so far; empty while that is still `in`
    *out = nullptr;
    i64 step = 0;
    while (step < K) {
        const symgpu_op_t cur = mine ? mine.op : in;
        if (cur->T == 0) {
            // every rotation is the identity on an operator without terms (np.all of an empty mask, base.py:1130-1133) and the
            // cleanup() that follows it returns 0 * I (base.py:631-632); the next step's cleanup() drops that term again
            symgpu_op_t z = nullptr;
            SG_TRY(zero_identity_op(in->Wq, &z));
            mine.adopt(z);
            clean = 0;
            ++step;
            continue;
        }
        if (clean && cur->T <= ((i64)1 << 22) && ks_host[step] >= 0) {
            // a run of Clifford rotations of a clean operator: no step drops or merges anything, so the reference's per-step cleanup()
            // is the identity and the whole run goes to the chain entry point
            i64 e = step;
            while (e < K && ks_host[e] >= 0) ++e;
            symgpu_op_t res = nullptr;
            SG_TRY(symgpu_rotate_clifford_chain_dev(cur, q_rows_host + step * W, ks_host + step, e - step, &res));
            mine.adopt(res);
            step = e;
            continue;
        }
        OwnedOp res;
        int allc = 1;
        SG_TRY(symgpu_rotate_single_dev(cur, q_rows_host + step * W, cos_t[step], sin_t[step], ks_host[step], thr, res.slot(), &allc));
        if (!allc && res && res->T == 0) {
            // The rotation itself has left no term.  Clifford: the rows are vstack([cleaned product, commuting rows]) = none, and the
            // cleanup() after it gives 0 * I.  Non-Clifford: the result is `commute_self + anticom_part` (base.py:1159-1161), an
            // append + cleanup that yields 0 * I when BOTH parts hold no row (then the loop's cleanup() drops its term: no terms) and
            // an operator without terms when commuting rows cancelled each other (then the loop's cleanup() gives 0 * I).
            bool zero_identity = true;
            if (ks_host[step] < 0) SG_TRY(any_row_commutes(cur, q_rows_host + step * W, &zero_identity));
            if (acted) acted[step] = 1;
            if (zero_identity) {
                SG_TRY(zero_identity_op(in->Wq, res.slot()));                // (the empty result goes first)
                clean = 0;
            } else {
                clean = 1;                                          // no terms, and the cleanup() of this step has been applied
            }
            mine.adopt(res.release());
            ++step;
            continue;
        }
        if (!allc) { if (acted) acted[step] = 1; mine.adopt(res.release()); }
        else res.reset();
        ++step;
        if (!clean) {
            symgpu_op_t cleaned = nullptr;
            SG_TRY(symgpu_cleanup_dev(mine ? mine.op : in, thr, 1, &cleaned));   // may leave no term (0 * I, or X + (-X) after an even multiple of pi/2)
            mine.adopt(cleaned);
            clean = 1;
        }
    }
    *n_done = step;
    *clean_out = clean;
    mine.hand_out(out);                                              // nullptr: the operator is unchanged, keep using `in`
    return SYMGPU_OK;
}

int symgpu_debug_rotation_trace(uint64_t *out, int max_workgroups, int *n_workgroups) {
    SG_ENTER();
    SG_REQUIRE(out && n_workgroups && max_workgroups >= 0, "debug_rotation_trace");
    return rotate_resident_trace(out, max_workgroups, n_workgroups);
}

int symgpu_rotate_single(const uint64_t *rows, const double *coeff, int64_t N, int Wq, const uint64_t *q_row, double cos_t, double sin_t,
                         int clifford_k, double thr, uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out,
                         int *all_commute) {
    SG_ENTER();
    SG_REQUIRE(N >= 0 && Wq >= 1 && q_row && all_commute && n_out, "rotate_single: arguments");
    SG_REQUIRE(N == 0 || (rows && coeff), "rotate_single: null input");
    OwnedOp in, res;
    SG_TRY(symgpu_op_upload(rows, coeff, N, Wq, in.slot()));
    SG_TRY(symgpu_rotate_single_dev(in.op, q_row, cos_t, sin_t, clifford_k, thr, res.slot(), all_commute));
    in.reset();
    if (*all_commute || !res) { *n_out = N; return SYMGPU_OK; }
    return finish_to_host(res, "rotate_single: capacity", out_rows, out_coeff, capacity, n_out);
}

int symgpu_rotate_clifford_chain_dev(symgpu_op_t in, const uint64_t *q_rows_host, const int *ks_host, int64_t K, symgpu_op_t *out) {
    SG_ENTER(in);
    SG_REQUIRE(in && out && K >= 0 && (K == 0 || (q_rows_host && ks_host)), "rotate_clifford_chain_dev: null argument");
    SG_REQUIRE(in->coeff || in->T == 0, "rotate_clifford_chain_dev: operator has no coefficients");
    SG_REQUIRE(in->dup_free, "rotate_clifford_chain_dev: the operator must come from a cleanup (no duplicate rows, |c| > threshold)");
    SG_REQUIRE(in->T <= ((i64)1 << 22), "rotate_clifford_chain_dev: more than 2^22 rows (rotate one by one)");
    for (i64 r = 0; r < K; ++r) SG_REQUIRE(ks_host[r] >= 0 && ks_host[r] <= 3, "rotate_clifford_chain_dev: k must be 0..3 (see rotation_args)");
    hipStream_t st = ctx().stream;
    const i64 T = in->T;
    const int Wq = in->Wq, W = 2 * Wq;
    *out = nullptr;
    const RotateSwitches sw = read_rotate_switches(true);
    OwnedOp a, b;                                                    // the two buffers the forms alternate between; `a` starts as the input
    SG_TRY(a.alloc(rows_or_one(T), 0, Wq, true));
    SG_TRY(b.alloc(rows_or_one(T), 0, Wq, true));
    SG_TRY(symgpu_op_copy_rows(a.op, 0, in, 0, T));
    Scratch qs, ks;
    int in_b = 0;
    if (T > 0 && K > 0) {
        SG_TRY(qs.alloc((size_t)K * W * 8));
        SG_TRY(ks.alloc((size_t)K * 4));
        HIP_TRY(hipMemcpyAsync(qs.p, q_rows_host, (size_t)K * W * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ks.p, ks_host, (size_t)K * 4, hipMemcpyHostToDevice, st));
        const ChainRun c{in, a.op, b.op, T, K, Wq, qs.as<u64>(), ks.as<int>(), ks_host, sw};
        SG_TRY(run_chain(plan_chain(T, Wq, sw), c, &in_b));          // returns with the stream synchronised
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    OwnedOp &res = in_b ? b : a;
    res->T = T;
    res->dup_free = 1;                                              // a permutation of distinct rows XORed with Q on a Q-anticommuting subset
    res.hand_out(out);
    return SYMGPU_OK;
}

}  // extern "C"
