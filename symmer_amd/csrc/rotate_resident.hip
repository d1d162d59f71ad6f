// rotate_resident.hip — the host side of the one-launch rotation (the kernel and what it computes: rotate_resident_kernel.hip): the plan of
// a call, and rotate_resident_try as its stages — row hashes, per-device state, kernel arguments, launch, the wait for the report, the result.
// Preconditions (plan_resident; else the call takes the multi-launch paths): the operator is known to be duplicate free
// (symgpu_op_s::dup_free) where rows could merge, has rows of <= 128 words (4,096 qubits), and the per-row state of a block fits the LDS
// (the rows themselves may stay in memory).
#include "rotate_resident.h"
#include <time.h>
#include <stdlib.h>

namespace symgpu {

static inline i64 host_ns() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (i64)ts.tv_sec * 1000000000LL + ts.tv_nsec; }

ResidentPlan plan_resident(i64 T, int Wq, bool dup_free, int clifford_k, int num_cu, const RotateSwitches &sw) {
    ResidentPlan p;
    if (T < 1 || 2 * Wq > RES_MAX_W || T >= JOIN_MAX_T) return p;
    const bool clifford = clifford_k >= 0;
    if ((!clifford || (clifford_k & 1)) && !dup_free) return p;                  // merges possible: the multi-launch paths check / handle them
    // geometry: at most one workgroup per CU, at least RES_MIN_ROWS rows each
    i64 G = (T + RES_MIN_ROWS - 1) / RES_MIN_ROWS;
    const i64 gmax = num_cu < RES_MAX_WG ? num_cu : RES_MAX_WG;
    if (G > gmax) G = gmax;
    const i64 R = (T + G - 1) / G;
    G = (T + R - 1) / R;
    if (R > RES_MAX_R) return p;                                                 // (implied by the layout below: 26 bytes of state a row bound R at 6,178)
    p.G = (int)G; p.R = (int)R;
    // the rows of the block in LDS; if they do not fit, the first two 1,024-chunk rounds of the load stay in registers (+32 KB per CU:
    // 1.46e5 -> 1.76e5 terms of 1,000 qubits — the operator a repeated rotation of 1e5 terms grows into, 1.5e5, is resident)
    const bool pow2 = Wq <= RES_REG_MAX_WQ && (Wq & (Wq - 1)) == 0;
    ResLayout L = res_layout(p.R, Wq, 0);
    if ((size_t)L.total > RES_LDS_MAX && pow2) { p.form = ResidentForm::Registers; p.nreg = RES_REG_ROUNDS; L = res_layout(p.R, Wq, p.nreg); }
    // beyond that: only the 26 bytes per row stay on the chip, the rows are read a second time when they are written out — 1e5 terms
    // of 2,000 qubits (51 MB): 73 us on the multi-launch path, see DESIGN 3.4
    if (((size_t)L.total > RES_LDS_MAX && sw.hbm != 0) || sw.hbm == 2) { p.form = ResidentForm::RowsInMemory; p.nreg = 0; p.hbm = 1; L = res_layout(p.R, Wq, 0, 1); }
    if ((size_t)L.total > RES_LDS_MAX) return p;
    p.lds_bytes = L.total;
    p.GA = row_lanes(Wq);
    p.applicable = true;
    return p;
}

int rotate_resident_trace(u64 *out, int max_wgs, int *n_wgs) {
    const ResidentState &s = ctx().res;
    if (!s.trace) { *n_wgs = 0; return SYMGPU_OK; }
    const int n = s.trace_wgs < max_wgs ? s.trace_wgs : max_wgs;
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    HIP_TRY(hipMemcpy(out, s.trace, (size_t)n * 16 * 8, hipMemcpyDeviceToHost));
    *n_wgs = n;
    return SYMGPU_OK;
}

// a duplicate-free operator without cached hashes (straight from a cleanup): hash its rows once, on the handle
static int ensure_row_hashes(symgpu_op_t in) {
    Context &c = ctx();
    SG_TRY(ensure_hash_tables(c.hash_tab ? c.hash_seed : 1));
    if (in->hash) { dev_free(in->hash); in->hash = nullptr; }
    SG_TRY(dev_alloc((size_t)in->capacity * 8 + 16, (void **)&in->hash));
    in->hash_seed = c.hash_seed;
    bump_counter(SYMGPU_CTR_OP_ROW_HASH_BUILDS);
    return hash_rows(in->rows, in->T, 2 * in->Wq, in->hash);
}

// `*buf` holds at least `want` elements of `elem` bytes, all zero: grown (to a power of two >= 4096) and cleared, or cleared after a
// launch that did not complete
static int zeroed_capacity(void **buf, size_t *cap, size_t want, size_t elem, bool dirty, hipStream_t st) {
    if (want > *cap) {
        if (*buf) { HIP_TRY(hipStreamSynchronize(st)); (void)hipFree(*buf); *buf = nullptr; *cap = 0; }
        size_t n = 4096;
        while (n < want) n <<= 1;
        HIP_TRY(hipMalloc(buf, n * elem));
        *cap = n;
        HIP_TRY(hipMemsetAsync(*buf, 0, n * elem, st));
    } else if (dirty) {
        HIP_TRY(hipMemsetAsync(*buf, 0, *cap * elem, st));
    }
    return SYMGPU_OK;
}

// The device's state for this launch: granules and failure words under a fresh epoch; non-Clifford: the join table (>= 4 slots per row)
// and the partner notes, all-zero; the trace buffer if asked for.  Fills the fields of `a` that point into it.
static int prepare_state(ResidentState &s, i64 T, int G, bool clifford, hipStream_t st, ResArgs &a) {
    if (!s.state) {
        HIP_TRY(hipMalloc((void **)&s.state, RES_STATE_WORDS * 8));
        s.epoch = 0;
    }
    if (s.epoch == 0 || s.epoch >= 16382) {                                       // fresh state, or the 16-bit granule tag wraps
        HIP_TRY(hipMemsetAsync(s.state, 0, RES_STATE_WORDS * 8, st));
        s.epoch = 0;
        s.finished_base = 0;
    }
    ++s.epoch;
    a.slots = nullptr; a.mask = 0; a.partner = nullptr;
    if (!clifford) {
        static const int slots_per_row = [] { const char *e = SG_TUNE("SYMGPU_RES_SLOTS"); const int v = e ? atoi(e) : 4; return v >= 2 && v <= 64 ? v : 4; }();
        size_t cap = 4096;
        while ((i64)cap < (i64)slots_per_row * T) cap <<= 1;
        SG_TRY(zeroed_capacity((void **)&s.table, &s.table_cap, cap, 8, s.dirty, st));
        SG_TRY(zeroed_capacity((void **)&s.partner, &s.partner_cap, (size_t)T, 4, s.dirty, st));
        s.dirty = false;
        a.slots = s.table; a.mask = (u32)(cap - 1); a.partner = s.partner;
    }
    a.gran1 = s.state; a.gran2 = s.state + RES_MAX_WG; a.fail = reinterpret_cast<u32 *>(s.state + 2 * RES_MAX_WG);
    a.finished = a.fail + 2; a.published = a.fail + 3;
    s.finished_base += (u32)G;
    a.finish_target = s.finished_base;
    a.epoch = s.epoch;
    a.trace = nullptr;
    if (const char *e = SG_TUNE("SYMGPU_RES_TRACE")) if (e[0] == '1') {
        if (!s.trace) { HIP_TRY(hipMalloc((void **)&s.trace, RES_TRACE_BYTES)); }
        HIP_TRY(hipMemsetAsync(s.trace, 0, RES_TRACE_BYTES, st));
        a.trace = s.trace;
        s.trace_wgs = G;
    }
    return SYMGPU_OK;
}

// everything of the kernel's arguments that the call and its plan decide (prepare_state: the device's state; the caller: the report
// words and the result's buffers)
static void fill_args(symgpu_op_t in, const u64 *q_host, double cos_t, double sin_t, int clifford_k, double thr, const RotateSwitches &sw,
                      const ResidentPlan &p, bool have_hash, ResArgs &a) {
    const int Wq = in->Wq, W = 2 * Wq;
    a.rows = reinterpret_cast<const u32x4 *>(in->rows); a.coeff = in->coeff; a.hin = have_hash ? in->hash : nullptr;
    a.T = in->T; a.Wq = Wq; a.R = p.R; a.GA = p.GA; a.nreg = p.nreg; a.hbm = p.hbm;
    a.yq = 0;
    for (int ww = 0; ww < Wq; ++ww) a.yq += (u32)__builtin_popcountll(q_host[ww] & q_host[Wq + ww]);
    a.cos_t = cos_t; a.sin_t = sin_t; a.thr = thr; a.k = clifford_k;
    a.hq = have_hash ? host_row_hash(q_host, W) : 0;
    a.inject = sw.resident == 3 ? 1 : 0;                                          // tests: the kernel reports a failed verification
    for (int ww = 0; ww < RES_MAX_W; ++ww) a.q.w[ww] = ww < W ? q_host[ww] : 0ULL;
}

// both words of the report carry this call's tag
static inline bool report_seen(const volatile u64 *host_words, u32 tag, u64 &w0, u64 &w1) {
    w0 = __atomic_load_n(host_words, __ATOMIC_ACQUIRE); w1 = __atomic_load_n(host_words + 1, __ATOMIC_ACQUIRE);
    return (u32)(w0 >> 48) == tag && (u32)(w1 >> 48) == tag;
}

// One workgroup reports the counts as soon as they are final (after the second all-gather, while the rows are still being written):
// poll the two tagged words in pinned memory instead of synchronising the stream — whatever the caller enqueues next is stream
// ordered behind the kernel, and its preparation overlaps the kernel's tail.  The kernel gives up by itself after ~1 s and then
// reports a failure code from its last workgroup; no report although the stream is idle: failure (code 1).
static hipError_t await_report(hipStream_t st, const volatile u64 *host_words, u32 tag, RotCounts *hc) {
    hipError_t e = hipSuccess;
    u64 w0 = 0, w1 = 0;
    bool seen = false;
    for (u64 spin = 0; spin < (1ULL << 34); ++spin) {
        if ((seen = report_seen(host_words, tag, w0, w1))) break;
        if ((spin & 0xFFFFF) == 0xFFFFF) {
            const hipError_t qe = hipStreamQuery(st);
            if (qe != hipErrorNotReady) {                                        // finished (or failed): one last look
                if (qe != hipSuccess) e = qe;
                seen = report_seen(host_words, tag, w0, w1);
                break;
            }
        }
    }
    if (!seen && e == hipSuccess) {
        e = hipStreamSynchronize(st);
        seen = report_seen(host_words, tag, w0, w1);
    }
    if (e != hipSuccess) return e;
    if (!seen) { w0 = 0; w1 = 1ULL << 44; }                                       // no report at all: code 1
    hc->nC = (u32)(w0 >> 22) & 0x3FFFFFu; hc->nA = (u32)w0 & 0x3FFFFFu; hc->nN = (u32)(w1 >> 22) & 0x3FFFFFu; hc->nAnti = (u32)w1 & 0x3FFFFFu;
    hc->dup = (u32)(w1 >> 44) & 0xFu;
    return hipSuccess;
}

// what the report says: a failure (the caller takes the multi-launch paths), the identity action, or the result
static int finish(ResidentState &s, const RotCounts &hc, symgpu_op_t in, bool clifford, OwnedOp &res, symgpu_op_t *out, int *all_commute, int *done) {
    if (hc.dup != 0) {                                                             // verification failed (2), timed out (3), or no report at all (1): res goes with its owner
        bump_counter(SYMGPU_CTR_RESIDENT_FAILED);
        if (hc.dup != 2) {                                                         // time-out: arrival counts are in an unknown state
            s.disabled = true; s.epoch = 0;
            note_degraded("one-launch rotation (k_rot_resident) off: an in-kernel wait timed out (workgroups not co-resident?); rotations take the multi-launch kernels");
        }
        // code 2 too: every owner zeroes its slot and note in phase B, but that relies on every workgroup getting there; one memset on a
        // path that is about to take the multi-launch kernels anyway makes the next launch independent of it
        s.dirty = true;
        return SYMGPU_OK;
    }
    *done = 1;
    bump_counter(SYMGPU_CTR_RESIDENT_DONE);
    if (hc.nAnti == 0) { *all_commute = 1; return SYMGPU_OK; }                     // identity action (base.py:1131-1133): res goes with its owner
    res->T = (i64)hc.nC + hc.nA + hc.nN;
    res->dup_free = clifford ? in->dup_free : 1;
    res.hand_out(out);
    *all_commute = 0;
    return SYMGPU_OK;
}

int rotate_resident_try(symgpu_op_t in, const u64 *q_host, double cos_t, double sin_t, int clifford_k, double thr, const RotateSwitches &sw,
                        const ResidentPlan &plan, symgpu_op_t *out, int *all_commute, int *done) {
    *done = 0;
    Context &c = ctx();
    ResidentState &s = c.res;
    const i64 t_enter = host_ns();
    // what the state of the process vetoes: switched off, an earlier time-out, a refused LDS size
    if (sw.resident == 0) return SYMGPU_OK;
    if (sw.resident == 2) s.disabled = false;
    if (s.disabled) return SYMGPU_OK;
    if (!resident_lds_attr_ok()) {
        (void)hipGetLastError(); s.disabled = true;
        note_degraded("one-launch rotation (k_rot_resident) off: the runtime refused its LDS size; rotations take the multi-launch kernels");
        return SYMGPU_OK;
    }
    const bool clifford = clifford_k >= 0;
    bool have_hash = in->hash && c.hash_tab && in->hash_seed == c.hash_seed;
    if (!clifford && !have_hash) { SG_TRY(ensure_row_hashes(in)); have_hash = true; }
    hipStream_t st = c.stream;
    ResArgs a;
    SG_TRY(prepare_state(s, in->T, plan.G, clifford, st, a));
    fill_args(in, q_host, cos_t, sin_t, clifford_k, thr, sw, plan, have_hash, a);
    // the report: bytes 32..55 of the context's pinned count block ([late 4 | - 4 | word0 8 | word1 8]); tags 1..65535 (the block starts zeroed)
    RotCounts *hcnt = nullptr, *hcnt_dev = nullptr;
    SG_TRY(host_counts(&hcnt, &hcnt_dev));
    volatile u32 *host_late = reinterpret_cast<u32 *>(hcnt) + 8;
    volatile u64 *host_words = reinterpret_cast<u64 *>(hcnt) + 5;
    if (*host_late != 0) {                                                        // a launch failed AFTER it had reported its counts
        s.disabled = true; s.epoch = 0; s.dirty = true;
        note_degraded("one-launch rotation (k_rot_resident) off: a launch failed after reporting; rotations take the multi-launch kernels");
        *host_late = 0;
        set_error("rotate resident: a previous launch failed after it had reported success; its result is invalid");
        return SYMGPU_E_HIP;
    }
    s.host_tag = s.host_tag >= 65535 ? 1 : s.host_tag + 1;
    a.host_late = reinterpret_cast<u32 *>(hcnt_dev) + 8; a.host_words = reinterpret_cast<u64 *>(hcnt_dev) + 5; a.host_tag = s.host_tag;
    OwnedOp res;
    SG_TRY(res.alloc(clifford ? in->T : 2 * in->T, 0, in->Wq, true));             // upper bound: no host round trip before the rows are written
    if (have_hash) {
        SG_TRY(res.attach_hash());
        res->hash_seed = in->hash_seed;
    }
    a.out_rows = reinterpret_cast<u32x4 *>(res->rows); a.out_coeff = res->coeff; a.out_hash = res->hash;
    const i64 t_launch = host_ns();
    hipError_t e = launch_resident(plan, clifford, st, a);
    const i64 t_wait = host_ns();
    bump_counter(SYMGPU_CTR_RESIDENT_NS_PREPARE, t_launch - t_enter); bump_counter(SYMGPU_CTR_RESIDENT_NS_LAUNCH, t_wait - t_launch);
    RotCounts hc;
    if (e == hipSuccess) e = await_report(st, host_words, s.host_tag, &hc);
    if (e != hipSuccess) { s.dirty = true; return hip_fail(e, "rotate resident", __FILE__, __LINE__); }
    bump_counter(SYMGPU_CTR_RESIDENT_NS_WAIT, host_ns() - t_wait);
    return finish(s, hc, in, clifford, res, out, all_commute, done);
}

}  // namespace symgpu
