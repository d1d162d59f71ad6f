// common.h — internal declarations shared by the libsymgpu translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/symgpu.h"

typedef uint64_t u64;
typedef int64_t i64;
typedef uint32_t u32;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

namespace symgpu {

// ---- error handling --------------------------------------------------------------------------
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return symgpu::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define SG_TRY(expr)                 \
    do {                             \
        int _rc = (expr);            \
        if (_rc != SYMGPU_OK) return _rc; \
    } while (0)

#define SG_REQUIRE(cond, msg)                       \
    do {                                            \
        if (!(cond)) {                              \
            symgpu::set_error("invalid argument: %s (%s)", msg, #cond); \
            return SYMGPU_E_INVALID;                \
        }                                           \
    } while (0)

#define KERNEL_CHECK() HIP_TRY(hipGetLastError())

// Environment switches.  The RUNTIME switches (one table: DESIGN.md, "Environment switches") are read with getenv where they act, on every
// call: each selects a path the library also takes by itself (a size limit, a refused attribute, a time-out), so that the tests can force it
// on inputs of any size.  Everything else — tuning knobs and variants that were measured slower — is compiled out of the default build:
// `make TUNING=1` (-DSYMGPU_TUNING) makes SG_TUNE read the environment again.
#ifdef SYMGPU_TUNING
#define SG_TUNE(name) getenv(name)
#else
#define SG_TUNE(name) (static_cast<const char *>(nullptr))
#endif

// ---- context ---------------------------------------------------------------------------------
struct EmitProbe { const void *key = nullptr; int phase = 0, choice = 0; u64 stamp = 0; float best[2] = {1e30f, 1e30f}; hipEvent_t ev[2] = {nullptr, nullptr}; };
// The per-device lock of a context (DeviceScope): every call that touches a context holds it for the whole call, so the calls on one device
// are serialised whole (its host state below — mail words, hash and join tables, epochs, probes — belongs to one call at a time).
// Recursive, because an entry point may call others.  Copying or assigning a context (symgpu_shutdown resets it with `c = Context()`)
// leaves the lock and its counter where they are.
struct ContextLock {
    std::recursive_mutex mu;
    std::atomic<int> inside{0};           // threads whose open calls use this context right now (SYMGPU_CTR_CTX_MAX_THREADS, context.hip ctx())
    ContextLock() {}
    ContextLock(const ContextLock &) {}
    ContextLock &operator=(const ContextLock &) { return *this; }
};
// What the one-launch rotation (rotate_resident.hip) keeps on a device between calls.
struct ResidentState {
    u64 *table = nullptr;          // join table [canonical-key tag 32 | row + 1 : 32], all-zero between launches (the kernel zeroes what it used)
    size_t table_cap = 0;          // entries (power of two)
    u32 *partner = nullptr;        // partner notes: row + 1 of the row that found this one in the table, zero between launches
    size_t partner_cap = 0;
    bool dirty = false;            // a launch did not complete: table and notes must be cleared before the next one
    u64 *state = nullptr;          // granules of the two in-launch all-gathers [tag 16 | counts 48], then {fail[0], fail[1]}, {finished, published}
    u32 epoch = 0;                 // tags the granules (2 epoch, 2 epoch + 1) and the failure words: 1 .. 16382, 0 = state to be cleared
    bool disabled = false;         // a barrier timed out once (workgroups not co-resident): the process keeps to the multi-launch paths
    u32 finished_base = 0;         // arrival counter base of the next launch (the counter runs on over the launches of an epoch range)
    u32 host_tag = 0;              // tag of the last report in pinned memory, 1 .. 65535
    u64 *trace = nullptr;          // [RES_MAX_WG][16] phase stamps of the last traced launch (SYMGPU_RES_TRACE=1) and its workgroups
    int trace_wgs = 0;
};
// What the scans and the radix sort (scan.hip, sort.hip, sort_coop.hip) keep on a device between calls; allocated on first use,
// released by sort_state_release (sort.h).
struct SortState {
    u32 *scan_ticket = nullptr;    // "last workgroup finishes the scan" tickets, zero between launches: [0] column scan of the sort, [1] exclusive scan
    u32 *coop_state = nullptr;     // one-launch sort: [0] barrier counter (monotonic over the launches; cleared before it can wrap), [1] time-out
                                   // flag, [64 ..] tile histograms
    u32 bar_base = 0;              // value of the barrier counter when the next launch starts
    bool coop_disabled = false;    // a barrier timed out once (workgroups not co-resident): the process keeps to a launch per step
};
struct Context {
    ContextLock lock;
    bool ready = false;
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;           // side stream: VALU-bound coefficient kernel overlaps the HBM-bound row stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    u32 *mail_host = nullptr, *mail_dev = nullptr;   // 64 bytes of mapped, coherent host memory: word 0 = sequence number, words 1.. = the few
    u32 mail_seq = 0;                                // status words / counts a call reads back in the middle of its work (read_back_words)
    bool mail_failed = false;
    int num_cu = 256;
    // linear-hash tables (cleanup): 8 byte positions x 256 values x {h1,h2}; reseeded on collision
    u64 *hash_tab = nullptr;       // device, [8][256][2]
    u64 hash_seed = 0;
    std::vector<u64> host_hash_tab;  // host copy of hash_tab (to hash single rows, e.g. a rotation's Q, with the SAME device's tables)
    u64 *xs_pow = nullptr;         // device, [32][64]: columns of M^(2^j), M = the hash's xorshift step (k_hash_rows_long, cleanup_hash.hip)
    // rotation hash join (rotate_analyze.hip, rotate_fast.hip): persistent open-addressing table of [tag 32 | generation 10 | row index + 1 : 22] entries.
    // An entry of another generation is empty, so the table is cleared once per 1023 rotations instead of once per rotation.
    u64 *rot_table = nullptr;
    size_t rot_table_cap = 0;      // entries (power of two)
    u32 rot_gen = 0;
    u32 *rot_flags = nullptr;      // device u32[4]: [0] = generation in which a duplicate input row was seen
    void *rot_host_cnt = nullptr, *rot_host_cnt_dev = nullptr;   // pinned host copy of a rotation's counts and its device address (rotate_analyze.hip)
    ResidentState res;             // one-launch rotation (rotate_resident.hip)
    SortState sort;                // scans and radix sort (sort.h)
    EmitProbe emit_probe[8];          // fused output stage of the cleanup: the output blocks whose block order is being / has been measured (cleanup.hip emit_order_begin)
    u64 emit_stamp = 0;
    u32 *m7_flags = nullptr;       // stream-K commutation kernel (commute_m4r7.hip): per-workgroup words compared with the launch's epoch
    u32 m7_epoch = 0;
};
// internal names shared by context.hip, alloc.hip, transfer.hip and op_handles.hip only: kept out of the library's dynamic symbols
#define SG_HIDDEN __attribute__((visibility("hidden")))
Context &ctx();                            // the calling thread's current device's context (inside a DeviceScope: counted as a use of it)
SG_HIDDEN int cur_index();                 // that device's index and nothing else: no use is counted (the allocator, require_ctx)
Context *ctx_of_device(int device);
void select_device(int device);            // this thread's current device (no HIP call; require_ctx binds the runtime)
int selected_device();
void forget_bound_device();                // after a library (RCCL) may have changed the thread's HIP device behind our back
// hipFuncSetAttribute acts on the CURRENT device's copy of a kernel, so "set once" means once per device: evaluates `expr` (-> bool) the
// first time the enclosing code runs on a device and remembers the answer for that device (the statics belong to the call site)
#define SG_DEVICE_ONCE(expr)                                                                          \
    ([&]() -> bool {                                                                                  \
        static std::atomic<u32> _done{0}, _ok{0};                                                     \
        const u32 _bit = 1u << symgpu::ctx().device;                                                  \
        if (!(_done.fetch_or(_bit) & _bit) && (expr)) _ok.fetch_or(_bit);                             \
        return (_ok.load() & _bit) != 0;                                                              \
    }())
extern std::atomic<i64> g_counters[SYMGPU_CTR_COUNT];   // debug counters (symgpu_debug_counter): one per entry of SYMGPU_COUNTER_LIST (symgpu.h)
inline void bump_counter(symgpu_counter which, i64 by = 1) { g_counters[which].fetch_add(by, std::memory_order_relaxed); }
inline void count_h2d(size_t bytes) { bump_counter(SYMGPU_CTR_H2D_BYTES, (i64)bytes); }
inline void count_d2h(size_t bytes) { bump_counter(SYMGPU_CTR_D2H_BYTES, (i64)bytes); }
int require_ctx();
// A call that is handed operator handles runs on THEIR device for its duration (and refuses handles of different devices), else on the
// thread's current device; once that device is settled the scope holds its context's lock until it ends, and the thread's own selection
// comes back.  Every exported entry point that touches a context enters one (SG_ENTER; tests/test_host_logic.py checks the sources).
// Lock order: a context lock may be held while the allocator's mutex is taken, never the reverse.
struct DeviceScope {
    int saved = -1;
    bool active = false;
    int held = -1;                 // the device whose context lock the scope holds
    u32 using_before = 0;          // the contexts this thread's outer scopes had used
    int enter(const struct ::symgpu_op_s *a = nullptr, const struct ::symgpu_op_s *b = nullptr, const struct ::symgpu_op_s *c = nullptr);
    ~DeviceScope();
};
#define SG_ENTER(...)                   \
    symgpu::DeviceScope _dev_scope;     \
    SG_TRY(_dev_scope.enter(__VA_ARGS__))
// A fast path gave up in this process (an in-kernel wait timed out because the workgroups were not co-resident — a shared or partitioned
// GPU —, or the runtime refused an LDS attribute) and a slower form has taken over: said ONCE on stderr and kept for symgpu_degraded().
void note_degraded(const char *what);

// per-launch event timing of one kernel class (bench.py roofline leg)
struct ProfScope {
    int cls; bool on;
    hipEvent_t a = nullptr, b = nullptr;
    explicit ProfScope(int kernel_class);
    ~ProfScope();
};

// alloc.hip — cached device allocator (hipMalloc is slow; rotations chain many small temporaries)
SG_HIDDEN void dev_alloc_init(int device);                        // once per device, from its init
int dev_alloc(size_t bytes, void **ptr);                          // on the CURRENT device
int dev_free(void *ptr);                                          // back to the OWNING device's lists
void dev_cache_release();                                         // the CURRENT device's parked blocks and idle arena chunks
// transfer.hip
void prefault_host(void *dst, size_t bytes);                      // touch the pages of a large D2H destination first
SG_HIDDEN int download_any(const void *dev, void *host, size_t bytes);   // device -> pageable host memory, any size; returns with the data there

// RAII scratch buffer on the cached allocator
struct Scratch {
    void *p = nullptr;
    Scratch() {}
    ~Scratch() { if (p) dev_free(p); }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    int alloc(size_t bytes) { if (p) { dev_free(p); p = nullptr; } return dev_alloc(bytes ? bytes : 16, &p); }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- launch grids ------------------------------------------------------------------------------
// workgroups of `block` threads for n elements, never none.  grid_for: at most `cap`, for kernels that stride over the grid;
// grid_each: one thread per element.
inline int grid_for(i64 n, int block = 256, int cap = 8192) {
    i64 g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
inline unsigned grid_each(i64 n, int block = 256) {
    const i64 g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace symgpu

// ---- device-resident operator ------------------------------------------------------------------
struct symgpu_op_s {
    int device = 0;          // the device whose memory holds the operator (set by symgpu_op_alloc)
    u64 *rows = nullptr;     // [capacity][2*Wq] row-major packed
    double *coeff = nullptr; // [capacity][2] or null
    i64 T = 0, capacity = 0;
    int Wq = 0;
    // cached word-major copy of rows[0..T) (layout.hip), padded to wm_pad terms; dropped whenever rows/T change
    u64 *wm = nullptr;
    i64 wm_pad = 0, wm_T = -1;
    // 1 = known to hold no two equal rows (result of a cleanup, or of a rotation of such an operator); 0 = unknown.
    // Reset by op_invalidate, i.e. whenever rows change.  The odd-k Clifford rotation needs to know (rotate_driver.hip).
    int dup_free = 0;
    // cached linear row hashes h1 of rows[0..T) under hash seed `hash_seed` (0 = none): a rotation hands them on to its result
    // for free (h(P ^ Q) = h(P) ^ h(Q)), so a chain of rotations hashes the operator once.  Dropped by op_invalidate.
    u64 *hash = nullptr;
    u64 hash_seed = 0;
    // cached bit-major copy of rows[0..T) for the Four-Russians commutation kernel (commute_m4r.hip): bt[c][jw], bt_pad words per
    // bit-row; valid while bt_T == T.  An adjacency matrix computed slab by slab transposes its right operand once.
    u64 *bt = nullptr;
    i64 bt_pad = 0, bt_T = -1;
    // cached Y counts |x & z| of rows[0..T) (product.hip: the coefficient expansion adds 3 (Y_i + Y_o) to the phase bytes);
    // valid while yc_T == T.  Dropped by op_invalidate.
    int *yc = nullptr;
    i64 yc_T = -1;
    // first[t] (optional; results of the *_indexed cleanups): the input index under which output term t was filed — its first occurrence:
    // the position of a plain cleanup's input row, (o << 32) | i of a product's pair.  Dropped by op_invalidate.
    u64 *first = nullptr;
};

namespace symgpu {

// What Scratch is for buffers, for operator handles: the one owner of a handle the library made for itself (symgpu_op_alloc, or adopted
// from symgpu_op_upload, cleanup_rows, cleanup_pairs, a nested symgpu_*_dev call).  The handle is freed when the owner goes unless it was
// handed out, so every error return may be a plain HIP_TRY / SG_TRY.  An error path may thus release a handle that queued work still
// uses, as ~Scratch does: a device's calls run on one stream, and dev_free only parks the block for a later call on that stream.
// No copies, no sharing: a handle has one owner at a time.
struct OwnedOp {
    symgpu_op_t op = nullptr;
    OwnedOp() {}
    ~OwnedOp() { reset(); }
    OwnedOp(const OwnedOp &) = delete;
    OwnedOp &operator=(const OwnedOp &) = delete;
    void reset() { if (op) symgpu_op_free(op); op = nullptr; }
    void adopt(symgpu_op_t fresh) { reset(); op = fresh; }
    symgpu_op_t *slot() { reset(); return &op; }                          // where a callee that makes a fresh handle puts it
    int alloc(i64 capacity, i64 T, int Wq, bool with_coeff) { SG_TRY(symgpu_op_alloc(capacity, Wq, with_coeff, slot())); op->T = T; return SYMGPU_OK; }
    symgpu_op_t release() { symgpu_op_t h = op; op = nullptr; return h; }
    void hand_out(symgpu_op_t *out) { *out = release(); }
    // the buffers that go with the handle (op_invalidate frees them): cached row hashes / first-occurrence indices of `capacity` rows
    int attach_hash() { return dev_alloc((size_t)op->capacity * 8 + 16, (void **)&op->hash); }
    int attach_first() { return dev_alloc((size_t)op->capacity * 8, (void **)&op->first); }
    symgpu_op_s *operator->() const { return op; }
    explicit operator bool() const { return op != nullptr; }
};
constexpr i64 rows_or_one(i64 n) { return n > 0 ? n : 1; }                // the capacity of a result of n rows: never an empty block
// a call that is handed a plan instead of an operator runs on the plan's device: the operator-shaped stand-in that SG_ENTER takes
inline symgpu_op_s scope_of_device(int device) {
    symgpu_op_s s;
    s.device = device;
    return s;
}

// layout.hip — word-major ("bit-sliced column") copy: out[w][t], t padded to Tpad (zero filled)
int to_wordmajor(const u64 *rows, i64 T, int W, u64 *out, i64 Tpad, hipStream_t st = nullptr);
// cached word-major copy of a whole operator (padded to a multiple of `mult` terms); built on the main stream
int op_wordmajor(symgpu_op_s *op, i64 mult, const u64 **out, i64 *pad);
// cached Y counts of a whole operator (int per term); built on the main stream
int op_ycount(symgpu_op_s *op, const int **out);
void op_invalidate(symgpu_op_s *op);

// the n_a + n_b <= 8 device words a[0..n_a) ++ b[0..n_b) to the host, behind everything queued on the stream so far (transfer.hip)
int read_back_words(const u32 *a, int n_a, const u32 *b, int n_b, u32 *host_out, const u32 *c1 = nullptr);
struct ReadBack { int n; u32 seq; u32 plain[8]; };
int read_back_post(const u32 *a, int n_a, const u32 *b, int n_b, ReadBack *rb, const u32 *c1 = nullptr /* one more word */);   // ... more work may be queued before the wait
int read_back_wait(ReadBack *rb, u32 *host_out);

// commute_driver.hip (what the commutation files share among themselves: commute_common.h)
// b_owner (may be null): the operator B's rows belong to (all of them), so that per-operand layouts can be cached on it
int commutes_dev(const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits, symgpu_op_s *b_owner = nullptr);
// ycount.hip
int ycount_dev(const u64 *rows, i64 T, int Wq, int *out);
// scan.hip — *out = 0 + v[0] + v[1] + ... + v[N - 1], added in that order per component (one wavefront: the order IS the contract)
int ordered_sum_dev(const f64x2 *v, i64 N, f64x2 *out);

// product.hip, product_pairs.hip, product_driver.hip (what they share among themselves: product_common.h)
// ---- shared device helpers ----------------------------------------------------------------------
// first position in the ascending v[0..n) holding a value >= key
template <typename T, typename I>
__device__ __forceinline__ I lower_bound(const T *v, I n, u64 key) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((u64)v[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// exact phase application: multiply (re, im) by i^e
__device__ __forceinline__ void apply_phase(double re, double im, int e, double &ore, double &oim) {
    const bool swap = e & 1;
    double a = swap ? im : re, b = swap ? re : im;
    // e=0: ( re,  im)  e=1: (-im,  re)  e=2: (-re, -im)  e=3: ( im, -re)
    const bool neg_a = (e == 1) || (e == 2), neg_b = (e == 2) || (e == 3);
    ore = neg_a ? -a : a;
    oim = neg_b ? -b : b;
}
// |re + i im| as NumPy's complex abs forms it (its SIMD loop, x86-64 with FMA): an infinite component gives inf, else a NaN gives NaN,
// else max * sqrt(fma(r, r, 1)) with r = min / max, every step correctly rounded.  It is not libm's hypot: the two differ by an ulp
// on about one coefficient in ten, and an ulp at |c| ~ thr decides whether a row is kept (tests/test_gpu_coeff_edges.py).
__device__ __forceinline__ double numpy_cabs(double re, double im) {
    const double a = fabs(re), b = fabs(im);
    if (a == __builtin_inf() || b == __builtin_inf()) return __builtin_inf();
    if (a != a || b != b) return __builtin_nan("");
    const double big = a > b ? a : b, small = a > b ? b : a;
    if (big == 0.0) return 0.0;
    const double r = __ddiv_rn(small, big);
    return __dmul_rn(__dsqrt_rn(__fma_rn(r, r, 1.0)), big);
}
// the keep rule of every cleanup and rotation: NumPy's np.abs(c) > thr (strict; NaN is dropped).  A component above thr decides it
// without the division when the other component is a number (|c| >= either component); with a NaN beside it only an inf keeps the term.
__device__ __forceinline__ bool above_thr(double re, double im, double thr) {
    const double a = fabs(re), b = fabs(im);
    if ((a > thr && b == b) || (b > thr && a == a)) return true;
    return numpy_cabs(a, b) > thr;
}
// plain IEEE complex product (no FMA contraction: matches numpy for exactly representable inputs) times i^e
__device__ __forceinline__ void pair_coefficient(double ar, double ai, double br, double bi, int e, double &ore, double &oim) {
    const double re = __dsub_rn(__dmul_rn(ar, br), __dmul_rn(ai, bi));
    const double im = __dadd_rn(__dmul_rn(ar, bi), __dmul_rn(ai, br));
    apply_phase(re, im, e, ore, oim);
}

// packed pair key of the fused product + cleanup: [hash: 64-F bits][e: 2][o: bo][i: bi], F = bi + bo + 2 (cleanup_common.h)
struct PairKeyArgs {
    const u64 *hI, *hO;     // per-operand row hashes
    u64 *keys;              // [No*Ni] out, index o*Ni + i  (squared mode: compacted, see below)
    int bi, bo;
    i64 o_base;             // absolute index of the launch's first outer row
    // squared mode (P * P, cleanup_driver.hip): only the pairs with i >= o get a key (the twin (o, i) of an off-diagonal pair is the
    // same row with the same or the opposite coefficient), compacted in pair-index order: slot(o, i) = o*Ni - o(o-1)/2 + (i - o)
    int squared = 0;
    // round 6, ebytes != null: instead of the 8-byte key ONE byte per pair at the key's index, e | (i == o) << 2 — all that the marking of
    // the single terms reads when the pairs that share a key are found from the operand hash tables (pair_dups.hip); `keys` is not written
    unsigned char *ebytes = nullptr;
};

int mul_coeff_dev(const u64 *inner, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end,
                  int Wq, int inner_is_left, double *out_coeff);
// packed (hash | phase exponent | o | i) keys of all pairs, for the fused product + cleanup
int mul_keys_dev(const u64 *inner, i64 Ni, const u64 *outer, i64 No, int Wq, int inner_is_left, PairKeyArgs ka);

// wide.hip — few pairs of very long rows: the word axis is the parallel one
bool wide_pairs_worthwhile(i64 Ni, i64 No, int Wq);
int wide_commutes_dev(const u64 *A, i64 N, const u64 *B, i64 M, int Wq, uint8_t *out, u64 *out_bits);
int wide_mul_coeff_dev(const u64 *inner, const double *ci, i64 Ni, const u64 *outer, const double *co, i64 o_begin, i64 o_end, int Wq,
                       int inner_is_left, double *out_coeff, const PairKeyArgs *keys);

// cleanup_hash.hip, cleanup_driver.hip
int ensure_hash_tables(u64 seed);
int hash_rows(const u64 *rows, i64 T, int W, u64 *out1);       // h1 of every row (current tables)
u64 host_row_hash(const u64 *row, int W);                       // the same hash on the host
// product + cleanup: term t = o * Ni + i is inner[i] ^ outer[o] with coefficient ci[i] * co[o] * i^e (product.hip)
struct PairOperands {
    const u64 *inner = nullptr, *outer = nullptr;
    const double *ci = nullptr, *co = nullptr;
    i64 Ni = 0, No = 0;
    int W = 0, Wq_out = 0;                                      // words of an operand row (2 * Wq) / chunks of a result row
    int inner_is_left = 1;
};
// *out is a fresh operator with the cleaned result; want_first: it carries symgpu_op_s::first
int cleanup_rows(const u64 *rows, const double *coeff, i64 T, int W, double thr, int use_thr, symgpu_op_t *out, int Wq_out, bool want_first = false);
int cleanup_pairs(const PairOperands &p, double thr, int use_thr, symgpu_op_t *out, bool want_first = false);
// the tail of the calls that take and return host arrays: *n_out, the capacity check (`what`: the call's words for it), the download
int finish_to_host(OwnedOp &res, const char *what, uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out);

// pair_dups.hip — the pairs of a product whose 64-bit key another pair shares, found without sorting the keys
bool pair_dups_fits(i64 Ni, i64 No, bool squared, i64 Tk, int *B_out, int *sb_out = nullptr);      // host-side: would pair_dups_dev take this product?
// why the pass gave up: the bits k_pd_bucket / k_pair_dups raise in *giveup, and the counter of each (order_flagged, cleanup_keys.hip)
constexpr u32 PD_GIVEUP_PRODUCT_BUCKET = 1u, PD_GIVEUP_COUNTER_SATURATED = 2u, PD_GIVEUP_LIST_OVERFLOW = 4u, PD_GIVEUP_OPERAND_BUCKET = 8u;
constexpr u32 PD_GIVEUP_BITS[4] = {PD_GIVEUP_PRODUCT_BUCKET, PD_GIVEUP_COUNTER_SATURATED, PD_GIVEUP_LIST_OVERFLOW, PD_GIVEUP_OPERAND_BUCKET};
constexpr symgpu_counter counter_of_giveup(u32 bit) { return (symgpu_counter)(SYMGPU_CTR_GIVEUP_PRODUCT_BUCKET + __builtin_ctz(bit)); }
static_assert(counter_of_giveup(PD_GIVEUP_PRODUCT_BUCKET) == SYMGPU_CTR_GIVEUP_PRODUCT_BUCKET &&
              counter_of_giveup(PD_GIVEUP_COUNTER_SATURATED) == SYMGPU_CTR_GIVEUP_COUNTER_SATURATED &&
              counter_of_giveup(PD_GIVEUP_LIST_OVERFLOW) == SYMGPU_CTR_GIVEUP_LIST_OVERFLOW &&
              counter_of_giveup(PD_GIVEUP_OPERAND_BUCKET) == SYMGPU_CTR_GIVEUP_OPERAND_BUCKET, "the give-up bits and their counters are in one order");
int pair_dups_dev(const u64 *hI, i64 Ni, const u64 *hO, i64 No, bool squared, i64 Tk, u64 *flags, u32 *giveup, bool *applies);

// gf2.hip
int rref_dev(u64 *rows, i64 R, i64 Wc, i64 *xor_count, i64 *pivots_host);

}  // namespace symgpu
