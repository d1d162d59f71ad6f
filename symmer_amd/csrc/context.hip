// context.hip — error text, the per-device contexts and their lock (DeviceScope), init / shutdown, timers, profiling, debug counters.
#include "common.h"
#include "sort.h"
#include <stdarg.h>
#include <stdio.h>

namespace symgpu {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    set_error("HIP error %d (%s) in `%s` at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    return e == hipErrorOutOfMemory ? SYMGPU_E_NOMEM : SYMGPU_E_HIP;
}

// One context per DEVICE, all of them in this process (round 5: single-process multi-device mode, SURVEY 8b "one host process ... driving
// <= 8 devices").  A host thread has a CURRENT device — the one it last selected with symgpu_set_device / symgpu_init, else the
// first device initialised in the process — and everything that is not handed a handle works on it.  A call that IS handed a handle runs
// on the handle's device for its duration (DeviceScope).
static Context g_ctxs[SYMGPU_MAX_DEVICES];
static int g_default_dev = -1;                    // the first device initialised in this process
static thread_local int t_cur_dev = -1;           // this thread's selection (-1: the default)
static thread_local int t_bound_dev = -1;         // the device hipSetDevice was last called with on this thread
std::atomic<i64> g_counters[SYMGPU_CTR_COUNT] = {};
// the list holds every id 0 .. SYMGPU_CTR_COUNT - 1 once: all in range, as many as the array has slots, and no two alike (the `case` labels
// of symgpu_debug_counter_name)
#define SG_COUNTER_IN_RANGE(name, id, text) static_assert(id >= 0 && id < SYMGPU_CTR_COUNT, "SYMGPU_COUNTER_LIST: id of " #name " out of range");
#define SG_COUNTER_ONE(name, id, text) +1
SYMGPU_COUNTER_LIST(SG_COUNTER_IN_RANGE)
static_assert(0 SYMGPU_COUNTER_LIST(SG_COUNTER_ONE) == SYMGPU_CTR_COUNT, "SYMGPU_COUNTER_LIST: an id is missing");
#undef SG_COUNTER_ONE
#undef SG_COUNTER_IN_RANGE
int cur_index() { return t_cur_dev >= 0 ? t_cur_dev : (g_default_dev >= 0 ? g_default_dev : 0); }
// Use of a context inside a call, recorded where the state is used (ctx()), whatever lock the call's DeviceScope took: a thread that
// uses a context whose lock it does not hold is counted (SYMGPU_CTR_CTX_UNLOCKED_USES), and so are the threads that use one context at the
// same time (the most of them: SYMGPU_CTR_CTX_MAX_THREADS).  Calls that take no lock on purpose (symgpu_comm_*, init, shutdown) open no scope and are
// not looked at.
static thread_local int t_scopes = 0;                            // DeviceScopes open on this thread
static thread_local int t_held[SYMGPU_MAX_DEVICES] = {};         // this thread's holds on each context's lock
static thread_local u32 t_using = 0;                             // contexts the open scopes of this thread have used (bit per device)
static void note_use(int d);
Context &ctx() {
    const int d = cur_index();
    if (t_scopes > 0 && !(t_using & (1u << d))) note_use(d);
    return g_ctxs[d];
}
Context *ctx_of_device(int device) { return device >= 0 && device < SYMGPU_MAX_DEVICES ? &g_ctxs[device] : nullptr; }
void select_device(int device) { t_cur_dev = device; }
int selected_device() { return t_cur_dev; }

static std::mutex g_deg_mu;
static std::string g_degraded;
void note_degraded(const char *what) {
    std::lock_guard<std::mutex> lk(g_deg_mu);
    if (g_degraded.find(what) != std::string::npos) return;
    if (!g_degraded.empty()) g_degraded += "; ";
    g_degraded += what;
    fprintf(stderr, "symgpu: warning: %s (results are unaffected; symgpu_degraded() lists what was switched off)\n", what);
}

int require_ctx() {
    Context &c = g_ctxs[cur_index()];          // (not ctx(): DeviceScope::enter calls this before it takes the lock)
    if (!c.ready) {
        set_error("symgpu_init() has not been called for this device (or no HIP device)");
        return SYMGPU_E_NODEVICE;
    }
    // HIP's current device is per host thread and starts at 0: a thread other than the one that called symgpu_init (e.g. the
    // watchdog thread of symmer_amd/parallel.py), or one that has moved on to another context, must be bound to the context's device
    // before it touches the runtime
    if (t_bound_dev != c.device) {
        HIP_TRY(hipSetDevice(c.device));
        t_bound_dev = c.device;
    }
    return SYMGPU_OK;
}
void forget_bound_device() { t_bound_dev = -1; }

static void note_use(int d) {
    t_using |= 1u << d;
    if (t_held[d] == 0) bump_counter(SYMGPU_CTR_CTX_UNLOCKED_USES);   // the call uses a context whose lock it does not hold
    const i64 users = g_ctxs[d].lock.inside.fetch_add(1) + 1;
    i64 most = g_counters[SYMGPU_CTR_CTX_MAX_THREADS].load(std::memory_order_relaxed);
    while (users > most && !g_counters[SYMGPU_CTR_CTX_MAX_THREADS].compare_exchange_weak(most, users, std::memory_order_relaxed)) {}
}

int DeviceScope::enter(const symgpu_op_s *a, const symgpu_op_s *b, const symgpu_op_s *c) {
    saved = t_cur_dev;
    active = true;
    const symgpu_op_s *first = a ? a : (b ? b : c);
    if (first) {
        if ((b && b->device != first->device) || (c && c->device != first->device)) {
            set_error("operands live on different devices (%d and %d): copy one over with symgpu_op_copy_rows first", first->device,
                      (b && b->device != first->device) ? b->device : c->device);
            return SYMGPU_E_INVALID;
        }
        t_cur_dev = first->device;
    }
    SG_TRY(require_ctx());
    const int d = cur_index();                        // the device the call runs on: the handles', else the thread's selection
    Context &cx = g_ctxs[d];
    if (!cx.lock.mu.try_lock()) {
        bump_counter(SYMGPU_CTR_CTX_WAITS);           // another thread's call is running on this device: wait for it to end
        cx.lock.mu.lock();
    }
    held = d;
    ++t_held[d];
    using_before = t_using;
    ++t_scopes;
    return SYMGPU_OK;
}
DeviceScope::~DeviceScope() {
    if (held >= 0) {
        --t_scopes;
        for (u32 m = t_using & ~using_before; m; m &= m - 1) g_ctxs[__builtin_ctz(m)].lock.inside.fetch_sub(1);   // this scope's uses end
        t_using = using_before;
        --t_held[held];
        g_ctxs[held].lock.mu.unlock();
    }
    if (active) t_cur_dev = saved;
}

// ---- per-launch profiling ---------------------------------------------------------------------------
struct ProfClass { bool on = false; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };
static ProfClass g_prof_all[SYMGPU_MAX_DEVICES][SYMGPU_PROF_CLASSES];
static ProfClass *prof() { return g_prof_all[cur_index()]; }     // the CURRENT device's classes

ProfScope::ProfScope(int kernel_class) : cls(kernel_class), on(false) {
    if (cls < 0 || cls >= SYMGPU_PROF_CLASSES || !prof()[cls].on) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { (void)hipGetLastError(); return; }
    on = true;
    (void)hipEventRecord(a, ctx().stream);
}
ProfScope::~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(b, ctx().stream);
    prof()[cls].ev.push_back({a, b});
}

// on-box bandwidth ceilings for the roofline (one 16-byte store / load+store per thread, one-shot grid)
typedef unsigned int u32x4p __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_probe_fill(u32x4p *out, i64 n, u32 v) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (u32x4p)(v);
}
__global__ __launch_bounds__(256) void k_probe_copy(const u32x4p *in, u32x4p *out, i64 n) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i];
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

const char *symgpu_last_error(void) { return g_err; }

int symgpu_device_count(int *n) {
    if (!n) return SYMGPU_E_INVALID;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
    *n = c;
    return SYMGPU_OK;
}

static int init_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SYMGPU_E_NODEVICE;
    }
    if (device < 0 || device >= n || device >= SYMGPU_MAX_DEVICES) {
        set_error("device %d out of range (have %d, at most %d per process)", device, n, SYMGPU_MAX_DEVICES);
        return SYMGPU_E_INVALID;
    }
    Context &c = g_ctxs[device];
    if (c.ready) return SYMGPU_OK;
    HIP_TRY(hipSetDevice(device));
    t_bound_dev = device;
    HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c.stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c.ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c.ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&c.ev0));
    HIP_TRY(hipEventCreate(&c.ev1));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c.device = device;
    dev_alloc_init(device);
    c.ready = true;
    if (g_default_dev < 0) g_default_dev = device;
    return SYMGPU_OK;
}

int symgpu_init(int device) {
    // creates the device's context if it does not exist yet and makes the device this thread's current one (one process per GPU: the
    // only call a rank makes; single-process multi-device: symgpu_init_all, then symgpu_set_device)
    SG_TRY(init_device(device));
    t_cur_dev = device;
    return require_ctx();
}

int symgpu_init_all(int n_devices) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SYMGPU_E_NODEVICE;
    }
    if (n_devices <= 0 || n_devices > n) n_devices = n;
    if (n_devices > SYMGPU_MAX_DEVICES) n_devices = SYMGPU_MAX_DEVICES;
    for (int d = 0; d < n_devices; ++d) SG_TRY(init_device(d));
    // peer access both ways between every pair: symgpu_op_copy_rows between devices and RCCL's transports use it (xGMI)
    for (int a = 0; a < n_devices; ++a) {
        HIP_TRY(hipSetDevice(a));
        for (int b = 0; b < n_devices; ++b) {
            if (a == b) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(b, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            }
        }
    }
    t_bound_dev = -1;
    if (t_cur_dev < 0) t_cur_dev = g_default_dev;
    return require_ctx();
}

int symgpu_set_device(int device) {
    SG_TRY(init_device(device));
    t_cur_dev = device;
    return require_ctx();
}

int symgpu_current_device(int *device) {
    SG_REQUIRE(device, "current_device: null argument");
    *device = ctx().ready ? ctx().device : -1;
    return SYMGPU_OK;
}

int symgpu_n_initialised(int *n) {
    SG_REQUIRE(n, "n_initialised: null argument");
    int k = 0;
    for (int d = 0; d < SYMGPU_MAX_DEVICES; ++d) k += g_ctxs[d].ready ? 1 : 0;
    *n = k;
    return SYMGPU_OK;
}

static void shutdown_device(int device) {
    Context &c = g_ctxs[device];
    if (!c.ready) return;
    const int saved = t_cur_dev;
    t_cur_dev = device;
    if (hipSetDevice(device) == hipSuccess) t_bound_dev = device;
    (void)hipStreamSynchronize(c.stream);
    if (c.rot_table) { dev_free(c.rot_table); c.rot_table = nullptr; c.rot_table_cap = 0; c.rot_gen = 0; }
    dev_cache_release();
    if (c.hash_tab) { (void)hipFree(c.hash_tab); c.hash_tab = nullptr; }
    if (c.xs_pow) { (void)hipFree(c.xs_pow); c.xs_pow = nullptr; }
    if (c.rot_flags) { (void)hipFree(c.rot_flags); c.rot_flags = nullptr; }
    sort_state_release(c.sort);
    if (c.m7_flags) { (void)hipFree(c.m7_flags); c.m7_flags = nullptr; }
    for (auto &q : c.emit_probe) {
        for (auto &ev : q.ev) if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
        q = EmitProbe();
    }
    for (void *p : {(void *)c.res.table, (void *)c.res.partner, (void *)c.res.state, (void *)c.res.trace}) if (p) (void)hipFree(p);
    c.res = ResidentState();
    if (c.rot_host_cnt) { (void)hipHostFree(c.rot_host_cnt); c.rot_host_cnt = nullptr; c.rot_host_cnt_dev = nullptr; }
    (void)hipEventDestroy(c.ev0);
    (void)hipEventDestroy(c.ev1);
    (void)hipStreamSynchronize(c.stream2);
    if (c.mail_host) { (void)hipHostFree(c.mail_host); c.mail_host = nullptr; c.mail_dev = nullptr; }
    (void)hipEventDestroy(c.ev_fork);
    (void)hipEventDestroy(c.ev_join);
    (void)hipStreamDestroy(c.stream2);
    (void)hipStreamDestroy(c.stream);
    c = Context();
    t_cur_dev = saved;
}

int symgpu_shutdown(void) {
    for (int d = 0; d < SYMGPU_MAX_DEVICES; ++d) shutdown_device(d);
    g_default_dev = -1;
    t_cur_dev = -1;
    t_bound_dev = -1;
    return SYMGPU_OK;
}

int symgpu_sync(void) {
    SG_ENTER();
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

int symgpu_device_sync(void) {
    SG_ENTER();
    HIP_TRY(hipDeviceSynchronize());
    return SYMGPU_OK;
}

int symgpu_device_name(char *buf, int len) {
    SG_ENTER();
    if (!buf || len <= 0) return SYMGPU_E_INVALID;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx().device));
    // (some driver stacks leave the marketing name empty: say so instead of printing nothing)
    snprintf(buf, (size_t)len, "%s (%s, %d CUs)", prop.name[0] ? prop.name : "AMD GPU, name not reported by the driver", prop.gcnArchName, prop.multiProcessorCount);
    return SYMGPU_OK;
}

int symgpu_mem_info(int64_t *free_bytes, int64_t *total_bytes) {
    SG_ENTER();
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return SYMGPU_OK;
}

int symgpu_timer_start(void) {
    SG_ENTER();
    HIP_TRY(hipEventRecord(ctx().ev0, ctx().stream));
    return SYMGPU_OK;
}

int symgpu_timer_stop(float *ms) {
    SG_ENTER();
    HIP_TRY(hipEventRecord(ctx().ev1, ctx().stream));
    HIP_TRY(hipEventSynchronize(ctx().ev1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, ctx().ev0, ctx().ev1));
    if (ms) *ms = t;
    return SYMGPU_OK;
}

int symgpu_membw_probe(int64_t bytes, double *fill_GBps, double *copy_GBps) {
    SG_ENTER();
    SG_REQUIRE(bytes >= (1 << 20), "membw_probe: at least 1 MiB");
    const i64 n = bytes / 16;
    Scratch a, b;
    SG_TRY(a.alloc((size_t)n * 16));
    SG_TRY(b.alloc((size_t)n * 16));
    Context &c = ctx();
    const unsigned grid = (unsigned)((n + 255) / 256);
    float best_fill = 1e30f, best_copy = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
        float ms = 0;
        HIP_TRY(hipEventRecord(c.ev0, c.stream));
        hipLaunchKernelGGL(k_probe_fill, dim3(grid), dim3(256), 0, c.stream, a.as<u32x4p>(), n, 7u + rep);
        HIP_TRY(hipEventRecord(c.ev1, c.stream));
        HIP_TRY(hipEventSynchronize(c.ev1));
        HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        if (rep && ms < best_fill) best_fill = ms;
        HIP_TRY(hipEventRecord(c.ev0, c.stream));
        hipLaunchKernelGGL(k_probe_copy, dim3(grid), dim3(256), 0, c.stream, a.as<u32x4p>(), b.as<u32x4p>(), n);
        HIP_TRY(hipEventRecord(c.ev1, c.stream));
        HIP_TRY(hipEventSynchronize(c.ev1));
        HIP_TRY(hipEventElapsedTime(&ms, c.ev0, c.ev1));
        if (rep && ms < best_copy) best_copy = ms;
    }
    KERNEL_CHECK();
    if (fill_GBps) *fill_GBps = (double)n * 16 / (best_fill * 1e-3) / 1e9;
    if (copy_GBps) *copy_GBps = 2.0 * (double)n * 16 / (best_copy * 1e-3) / 1e9;
    return SYMGPU_OK;
}

int symgpu_prof_enable(int kernel_class, int on) {
    SG_ENTER();
    SG_REQUIRE(kernel_class >= 0 && kernel_class < SYMGPU_PROF_CLASSES, "prof_enable: class");
    prof()[kernel_class].on = on != 0;
    return SYMGPU_OK;
}

int symgpu_debug_counter(int which, int64_t *value) {
    SG_REQUIRE(value && which >= 0 && which < SYMGPU_CTR_COUNT, "debug_counter: which is an id of SYMGPU_COUNTER_LIST (include/symgpu.h; symgpu_debug_counter_name spells them)");
    *value = g_counters[which].load(std::memory_order_relaxed);
    return SYMGPU_OK;
}

const char *symgpu_debug_counter_name(int which) {
    switch (which) {
#define SG_COUNTER_NAME(name, id, text) case id: return #name;
        SYMGPU_COUNTER_LIST(SG_COUNTER_NAME)
#undef SG_COUNTER_NAME
        default: return nullptr;
    }
}

int symgpu_degraded(char *buf, int len) {
    if (!buf || len <= 0) return SYMGPU_E_INVALID;
    std::lock_guard<std::mutex> lk(g_deg_mu);
    snprintf(buf, (size_t)len, "%s", g_degraded.c_str());
    return SYMGPU_OK;
}

int symgpu_prof_read(int kernel_class, int64_t *n_launches, double *total_ms) {
    SG_ENTER();
    SG_REQUIRE(kernel_class >= 0 && kernel_class < SYMGPU_PROF_CLASSES, "prof_read: class");
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    double tot = 0;
    for (auto &p : prof()[kernel_class].ev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) tot += ms;
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    if (n_launches) *n_launches = (int64_t)prof()[kernel_class].ev.size();
    if (total_ms) *total_ms = tot;
    prof()[kernel_class].ev.clear();
    return SYMGPU_OK;
}

}  // extern "C"
