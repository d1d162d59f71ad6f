// transfer.hip — large downloads (page prefault, pipelined copy), raw buffer upload / download, the read-back mailbox.
#include "common.h"
#include <chrono>
#include <thread>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

namespace symgpu {

// Large device -> host copies into FRESH pageable memory (np.empty) are bound by first-touch page faults taken inside the
// runtime's pinning path: 9-18 GB/s, against 43-55 GB/s once the pages exist (tools/ubench_d2h.hip, MI355X box).  Touch the
// destination pages first, from a few threads; the copy overwrites the whole range anyway.
static void touch_pages(char *base, size_t lo, size_t hi) {
    for (size_t o = lo; o < hi; o += 4096) reinterpret_cast<volatile char *>(base)[o] = 0;
    if (hi > lo) reinterpret_cast<volatile char *>(base)[hi - 1] = 0;
}

static int prefault_threads() {
    const unsigned hw = std::thread::hardware_concurrency();
    return hw >= 16 ? 8 : (hw >= 4 ? 4 : 1);
}

// first touch of [lo, hi) of a large D2H destination from several threads (the runtime's own pinning path takes the first-touch faults
// at 9-18 GB/s, tools/ubench_d2h.hip); the workers are returned running, the caller joins them
static std::vector<std::thread> prefault_start(char *base, size_t lo, size_t hi) {
    std::vector<std::thread> workers;
    const size_t page = 4096;
    const int n_threads = prefault_threads();
    const size_t chunk = ((hi - lo) / n_threads + page - 1) / page * page;
    for (int k = 0; k < n_threads && chunk; ++k) {
        const size_t a = lo + (size_t)k * chunk, b = a + chunk < hi ? a + chunk : hi;
        if (a >= b) break;
        workers.emplace_back(touch_pages, base, a, b);
    }
    return workers;
}

static void ask_for_huge_pages(void *dst, size_t bytes) {
    // transparent huge pages on the page-aligned interior (honoured where THP is 'always' or 'madvise'): 512x fewer faults
    const size_t page = 4096;
    const uintptr_t a = (reinterpret_cast<uintptr_t>(dst) + page - 1) & ~(uintptr_t)(page - 1);
    const uintptr_t b = (reinterpret_cast<uintptr_t>(dst) + bytes) & ~(uintptr_t)(page - 1);
    if (b > a) (void)madvise(reinterpret_cast<void *>(a), b - a, MADV_HUGEPAGE);
}

void prefault_host(void *dst, size_t bytes) {
    if (!dst || bytes < ((size_t)64 << 20)) return;
    ask_for_huge_pages(dst, bytes);
    for (auto &w : prefault_start(static_cast<char *>(dst), 0, bytes)) w.join();
}

// A large device-to-host copy into pageable memory, in pieces: while piece k travels (the copy call blocks its thread) the pages of
// piece k + 1 are touched by the worker threads, so the first-touch faults of a fresh destination (a 40 GB commutation table: ~0.2 s) hide
// behind the PCIe transfer; the first piece is touched while the kernels queued ahead of the copy are still running.
static int download_pipelined(const char *dev, char *host, size_t bytes) {
    const size_t piece = (size_t)1 << 30;
    ask_for_huge_pages(host, bytes);
    for (auto &w : prefault_start(host, 0, piece < bytes ? piece : bytes)) w.join();
    for (size_t off = 0; off < bytes; off += piece) {
        const size_t n = bytes - off < piece ? bytes - off : piece;
        std::vector<std::thread> next;
        if (off + piece < bytes) next = prefault_start(host, off + piece, off + 2 * piece < bytes ? off + 2 * piece : bytes);
        const hipError_t e1 = hipMemcpyAsync(host + off, dev + off, n, hipMemcpyDeviceToHost, ctx().stream);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(ctx().stream) : e1;
        for (auto &w : next) w.join();
        HIP_TRY(e2);
    }
    return SYMGPU_OK;
}

// device -> pageable host memory, any size: small copies as one call, large ones pipelined (see above); returns with the data on the host
int download_any(const void *dev, void *host, size_t bytes) {
    if (bytes >= ((size_t)2 << 30)) return download_pipelined(static_cast<const char *>(dev), static_cast<char *>(host), bytes);
    prefault_host(host, bytes);
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

// ---- a few words back to the host in the middle of a call ---------------------------------------------------------------------------
// hipMemcpyAsync of a few bytes + hipStreamSynchronize costs two host round trips on this runtime (the stream is drained, THEN a blit
// kernel is queued, then drained again: 35 + 25 us of idle GPU per read-back, rocprofv3 timeline of cfg3).  Instead a one-wavefront kernel
// at the end of the queue stores the words into mapped, coherent host memory and a sequence number behind them (system-scope release);
// the host polls the sequence number.  Nothing else of the runtime is involved; after 2 s without an answer (a kernel fault upstream)
// the stream is synchronised the ordinary way and its error reported.
__global__ void k_mail_words(const u32 *__restrict__ a, int n_a, const u32 *__restrict__ b, int n_b, const u32 *__restrict__ c1, u32 *__restrict__ mail, u32 seq) {
    const int t = threadIdx.x;
    if (t < n_a) __hip_atomic_store(mail + 1 + t, a[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (t < n_a + n_b) __hip_atomic_store(mail + 1 + t, b[t - n_a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (t == n_a + n_b && c1) __hip_atomic_store(mail + 1 + t, *c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __builtin_amdgcn_s_barrier();
    if (t == 0) __hip_atomic_store(mail, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static bool mail_ready() {
    Context &c = ctx();
    const char *plain = getenv("SYMGPU_READBACK_PLAIN");
    if (plain && plain[0] == '1') return false;
    if (!c.mail_host && !c.mail_failed) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
            memset(h, 0, 64);
            c.mail_host = static_cast<u32 *>(h);
            c.mail_dev = static_cast<u32 *>(d);
        } else {
            (void)hipGetLastError();
            if (h) (void)hipHostFree(h);
            c.mail_failed = true;
            note_degraded("read-back through mapped host memory unavailable: every mid-call read-back is a copy + stream synchronisation");
        }
    }
    return c.mail_host != nullptr;
}
// post: queue the words' way home (more work may be queued behind it before the wait); wait: poll, copy out.  One read-back in flight per
// context.
int read_back_post(const u32 *a, int n_a, const u32 *b, int n_b, ReadBack *rb, const u32 *c1) {
    Context &c = ctx();
    rb->n = n_a + n_b + (c1 ? 1 : 0); rb->seq = 0;
    if (rb->n > 8) { set_error("read_back: %d words", rb->n); return SYMGPU_E_INVALID; }
    if (!mail_ready()) {                                                // the copies are queued here, the synchronisation is the wait
        if (n_a) HIP_TRY(hipMemcpyAsync(rb->plain, a, (size_t)n_a * 4, hipMemcpyDeviceToHost, c.stream));
        if (n_b) HIP_TRY(hipMemcpyAsync(rb->plain + n_a, b, (size_t)n_b * 4, hipMemcpyDeviceToHost, c.stream));
        if (c1) HIP_TRY(hipMemcpyAsync(rb->plain + n_a + n_b, c1, 4, hipMemcpyDeviceToHost, c.stream));
        return SYMGPU_OK;
    }
    ++c.mail_seq;
    if (c.mail_seq == 0) ++c.mail_seq;                                  // never 0
    rb->seq = c.mail_seq;
    hipLaunchKernelGGL(k_mail_words, dim3(1), dim3(64), 0, c.stream, a, n_a, b, n_b, c1, c.mail_dev, rb->seq);
    KERNEL_CHECK();
    return SYMGPU_OK;
}
int read_back_wait(ReadBack *rb, u32 *host_out) {
    Context &c = ctx();
    const int n = rb->n;
    if (rb->seq == 0) {
        HIP_TRY(hipStreamSynchronize(c.stream));
        for (int k = 0; k < n; ++k) host_out[k] = rb->plain[k];
        return SYMGPU_OK;
    }
    volatile u32 *mail = c.mail_host;
    const auto t0 = std::chrono::steady_clock::now();
    for (u64 spin = 0;; ++spin) {
        if (__atomic_load_n(&mail[0], __ATOMIC_ACQUIRE) == rb->seq) break;
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIP_TRY(hipStreamSynchronize(c.stream));                    // reports a fault upstream; otherwise the words are there now
            if (__atomic_load_n(&mail[0], __ATOMIC_ACQUIRE) != rb->seq) { set_error("read_back: no answer from the device"); return SYMGPU_E_HIP; }
            break;
        }
    }
    for (int k = 0; k < n; ++k) host_out[k] = mail[1 + k];
    return SYMGPU_OK;
}
int read_back_words(const u32 *a, int n_a, const u32 *b, int n_b, u32 *host_out, const u32 *c1) {
    ReadBack rb;
    SG_TRY(read_back_post(a, n_a, b, n_b, &rb, c1));
    return read_back_wait(&rb, host_out);
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_dev_download(const void *dev, void *host, int64_t bytes) {
    SG_ENTER();
    SG_REQUIRE(dev && host && bytes >= 0, "dev_download");
    SG_TRY(download_any(dev, host, (size_t)bytes));
    count_d2h((size_t)bytes);
    return SYMGPU_OK;
}

int symgpu_dev_upload(void *dev, const void *host, int64_t bytes) {
    SG_ENTER();
    SG_REQUIRE(dev && host && bytes >= 0, "dev_upload");
    HIP_TRY(hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, ctx().stream));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    count_h2d((size_t)bytes);
    return SYMGPU_OK;
}

}  // extern "C"
