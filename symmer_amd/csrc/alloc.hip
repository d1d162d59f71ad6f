// alloc.hip — the cached device allocator: size classes, parked blocks, arena chunks, canary.
#include "common.h"
#include <map>
#include <stdio.h>
#include <stdlib.h>

namespace symgpu {

// Size classes (power-of-two-ish), freed blocks parked per class until shutdown / release.  A class that has no parked block is
// carved from an ARENA — 4 GiB chunks, bump pointer, blocks up to 1 GiB — instead of going to hipMalloc (100 us .. 10 ms per call):
// a chain of rotations whose term count grows meets a new size class with every step, and with the arena its first pass costs what
// every later pass costs (round 2 needed a warm-up pass in the bench for that).  Carved blocks are never returned to the runtime
// one by one; a chunk is released as a whole when none of its blocks is in use (dev_cache_release).
static std::mutex g_alloc_mu;
struct LiveBlock { size_t cls; int chunk; int dev; size_t req = 0; };   // req: requested bytes (canary mode only)   // chunk: index into the device's chunks, -1 = its own hipMalloc
static std::map<void *, LiveBlock> g_live;        // block in use -> class / origin (device pointers are unique across the devices)
struct Chunk { char *base; size_t size, used; i64 live; };
struct DevAlloc {                                 // the allocator's state of ONE device
    std::multimap<size_t, void *> free_;          // size class -> parked block
    std::map<void *, int> parked_chunk;           // parked block -> origin (only arena blocks)
    std::vector<Chunk> chunks;
    size_t cached_bytes = 0;
    size_t cache_limit = (size_t)64 << 30;        // parked blocks: at most 64 GiB, raised to half of the device memory at init
                                                  // (hipMalloc / hipFree of multi-GB blocks cost ~10 ms per GB)
    bool arena_on = true;
};
static DevAlloc g_alloc[SYMGPU_MAX_DEVICES];
static const size_t ARENA_CHUNK = (size_t)4 << 30, ARENA_MAX_BLOCK = (size_t)1 << 30;

// at the device's init (the device is the thread's HIP device): its cache limit and the arena switch
void dev_alloc_init(int device) {
    DevAlloc &A = g_alloc[device];
    size_t f = 0, t = 0;
    if (hipMemGetInfo(&f, &t) == hipSuccess && t / 2 > A.cache_limit) A.cache_limit = t / 2;
    if (const char *e = SG_TUNE("SYMGPU_ARENA")) A.arena_on = !(e[0] == '0');       // 0: every size class straight from hipMalloc (round 2's allocator)
}

static size_t size_class(size_t b) {
    if (b < 256) b = 256;
    if (b <= ((size_t)1 << 20)) {           // <= 1 MiB: next power of two
        size_t c = 256;
        while (c < b) c <<= 1;
        return c;
    }
    size_t g = (size_t)1 << 20;             // above: 1 MiB granularity rounded to 1/8 of the leading power
    size_t p = g;
    while ((p << 1) <= b) p <<= 1;
    size_t step = p >> 3;
    if (step < g) step = g;
    return (b + step - 1) / step * step;
}

// carve `c` bytes (a multiple of 256) from A's arena; nullptr if the arena is off, the block is too large or memory is short
static void *arena_carve(DevAlloc &A, size_t c, int *chunk) {
    if (!A.arena_on || c > ARENA_MAX_BLOCK) return nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = (int)A.chunks.size() - 1; i >= 0; --i) {
            Chunk &ch = A.chunks[i];
            if (ch.base && ch.size - ch.used >= c) {
                void *p = ch.base + ch.used;
                ch.used += c;
                ++ch.live;
                *chunk = i;
                return p;
            }
        }
        if (pass == 1) break;
        void *base = nullptr;
        bump_counter(SYMGPU_CTR_DEV_MALLOC_CALLS);
        if (hipMalloc(&base, ARENA_CHUNK) != hipSuccess) { (void)hipGetLastError(); A.arena_on = false; return nullptr; }
        A.chunks.push_back(Chunk{static_cast<char *>(base), ARENA_CHUNK, 0, 0});
    }
    return nullptr;
}

// Debug aid (tuning build, SYMGPU_ALLOC_CANARY=1): every block gets 256 bytes of 0xA5 behind the bytes that were asked for, checked when
// the block is freed — a kernel that writes past the end of a buffer is reported on stderr with the block's size (size classes round up, so
// such a write otherwise lands in padding and goes unnoticed).  Reads past the end cannot be caught this way.
constexpr size_t CANARY = 256;
static bool canary_on() { static const bool on = [] { const char *e = SG_TUNE("SYMGPU_ALLOC_CANARY"); return e && e[0] == '1'; }(); return on; }
static void canary_set(void *p, size_t bytes) {
    (void)hipMemsetAsync(static_cast<char *>(p) + bytes, 0xA5, CANARY, ctx().stream);
}
static void canary_check(void *p, size_t bytes) {
    unsigned char h[CANARY];
    (void)hipDeviceSynchronize();
    if (hipMemcpy(h, static_cast<char *>(p) + bytes, CANARY, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    for (size_t k = 0; k < CANARY; ++k)
        if (h[k] != 0xA5) {
            fprintf(stderr, "symgpu CANARY: block of %zu bytes overwritten at +%zu behind its end (value 0x%02x)\n", bytes, k, h[k]);
            bump_counter(SYMGPU_CTR_CANARY_HITS);
            return;
        }
}
// file block `p` as in use (under g_alloc_mu); returns p
static void *record_live(void *p, const LiveBlock &blk) {
    g_live[p] = blk;
    bump_counter(SYMGPU_CTR_DEV_BLOCKS_LIVE);
    if (canary_on()) canary_set(p, blk.req);
    return p;
}
// take the parked block `it` of A (device `dev`) back into use (under g_alloc_mu); it keeps the class it was parked under
static void *take_parked(DevAlloc &A, std::multimap<size_t, void *>::iterator it, int dev, size_t req) {
    const size_t cls = it->first;
    void *p = it->second;
    A.free_.erase(it);
    A.cached_bytes -= cls;
    int chunk = -1;
    auto pc = A.parked_chunk.find(p);
    if (pc != A.parked_chunk.end()) { chunk = pc->second; A.parked_chunk.erase(pc); ++A.chunks[chunk].live; }
    return record_live(p, LiveBlock{cls, chunk, dev, req});
}

int dev_alloc(size_t bytes, void **ptr) {
    SG_TRY(require_ctx());
    const int dev = cur_index();                       // (not ctx(): allocating is not counted as a use of the context)
    DevAlloc &A = g_alloc[dev];                        // the CURRENT device's lists
    const size_t req = bytes;
    if (canary_on()) bytes += CANARY;
    size_t c = size_class(bytes);
    {
        std::lock_guard<std::mutex> lk(g_alloc_mu);
        auto it = A.free_.find(c);
        if (it != A.free_.end()) { *ptr = take_parked(A, it, dev, req); return SYMGPU_OK; }
        int chunk = -1;
        if (void *p = arena_carve(A, c, &chunk)) { *ptr = record_live(p, LiveBlock{c, chunk, dev, req}); return SYMGPU_OK; }
    }
    hipError_t e = hipMalloc(ptr, c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        dev_cache_release();
        e = hipMalloc(ptr, c);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            // Last resort: a parked block of a LARGER class.  dev_cache_release cannot return arena blocks whose chunk still holds
            // a live block (one long-lived handle pins its 4 GiB chunk), so their memory would otherwise be lost to this request.
            // The block keeps its own class and goes back to it when freed.
            std::lock_guard<std::mutex> lk(g_alloc_mu);
            auto it = A.free_.lower_bound(c);
            if (it != A.free_.end()) { *ptr = take_parked(A, it, dev, req); return SYMGPU_OK; }
            set_error("device allocation of %zu bytes failed: %s", c, hipGetErrorString(e));
            *ptr = nullptr;
            return SYMGPU_E_NOMEM;
        }
    }
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    bump_counter(SYMGPU_CTR_DEV_MALLOC_CALLS);
    record_live(*ptr, LiveBlock{c, -1, dev, req});
    return SYMGPU_OK;
}

int dev_free(void *ptr) {
    if (!ptr) return SYMGPU_OK;
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    auto it = g_live.find(ptr);
    if (it == g_live.end()) {
        bump_counter(SYMGPU_CTR_DEV_FREE_UNKNOWN);
        set_error("dev_free: unknown pointer");
        return SYMGPU_E_INVALID;
    }
    const LiveBlock blk = it->second;
    g_live.erase(it);
    bump_counter(SYMGPU_CTR_DEV_BLOCKS_LIVE, -1);
    if (canary_on()) canary_check(ptr, blk.req);
    DevAlloc &A = g_alloc[blk.dev];                    // the OWNING device's lists (a handle may be dropped while another device is current)
    if (blk.chunk >= 0) {                              // arena block: parked, whatever the limit says (it cannot go back on its own)
        --A.chunks[blk.chunk].live;
        A.parked_chunk[ptr] = blk.chunk;
    } else if (A.cached_bytes + blk.cls > A.cache_limit) {
        (void)hipFree(ptr);                            // stream-ordered safety: everything runs on one stream per device, but hipFree synchronises anyway
        return SYMGPU_OK;
    }
    A.free_.insert({blk.cls, ptr});
    A.cached_bytes += blk.cls;
    return SYMGPU_OK;
}

void dev_cache_release() {
    DevAlloc &A = g_alloc[cur_index()];                // the CURRENT device's cache only (symgpu_shutdown selects each device in turn)
    std::lock_guard<std::mutex> lk(g_alloc_mu);
    if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);
    for (auto it = A.free_.begin(); it != A.free_.end();) {
        auto pc = A.parked_chunk.find(it->second);
        if (pc == A.parked_chunk.end()) {              // its own hipMalloc
            (void)hipFree(it->second);
            A.cached_bytes -= it->first;
            it = A.free_.erase(it);
        } else if (A.chunks[pc->second].live == 0) {   // arena block of a chunk nobody uses: goes with its chunk below
            A.cached_bytes -= it->first;
            A.parked_chunk.erase(pc);
            it = A.free_.erase(it);
        } else {
            ++it;
        }
    }
    for (Chunk &ch : A.chunks)
        if (ch.base && ch.live == 0) { (void)hipFree(ch.base); ch.base = nullptr; ch.size = ch.used = 0; }
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_dev_alloc(int64_t bytes, void **ptr) {
    SG_ENTER();
    SG_REQUIRE(ptr && bytes >= 0, "dev_alloc");
    return dev_alloc((size_t)bytes, ptr);
}
int symgpu_dev_free(void *ptr) { return dev_free(ptr); }   // no context: dev_free files the block under its owning device, under the allocator's mutex

}  // extern "C"
