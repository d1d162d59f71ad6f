// sort.h — host-side API of the device-wide scans (scan.hip) and of the stable LSD radix sort (sort.hip, sort_coop.hip), for the files
// that scan or sort.  Everything runs on the context's stream; nothing here waits for it.
#pragma once
#include "common.h"

namespace symgpu {

// ---- scan.hip ----------------------------------------------------------------------------------------------------------------------
// out may alias in.  total_dev (optional, device) receives the sum of all n inputs.
int exclusive_scan_u32(const u32 *in, u32 *out, i64 n, u32 *total_dev /* may be null: device u32 */);
// bitmaps of up to POPC_SCAN_SMALL_MAX 64-bit words: out[w] = set bits in the words before w, *total_dev = all of them, one launch (n32: see scan.hip)
constexpr i64 POPC_SCAN_SMALL_MAX = (i64)1 << 13;
int popc_scan_small(const u64 *bits, i64 n, i64 n32, u32 *out, u32 *total_dev);

// ---- sort.hip ----------------------------------------------------------------------------------------------------------------------
constexpr int SORT_TILE = 4096;
// The two forms of one sort: a launch per step of every pass (histogram, column scan, scatter), or ALL passes in one persistent launch
// whose workgroups meet at in-kernel barriers (sort_coop.hip; at 10^5 keys the launches are what a pass costs).  A caller says what it
// wants; sort_form decides.
constexpr int SORT_ONE_LAUNCH_MAX_TILES = 128;       // the workgroups of the one launch must be co-resident: up to 2^19 keys
// where the one launch beats a launch per step (round 6, P * P and plain cleanups of 100 qubits): keys alone up to ~2e5 (245,350 keys: 182
// against 178 us; 125,250: 158 against 184), keys with values up to ~1.3e5 (100,000 rows: 116 against 121 us; 200,000: 140 against 127)
constexpr int SORT_ONE_LAUNCH_TILES_KEYS = 48, SORT_ONE_LAUNCH_TILES_PAIRS = 32;
enum class SortForm {
    Launches,               // a launch per step
    OneLaunchIfFits,        // one launch up to SORT_ONE_LAUNCH_MAX_TILES tiles (the caller's next step is launch bound as well)
    OneLaunchWherePays,     // one launch up to the measured thresholds (the caller has no better use for the answer than "sort these")
};
// Sort n keys — with a 32-bit value each, if vals != null — by key bits [begin_bit, end_bit) (a multiple of 8 wide), stable.  The passes
// ping-pong between the given buffers and their temporaries.
struct SortRequest {
    u64 *keys, *keys_tmp;
    u32 *vals, *vals_tmp;           // vals null: keys only
    i64 n;
    int begin_bit, end_bit;
    // optional, device, 256 * ceil(n / SORT_TILE) u32: the TILE-major ([tile][256]) tile histograms of the FIRST pass
    // (hist[tile * 256 + digit] = keys of tile `tile` whose bits [begin_bit, begin_bit + 8) equal `digit`), formed by a kernel of the
    // caller's that reads the keys anyway; the buffer then serves the later passes
    u32 *first_hist;
    SortForm want;
};
struct SortResult {
    u64 *keys, *spare_keys;         // where the sorted keys are / the other buffer of the request
    u32 *vals, *spare_vals;
    bool one_launch;                // the one launch ran: after its stream synchronisation the caller must look at the give-up flag (below)
};
// true: all passes in one launch.  Every rule is here: asked for at all; a first-pass histogram at hand means a launch per step (the
// histogram is a third of a pass already paid); the size limits of SortForm; the tuning switch SYMGPU_SORT_COOP=0; `one_launch_off`, the
// form having given up once in this process (SortState::coop_disabled).  n <= 1 launches nothing and counts as the form asked for.
bool sort_form(i64 n, bool has_vals, bool has_first_hist, SortForm want, bool one_launch_off);
int radix_sort(const SortRequest &rq, SortResult *res);

// ---- sort_coop.hip -----------------------------------------------------------------------------------------------------------------
int sort_one_launch(const SortRequest &rq);            // radix_sort's one-launch form (sort_form has said that it applies)
int sort_scan_ticket(u32 **ticket);                    // SortState::scan_ticket, allocated on first use
void sort_state_release(SortState &s);                 // the device memory of a context's SortState, at shutdown
// After the stream has been synchronised: did a one-launch sort since the last check give up at a barrier?  Then its output is garbage;
// the form is switched off for the rest of the process and the caller reports the failure.
int radix_sort_coop_check(bool *timed_out);
// the same in two steps, for callers that read the flag back together with their own status words: the device word a one-launch sort
// raises when it gives up (null: no such sort has run), and what to do with its value once it is on the host
const u32 *radix_sort_coop_flag();
void radix_sort_coop_note(u32 flag, bool *timed_out);

}  // namespace symgpu
