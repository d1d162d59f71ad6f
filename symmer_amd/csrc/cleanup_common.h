// cleanup_common.h — what the files of the cleanup share; private to them (the rest of the library calls cleanup_rows / cleanup_pairs,
// common.h).  Stages of one call, each file holding its kernels and the host function that launches them:
//   cleanup_hash.hip      row hashes (hash tables, k_hash_rows*)
//   cleanup_keys.hip      hash and key: pair keys or key bytes, coefficient floor, marking of the single terms;
//                         order: complete sort, or partial sort + flag pass (k_find_suspects / pair_dups.hip) + compaction
//   cleanup_segments.hip  fix-ups of the truncated sort, identity segment of P * P, segment sums (k_heads_sums)
//   cleanup.hip           output stage (k_emit_*)
//   cleanup_driver.hip    switches, plan, attempt loop, C ABI
#pragma once
#include "common.h"
#include "sort.h"

namespace symgpu {

// PACKED pair keys (written by product.hip's k_mul_coeff<.., KEYS>): one u64 per pair
//     [hash: 64-F bits][e: 2 bits][o: bo bits][i: bi bits],   F = bi + bo + 2,  bi/bo = bits of Ni-1 / No-1  (bi + bo <= 32)
// The radix sort then moves 8 instead of 12 bytes per element and pass, nothing on the path divides by Ni, the 16-byte pair
// coefficient is never materialised (c_i * c_o * i^e is rebuilt from e and the two cache-resident operand tables when the
// sorted order is known), and the full 64-bit key of a sorted element is recomputed from its (i, o) fields with two lookups
// in the per-operand hash tables whenever it is needed.  The LSD sort only touches hash bits and is stable, so equal keys
// stay in ascending pair-index order exactly as with separate index values.
struct PackedLayout {
    int bi, bo;
    __host__ __device__ int F() const { return bi + bo + 2; }
    __device__ __forceinline__ u32 i(u64 k) const { return (u32)(k & ((1ULL << bi) - 1ULL)); }
    __device__ __forceinline__ u32 o(u64 k) const { return (u32)((k >> bi) & ((1ULL << bo) - 1ULL)); }
    __device__ __forceinline__ int e(u64 k) const { return (int)((k >> (bi + bo)) & 3ULL); }
    __device__ __forceinline__ u32 fields(u64 k) const { return (u32)(k & ((1ULL << (bi + bo)) - 1ULL)); }   // (o << bi) | i
    __device__ __forceinline__ u64 full_key(const u64 *__restrict__ hI, const u64 *__restrict__ hO, u64 k) const { return hI[i(k)] ^ hO[o(k)]; }
};
// squared mode: slot of the pair (o, i), i >= o, in pair-index order, and back
__device__ __forceinline__ u32 tri_slot(u32 o, u32 i, u32 N) { return (u32)((u64)o * N - (u64)o * (o - 1) / 2 - o + i); }   // o*(o-1)/2 = 0 for o = 0 (u64 wraps twice)
__device__ __forceinline__ void tri_pair(u32 p, u32 N, u32 &o, u32 &i) {
    // rows o start at off(o) = o*N - o(o-1)/2: largest o with off(o) <= p; float estimate, then exact correction
    const double b = 2.0 * N + 1.0;
    i64 oo = (i64)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    if (oo < 0) oo = 0;
    if (oo > (i64)N - 1) oo = (i64)N - 1;
    auto off = [&](i64 x) { return x * (i64)N - x * (x - 1) / 2; };
    while (oo > 0 && off(oo) > (i64)p) --oo;
    while (oo + 1 < (i64)N && off(oo + 1) <= (i64)p) ++oo;
    o = (u32)oo;
    i = (u32)((i64)p - off(oo) + oo);
}

constexpr int SUS_RUN_BITS = 16;                                       // the flag pass's partial sort: key bits [32, 48)

// top key bits a radix sort of n keys orders (at most `cap`): ~1-3 % of the keys then share a prefix with another key, which the fix-up
// passes (cleanup_segments.hip) put in order cheaply
static int sorted_bits(i64 n, int cap) {
    int lg = 0;
    while (((i64)1 << lg) < n) ++lg;
    const int want = (lg + 5 + 7) / 8 * 8;
    return want < cap ? want : cap;
}

// Every switch the cleanup reads, read at the top of each call: tests flip them between calls of one process.
struct CleanupSwitches {
    bool unpacked = false;           // SYMGPU_CLEANUP_UNPACKED=1: 64-bit keys + index sort for products too
    bool nosquare = false;           // SYMGPU_CLEANUP_NOSQUARE=1: P * P on the general pair path
    int lazy = -1;                   // SYMGPU_CLEANUP_LAZY: -1 unset, 0 off, 1 everywhere
    int suspects = 1;                // SYMGPU_CLEANUP_SUSPECTS: 0 complete sort, 2 as if most keys were flagged
    bool key_bytes = true;           // SYMGPU_CLEANUP_KEYBYTES=0: 8-byte keys + k_mark_singles on the hash-table flag pass
    bool nofloor = false;            // SYMGPU_CLEANUP_NOFLOOR: the marking looks at every coefficient
    bool emit_fused = true;          // SYMGPU_EMIT_FUSED=0: batched output stage
    // tuning knobs (SG_TUNE: compiled out of the default build)
    i64 hs_waves = (i64)1 << 21;     // SYMGPU_HS_WAVES: wavefronts of k_heads_sums
    bool zero_seg = true;            // SYMGPU_CLEANUP_ZEROSEG=0: the identity segment summed by k_heads_sums
    int emit_touch = -1;             // SYMGPU_EMIT_TOUCH: -1 unset (touch ahead of the read-back), 0 no touch, else touch in the output stage
    bool emit_no_one_outer = false;  // SYMGPU_EMIT_NO_ONE_OUTER
    int emit_shape = 2 * 16 + 4;     // SYMGPU_EMIT_SHAPE "NW,U": NW * 16 + U
    int emit_rc = 2;                 // SYMGPU_EMIT_RC: chunks per lane of k_emit_stream
    bool fused(int Wq) const { return Wq <= 64 && emit_fused; }
};

// One call: T plain rows, or the T = Ni * No pairs of a product (pair: term t = o * Ni + i, see PairOperands).
struct CleanupRequest {
    bool pair = false;
    const u64 *rows = nullptr;
    const double *coeff = nullptr;
    PairOperands p;
    i64 T = 0;
    int W = 0, Wq_out = 0;
    double thr = 0.0;
    int use_thr = 0;
    bool want_first = false;
};

// How a call runs (plan_cleanup): decided from the sizes and the switches before the first attempt, and again after a long mixed prefix run.
struct CleanupPlan {
    PackedLayout L{0, 0};
    bool packed = false;             // pair mode on PACKED keys (hash | e | o | i); else 64-bit keys + a separate index sort
    bool squared = false;            // P * P: keys for the pairs with i >= o only (implies packed)
    i64 Tk = 0;                      // keys sorted; also the index space of the kept-term bitmap and the filed sums
    int nbits = 64;                  // top key bits the radix sort orders; the fix-up passes handle the rest
    bool lazy_call = false;          // the lazy flow's buffers are allocated
    bool lazy = false;               // singles decided in index order (k_mark_singles / k_mark_bytes)
    bool sus_try = false;            // the flag pass instead of a complete sort
    bool key_bytes = false;          // one byte per pair instead of the 8-byte key
};

// where k_emit_meta takes a kept term's coefficient from: mode 0 = the filed sums only; 1 / 2 = filed sums for patched terms, the
// operand tables (packed products) / the input coefficients (indexed operators) for all others (k_mark_singles)
struct LazyEmit {
    int mode = 0, squared = 0, no_one_outer = 0;
    const u32 *patchbits = nullptr, *e_lo = nullptr, *e_hi = nullptr;
    const double *ci = nullptr, *co = nullptr, *coeff = nullptr;
};
// the output stage's prefix over the kept-term bitmap: formed and its count read back with the status words of an attempt (one host round
// trip instead of two)
struct EmitPrefix { Scratch wordprefix, total; i64 n_out = -1; bool touched = false, wide = false; };


// The buffers of one call, and what the stages of an attempt hand each other.
struct CleanupRun {
    CleanupRequest rq;
    CleanupSwitches sw;
    CleanupPlan pl;
    hipStream_t st = nullptr;
    bool same_rows = false;          // one operand for both factors: hO_p is hI
    const u64 *hO_p = nullptr;
    const double *coeff = nullptr;   // the terms' coefficients where they are materialised (plain; unpacked pairs: pair_coeff)
    u64 seed = 1;
    Scratch keys, keys2, idx, idx2, fixlist, collision, hI, hO, pair_coeff, markbits, sum_of, zpart, zcount, patchbits, e_lo, e_hi, dirtybits, sort_hist, cfloor;
    Scratch diag_seq;                // P * P: the identity coefficient in the reference's order (k_diag_seq_sum)
    bool diag_side = false;          // ... formed on the side stream, not joined yet
    EmitPrefix pre;
    struct Attempt {
        u32 *first_hist = nullptr;   // the first sort pass's histograms, formed by k_mark_singles
        // what the stages after the sort see: `Tsort` keys ordered by their top `fix_bits` bits — all Tk keys, or (sus_active) only
        // the keys that the flag pass flagged
        i64 Tsort = 0;
        int fix_bits = 64;
        bool sus_active = false, sus_coop = false;   // sus_coop: the attempt's last sort was the one launch (its give-up flag is read back)
        u64 *ks = nullptr;           // the sorted keys (in keys or keys2) and, unpacked, their indices (in idx or idx2)
        u32 *is = nullptr;
        bool mark_zeroed = false, merges_found = false, patch_zeroed = false;   // lazy: dirtybits already filled by the fix-up passes
        bool lazy = false;           // the plan's lazy flow, unless the segment sums gave it up
        Attempt() {}
        explicit Attempt(const CleanupPlan &pl) : Tsort(pl.Tk), fix_bits(pl.nbits), lazy(pl.lazy) {}
    } a;
};

// cleanup_hash.hip
int hash_rows_any(const u64 *rows, i64 T, int W, u64 seed, u64 *out1, u32 *iota);
// cleanup_keys.hip
int cleanup_hash_keys(CleanupRun &r);
int cleanup_order(CleanupRun &r);
// cleanup_segments.hip
int zero_two(void *a, size_t bytes_a, void *b, size_t bytes_b, void *c = nullptr, size_t bytes_c = 0);
int cleanup_diag_begin(CleanupRun &r);
int cleanup_fixups(CleanupRun &r);
int cleanup_segment_sums(CleanupRun &r);
// cleanup.hip
int emit_prefix(const u32 *markbits_p, i64 T, Scratch &wordprefix, Scratch &total, bool wide);
int emit_touch(const u32 *markbits_p, i64 T, const LazyEmit &lz, EmitPrefix &pre);
int cleanup_finish(u32 *markbits_p, const double *sum_of_p, i64 T, bool pair, const u64 *rows, int W, const u64 *inner, i64 Ni,
                   const u64 *outer, symgpu_op_t *out, int Wq_out, bool tri, const LazyEmit &lz, bool want_first, const CleanupSwitches &sw,
                   EmitPrefix &pre);

}  // namespace symgpu
