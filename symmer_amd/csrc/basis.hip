// basis.hip — one layer of H (X-qubits) and H S^+ (Y-qubits) on a dense statevector, in place: the change of basis after which every
// measured qubit is read in Z (include/symgpu.h, section f10; conventions of matvec.hip: qubit q is bit n-1-q of a basis
// index).  On the pair (a0, a1) of a measured index bit (a1: bit set):  Y-qubit first a1 <- (a1.im, -a1.re)  [S^+, exact];  then
//   a0' = (a0 + a1) r,  a1' = (a0 - a1) r   per component, every sum and product rounded once, r = the double nearest 1/sqrt 2.
// The measured bits are taken in ASCENDING INDEX BIT (descending qubit number): the order is part of the contract, it changes the bits.
// DIRECT: one launch per measured bit over the 2^(n-1) pairs.  TILED: the measured bits go, ascending, into groups; a group's tile bits S
// are the 4 lowest index bits (pieces of 256 bytes) and its measured bits while |S| <= min(n, 12) (2^12 amplitudes = 64 KiB of LDS),
// filled with the lowest free bits up to min(n, 10); a workgroup loads the 2^|S| amplitudes that agree outside S, runs the group's
// butterflies in LDS in the same order with a barrier between them, and writes them back: one pass over the vector per group.
#include "matvec.h"
#include <stdlib.h>
#include <string.h>

namespace symgpu {

constexpr int BS_WG = 256;
constexpr int BS_LOW = 4;                 // the lowest index bits are always tile bits
constexpr int BS_MAX_TILE = 12;           // 2^12 amplitudes x 16 bytes = 64 KiB of LDS
constexpr int BS_FILL = 10;               // a smaller tile takes the lowest free bits up to this many
constexpr double BS_R = 0x1.6a09e667f3bcdp-1;   // 0x3FE6A09E667F3BCD

// the bits of v, lowest first, to the set positions of mask, lowest first
__host__ __device__ __forceinline__ u64 bs_deposit(u64 v, u64 mask) {
    u64 r = 0;
    while (mask) {
        const u64 low = mask & (~mask + 1);
        if (v & 1) r |= low;
        v >>= 1;
        mask ^= low;
    }
    return r;
}
// the bits of v at the set positions of mask, packed lowest first
static u64 bs_extract(u64 v, u64 mask) {
    u64 r = 0;
    for (int at = 0; mask; mask &= mask - 1, ++at)
        if (v & mask & (~mask + 1)) r |= (u64)1 << at;
    return r;
}

__device__ __forceinline__ void bs_butterfly(f64x2 &a0, f64x2 &a1, bool is_y) {
    if (is_y) a1 = f64x2{a1.y, -a1.x};
    const f64x2 p = f64x2{__dmul_rn(__dadd_rn(a0.x, a1.x), BS_R), __dmul_rn(__dadd_rn(a0.y, a1.y), BS_R)};
    const f64x2 q = f64x2{__dmul_rn(__dsub_rn(a0.x, a1.x), BS_R), __dmul_rn(__dsub_rn(a0.y, a1.y), BS_R)};
    a0 = p;
    a1 = q;
}

// DIRECT: pair t of index bit `bit`
__global__ __launch_bounds__(BS_WG) void k_bs_direct(f64x2 *__restrict__ psi, u64 pairs, int bit, int is_y) {
    const u64 t = (u64)blockIdx.x * BS_WG + threadIdx.x;
    if (t >= pairs) return;
    const u64 low = t & (((u64)1 << bit) - 1);
    const u64 b0 = ((t >> bit) << (bit + 1)) | low, b1 = b0 | ((u64)1 << bit);
    f64x2 a0 = psi[b0], a1 = psi[b1];
    bs_butterfly(a0, a1, is_y != 0);
    psi[b0] = a0;
    psi[b1] = a1;
}

// TILED: S the tile bits (m of them), outside the others; pm / ym: the measured / the Y bits of the group as bits of a tile slot
__global__ __launch_bounds__(BS_WG) void k_bs_tile(f64x2 *__restrict__ psi, u64 S, u64 outside, int m, u32 pm, u32 ym) {
    extern __shared__ f64x2 bs_tile[];
    const u32 L = 1u << m, t = threadIdx.x;
    const u64 base = bs_deposit((u64)blockIdx.x, outside);
    for (u32 l = t; l < L; l += BS_WG) bs_tile[l] = psi[base | bs_deposit((u64)l, S)];
    __syncthreads();
    for (u32 rest = pm; rest; rest &= rest - 1) {
        const int p = __ffs(rest) - 1;
        const bool is_y = (ym >> p) & 1;
        for (u32 j = t; j < (L >> 1); j += BS_WG) {
            const u32 i0 = ((j >> p) << (p + 1)) | (j & ((1u << p) - 1)), i1 = i0 | (1u << p);
            f64x2 a0 = bs_tile[i0], a1 = bs_tile[i1];
            bs_butterfly(a0, a1, is_y);
            bs_tile[i0] = a0;
            bs_tile[i1] = a1;
        }
        __syncthreads();
    }
    for (u32 l = t; l < L; l += BS_WG) psi[base | bs_deposit((u64)l, S)] = bs_tile[l];
}

static int bs_popc(u64 v) { return __builtin_popcountll(v); }

static int bs_form_wanted() {
    const char *f = getenv("SYMGPU_BASIS_FORM");
    return f && !strcmp(f, "direct") ? SYMGPU_BASIS_DIRECT : SYMGPU_BASIS_TILED;
}

// measured / ybits: index bits.  Returns the launches through *launches.
static int bs_run(f64x2 *psi, int n, u64 measured, u64 ybits, int form, int *launches) {
    hipStream_t st = ctx().stream;
    const u64 all = n == 64 ? ~(u64)0 : ((u64)1 << n) - 1;
    *launches = 0;
    if (form == SYMGPU_BASIS_DIRECT) {
        const u64 pairs = (u64)1 << (n - 1);
        for (u64 rest = measured; rest; rest &= rest - 1) {
            const int bit = __builtin_ctzll(rest);
            hipLaunchKernelGGL(k_bs_direct, dim3(grid_each((i64)pairs, BS_WG)), dim3(BS_WG), 0, st, psi, pairs, bit, (int)((ybits >> bit) & 1));
            ++*launches;
        }
        KERNEL_CHECK();
        return SYMGPU_OK;
    }
    const int budget = n < BS_MAX_TILE ? n : BS_MAX_TILE, fill = n < BS_FILL ? n : BS_FILL;
    const u64 low = ((u64)1 << (n < BS_LOW ? n : BS_LOW)) - 1;
    u64 rest = measured;
    while (rest) {
        u64 S = low, group = 0;
        while (rest) {
            const u64 b = rest & (~rest + 1);
            if (bs_popc(S | b) > budget) break;
            S |= b;
            group |= b;
            rest ^= b;
        }
        while (bs_popc(S) < fill) S |= (~S & all) & (~(~S & all) + 1);
        const int m = bs_popc(S);
        hipLaunchKernelGGL(k_bs_tile, dim3((unsigned)((u64)1 << (n - m))), dim3(BS_WG), (size_t)16 << m, st, psi, S, all & ~S, m, (u32)bs_extract(group, S),
                           (u32)bs_extract(group & ybits, S));
        ++*launches;
    }
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_basis_change(double *psi_dev, int n_qubits, uint64_t x_mask, uint64_t y_mask, int *form) {
    SG_ENTER();
    if (form) *form = 0;
    SG_REQUIRE(psi_dev, "basis_change: null vector");
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32, "basis_change: 1 <= n_qubits <= 32");
    SG_REQUIRE((x_mask & y_mask) == 0, "basis_change: a qubit is in both masks");
    SG_REQUIRE(((x_mask | y_mask) >> n_qubits) == 0, "basis_change: a mask names a qubit beyond n_qubits");
    // qubit q -> index bit n-1-q
    u64 measured = 0, ybits = 0;
    for (int q = 0; q < n_qubits; ++q) {
        if (((x_mask | y_mask) >> q) & 1) measured |= (u64)1 << (n_qubits - 1 - q);
        if ((y_mask >> q) & 1) ybits |= (u64)1 << (n_qubits - 1 - q);
    }
    if (!measured) return SYMGPU_OK;
    const int want = bs_form_wanted();
    int launches = 0;
    SG_TRY(bs_run(reinterpret_cast<f64x2 *>(psi_dev), n_qubits, measured, ybits, want, &launches));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    if (form) *form = want;
    return SYMGPU_OK;
}

}  // extern "C"
