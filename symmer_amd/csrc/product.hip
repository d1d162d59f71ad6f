// product.hip — the row streams of the all-pairs Pauli product (reference: PauliwordOp._multiply_by_operator,
// symmer/operators/base.py:764-794; operand swap of __mul__ base.py:847-852 folded into `inner_is_left`).
//
//   row  o*Ni + i  =  inner[i] xor outer[o]
//   coeff          =  c_i * c_o * i^e ,  e = (3(Y_i+Y_o) + Y_out + 2|x_left & z_right|) mod 4
//
// Three streaming kernels, each bound by the HBM write rate:
//  * k_mul_rows — 16*Wq B/pair.  Every lane owns 16-byte chunks of inner rows (held in VGPRs across the outer loop) and streams
//    chunk ^ outer[o][chunk % Wq]  with non-temporal 16-byte stores, 1 KiB per wave instruction, perfectly coalesced.  Inputs stay in L2;
//    algorithmic bytes == HBM bytes.  This is the kernel the north-star roofline is quoted on.
//  * k_mul_rows_e — the same stream where a row is a power-of-two number of 16-byte chunks (n <= 64, 65..128, 193..256, 449..512, 961..1024,
//    1985..2048, 4033..4096 qubits).  The row stream has its VALU idle, and in the row-major layout the X and the Z words of a term sit in the
//    two halves of an aligned lane group: the phase sum  Y_out + 2|x_left & z_right|  of every output row is formed on the way (DPP lane
//    exchange, v_bcnt, three DPP adds: measured free, tools/ubench_fused.hip) and leaves as 2 bits per pair, four pairs to a byte.
//  * k_mul_coeff_expand — expands the phase bytes to coefficients, 1 B read and 16 B written per pair: one contiguous 4 KiB piece of one outer
//    row per workgroup, dispatch order = address order: 409.6 MB of coefficients per 256-row slab at n = 1000 in 66 us = 6.2 TB/s.
//
// Phase bytes: a workgroup of k_mul_rows_e covers R = 256/Wq output rows and leaves R/4 bytes, row 4k + j of the workgroup in bits 2j, 2j + 1
// of byte k; the bytes of workgroup (bx, o) of a launch with grid.x = gx start at (o * gx + (bx % 8) * (gx / 8) + bx / 8) * R/4.
//
// XCD round robin: workgroups go to the 8 XCDs round-robin by linear id (= by * gx + bx).  With gx a multiple of 8 the inner chunk bx is
// ALWAYS read by XCD bx % 8, so each XCD's 4 MB L2 only ever sees its own eighth of the inner operand (3.2 MB of 25.6 MB at the benchmark
// size) and keeps it.  The re-reads of the inner operand then stop at the L2 instead of crossing the fabric, which makes ONE output row per
// block affordable — and that is the sequential write pattern the HBM likes (tools/ubench_rows.hip: 12 rows per block 6.27 TB/s either way;
// 1 row per block 3.76 TB/s unpadded, 7.14 TB/s padded).  The surplus blocks exit.  An inner operand whose eighth does NOT fit (10^5 terms
// of 2,000 qubits = 6.4 MB per XCD, 0.47 of the HBM peak against 0.8 for 10^4 terms) is cut into tiles that do (inner_tile_chunks): every
// tile is a launch over all outer rows.  For the same reason the phase bytes of consecutive workgroups OF ONE XCD are adjacent (above), and
// the expansion's piece bx is always expanded by XCD bx % 8, whose L2 keeps its eighth of c_i / Y_i across the outer rows.
//
// The path decision and the loops over tiles and grid.y batches are in product_driver.hip; product_common.h lists the files.
#include "product_common.h"

namespace symgpu {

// ---- the HBM-write stream ------------------------------------------------------------------------
// RCT = 16-byte chunks per lane, NT = non-temporal stores, rto = outer rows per block (runtime).
template <int RCT, bool NT>
__global__ __launch_bounds__(1024) void k_mul_rows(const u32x4 *__restrict__ inner, i64 n_chunks, const u32x4 *__restrict__ outer,
                                                    int Wq, i64 o_count, u32x4 *__restrict__ out, int rto, i64 out_stride) {
    const int BT = blockDim.x;                                      // 256 (default) .. 1024 threads: BT * 16 contiguous bytes per row
    const i64 c0 = (i64)blockIdx.x * (BT * RCT) + threadIdx.x;
    u32x4 v[RCT];
    int wq[RCT];
    bool ok[RCT];
#pragma unroll
    for (int k = 0; k < RCT; ++k) {
        const i64 c = c0 + BT * k;
        ok[k] = c < n_chunks;
        v[k] = ok[k] ? inner[c] : (u32x4)(0u);
        wq[k] = ok[k] ? (int)(c % Wq) : 0;
    }
    const i64 ob = (i64)blockIdx.y * rto;
    const i64 oe = ob + rto < o_count ? ob + rto : o_count;
    for (i64 o = ob; o < oe; ++o) {
        const u32x4 *orow = outer + o * Wq;
        u32x4 *dst = out + o * out_stride + c0;
#pragma unroll
        for (int k = 0; k < RCT; ++k) {
            if (ok[k]) {
                u32x4 r = v[k] ^ orow[wq[k]];
                if (NT) __builtin_nontemporal_store(r, dst + BT * k);
                else dst[BT * k] = r;
            }
        }
    }
}


// ---- the HBM-write stream that also leaves the phase sums ----------------------------------------
// WQ = 16-byte chunks per row (= words per X block), a power of two <= 64: a row occupies an aligned group of WQ lanes, its X
// words in the lower half and its Z words in the upper half, so lane ^ WQ/2 holds the other half of the same qubits.
template <int CTRL> __device__ __forceinline__ u32 dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_ROR8 = 0x128;
template <int WQ> __device__ __forceinline__ u32 other_half(u32 v) {
    if (WQ == 2) return dpp<DPP_XOR1>(v);
    if (WQ == 4) return dpp<DPP_XOR2>(v);
    if (WQ == 16) return dpp<DPP_ROR8>(v);
    return (u32)__shfl_xor((int)v, WQ / 2);
}
// sum over the WQ/2 lanes of the half of the row the lane sits in (butterfly; every lane of the half gets the sum)
template <int WQ> __device__ __forceinline__ u32 half_row_sum(u32 s) {
    if (WQ >= 4) s += dpp<DPP_XOR1>(s);
    if (WQ >= 8) s += dpp<DPP_XOR2>(s);
    if (WQ >= 16) s += dpp<DPP_HALF_MIRROR>(s);     // quads hold equal values: lane 7-L supplies the other quad's
    if (WQ >= 32) s += dpp<DPP_MIRROR>(s);
    if (WQ >= 64) s += (u32)__shfl_xor((int)s, 16);
    return s;
}

// One output row segment per block (the sequential write pattern of k_mul_rows<1, true>, rto = 1) plus, per output row, the 2-bit
// phase sum (Y_out + 2 |x_left & z_right|) mod 4, four rows to a byte (row 4k + j in bits 2j, 2j + 1).  The R = 256/WQ sums of a block
// are gathered in LDS and leave as R/4 bytes (4 at WQ = 16, 1 at WQ = 64) stored by the first lanes of wave 0.
// Byte index: (o * gx + (bx % 8) * (gx / 8) + bx / 8) * R/4 + row in block / 4: workgroups go to the XCDs round robin, so the bytes
// of consecutive blocks OF ONE XCD are adjacent and fill whole lines in that XCD's L2 (plain stores) — bytes of neighbouring blocks
// interleaved from 8 different L2s cost partial-line write-backs.
template <int WQ, bool INNER_LEFT>
__global__ __launch_bounds__(256) void k_mul_rows_e(const u32x4 *__restrict__ inner, i64 n_chunks, const u32x4 *__restrict__ outer,
                                                     u32x4 *__restrict__ out, unsigned char *__restrict__ eb, i64 out_stride) {
    constexpr int R = 256 / WQ;
    static_assert(R % 4 == 0, "four row sums per byte: WQ <= 64");
    __shared__ __attribute__((aligned(16))) unsigned char sb[R];
    const i64 cb = (i64)blockIdx.x * 256;
    if (cb >= n_chunks) return;                                      // surplus block of the padded grid
    const i64 c0 = cb + threadIdx.x;
    const bool ok = c0 < n_chunks;
    const u32x4 v = ok ? inner[c0] : (u32x4)(0u);
    const i64 o = blockIdx.y;
    const u32x4 r = outer[o * WQ + (threadIdx.x & (WQ - 1))];
    const u32x4 x = v ^ r;
    if (ok) __builtin_nontemporal_store(x, out + o * out_stride + c0);
    u32 s;
    if constexpr (WQ == 1) {                                         // the chunk is the whole row: x word, z word
        const u32 cy = __popc(x.x & x.z) + __popc(x.y & x.w);
        const u32 cf = INNER_LEFT ? __popc(v.x & r.z) + __popc(v.y & r.w) : __popc(v.z & r.x) + __popc(v.w & r.y);
        s = cy + 2u * cf;
    } else {
        // Y_out: both halves of the row form the same x & z words.  flip: lower half x_inner & z_outer, upper half z_inner & x_outer.
        u32 cy = __popc(x.x & other_half<WQ>(x.x));
        cy += __popc(x.y & other_half<WQ>(x.y));
        cy += __popc(x.z & other_half<WQ>(x.z));
        cy += __popc(x.w & other_half<WQ>(x.w));
        u32 cf = __popc(v.x & other_half<WQ>(r.x));
        cf += __popc(v.y & other_half<WQ>(r.y));
        cf += __popc(v.z & other_half<WQ>(r.z));
        cf += __popc(v.w & other_half<WQ>(r.w));
        s = half_row_sum<WQ>(cy + 2u * cf);
    }
    // the first lane of the half that holds x_left & z_right files the byte
    if ((threadIdx.x & (WQ - 1)) == (INNER_LEFT ? 0 : WQ / 2)) sb[threadIdx.x / WQ] = (unsigned char)(s & 3u);
    __syncthreads();
    if (threadIdx.x < R / 4) {
        const u32 q = reinterpret_cast<const u32 *>(sb)[threadIdx.x];      // the sums of rows 4t .. 4t + 3, one per byte
        const i64 gx = gridDim.x;
        eb[(o * gx + (i64)(blockIdx.x & 7) * (gx >> 3) + (i64)(blockIdx.x >> 3)) * (R / 4) + threadIdx.x] =
            (unsigned char)((q | q >> 6 | q >> 12 | q >> 18) & 0xffu);
    }
}

// phase sums -> coefficients: c_i * c_o * i^e, e = (3 (Y_i + Y_o) + s) mod 4, s the pair's 2-bit sum from k_mul_rows_e.  One lane per
// inner term, one workgroup per 256 consecutive inner terms of ONE outer row: every workgroup writes one contiguous 4 KiB piece with
// 16-byte non-temporal stores, and dispatch order (by * gx + bx) is address order — the sequential stream of the row kernel (four outer
// rows per workgroup, four interleaved streams Ni * 16 B apart, ran at 5.4 TB/s).  gx is a multiple of 8, so piece bx is always expanded
// by XCD bx % 8, whose L2 keeps its eighth of c_i / Y_i across the outer rows (file header); the surplus workgroups exit.  A byte
// holds the sums of 4 consecutive inner terms of one row block, which sit in one 256-term piece (R and 256 are multiples of 4).
// egx = grid.x of the row kernel, rshift = log2 R.
__global__ __launch_bounds__(256) void k_mul_coeff_expand(const unsigned char *__restrict__ eb, i64 egx, int rshift, const int *__restrict__ yi,
                                                           const int *__restrict__ yo, const double *__restrict__ ci, const double *__restrict__ co,
                                                           i64 Ni, double *__restrict__ out, i64 out_stride) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= Ni) return;
    const i64 o = blockIdx.y;
    const i64 R = 1LL << rshift, bx = i >> rshift, r = i & (R - 1);
    const u32 p = eb[(o * egx + (bx & 7) * (egx >> 3) + (bx >> 3)) * (R >> 2) + (r >> 2)];
    const double cor = co[2 * o], coi = co[2 * o + 1];                  // wave-uniform: scalar loads
    const int e = (int)((3u * ((u32)yi[i] + (u32)yo[o]) + (p >> (2 * (r & 3)))) & 3u);
    double re, im;
    pair_coefficient(ci[2 * i], ci[2 * i + 1], cor, coi, e, re, im);
    const f64x2 w = {re, im};
    __builtin_nontemporal_store(w, reinterpret_cast<f64x2 *>(out) + o * out_stride + i);
}

// Chunks (16 B) of the inner operand per launch of a row stream: all of it while an eighth fits an XCD's L2 with room to spare (3.5 MiB of
// 4), else equal tiles of at most 3 MiB per XCD — whole rows, whole 256-chunk blocks, gx a multiple of 8.  tile_mb > 0 (tests) sets the tile
// size in MiB of inner operand.
i64 inner_tile_chunks(i64 n_chunks, int Wq, double tile_mb) {
    i64 budget = (i64)24 << 20, whole = (i64)28 << 20;
    if (tile_mb > 0) budget = whole = (i64)(tile_mb * 1048576.0);
    if (n_chunks * 16 <= whole) return n_chunks;
    const i64 n_tiles = (n_chunks * 16 + budget - 1) / budget;
    i64 unit = 2048;                                                // 8 blocks of 256 chunks ...
    while (unit % Wq) unit += 2048;                                 // ... and whole rows (a power-of-two Wq <= 64 divides 2048)
    const i64 per = (n_chunks + n_tiles - 1) / n_tiles;
    return (per + unit - 1) / unit * unit;
}

// ---- launches: the switch over the template arguments of each kernel ------------------------------
template <bool NT> static auto rows_kernel(int rc) { return rc == 1 ? k_mul_rows<1, NT> : rc == 2 ? k_mul_rows<2, NT> : rc == 8 ? k_mul_rows<8, NT> : k_mul_rows<4, NT>; }
int launch_rows(const RowsVariant &rv, dim3 grid, const u32x4 *inner, i64 n_chunks, const u32x4 *outer, int Wq, i64 o_count, u32x4 *out, i64 out_stride) {
    ProfScope prof(0);
    hipLaunchKernelGGL(rv.nt ? rows_kernel<true>(rv.rc) : rows_kernel<false>(rv.rc), grid, dim3(rv.threads), 0, ctx().stream, inner, n_chunks, outer, Wq,
                       o_count, out, rv.rto, out_stride);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

template <int WQ> static auto rows_e_kernel(int inner_is_left) { return inner_is_left ? k_mul_rows_e<WQ, true> : k_mul_rows_e<WQ, false>; }
int launch_rows_e(int Wq, int inner_is_left, dim3 grid, const u32x4 *inner, i64 n_chunks, const u32x4 *outer, u32x4 *out, unsigned char *eb,
                  i64 out_stride) {
    ProfScope prof(0);
    const int l = inner_is_left;
    const auto kernel = Wq == 1 ? rows_e_kernel<1>(l) : Wq == 2 ? rows_e_kernel<2>(l) : Wq == 4 ? rows_e_kernel<4>(l) : Wq == 8 ? rows_e_kernel<8>(l)
                      : Wq == 16 ? rows_e_kernel<16>(l) : Wq == 32 ? rows_e_kernel<32>(l) : rows_e_kernel<64>(l);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx().stream, inner, n_chunks, outer, out, eb, out_stride);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

int launch_coeff_expand(dim3 grid, const unsigned char *eb, i64 egx, int rshift, const int *yi, const int *yo, const double *ci, const double *co,
                        i64 Ni, double *out, i64 out_stride) {
    hipLaunchKernelGGL(k_mul_coeff_expand, grid, dim3(256), 0, ctx().stream, eb, egx, rshift, yi, yo, ci, co, Ni, out, out_stride);
    KERNEL_CHECK();
    return SYMGPU_OK;
}

}  // namespace symgpu
