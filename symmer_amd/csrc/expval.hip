// expval.hip — every term of <phi|H|psi> in one call (reference PauliwordOp.expval / single_term_expval, symmer/operators/base.py:796-819,
// 2438-2471, which run one operator x state product pair per term):
//   symgpu_expval_terms_dev   for a term with symplectic row (x, z) and Y count y = |x & z|
//                                 <phi|P|psi> = i^y  sum over b in supp psi with b ^ x in supp phi of  conj(phi[b ^ x]) psi[b] (-1)^|z & b|
//                             No product is materialised: one look-up of b ^ x among phi's basis strings per (term, basis state).
// The look-up is an open-addressing table over phi's rows (as k_join_insert / k_join_probe of project.hip).  The cleanup hash is GF(2)-linear
// and the row of the basis string b ^ x is row_b ^ (x, x) (the Z half of a state's row is ~X below n), so the key of (k, b) is
// h(row_b) ^ h((x_k, x_k)): one hash per state, one per term, none per pair.  Exactness never rests on the hash: a slot is confirmed by
// comparing the X-half words.
// Mapping: lanes over terms, the basis state wave-uniform; the state axis is cut into chunks whose size depends on the number of states
// only (ev_chunk), every chunk's sum runs in state order, and a second kernel adds the chunks in ascending order: no floating-point
// atomics, no cross-lane reduction, the same bits on every run and in both forms.  The forms differ in where phi's side lives:
//   SYMGPU_EXPVAL_LDS      table, phi's coefficients and phi's X halves staged into LDS once per workgroup (ev_lds_bytes <= EV_LDS_MAX)
//   SYMGPU_EXPVAL_GLOBAL   all three stay in memory
#include "common.h"
#include "rotate_common.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace symgpu {

constexpr size_t EV_LDS_MAX = 64 * 1024;      // bytes of LDS the staged form may take (a workgroup's default limit: no attribute to ask for)
constexpr int EV_UB = 4;                      // basis states whose first table slot is loaded before any of them is followed up

// slots of the table over S rows: a power of two, at least 2 S (and 64)
static size_t ev_table_cap(i64 S) {
    size_t cap = 64;
    while ((i64)cap < 2 * S) cap <<= 1;
    return cap;
}
// what the staged form keeps in LDS: 16 bytes of coefficient and Wq words of X half per row of phi, 4 bytes per table slot
static size_t ev_lds_bytes(i64 S, int Wq) { return (size_t)S * (16 + 8 * (size_t)Wq) + 4 * ev_table_cap(S); }
// states per chunk: 64, or the power of two at or above S / 64 where that is more (at most 64 chunks; 64 up to S = 4096, so that
// a molecular-size state still spreads over tens of workgroups per term tile)
static i64 ev_chunk(i64 S) {
    i64 c = 64;
    while (c * 64 < S) c <<= 1;
    return c;
}

// (x_k, x_k) of every term: the row that takes a state's row to the row of the state P_k maps it to
__global__ __launch_bounds__(256) void k_ev_xx_rows(const u64 *__restrict__ rows, i64 T, int Wq, u64 *__restrict__ xx) {
    const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * Wq) return;
    const i64 k = idx / Wq;
    const int w = (int)(idx - k * Wq);
    const u64 x = rows[k * 2 * Wq + w];
    xx[k * 2 * Wq + w] = x;
    xx[k * 2 * Wq + Wq + w] = x;
}

__global__ __launch_bounds__(256) void k_ev_insert(const u64 *__restrict__ h, i64 S, u32 *__restrict__ table, u32 mask) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    u32 p = (u32)mix64(h[j]) & mask;
    while (atomicCAS(&table[p], 0u, (u32)(j + 1)) != 0u) p = (p + 1) & mask;
}

struct EvArgs {
    const u64 *op_rows;                        // [T][2 Wq]
    const u64 *hx;                             // [T] h((x_k, x_k))
    i64 T;
    int Wq;
    const u64 *psi_rows;                       // [S_psi][2 Wq]
    const double *psi_c;
    const u64 *hpsi;                           // [S_psi] h(row_b)
    i64 S_psi;
    const u64 *phi_rows;                       // [S_phi][2 Wq]
    const double *phi_c;
    i64 S_phi;
    const u32 *table;                          // [mask + 1]: row of phi + 1, 0 = empty
    u32 mask;
    i64 chunk;                                 // states per blockIdx.y
    f64x2 *partial;                            // [chunks][T]
};

// partial[c][k] = sum over the states b of chunk c, in order, of conj(phi[b ^ x_k]) psi[b] (-1)^|z_k & b| (without i^y)
template <bool WQ1, bool LDS>
__global__ __launch_bounds__(256) void k_ev_probe(const EvArgs a) {
    extern __shared__ __align__(16) unsigned char ev_lds[];
    const int Wq = WQ1 ? 1 : a.Wq;
    const u32 *tab = a.table;
    const u64 *px = a.phi_rows;
    const f64x2 *pc = reinterpret_cast<const f64x2 *>(a.phi_c);
    int pstride = 2 * Wq;
    if constexpr (LDS) {
        f64x2 *s_c = reinterpret_cast<f64x2 *>(ev_lds);
        u64 *s_x = reinterpret_cast<u64 *>(s_c + a.S_phi);
        u32 *s_t = reinterpret_cast<u32 *>(s_x + a.S_phi * Wq);
        for (i64 j = threadIdx.x; j < a.S_phi; j += 256) s_c[j] = pc[j];
        for (i64 i = threadIdx.x; i < a.S_phi * Wq; i += 256) s_x[i] = px[(i / Wq) * 2 * Wq + (i % Wq)];
        for (u32 p = threadIdx.x; p <= a.mask; p += 256) s_t[p] = tab[p];
        __syncthreads();
        tab = s_t; px = s_x; pc = s_c; pstride = Wq;
    }
    const i64 k_raw = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool live = k_raw < a.T;
    const i64 k = live ? k_raw : a.T - 1;                            // a lane past the end repeats the last term and writes nothing
    const u64 *term = a.op_rows + k * 2 * Wq;
    const u64 hxk = a.hx[k];
    const u64 x0 = term[0], z0 = term[Wq];
    const u32 mask = a.mask;
    const i64 b_lo = (i64)blockIdx.y * a.chunk;
    const i64 b_hi = b_lo + a.chunk < a.S_psi ? b_lo + a.chunk : a.S_psi;
    const f64x2 *qc = reinterpret_cast<const f64x2 *>(a.psi_c);
    double re = 0.0, im = 0.0;
    for (i64 b0 = b_lo; b0 < b_hi; b0 += EV_UB) {
        u32 p[EV_UB], e[EV_UB];
#pragma unroll
        for (int u = 0; u < EV_UB; ++u) {
            const i64 b = b0 + u < b_hi ? b0 + u : b_hi - 1;
            p[u] = (u32)mix64(a.hpsi[b] ^ hxk) & mask;
            e[u] = tab[p[u]];
        }
#pragma unroll
        for (int u = 0; u < EV_UB; ++u) {
            const i64 b = b0 + u;
            if (b >= b_hi) break;                                   // uniform
            const u64 *brow = a.psi_rows + b * 2 * Wq;               // uniform: the state's X half
            u32 pp = p[u], ee = e[u];
            while (ee != 0u) {
                const i64 j = (i64)ee - 1;
                bool same;
                if constexpr (WQ1) same = px[j * pstride] == (brow[0] ^ x0);
                else {
                    same = true;
                    for (int w = 0; w < Wq; ++w) same &= px[j * pstride + w] == (brow[w] ^ term[w]);
                }
                if (same) {
                    u64 par;
                    if constexpr (WQ1) par = z0 & brow[0];
                    else {
                        par = 0;
                        for (int w = 0; w < Wq; ++w) par ^= term[Wq + w] & brow[w];
                    }
                    const f64x2 f = pc[j], c = qc[b];
                    const double pr = __dadd_rn(__dmul_rn(f.x, c.x), __dmul_rn(f.y, c.y));      // conj(f) * c
                    const double pi = __dsub_rn(__dmul_rn(f.x, c.y), __dmul_rn(f.y, c.x));
                    const bool neg = __popcll(par) & 1;
                    re = __dadd_rn(re, neg ? -pr : pr);
                    im = __dadd_rn(im, neg ? -pi : pi);
                    break;
                }
                pp = (pp + 1) & mask;
                ee = tab[pp];
            }
        }
    }
    if (live) a.partial[(i64)blockIdx.y * a.T + k] = f64x2{re, im};
}

// terms[k] = i^y_k (0 + partial[0][k] + partial[1][k] + ...), prod[k] = c_k terms[k]
__global__ __launch_bounds__(256) void k_ev_combine(const f64x2 *__restrict__ partial, i64 T, int chunks, const u64 *__restrict__ rows, int Wq,
                                                     const double *__restrict__ coeff, f64x2 *__restrict__ terms, f64x2 *__restrict__ prod) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= T) return;
    double re = 0.0, im = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const f64x2 v = partial[(i64)c * T + k];
        re = __dadd_rn(re, v.x);
        im = __dadd_rn(im, v.y);
    }
    int y = 0;
    for (int w = 0; w < Wq; ++w) y += __popcll(rows[k * 2 * Wq + w] & rows[k * 2 * Wq + Wq + w]);
    double er, ei;
    apply_phase(re, im, y & 3, er, ei);
    terms[k] = f64x2{er, ei};
    const f64x2 c = reinterpret_cast<const f64x2 *>(coeff)[k];
    double qr, qi;
    pair_coefficient(c.x, c.y, er, ei, 0, qr, qi);
    prod[k] = f64x2{qr, qi};
}

template <bool WQ1, bool LDS>
static void ev_launch(const EvArgs &a, dim3 grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((k_ev_probe<WQ1, LDS>), grid, dim3(256), lds, st, a);
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_expval_terms_dev(symgpu_op_t op, symgpu_op_t phi, symgpu_op_t psi, double *out_terms, double *out_total, int *form) {
    SG_ENTER(op, phi, psi);
    if (form) *form = 0;
    SG_REQUIRE(op && phi && psi && out_total, "expval_terms_dev: null argument");
    SG_REQUIRE(phi->Wq == op->Wq && psi->Wq == op->Wq, "expval_terms_dev: the states' Wq differs from the operator's");
    SG_REQUIRE(op->coeff || op->T == 0, "expval_terms_dev: operator has no coefficients");
    SG_REQUIRE((phi->coeff || phi->T == 0) && (psi->coeff || psi->T == 0), "expval_terms_dev: states have no coefficients");
    SG_REQUIRE(phi->dup_free && psi->dup_free, "expval_terms_dev: both states must come from a cleanup");
    const i64 T = op->T, S_phi = phi->T, S_psi = psi->T;
    SG_REQUIRE(S_phi < ((i64)1 << 31) && S_psi < ((i64)1 << 31), "expval_terms_dev: too many basis states");
    out_total[0] = out_total[1] = 0.0;
    if (out_terms && T > 0) memset(out_terms, 0, (size_t)T * 16);
    if (T == 0 || S_phi == 0 || S_psi == 0) return SYMGPU_OK;
    hipStream_t st = ctx().stream;
    const int Wq = op->Wq, W = 2 * Wq;
    const size_t cap = ev_table_cap(S_phi), lds = ev_lds_bytes(S_phi, Wq);
    const char *forced = getenv("SYMGPU_EXPVAL_FORM");
    const bool use_lds = lds <= EV_LDS_MAX && !(forced && strcmp(forced, "global") == 0);
    const i64 chunk = ev_chunk(S_psi);
    const int chunks = (int)((S_psi + chunk - 1) / chunk);
    const i64 tiles = (T + 255) / 256;
    SG_REQUIRE(tiles < ((i64)1 << 31), "expval_terms_dev: too many terms");

    Scratch hphi, hpsi, xx, hx, table, partial, result;              // result: terms [T], the total, then the products [T]
    SG_TRY(hphi.alloc((size_t)S_phi * 8));
    if (psi != phi) SG_TRY(hpsi.alloc((size_t)S_psi * 8));
    SG_TRY(xx.alloc((size_t)T * W * 8));
    SG_TRY(hx.alloc((size_t)T * 8));
    SG_TRY(table.alloc(cap * 4));
    SG_TRY(partial.alloc((size_t)chunks * T * 16));
    SG_TRY(result.alloc((size_t)(2 * T + 1) * 16));
    SG_TRY(ensure_hash_tables(ctx().hash_tab ? ctx().hash_seed : 1));
    SG_TRY(hash_rows(phi->rows, S_phi, W, hphi.as<u64>()));
    if (psi != phi) SG_TRY(hash_rows(psi->rows, S_psi, W, hpsi.as<u64>()));
    hipLaunchKernelGGL(k_ev_xx_rows, dim3(grid_each(T * Wq)), dim3(256), 0, st, op->rows, T, Wq, xx.as<u64>());
    KERNEL_CHECK();
    SG_TRY(hash_rows(xx.as<u64>(), T, W, hx.as<u64>()));
    HIP_TRY(hipMemsetAsync(table.p, 0, cap * 4, st));
    hipLaunchKernelGGL(k_ev_insert, dim3(grid_each(S_phi)), dim3(256), 0, st, hphi.as<u64>(), S_phi, table.as<u32>(), (u32)(cap - 1));
    KERNEL_CHECK();

    EvArgs a;
    a.op_rows = op->rows; a.hx = hx.as<u64>(); a.T = T; a.Wq = Wq;
    a.psi_rows = psi->rows; a.psi_c = psi->coeff; a.hpsi = psi != phi ? hpsi.as<u64>() : hphi.as<u64>(); a.S_psi = S_psi;
    a.phi_rows = phi->rows; a.phi_c = phi->coeff; a.S_phi = S_phi;
    a.table = table.as<u32>(); a.mask = (u32)(cap - 1);
    a.chunk = chunk; a.partial = partial.as<f64x2>();
    const dim3 grid((unsigned)tiles, (unsigned)chunks);
    if (use_lds) { if (Wq == 1) ev_launch<true, true>(a, grid, lds, st); else ev_launch<false, true>(a, grid, lds, st); }
    else         { if (Wq == 1) ev_launch<true, false>(a, grid, 0, st); else ev_launch<false, false>(a, grid, 0, st); }
    KERNEL_CHECK();
    f64x2 *terms = result.as<f64x2>(), *total = terms + T, *prod = total + 1;
    hipLaunchKernelGGL(k_ev_combine, dim3((unsigned)tiles), dim3(256), 0, st, partial.as<f64x2>(), T, chunks, op->rows, Wq, op->coeff, terms, prod);
    KERNEL_CHECK();
    SG_TRY(ordered_sum_dev(prod, T, total));                         // in term order
    // the one read-back: the total alone through the mailbox, or the terms with the total behind them
    if (!out_terms) {
        u32 w[4] = {0, 0, 0, 0};
        SG_TRY(read_back_words(reinterpret_cast<const u32 *>(total), 4, nullptr, 0, w));
        memcpy(out_total, w, 16);
    } else {
        std::vector<double> host((size_t)(T + 1) * 2);
        SG_TRY(download_any(terms, host.data(), (size_t)(T + 1) * 16));
        memcpy(out_terms, host.data(), (size_t)T * 16);
        memcpy(out_total, host.data() + 2 * T, 16);
        count_d2h((size_t)(T + 1) * 16);
    }
    if (form) *form = use_lds ? SYMGPU_EXPVAL_LDS : SYMGPU_EXPVAL_GLOBAL;
    return SYMGPU_OK;
}

}  // extern "C"
