// ansatz.hip — |psi(theta)> = prod_k exp(i theta_k P_k) |ref> on a dense statevector, <psi|H|psi>, its gradient by one reverse (adjoint)
// sweep, and the gradient of a whole operator pool (conventions of matvec.hip: qubit 0 the MOST significant bit of b, x, z).
//   (P psi)[b] = (-i)^Y (-1)^{|b & z|} psi[b ^ x],   exp(i theta P) = cos theta + i sin theta P
// A rotation is one pass: the 2^(n-1) SLOTS t each own two elements — for x != 0 the pair (b0, b0 ^ x), b0 = t with a clear bit inserted
// at the top set bit of x; for x = 0 the elements t and t + 2^(n-1) — read both, write both.  Per element, every operation rounded once,
//   psi'[b] = (c a.re + w.re, c a.im + w.im),   w = (+-s p.re, +-s p.im) for odd Y, (-+s p.im, +-s p.re) for even Y,   p = psi[b ^ x],
// the sign from the parity of b & z and from Y >> 1 (exact sign changes), so a NumPy restatement gives the same bits.
// The sweep (symgpu_ansatz_energy_grad): lambda = H psi_K; for k = K-1 .. 0 one launch adds Im conj(lambda[b]) (P_k psi)[b] over the slots
// of a chunk from the values before the update and applies exp(-i theta_k P_k) to psi and lambda; g_k = -2 (sum of the chunk sums).
// Reductions: slots (sweep) or elements (pool) are cut into chunks of C = max(256, count / 1024) consecutive ones; thread t of 256 adds
// the terms of t, t + 256, ... of its chunk to 0 in ascending order (a slot's two terms added to each other first, b0's + b1's), the 256
// thread sums are folded by halving, and one launch adds the chunk sums to 0 in ascending chunk order.  No floating-point atomics.
// The TILED form of the forward rotations: fermionic excitations come as runs of generators that share a few X/Y positions, so the plan
// cuts the sequence greedily into runs whose X-supports, together with the AN_LOW lowest index bits, fit AN_TILE_BITS tile bits S; a
// workgroup loads the 2^|S| amplitudes that agree outside S into LDS, applies the run's rotations there (the same arithmetic per
// amplitude, the sign of the bits outside S uniform to the workgroup, a barrier between rotations) and writes the tile back: one pass
// over the vector per run instead of one per rotation.  A generator whose own support does not fit takes the direct pass.
#include "matvec.h"
#include <memory>
#include <vector>
#include <stdlib.h>
#include <string.h>

namespace symgpu {
struct AnSeg { i64 k0, k1; u32 S; int m; bool tiled; };   // generators k0 .. k1-1: one tiled run over the tile bits S (m of them), or direct passes
}

struct symgpu_ansatz_s {
    int device = 0;
    int n = 0;
    int64_t K = 0;
    int64_t n_runs = 0;                          // tiled runs among the segments
    symgpu::Scratch gens;                        // AnGen [K]
    symgpu::Scratch tgens;                       // AnGen [K]: x and z of a run's generator gathered to its tile bits, pad = z outside them
    std::vector<symgpu::AnSeg> segs;             // the whole sequence, in order
};

namespace symgpu {

constexpr int AN_WG = 256;
constexpr int AN_LOW = 4;                        // the lowest index bits belong to every tile: contiguous pieces of 2^4 amplitudes = 256 bytes
constexpr int AN_TILE_BITS = 12;                 // at most 2^12 amplitudes = 64 KiB of LDS a tile
constexpr int AN_PAD_BITS = 10;                  // a run that needs fewer tile bits takes the lowest free ones up to here (longer pieces, full workgroups)

struct AnGen { u32 x, z, y, pad; };              // X and Z part as n-bit integers, Y = |x & z| mod 4

static u64 an_chunk(u64 count) { return (count >> 10) > AN_WG ? (count >> 10) : AN_WG; }
static unsigned an_chunks(u64 count) { return (unsigned)((count + an_chunk(count) - 1) / an_chunk(count)); }

__device__ __forceinline__ AnGen an_gen_of_row(const u64 *__restrict__ rows, i64 t, int n) {
    const u32 x = (u32)(__brevll(rows[2 * t]) >> (64 - n)), z = (u32)(__brevll(rows[2 * t + 1]) >> (64 - n));
    return AnGen{x, z, (u32)__popc(x & z) & 3u, 0u};
}

__global__ __launch_bounds__(AN_WG) void k_an_gens(const u64 *__restrict__ rows, i64 K, int n, AnGen *__restrict__ gens) {
    const i64 t = (i64)blockIdx.x * AN_WG + threadIdx.x;
    if (t < K) gens[t] = an_gen_of_row(rows, t, n);
}

// the two elements of slot t < 2^(n-1)
__device__ __forceinline__ void an_slot(u32 x, int n, u64 t, u64 &b0, u64 &b1) {
    const int h = x ? 31 - __clz(x) : n - 1;
    b0 = ((t >> h) << (h + 1)) | (t & (((u64)1 << h) - 1));
    b1 = x ? b0 ^ (u64)x : b0 | ((u64)1 << h);
}

// c a + w o p, w = i s (-i)^Y (-1)^{|b & z|}
__device__ __forceinline__ f64x2 an_rot(f64x2 a, f64x2 p, double c, double s, u32 y, u64 b, u32 z) {
    const u32 neg = ((u32)__popcll(b & (u64)z) ^ (y >> 1)) & 1u;
    const double ss = neg ? -s : s;
    const double wr = (y & 1u) ? __dmul_rn(ss, p.x) : -__dmul_rn(ss, p.y);
    const double wi = (y & 1u) ? __dmul_rn(ss, p.y) : __dmul_rn(ss, p.x);
    return f64x2{__dadd_rn(__dmul_rn(c, a.x), wr), __dadd_rn(__dmul_rn(c, a.y), wi)};
}

// Im conj(l) (P psi)[b], p = psi[b ^ x]: (P psi)[b] = (-i)^Y sigma p
__device__ __forceinline__ double an_im_term(f64x2 l, f64x2 p, u32 y, u64 b, u32 z) {
    const u32 neg = ((u32)__popcll(b & (u64)z) ^ (y >> 1) ^ y) & 1u;      // Y: 0 -> +p, 1 -> -i p, 2 -> -p, 3 -> +i p
    const double qr = (y & 1u) ? -p.y : p.x, qi = (y & 1u) ? p.x : p.y;   // +i p for odd Y, the sign below
    const double v = __dsub_rn(__dmul_rn(l.x, qi), __dmul_rn(l.y, qr));
    return neg ? -v : v;
}

__device__ __forceinline__ double an_fold(double v, double *sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int h = AN_WG / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] = __dadd_rn(sm[threadIdx.x], sm[threadIdx.x + h]);
        __syncthreads();
    }
    return sm[0];
}

// psi <- exp(i theta_k P_k) psi, (c, s) = (cos, sin) theta_k: one thread per slot
__global__ __launch_bounds__(AN_WG) void k_an_apply(const AnGen *__restrict__ gens, i64 k, int n, double c, double s, f64x2 *psi) {
    const u64 t = (u64)blockIdx.x * AN_WG + threadIdx.x;
    if (t >= ((u64)1 << (n - 1))) return;
    const AnGen g = gens[k];
    u64 b0, b1;
    an_slot(g.x, n, t, b0, b1);
    const f64x2 a0 = psi[b0], a1 = psi[b1];
    psi[b0] = an_rot(a0, g.x ? a1 : a0, c, s, g.y, b0, g.z);
    psi[b1] = an_rot(a1, g.x ? a0 : a1, c, s, g.y, b1, g.z);
}

// partial[k][chunk] = sum over the chunk's slots of Im conj(lam[b]) (P_k psi)[b]; then psi <- U_k^+ psi, lam <- U_k^+ lam (s = -sin theta_k)
__global__ __launch_bounds__(AN_WG) void k_an_sweep(const AnGen *__restrict__ gens, i64 k, int n, double c, double s, f64x2 *psi, f64x2 *lam, u64 chunk,
                                                    unsigned chunks, double *__restrict__ partial) {
    __shared__ double sm[AN_WG];
    const u64 half = (u64)1 << (n - 1);
    const AnGen g = gens[k];
    const u64 t0 = (u64)blockIdx.x * chunk;
    const u64 t1 = t0 + chunk < half ? t0 + chunk : half;
    double im = 0.0;
    for (u64 t = t0 + threadIdx.x; t < t1; t += AN_WG) {
        u64 b0, b1;
        an_slot(g.x, n, t, b0, b1);
        const f64x2 a0 = psi[b0], a1 = psi[b1], l0 = lam[b0], l1 = lam[b1];
        const f64x2 p0 = g.x ? a1 : a0, p1 = g.x ? a0 : a1;
        im = __dadd_rn(im, __dadd_rn(an_im_term(l0, p0, g.y, b0, g.z), an_im_term(l1, p1, g.y, b1, g.z)));
        psi[b0] = an_rot(a0, p0, c, s, g.y, b0, g.z);
        psi[b1] = an_rot(a1, p1, c, s, g.y, b1, g.z);
        lam[b0] = an_rot(l0, g.x ? l1 : l0, c, s, g.y, b0, g.z);
        lam[b1] = an_rot(l1, g.x ? l0 : l1, c, s, g.y, b1, g.z);
    }
    const double total = an_fold(im, sm);
    if (threadIdx.x == 0) partial[(u64)k * chunks + blockIdx.x] = total;
}

// partial[j][chunk] = sum over the chunk's elements of Im conj(phi[b]) (P_j psi)[b], j = j0 + blockIdx.y a row of the pool
__global__ __launch_bounds__(AN_WG) void k_an_pool(const u64 *__restrict__ rows, i64 j0, int n, const f64x2 *__restrict__ psi, const f64x2 *__restrict__ phi,
                                                   u64 chunk, unsigned chunks, double *__restrict__ partial) {
    __shared__ double sm[AN_WG];
    const u64 N = (u64)1 << n;
    const i64 j = j0 + blockIdx.y;
    const AnGen g = an_gen_of_row(rows, j, n);
    const u64 b0 = (u64)blockIdx.x * chunk;
    const u64 b1 = b0 + chunk < N ? b0 + chunk : N;
    double im = 0.0;
    for (u64 b = b0 + threadIdx.x; b < b1; b += AN_WG) im = __dadd_rn(im, an_im_term(phi[b], psi[b ^ (u64)g.x], g.y, b, g.z));
    const double total = an_fold(im, sm);
    if (threadIdx.x == 0) partial[(u64)j * chunks + blockIdx.x] = total;
}

// out[i] = -2 (0 + partial[i][0] + partial[i][1] + ...)
__global__ __launch_bounds__(AN_WG) void k_an_grad(const double *__restrict__ partial, unsigned chunks, i64 count, double *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * AN_WG + threadIdx.x;
    if (i >= count) return;
    double im = 0.0;
    for (unsigned c = 0; c < chunks; ++c) im = __dadd_rn(im, partial[(u64)i * chunks + c]);
    out[i] = __dmul_rn(-2.0, im);
}

// the bits of v, lowest first, to the set positions of mask, lowest first
__host__ __device__ __forceinline__ u64 an_deposit(u64 v, u64 mask) {
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
static u32 an_extract(u32 v, u32 mask) {
    u32 r = 0;
    for (int at = 0; mask; mask &= mask - 1, ++at)
        if (v & mask & (~mask + 1)) r |= 1u << at;
    return r;
}

// one run in LDS: workgroup = tile (the 2^m amplitudes that agree outside S); rotations k0 .. k1-1 (reverse: from the last down);
// cs = cos [K] then sin [K]
__global__ __launch_bounds__(AN_WG) void k_an_tile(const AnGen *__restrict__ tgens, const double *__restrict__ cs, i64 K, i64 k0, i64 k1, int reverse, u32 S,
                                                   int m, int n, f64x2 *psi) {
    extern __shared__ f64x2 an_tile[];
    const u64 base = an_deposit((u64)blockIdx.x, (((u64)1 << n) - 1) & ~(u64)S);      // the tile number spread over the bits outside S
    const u32 L = 1u << m;
    for (u32 l = threadIdx.x; l < L; l += AN_WG) an_tile[l] = psi[base | an_deposit(l, S)];
    __syncthreads();
    for (i64 i = 0; i < k1 - k0; ++i) {
        const i64 k = reverse ? k1 - 1 - i : k0 + i;
        const AnGen g = tgens[k];
        const double c = cs[k], s = cs[K + k];
        const u32 y = g.y ^ (((u32)__popcll(base & (u64)g.pad) & 1u) << 1);      // the sign of the bits outside the tile joins Y >> 1
        for (u32 t = threadIdx.x; t < (L >> 1); t += AN_WG) {
            u64 b0, b1;
            an_slot(g.x, m, t, b0, b1);
            const f64x2 a0 = an_tile[b0], a1 = an_tile[b1];
            an_tile[b0] = an_rot(a0, g.x ? a1 : a0, c, s, y, b0, g.z);
            an_tile[b1] = an_rot(a1, g.x ? a0 : a1, c, s, y, b1, g.z);
        }
        __syncthreads();
    }
    for (u32 l = threadIdx.x; l < L; l += AN_WG) psi[base | an_deposit(l, S)] = an_tile[l];
}

// The cut rule.  Walk the generators in order; the open run's tile bits S start as the AN_LOW lowest bits and grow by each generator's
// X-part while |S| <= min(n, AN_TILE_BITS); x = 0 joins any open run; a generator that does not fit closes the run and opens the next
// with its own X-part, or, if AN_LOW bits and its own X-part exceed the budget, takes a direct pass.  A closed run with fewer than
// min(n, AN_PAD_BITS) tile bits takes the lowest free bits up to that number (the cuts do not depend on it).
static void an_plan_runs(const std::vector<AnGen> &g, int n, std::vector<AnSeg> *segs, int64_t *n_runs) {
    const int cap = n < AN_TILE_BITS ? n : AN_TILE_BITS, pad = n < AN_PAD_BITS ? n : AN_PAD_BITS;
    const u32 low = (1u << (n < AN_LOW ? n : AN_LOW)) - 1;
    bool open = false;
    u32 S = low;
    i64 k0 = 0;
    auto close = [&](i64 k) {
        if (!open) return;
        for (int bit = 0; __builtin_popcount(S) < pad; ++bit) S |= 1u << bit;
        segs->push_back(AnSeg{k0, k, S, __builtin_popcount(S), true});
        ++*n_runs;
        open = false;
    };
    for (i64 k = 0; k < (i64)g.size(); ++k) {
        const u32 x = g[k].x;
        if (open && __builtin_popcount(S | x) <= cap) {
            S |= x;
            continue;
        }
        close(k);
        if (__builtin_popcount(low | x) <= cap) {
            open = true;
            S = low | x;
            k0 = k;
        } else if (!segs->empty() && !segs->back().tiled && segs->back().k1 == k) {
            segs->back().k1 = k + 1;
        } else {
            segs->push_back(AnSeg{k, k + 1, 0, 0, false});
        }
    }
    close((i64)g.size());
}

static bool an_force_direct() {
    const char *f = getenv("SYMGPU_ANSATZ_FORM");
    return f && !strcmp(f, "direct");
}

// rotations k_begin .. k_end-1 with direct passes (reverse: from the last down) on the context's stream; sign = -1 applies the inverses
static int an_rotate_direct(const symgpu_ansatz_s *p, const double *cos_t, const double *sin_t, i64 k_begin, i64 k_end, bool reverse, double sign, f64x2 *psi) {
    hipStream_t st = ctx().stream;
    const unsigned grid = grid_each((i64)1 << (p->n - 1), AN_WG);
    for (i64 i = k_begin; i < k_end; ++i) {
        const i64 k = reverse ? k_end - 1 - (i - k_begin) : i;
        hipLaunchKernelGGL(k_an_apply, dim3(grid), dim3(AN_WG), 0, st, p->gens.as<AnGen>(), k, p->n, cos_t[k], sign * sin_t[k], psi);
    }
    if (k_end > k_begin) KERNEL_CHECK();
    return SYMGPU_OK;
}

// The same rotations by the plan's segments, each clipped to the range: a tiled run is one launch, cos and sin read from `cs` (device,
// cos [K] then sin [K], uploaded here into the caller's scratch of 16 K bytes).  *form: SYMGPU_ANSATZ_* of what ran.
static int an_rotate(const symgpu_ansatz_s *p, const double *cos_t, const double *sin_t, i64 k_begin, i64 k_end, bool reverse, f64x2 *psi, Scratch *cs, int *form) {
    *form = 0;
    if (k_end <= k_begin) return SYMGPU_OK;
    if (p->n_runs == 0 || an_force_direct()) {
        *form = SYMGPU_ANSATZ_DIRECT;
        return an_rotate_direct(p, cos_t, sin_t, k_begin, k_end, reverse, 1.0, psi);
    }
    hipStream_t st = ctx().stream;
    const i64 K = p->K;
    SG_TRY(cs->alloc((size_t)K * 16));
    HIP_TRY(hipMemcpyAsync(cs->p, cos_t, (size_t)K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(cs->as<double>() + K, sin_t, (size_t)K * 8, hipMemcpyHostToDevice, st));
    const i64 n_segs = (i64)p->segs.size();
    for (i64 i = 0; i < n_segs; ++i) {
        const AnSeg &sg = p->segs[reverse ? n_segs - 1 - i : i];
        const i64 k0 = sg.k0 > k_begin ? sg.k0 : k_begin, k1 = sg.k1 < k_end ? sg.k1 : k_end;
        if (k0 >= k1) continue;
        if (!sg.tiled) {
            SG_TRY(an_rotate_direct(p, cos_t, sin_t, k0, k1, reverse, 1.0, psi));
            *form |= SYMGPU_ANSATZ_DIRECT;
            continue;
        }
        hipLaunchKernelGGL(k_an_tile, dim3((unsigned)((u64)1 << (p->n - sg.m))), dim3(AN_WG), (size_t)16 << sg.m, st, p->tgens.as<AnGen>(), cs->as<double>(), K, k0,
                           k1, reverse ? 1 : 0, sg.S, sg.m, p->n, psi);
        KERNEL_CHECK();
        *form |= SYMGPU_ANSATZ_TILED;
    }
    return SYMGPU_OK;
}

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_ansatz_plan(symgpu_op_t gens, int n_qubits, struct symgpu_ansatz_s **plan) {
    SG_ENTER(gens);
    SG_REQUIRE(gens && plan, "ansatz_plan: arguments");
    *plan = nullptr;
    SG_REQUIRE(n_qubits >= 1 && n_qubits <= 32, "ansatz_plan: 1 <= n_qubits <= 32");
    SG_REQUIRE(gens->Wq == 1, "ansatz_plan: the generators' rows have more than one word per half (Wq = 1 wanted)");
    SG_REQUIRE(gens->T < ((i64)1 << 31), "ansatz_plan: K >= 2^31");
    std::unique_ptr<symgpu_ansatz_s> p(new symgpu_ansatz_s());
    p->device = gens->device;
    p->n = n_qubits;
    p->K = gens->T;
    if (p->K > 0) {
        SG_TRY(matvec_require_memory(2 * (u64)p->K * sizeof(AnGen) + 4096, "the ansatz plan"));
        SG_TRY(p->gens.alloc((size_t)p->K * sizeof(AnGen)));
        hipLaunchKernelGGL(k_an_gens, dim3(grid_each(p->K, AN_WG)), dim3(AN_WG), 0, ctx().stream, gens->rows, p->K, n_qubits, p->gens.as<AnGen>());
        KERNEL_CHECK();
        std::vector<AnGen> host((size_t)p->K);
        SG_TRY(download_any(p->gens.p, host.data(), (size_t)p->K * sizeof(AnGen)));    // the operator is not referenced once the call has returned
        an_plan_runs(host, n_qubits, &p->segs, &p->n_runs);
        for (const AnSeg &sg : p->segs)
            for (i64 k = sg.k0; k < sg.k1 && sg.tiled; ++k)
                host[(size_t)k] = AnGen{an_extract(host[(size_t)k].x, sg.S), an_extract(host[(size_t)k].z, sg.S), host[(size_t)k].y, host[(size_t)k].z & ~sg.S};
        if (p->n_runs > 0) {
            SG_TRY(p->tgens.alloc((size_t)p->K * sizeof(AnGen)));
            SG_TRY(symgpu_dev_upload(p->tgens.p, host.data(), p->K * (int64_t)sizeof(AnGen)));
        }
    }
    *plan = p.release();
    return SYMGPU_OK;
}

int symgpu_ansatz_free(struct symgpu_ansatz_s *plan) {
    SG_REQUIRE(plan, "ansatz_free: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    delete plan;
    return SYMGPU_OK;
}

int symgpu_ansatz_info(struct symgpu_ansatz_s *plan, int *n_qubits, int64_t *n_generators, int64_t *n_runs, int64_t *device_bytes) {
    SG_REQUIRE(plan, "ansatz_info: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (n_qubits) *n_qubits = plan->n;
    if (n_generators) *n_generators = plan->K;
    if (n_runs) *n_runs = plan->n_runs;
    if (device_bytes) *device_bytes = plan->K * (int64_t)sizeof(AnGen) * (plan->n_runs > 0 ? 2 : 1);
    return SYMGPU_OK;
}

int symgpu_ansatz_apply(struct symgpu_ansatz_s *plan, const double *cos_t, const double *sin_t, int64_t k_begin, int64_t k_end, int reverse, double *psi_dev,
                        int *form) {
    SG_REQUIRE(plan, "ansatz_apply: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    if (form) *form = 0;
    SG_REQUIRE(psi_dev, "ansatz_apply: null state");
    SG_REQUIRE(k_begin >= 0 && k_begin <= k_end && k_end <= plan->K, "ansatz_apply: 0 <= k_begin <= k_end <= K");
    SG_REQUIRE((cos_t && sin_t) || k_begin == k_end, "ansatz_apply: null angles");
    if (k_end > k_begin && plan->n_runs > 0) SG_TRY(matvec_require_memory((u64)plan->K * 16 + 4096, "the angles"));
    Scratch cs;
    int ran = 0;
    SG_TRY(an_rotate(plan, cos_t, sin_t, k_begin, k_end, reverse != 0, reinterpret_cast<f64x2 *>(psi_dev), &cs, &ran));
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    if (form) *form = ran;
    return SYMGPU_OK;
}

int symgpu_ansatz_energy_grad(struct symgpu_ansatz_s *plan, struct symgpu_matvec_s *plan_H, const double *cos_t, const double *sin_t, const double *ref_dev,
                              double *psi_out_dev, double *energy, double *grad_host) {
    SG_REQUIRE(plan && plan_H, "ansatz_energy_grad: null plan");
    const symgpu_op_s scope_op = scope_of_device(plan->device);
    SG_ENTER(&scope_op);
    SG_REQUIRE(plan_H->device == plan->device && plan_H->xg.n == plan->n, "ansatz_energy_grad: the two plans differ in device or qubit count");
    SG_REQUIRE(ref_dev && energy, "ansatz_energy_grad: arguments");
    const i64 K = plan->K;
    SG_REQUIRE((cos_t && sin_t) || K == 0, "ansatz_energy_grad: null angles");
    hipStream_t st = ctx().stream;
    const int n = plan->n;
    const u64 N = (u64)1 << n, half = N >> 1;
    const unsigned chunks = an_chunks(half);
    const bool grad = grad_host && K > 0;
    const u64 partial_bytes = grad ? (u64)K * chunks * 8 : 0;
    SG_TRY(matvec_require_memory(2 * N * 16 + partial_bytes + (u64)lz_chunks(N) * 16 + (u64)(K + 1) * 8 + (u64)K * 16 + 4096, "the energy and gradient"));
    Scratch psi, phi, dots, h, res, partial, cs;
    int ran = 0;
    SG_TRY(psi.alloc((size_t)N * 16));
    SG_TRY(phi.alloc((size_t)N * 16));
    SG_TRY(dots.alloc((size_t)lz_chunks(N) * 16));
    SG_TRY(h.alloc(16));
    SG_TRY(res.alloc((size_t)(K + 1) * 8));                    // g_0 .. g_{K-1}, E
    if (grad) SG_TRY(partial.alloc((size_t)partial_bytes));
    HIP_TRY(hipMemcpyAsync(psi.p, ref_dev, (size_t)N * 16, hipMemcpyDeviceToDevice, st));
    SG_TRY(an_rotate(plan, cos_t, sin_t, 0, K, false, psi.as<f64x2>(), &cs, &ran));
    SG_TRY(matvec_launch(plan_H, psi.as<f64x2>(), phi.as<f64x2>(), nullptr, nullptr));
    SG_TRY(lz_inner(psi.as<f64x2>(), phi.as<f64x2>(), N, dots.as<f64x2>(), h.as<f64x2>(), res.as<double>() + K));
    if (psi_out_dev) HIP_TRY(hipMemcpyAsync(psi_out_dev, psi.p, (size_t)N * 16, hipMemcpyDeviceToDevice, st));
    if (grad) {
        for (i64 k = K - 1; k >= 0; --k)
            hipLaunchKernelGGL(k_an_sweep, dim3(chunks), dim3(AN_WG), 0, st, plan->gens.as<AnGen>(), k, n, cos_t[k], -sin_t[k], psi.as<f64x2>(), phi.as<f64x2>(),
                               an_chunk(half), chunks, partial.as<double>());
        hipLaunchKernelGGL(k_an_grad, dim3(grid_each(K, AN_WG)), dim3(AN_WG), 0, st, partial.as<double>(), chunks, K, res.as<double>());
        KERNEL_CHECK();
        std::unique_ptr<double[]> back(new double[K + 1]);
        SG_TRY(download_any(res.p, back.get(), (size_t)(K + 1) * 8));
        memcpy(grad_host, back.get(), (size_t)K * 8);
        *energy = back[K];
    } else {
        SG_TRY(download_any(res.as<double>() + K, energy, 8));
    }
    return SYMGPU_OK;
}

int symgpu_pool_gradient(struct symgpu_matvec_s *plan_H, symgpu_op_t pool, const double *psi_dev, double *energy, double *grad_host) {
    SG_REQUIRE(plan_H && pool, "pool_gradient: arguments");
    SG_ENTER(pool);
    SG_REQUIRE(plan_H->device == pool->device, "pool_gradient: the plan and the pool live on two devices");
    SG_REQUIRE(pool->Wq == 1, "pool_gradient: the pool's rows have more than one word per half (Wq = 1 wanted)");
    SG_REQUIRE(pool->T < ((i64)1 << 31), "pool_gradient: M >= 2^31");
    const i64 M = pool->T;
    if (M == 0 && !energy) return SYMGPU_OK;
    SG_REQUIRE(psi_dev && (grad_host || M == 0), "pool_gradient: null buffers");
    hipStream_t st = ctx().stream;
    const int n = plan_H->xg.n;
    const u64 N = (u64)1 << n;
    const unsigned chunks = an_chunks(N);
    SG_TRY(matvec_require_memory(N * 16 + (u64)M * chunks * 8 + (u64)lz_chunks(N) * 16 + (u64)(M + 1) * 8 + 4096, "the pool gradient"));
    Scratch phi, dots, h, res, partial;
    SG_TRY(phi.alloc((size_t)N * 16));
    SG_TRY(dots.alloc((size_t)lz_chunks(N) * 16));
    SG_TRY(h.alloc(16));
    SG_TRY(res.alloc((size_t)(M + 1) * 8));                    // g_0 .. g_{M-1}, E
    SG_TRY(partial.alloc((size_t)M * chunks * 8));
    const f64x2 *psi = reinterpret_cast<const f64x2 *>(psi_dev);
    SG_TRY(matvec_launch(plan_H, psi, phi.as<f64x2>(), nullptr, nullptr));
    SG_TRY(lz_inner(psi, phi.as<f64x2>(), N, dots.as<f64x2>(), h.as<f64x2>(), res.as<double>() + M));
    for (i64 j0 = 0; j0 < M; j0 += 32768) {
        const unsigned rows_now = (unsigned)(M - j0 < 32768 ? M - j0 : 32768);
        hipLaunchKernelGGL(k_an_pool, dim3(chunks, rows_now), dim3(AN_WG), 0, st, pool->rows, j0, n, psi, phi.as<f64x2>(), an_chunk(N), chunks, partial.as<double>());
    }
    if (M > 0) hipLaunchKernelGGL(k_an_grad, dim3(grid_each(M, AN_WG)), dim3(AN_WG), 0, st, partial.as<double>(), chunks, M, res.as<double>());
    KERNEL_CHECK();
    std::unique_ptr<double[]> back(new double[M + 1]);
    SG_TRY(download_any(res.p, back.get(), (size_t)(M + 1) * 8));
    if (M > 0) memcpy(grad_host, back.get(), (size_t)M * 8);
    if (energy) *energy = back[M];
    return SYMGPU_OK;
}

}  // extern "C"
