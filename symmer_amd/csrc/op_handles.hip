// op_handles.hip — operator handles: allocation, upload / download (packed and np.bool_ layout), copy, clone, scale, random; their small kernels.
#include "common.h"
#include <stdlib.h>

namespace symgpu {

__device__ __forceinline__ u64 splitmix64(u64 x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

// synthetic operator: each bit set with probability `density` (compared on 16-bit slices of a counter hash),
// coefficients from a Box-Muller pair; padding bits zero.
__global__ void k_random_op(u64 *__restrict__ rows, double *__restrict__ coeff, i64 T, int n, int Wq, u32 thresh16, u64 seed) {
    i64 total = T * (i64)(2 * Wq);
    for (i64 idx = (i64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (i64)gridDim.x * blockDim.x) {
        int w = (int)(idx % (2 * Wq));
        int wq = w % Wq;
        u64 word = 0;
        for (int g = 0; g < 16; ++g) {
            u64 r = splitmix64(seed ^ (u64)idx * 16 + g);
            for (int k = 0; k < 4; ++k) {
                int bit = g * 4 + k;
                if (((r >> (16 * k)) & 0xffff) < thresh16 && wq * 64 + bit < n) word |= 1ULL << bit;
            }
        }
        rows[idx] = word;
    }
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += (i64)gridDim.x * blockDim.x) {
        u64 a = splitmix64(seed ^ 0xabcdef12345ULL ^ (u64)t * 2), b = splitmix64(seed ^ 0xabcdef12345ULL ^ ((u64)t * 2 + 1));
        double u1 = ((a >> 11) + 1.0) * (1.0 / 9007199254740993.0), u2 = (b >> 11) * (1.0 / 9007199254740992.0);
        double r = sqrt(-2.0 * log(u1));
        coeff[2 * t] = r * cos(6.283185307179586 * u2);
        coeff[2 * t + 1] = r * sin(6.283185307179586 * u2);
    }
}

// coefficients in place: c <- (conjugate_first ? conj(c) : c) * (re + i im), plain IEEE products: every partial product and the sum are
// rounded once, no contraction.  That is NumPy's complex128 SCALAR multiply bit for bit; NumPy's ARRAY multiply contracts with FMA in its
// SIMD loop on x86-64 and differs by an ulp on about two general products in five ("Product coefficients").
__global__ __launch_bounds__(256) void k_scale_coeff(double *__restrict__ c, i64 T, double re, double im, int conjugate_first) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double2 v = reinterpret_cast<double2 *>(c)[t];
    if (conjugate_first) v.y = -v.y;
    double2 o;
    o.x = __dsub_rn(__dmul_rn(v.x, re), __dmul_rn(v.y, im));
    o.y = __dadd_rn(__dmul_rn(v.x, im), __dmul_rn(v.y, re));
    reinterpret_cast<double2 *>(c)[t] = o;
}

// reference layout (np.bool_ [T][2n], X columns then Z columns, base.py:42-74) <-> packed rows: one wavefront per (term, word); lane l owns
// qubit 64 w + l, so the packed word IS the wavefront's ballot (and a word's 64 bytes are one coalesced store on the way back)
__global__ __launch_bounds__(256) void k_pack_bool(const uint8_t *__restrict__ symp, i64 T, int n, int Wq, u64 *__restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const i64 n_words = T * 2 * Wq;
    for (i64 idx = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); idx < n_words; idx += (i64)gridDim.x * 4) {
        const i64 t = idx / (2 * Wq);
        const int w = (int)(idx % (2 * Wq));
        const int half = w >= Wq, q = (half ? w - Wq : w) * 64 + lane;
        const bool bit = q < n && symp[t * 2 * n + (half ? n : 0) + q] != 0;
        const u64 word = __ballot(bit);
        if (lane == 0) rows[idx] = word;
    }
}
__global__ __launch_bounds__(256) void k_unpack_bool(const u64 *__restrict__ rows, i64 T, int n, int Wq, uint8_t *__restrict__ symp) {
    const int lane = threadIdx.x & 63;
    const i64 n_words = T * 2 * Wq;
    for (i64 idx = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); idx < n_words; idx += (i64)gridDim.x * 4) {
        const i64 t = idx / (2 * Wq);
        const int w = (int)(idx % (2 * Wq));
        const int half = w >= Wq, q = (half ? w - Wq : w) * 64 + lane;
        const u64 word = rows[idx];
        if (q < n) symp[t * 2 * n + (half ? n : 0) + q] = (uint8_t)((word >> lane) & 1);
    }
}

// grid of k_pack_bool / k_unpack_bool: four wavefronts per workgroup, one (term, word) each per step
static unsigned bool_grid(i64 n_words) { return (unsigned)((n_words + 3) / 4 < 65536 * 16 ? (n_words + 3) / 4 : 65536 * 16); }

}  // namespace symgpu

using namespace symgpu;

extern "C" {

int symgpu_op_alloc(int64_t capacity_rows, int Wq, int with_coeff, symgpu_op_t *out) {
    SG_ENTER();
    SG_REQUIRE(out && capacity_rows >= 0 && Wq >= 1, "op_alloc");
    symgpu_op_s *op = new symgpu_op_s();
    op->device = ctx().device;
    op->Wq = Wq;
    op->capacity = capacity_rows;
    op->T = 0;
    int rc = dev_alloc((size_t)capacity_rows * 2 * Wq * sizeof(u64), (void **)&op->rows);
    if (rc == SYMGPU_OK && with_coeff) rc = dev_alloc((size_t)capacity_rows * 2 * sizeof(double), (void **)&op->coeff);
    if (rc != SYMGPU_OK) {
        if (op->rows) dev_free(op->rows);
        delete op;
        return rc;
    }
    *out = op;
    return SYMGPU_OK;
}

static void release_op(symgpu_op_t op) {
    op_invalidate(op);
    if (op->rows) dev_free(op->rows);
    if (op->coeff) dev_free(op->coeff);
    delete op;
}

int symgpu_op_free(symgpu_op_t op) {
    if (!op) return SYMGPU_OK;
    const Context *oc = ctx_of_device(op->device);
    if (oc && oc->ready) {
        SG_ENTER(op);
        release_op(op);
        return SYMGPU_OK;
    }
    release_op(op);           // a handle that outlived symgpu_shutdown: dev_free files its blocks under their device without a context
    return SYMGPU_OK;
}

int symgpu_op_set_rows(symgpu_op_t op, int64_t T) {
    SG_ENTER(op);
    SG_REQUIRE(op && T >= 0 && T <= op->capacity, "op_set_rows");
    if (T != op->T) op_invalidate(op);
    op->T = T;
    return SYMGPU_OK;
}

int symgpu_op_write(symgpu_op_t op, int64_t row_offset, const uint64_t *rows, const double *coeff, int64_t count) {
    SG_ENTER(op);
    SG_REQUIRE(op && row_offset >= 0 && count >= 0 && row_offset + count <= op->capacity, "op_write: row range exceeds the capacity");
    SG_REQUIRE(count == 0 || rows, "op_write: null rows");
    const size_t W = (size_t)2 * op->Wq;
    if (count > 0) {
        HIP_TRY(hipMemcpyAsync(op->rows + (size_t)row_offset * W, rows, (size_t)count * W * 8, hipMemcpyHostToDevice, ctx().stream));
        if (coeff && op->coeff)
            HIP_TRY(hipMemcpyAsync(op->coeff + 2 * (size_t)row_offset, coeff, (size_t)count * 16, hipMemcpyHostToDevice, ctx().stream));
        HIP_TRY(hipStreamSynchronize(ctx().stream));
        count_h2d((size_t)count * W * 8 + ((coeff && op->coeff) ? (size_t)count * 16 : 0));
        bump_counter(SYMGPU_CTR_OP_UPLOADS);
    }
    op_invalidate(op);
    if (row_offset + count > op->T) op->T = row_offset + count;
    return SYMGPU_OK;
}

int symgpu_op_copy_rows(symgpu_op_t dst, int64_t dst_offset, symgpu_op_t src, int64_t src_offset, int64_t count) {
    SG_REQUIRE(dst && src && dst != src && dst->Wq == src->Wq, "op_copy_rows: handles");
    SG_ENTER(dst);                                                     // runs on the destination's device, under its lock only
    SG_REQUIRE(count >= 0 && dst_offset >= 0 && src_offset >= 0 && dst_offset + count <= dst->capacity && src_offset + count <= src->T,
               "op_copy_rows: row range");
    const size_t W = (size_t)2 * dst->Wq;
    if (count > 0 && src->device != dst->device) {
        // the one call that crosses devices: a peer copy (xGMI) on the destination's stream, after the source's stream has drained.
        // The source's context is not locked (two copies in opposite directions must not wait for each other): its stream is only
        // synchronised, and the caller keeps `src` from being written or freed meanwhile, as for any handle it owns
        Context *sc = ctx_of_device(src->device);
        SG_REQUIRE(sc && sc->ready, "op_copy_rows: the source's device has no context");
        HIP_TRY(hipStreamSynchronize(sc->stream));
        HIP_TRY(hipMemcpyPeerAsync(dst->rows + (size_t)dst_offset * W, dst->device, src->rows + (size_t)src_offset * W, src->device, (size_t)count * W * 8, ctx().stream));
        if (dst->coeff && src->coeff)
            HIP_TRY(hipMemcpyPeerAsync(dst->coeff + 2 * (size_t)dst_offset, dst->device, src->coeff + 2 * (size_t)src_offset, src->device, (size_t)count * 16, ctx().stream));
    } else if (count > 0) {
        HIP_TRY(hipMemcpyAsync(dst->rows + (size_t)dst_offset * W, src->rows + (size_t)src_offset * W, (size_t)count * W * 8, hipMemcpyDeviceToDevice, ctx().stream));
        if (dst->coeff && src->coeff)
            HIP_TRY(hipMemcpyAsync(dst->coeff + 2 * (size_t)dst_offset, src->coeff + 2 * (size_t)src_offset, (size_t)count * 16, hipMemcpyDeviceToDevice, ctx().stream));
    }
    op_invalidate(dst);
    if (dst_offset + count > dst->T) dst->T = dst_offset + count;
    return SYMGPU_OK;
}

int symgpu_op_upload(const uint64_t *rows, const double *coeff, int64_t T, int Wq, symgpu_op_t *out) {
    SG_ENTER();
    SG_REQUIRE(out && T >= 0 && Wq >= 1 && (rows || T == 0), "op_upload");
    OwnedOp f;
    SG_TRY(f.alloc(T, T, Wq, coeff != nullptr));
    if (T > 0) {
        HIP_TRY(hipMemcpyAsync(f->rows, rows, (size_t)T * 2 * Wq * sizeof(u64), hipMemcpyHostToDevice, ctx().stream));
        if (coeff) HIP_TRY(hipMemcpyAsync(f->coeff, coeff, (size_t)T * 2 * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
        HIP_TRY(hipStreamSynchronize(ctx().stream));                   // host buffers are not retained past the call
        count_h2d((size_t)T * 2 * Wq * sizeof(u64) + (coeff ? (size_t)T * 16 : 0));
        bump_counter(SYMGPU_CTR_OP_UPLOADS);
    }
    f.hand_out(out);
    return SYMGPU_OK;
}

int symgpu_op_download(symgpu_op_t op, uint64_t *rows, double *coeff, int64_t capacity_rows) {
    SG_ENTER(op);
    SG_REQUIRE(op, "op_download: null handle");
    if (capacity_rows < op->T) {
        set_error("op_download: capacity %lld < %lld rows", (long long)capacity_rows, (long long)op->T);
        return SYMGPU_E_CAPACITY;
    }
    if (op->T > 0) {
        if (rows) {
            SG_TRY(download_any(op->rows, rows, (size_t)op->T * 2 * op->Wq * sizeof(u64)));
            count_d2h((size_t)op->T * 2 * op->Wq * sizeof(u64));
        }
        if (coeff) {
            SG_REQUIRE(op->coeff, "op_download: operator has no coefficients");
            prefault_host(coeff, (size_t)op->T * 2 * sizeof(double));
            HIP_TRY(hipMemcpyAsync(coeff, op->coeff, (size_t)op->T * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
            count_d2h((size_t)op->T * 16);
        }
        if (rows || coeff) bump_counter(SYMGPU_CTR_OP_DOWNLOADS);
    }
    HIP_TRY(hipStreamSynchronize(ctx().stream));
    return SYMGPU_OK;
}

// ---- handle-level primitives behind the device-resident drop-in classes (symmer_amd/operators/base.py) -----------------------------------
int symgpu_op_clone(symgpu_op_t in, symgpu_op_t *out) {
    SG_ENTER(in);
    SG_REQUIRE(in && out, "op_clone: null argument");
    OwnedOp f;
    SG_TRY(f.alloc(in->T, in->T, in->Wq, in->coeff != nullptr));
    if (in->T > 0) {
        HIP_TRY(hipMemcpyAsync(f->rows, in->rows, (size_t)in->T * 2 * in->Wq * sizeof(u64), hipMemcpyDeviceToDevice, ctx().stream));
        if (in->coeff) HIP_TRY(hipMemcpyAsync(f->coeff, in->coeff, (size_t)in->T * 16, hipMemcpyDeviceToDevice, ctx().stream));
    }
    f->dup_free = in->dup_free;        // the rows are the same rows
    f.hand_out(out);
    return SYMGPU_OK;
}

int symgpu_op_set_coeff(symgpu_op_t op, const double *coeff_host) {
    SG_ENTER(op);
    SG_REQUIRE(op && (coeff_host || op->T == 0), "op_set_coeff: null argument");
    if (!op->coeff) SG_TRY(dev_alloc((size_t)(op->capacity > 0 ? op->capacity : 1) * 16, (void **)&op->coeff));
    if (op->T > 0) {
        HIP_TRY(hipMemcpyAsync(op->coeff, coeff_host, (size_t)op->T * 16, hipMemcpyHostToDevice, ctx().stream));
        HIP_TRY(hipStreamSynchronize(ctx().stream));              // host buffers are not retained past the call
        count_h2d((size_t)op->T * 16);
        bump_counter(SYMGPU_CTR_OP_UPLOADS);
    }
    return SYMGPU_OK;                                             // the rows did not change: per-handle caches stay
}

int symgpu_op_scale(symgpu_op_t op, double re, double im, int conjugate_first) {
    SG_ENTER(op);
    SG_REQUIRE(op && (op->coeff || op->T == 0), "op_scale: operator has no coefficients");
    if (op->T > 0) {
        hipLaunchKernelGGL(k_scale_coeff, dim3((unsigned)((op->T + 255) / 256)), dim3(256), 0, ctx().stream, op->coeff, op->T, re, im, conjugate_first);
        KERNEL_CHECK();
    }
    return SYMGPU_OK;
}

int symgpu_op_ycount(symgpu_op_t op, int64_t *out_host) {
    SG_ENTER(op);
    SG_REQUIRE(op && (out_host || op->T == 0), "op_ycount: null argument");
    if (op->T == 0) return SYMGPU_OK;
    const int *yc = nullptr;
    SG_TRY(op_ycount(op, &yc));
    int *h = (int *)malloc((size_t)op->T * sizeof(int));
    if (!h) { set_error("host allocation failed"); return SYMGPU_E_NOMEM; }
    hipError_t e = hipMemcpyAsync(h, yc, (size_t)op->T * sizeof(int), hipMemcpyDeviceToHost, ctx().stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) { free(h); return hip_fail(e, "op_ycount download", __FILE__, __LINE__); }
    count_d2h((size_t)op->T * sizeof(int));
    for (i64 t = 0; t < op->T; ++t) out_host[t] = h[t];
    free(h);
    return SYMGPU_OK;
}

int symgpu_op_upload_bool(const uint8_t *symp, const double *coeff, int64_t T, int n_qubits, symgpu_op_t *out) {
    SG_ENTER();
    SG_REQUIRE(out && T >= 0 && n_qubits >= 1 && (symp || T == 0), "op_upload_bool");
    const int Wq = (n_qubits + 63) / 64;
    OwnedOp f;
    SG_TRY(f.alloc(T, T, Wq, coeff != nullptr));
    if (T > 0) {
        const size_t nb = (size_t)T * 2 * n_qubits;
        Scratch stage;
        SG_TRY(stage.alloc(nb));
        HIP_TRY(hipMemcpyAsync(stage.p, symp, nb, hipMemcpyHostToDevice, ctx().stream));
        if (coeff) HIP_TRY(hipMemcpyAsync(f->coeff, coeff, (size_t)T * 16, hipMemcpyHostToDevice, ctx().stream));
        // one wavefront per (row, word): lane l reads the byte of qubit 64 w + l, the ballot is the packed word
        hipLaunchKernelGGL(k_pack_bool, dim3(bool_grid(T * 2 * Wq)), dim3(256), 0, ctx().stream, stage.as<uint8_t>(), T, n_qubits, Wq, f->rows);
        KERNEL_CHECK();
        HIP_TRY(hipStreamSynchronize(ctx().stream));                   // host buffers are not retained past the call (and the staging buffer goes)
        count_h2d(nb + (coeff ? (size_t)T * 16 : 0));
        bump_counter(SYMGPU_CTR_OP_UPLOADS);
    }
    f.hand_out(out);
    return SYMGPU_OK;
}

int symgpu_op_download_bool(symgpu_op_t op, int n_qubits, uint8_t *symp_out, int64_t capacity_rows) {
    SG_ENTER(op);
    SG_REQUIRE(op && n_qubits >= 1 && (n_qubits + 63) / 64 == op->Wq, "op_download_bool: qubit count does not match the packed width");
    if (capacity_rows < op->T) {
        set_error("op_download_bool: capacity %lld < %lld rows", (long long)capacity_rows, (long long)op->T);
        return SYMGPU_E_CAPACITY;
    }
    if (op->T == 0) return SYMGPU_OK;
    SG_REQUIRE(symp_out, "op_download_bool: null output");
    const size_t nb = (size_t)op->T * 2 * n_qubits;
    Scratch stage;
    SG_TRY(stage.alloc(nb));
    hipLaunchKernelGGL(k_unpack_bool, dim3(bool_grid(op->T * 2 * op->Wq)), dim3(256), 0, ctx().stream, op->rows, op->T, n_qubits, op->Wq, stage.as<uint8_t>());
    KERNEL_CHECK();
    SG_TRY(download_any(stage.p, symp_out, nb));
    count_d2h(nb);
    bump_counter(SYMGPU_CTR_OP_DOWNLOADS);
    return SYMGPU_OK;
}

int symgpu_op_info(symgpu_op_t op, int64_t *T, int *Wq, int64_t *capacity_rows) {
    SG_REQUIRE(op, "op_info: null handle");
    if (T) *T = op->T;
    if (Wq) *Wq = op->Wq;
    if (capacity_rows) *capacity_rows = op->capacity;
    return SYMGPU_OK;
}

int symgpu_op_random(int64_t T, int n_qubits, double density, uint64_t seed, symgpu_op_t *out) {
    SG_ENTER();
    SG_REQUIRE(out && T >= 0 && n_qubits >= 1 && density >= 0.0 && density <= 1.0, "op_random");
    int Wq = (n_qubits + 63) / 64;
    OwnedOp f;
    SG_TRY(f.alloc(T, T, Wq, true));
    if (T > 0) {
        u32 th = (u32)(density * 65536.0 + 0.5);
        hipLaunchKernelGGL(k_random_op, dim3(4096), dim3(256), 0, ctx().stream, f->rows, f->coeff, T, n_qubits, Wq, th, seed);
        KERNEL_CHECK();
    }
    f.hand_out(out);
    return SYMGPU_OK;
}

}  // extern "C"
