// matvec.h — what matvec.hip (the plan and y = H x), lanczos.hip (the vector kernels of the eigen-iteration), ansatz.hip (rotations
// exp(i theta P) on a statevector, energy and gradients) and evolve.hip (Chebyshev polynomials of H on a statevector) share; rdm.hip
// takes the memory check.
#pragma once
#include "xgroups.h"

// the grouped terms of one operator, resident on `device` (symgpu_matvec_plan); nothing of the operator handle is kept
struct symgpu_matvec_s {
    int device = 0;
    symgpu::XGroups xg;                          // without tg
};

namespace symgpu {

constexpr int MV_TILE = 256;                      // rows per workgroup (64 and 128 measured the same within 4 %)

// ---- the row sum of y = H x, one text for every kernel that forms it (k_mv_apply, k_cheb_step) ------------------------------------------
struct MvTerms {
    const u32 *tz;
    const f64x2 *tc;
    const u32 *gx;
    const u32 *gstart;
    u32 G;
    int n;
};

__device__ __forceinline__ f64x2 mv_signed(f64x2 c, u32 b, u32 z) {
    const long long neg = (long long)((u64)(__popc(b & z) & 1) << 63);
    return f64x2{__longlong_as_double(__double_as_longlong(c.x) ^ neg), __longlong_as_double(__double_as_longlong(c.y) ^ neg)};
}

// D_g(b), the terms of group g added in operator order from the first one
__device__ __forceinline__ f64x2 mv_group_sum(const MvTerms &P, u32 g, u32 b) {
    const u32 t0 = P.gstart[g], t1 = P.gstart[g + 1];
    f64x2 d = mv_signed(P.tc[t0], b, P.tz[t0]);
    for (u32 t = t0 + 1; t < t1; ++t) {
        const f64x2 v = mv_signed(P.tc[t], b, P.tz[t]);
        d = f64x2{__dadd_rn(d.x, v.x), __dadd_rn(d.y, v.y)};
    }
    return d;
}

static inline MvTerms mv_terms_of(const symgpu_matvec_s *p) {
    const XGroups &g = p->xg;
    return MvTerms{g.tz.as<u32>(), g.tc.as<f64x2>(), g.gx.as<u32>(), g.gstart.as<u32>(), g.G, g.n};
}

// y = keep o (H x) on the context's stream: keep (uint8 [2^n], may be null) zeroes the rows it does not keep.  *form: SYMGPU_MATVEC_*.
int matvec_launch(const symgpu_matvec_s *p, const f64x2 *x, f64x2 *y, const uint8_t *keep, int *form);
// SYMGPU_E_NOMEM (with the text) unless `bytes` more fit the device, parked blocks of the allocator given back first
int matvec_require_memory(u64 bytes, const char *what);
// lanczos.hip: *re_out (device) = Re<v, w> in the two-level order of symgpu_lanczos_step; partial: f64x2 [lz_chunks(N)], h: f64x2 [1]
unsigned lz_chunks(u64 N);
int lz_inner(const f64x2 *v, const f64x2 *w, u64 N, f64x2 *partial, f64x2 *h, double *re_out);

}  // namespace symgpu
