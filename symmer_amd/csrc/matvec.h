// matvec.h — what matvec.hip (the plan and y = H x), lanczos.hip (the vector kernels of the eigen-iteration) and ansatz.hip (rotations
// exp(i theta P) on a statevector, energy and gradients) share; rdm.hip takes the memory check.
#pragma once
#include "xgroups.h"

// the grouped terms of one operator, resident on `device` (symgpu_matvec_plan); nothing of the operator handle is kept
struct symgpu_matvec_s {
    int device = 0;
    symgpu::XGroups xg;                          // without tg
};

namespace symgpu {

// y = keep o (H x) on the context's stream: keep (uint8 [2^n], may be null) zeroes the rows it does not keep.  *form: SYMGPU_MATVEC_*.
int matvec_launch(const symgpu_matvec_s *p, const f64x2 *x, f64x2 *y, const uint8_t *keep, int *form);
// SYMGPU_E_NOMEM (with the text) unless `bytes` more fit the device, parked blocks of the allocator given back first
int matvec_require_memory(u64 bytes, const char *what);
// lanczos.hip: *re_out (device) = Re<v, w> in the two-level order of symgpu_lanczos_step; partial: f64x2 [lz_chunks(N)], h: f64x2 [1]
unsigned lz_chunks(u64 N);
int lz_inner(const f64x2 *v, const f64x2 *w, u64 N, f64x2 *partial, f64x2 *h, double *re_out);

}  // namespace symgpu
