// matvec.h — what matvec.hip (the plan and y = H x) and lanczos.hip (the vector kernels of the eigen-iteration) share.
#pragma once
#include "common.h"

// the grouped terms of one operator, resident on `device` (symgpu_matvec_plan); nothing of the operator handle is kept
struct symgpu_matvec_s {
    int device = 0;
    int n = 0;
    i64 T = 0;
    u32 G = 0;                                   // groups = distinct X-parts
    void *tz = nullptr;                          // u32 [T]: z of the sorted terms as n-bit integers (qubit 0 the most significant bit)
    void *tc = nullptr;                          // f64x2 [T]: c' = c (-i)^Y of the sorted terms
    void *gx = nullptr;                          // u32 [G]: x of every group, ascending
    void *gstart = nullptr;                      // u32 [G + 1]: first sorted term of every group, then T
    i64 device_bytes = 0;
};

namespace symgpu {

// y = keep o (H x) on the context's stream: keep (uint8 [2^n], may be null) zeroes the rows it does not keep.  *form: SYMGPU_MATVEC_*.
int matvec_launch(const symgpu_matvec_s *p, const f64x2 *x, f64x2 *y, const uint8_t *keep, int *form);
// SYMGPU_E_NOMEM (with the text) unless `bytes` more fit the device, parked blocks of the allocator given back first
int matvec_require_memory(u64 bytes, const char *what);
// a call that is handed a plan runs on the plan's device: the operator-shaped stand-in that SG_ENTER takes
inline symgpu_op_s matvec_scope(const symgpu_matvec_s *p) {
    symgpu_op_s s;
    s.device = p->device;
    return s;
}

}  // namespace symgpu
