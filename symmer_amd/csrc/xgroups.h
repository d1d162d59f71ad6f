// xgroups.h — the terms of an operator of n <= 32 qubits (Wq = 1) grouped by X-part: what to_sparse_matrix (sparse_matrix.hip) and the
// matrix-free product (matvec.hip) both sum over.  Both promise the bits of one NumPy contract — per row b and group g,
// D_g(b) = sum over the terms k of g, in operator order, of c_k (-i)^{Y_k} (-1)^{|b & z_k|} — so the groups, their order and the term
// order inside each are defined here and nowhere else (xgroups.hip).
#pragma once
#include "common.h"

namespace symgpu {

// tg[s] = group of sorted term s | CSR_FIRST at the first term of a group | CSR_LAST at its last (k_csr_count, k_csr_fill walk these)
constexpr u32 CSR_FIRST = 1u << 31, CSR_LAST = 1u << 30, CSR_GID = CSR_LAST - 1;

// Owns its device buffers as Scratch does.  Integers are n-bit with qubit 0 the MOST significant bit; the groups ascend in x, the terms
// of a group keep their operator order (a stable sort).
struct XGroups {
    i64 T = 0;                                   // terms
    u32 G = 0;                                   // groups = distinct X-parts
    int n = 0;
    Scratch tz;                                  // u32 [T]: z of the sorted terms
    Scratch tc;                                  // f64x2 [T]: c' = c (-i)^Y of the sorted terms (an exact component swap)
    Scratch gx;                                  // u32 [G]: x of every group, ascending
    Scratch gstart;                              // u32 [G + 1]: first sorted term of every group, then T
    Scratch tg;                                  // u32 [T], only when asked for: see above (the group id lives in 30 bits: T < 2^30)
    i64 device_bytes() const { return T ? T * (tg.p ? 24 : 20) + (i64)G * 8 + 4 : 0; }
};

// Groups the T terms of `op` on the context's stream: key = x, stable radix sort of (key, term index), head flags, scan, ONE read-back
// (the group count), then one kernel that writes every buffer.  The caller has checked n, T, Wq = 1 and the coefficients; it
// synchronises the stream before `op` may change.  T = 0: G = 0, no buffers, no launch.
int xgroups_build(symgpu_op_t op, int n, bool want_tg, XGroups *out);

}  // namespace symgpu
