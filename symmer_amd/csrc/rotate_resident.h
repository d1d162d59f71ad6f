// rotate_resident.h — what the two files of the one-launch rotation share; private to them:
//   rotate_resident.hip         host: plan_resident, and rotate_resident_try with its stages
//   rotate_resident_kernel.hip  k_rot_resident with its phases, and the function that launches a planned call
// (ResidentPlan itself is declared in rotate_common.h: the driver keeps it in its RotationPlan.)
#pragma once
#include "rotate_common.h"

namespace symgpu {

constexpr int RES_THREADS = 1024;
constexpr int RES_MAX_WG = 256;                   // granules are swept by ONE wavefront, four per lane
constexpr u32 RES_SPIN_LIMIT = 1u << 20;          // ~1 s of polling: the workgroups are not co-resident (another process on the GPU)
constexpr size_t RES_LDS_MAX = 160 * 1024;
constexpr int RES_MIN_ROWS = 64;                  // rows per workgroup below which more workgroups only lengthen the all-gathers
constexpr int RES_MAX_R = 16384;                  // rows per workgroup: 16 ranking passes of 1,024, 16-bit counts in a granule
constexpr int RES_LD_UNROLL = 8;                  // 16-byte loads in flight per lane (cfg2: 6,256 chunks per block = one round of 8,192)
constexpr int RES_REG_ROUNDS = 2;                 // 1,024-chunk rounds of the row load that the Registers form keeps in registers
constexpr int RES_REG_MAX_WQ = 32;                // ... for rows of a power-of-two number of chunks up to here
constexpr int RES_MAX_W = 128;                    // words per row (4,096 qubits)
constexpr u32 RES_NO_SLOT = 0xFFFFFFFFu;
constexpr u64 RES_GRAN_FAIL = 1ULL << 47;         // bit 47 of a granule: its workgroup failed a verification or gave up
constexpr size_t RES_STATE_WORDS = 2 * RES_MAX_WG + 2;   // ResidentState::state: granules, {fail[0], fail[1]}, {finished, published}
constexpr size_t RES_TRACE_BYTES = (size_t)RES_MAX_WG * 16 * 8;
// class byte of a row: bits 0-2 = kept commuting row / kept anticommuting row / kept new row (what is written out); bit 3 = the row has
// a partner (its coefficient in LDS is final); join state in s_ps: bit 4 = it claimed slot s_ps, bit 5 = it found its partner s_ps,
// bit 6 = its first probe met the occupant {s_posn : s_ps} (resolved after the loads)
enum { CL_C = 1, CL_A = 2, CL_N = 4, CL_MATCHED = 8, CL_CLAIMED = 16, CL_SECOND = 32, CL_PENDING = 64 };

// LDS of one workgroup: the rows' 16-byte chunks (minus the first `nreg` x 1,024, which stay in registers), then 26 bytes per row:
// coefficient (16), one word that is first the row's join state (claimed slot / partner / occupant) and later its rank (4), the rank
// of its new row (4), info and class bytes.  Hashes are read from HBM where they are needed (twice, coalesced).
// hbm: the rows are NOT kept on the chip (operators beyond the 38 MB of LDS + registers): only the 26 bytes per row stay in LDS, the
// rows are read a second time — from the Infinity Cache, mostly — when they are written out
struct ResLayout { int rows, coef, ps, posn, info, cls, q, wtot, misc, total, lds_chunks; };
__host__ __device__ inline ResLayout res_layout(int R, int Wq, int nreg, int hbm = 0) {
    ResLayout L;
    int o = 0;
    L.lds_chunks = hbm ? 0 : R * Wq - nreg * 1024;
    if (L.lds_chunks < 0) L.lds_chunks = 0;
    L.rows = o; o += L.lds_chunks * 16;
    L.coef = o; o += R * 16;
    L.ps = o; o += R * 4;
    L.posn = o; o += R * 4;
    L.info = o; o += R;
    L.cls = o; o += R;
    o = (o + 15) & ~15;
    L.q = o; o += RES_MAX_W * 8;
    L.wtot = o; o += 256 * 8;
    L.misc = o; o += 32 * 4;
    L.total = o;
    return L;
}

struct QArgW { u64 w[RES_MAX_W]; };
struct ResArgs {
    const u32x4 *rows; const double *coeff; const u64 *hin;
    i64 T; int Wq, R, GA, nreg; u32 yq;          // nreg: 1,024-chunk rounds of the row load that stay in registers (0 or 2)
    int hbm;                                      // 1: rows are not kept on the chip (res_layout)
    u32x4 *out_rows; double *out_coeff; u64 *out_hash;
    double cos_t, sin_t, thr; int k;
    u64 hq;
    u64 *slots; u32 mask; u32 *partner;           // join table [canonical-key tag 32 | row + 1 : 32] and partner notes (row + 1), zero between launches
    u64 *gran1, *gran2; u32 *fail;                // fail[0] / fail[1] = epoch of a failed verification / of a time-out
    u32 *finished; u32 finish_target;             // fail[2]: workgroups that have left, counted over all launches; the one that reaches the target reports
    u32 epoch;
    u64 *trace;                                   // [G][16] wall-clock stamps of the phases (SYMGPU_RES_TRACE=1), else null
    int inject;                                   // tests: the last workgroup leaves at once without a word (SYMGPU_ROT_RESIDENT=3)
    u64 *host_words; u32 *host_late; u32 host_tag; u32 *published;   // pinned host memory: the report (res_report) and the late-failure word
    QArgW q;
};

// rotate_resident_kernel.hip
bool resident_lds_attr_ok();                      // k_rot_resident may use RES_LDS_MAX of LDS (once per device)
// the one launch of a planned call; which form it was is counted (counter_of(ResidentForm)) here and nowhere else
hipError_t launch_resident(const ResidentPlan &p, bool clifford, hipStream_t st, const ResArgs &a);

}  // namespace symgpu
