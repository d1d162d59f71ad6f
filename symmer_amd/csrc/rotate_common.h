// rotate_common.h — what the files of the rotation share; private to them.  Forms of one rotation, each file holding its kernels and the
// host function that launches them:
//   rotate_analyze.hip      flags + phase exponents of every row (k_rot_analyze*), join-table insert, the persistent join table
//   rotate_fast.hip         hash join (non-Clifford) and the Clifford fast path: match / classify, scan, write
//   rotate_general.hip      general path: stacked operator + cleanup (operators with duplicate rows, SYMGPU_ROTATE_GENERAL)
//   rotate_resident.hip     the whole rotation as one persistent launch: its plan and the host stages of a call
//   rotate_resident_kernel.hip  ... its kernel, phase by phase, and the launch (the two share rotate_resident.h)
//   rotate_chain.hip        a run of Clifford rotations with the rows in registers
//   rotate_chain_forms.hip  the other forms of a run: LDS-resident, single workgroup, two and four launches per rotation
//   rotate_driver.hip       switches, plans, C ABI
#pragma once
#include "common.h"
#include <type_traits>

namespace symgpu {

// Generation-tagged entries of the persistent join table (Context::rot_table): [tag = hash >> 32 | generation : 10 | row + 1 : 22].
struct JoinTable {
    u64 *slots;
    u32 mask;          // capacity - 1
    u32 gen;           // 1 .. 1023
    u32 *flags;        // [0] = gen when a duplicate input row was seen
};
__device__ __forceinline__ u64 mix64(u64 h) { h ^= h >> 33; h *= 0xff51afd7ed558ccdULL; h ^= h >> 29; return h; }
__device__ __forceinline__ u32 jt_gen(u64 v) { return (u32)(v >> 22) & 1023u; }
__device__ __forceinline__ i64 jt_row(u64 v) { return (i64)(v & 0x3FFFFFULL) - 1; }

// The rotation's Pauli row Q BY VALUE in the kernel arguments (rows of <= 64 words): no host-to-device copy in front of a rotation.
struct QArg { u64 w[64]; };

__device__ __forceinline__ void phase_mul(double re, double im, int e, double &ore, double &oim) {
    switch (e & 3) {
        case 0: ore = re; oim = im; break;
        case 1: ore = -im; oim = re; break;
        case 2: ore = -re; oim = -im; break;
        default: ore = im; oim = -re; break;
    }
}

// lane exchange inside an aligned group of WQ lanes that holds one row, 16 bytes per lane (X words in the lower, Z words in the upper half)
template <int CTRL> __device__ __forceinline__ u32 rot_dpp(u32 v) { return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }
template <int WQ> __device__ __forceinline__ u32 rot_other_half(u32 v) {
    if (WQ == 2) return rot_dpp<0xB1>(v);
    if (WQ == 4) return rot_dpp<0x4E>(v);
    if (WQ == 16) return rot_dpp<0x128>(v);
    return (u32)__shfl_xor((int)v, WQ / 2);
}
template <int WQ> __device__ __forceinline__ u32 rot_row_sum(u32 s) {          // over the WQ lanes of the row (butterfly)
    if (WQ >= 2) s += rot_dpp<0xB1>(s);
    if (WQ >= 4) s += rot_dpp<0x4E>(s);
    if (WQ >= 8) s += rot_dpp<0x141>(s);
    if (WQ >= 16) s += rot_dpp<0x140>(s);
    if (WQ >= 32) s += (u32)__shfl_xor((int)s, 16);
    if (WQ >= 64) s += (u32)__shfl_xor((int)s, 32);
    return s;
}

// switch (w) { case WS: f(integral_constant<int, WS>) ...; default: f(integral_constant<int, DEFAULT>) } — one host launch site per kernel
// template with the row width (or another small count) as a compile-time constant; instantiates f for exactly WS... and DEFAULT
template <int DEFAULT, class F> inline decltype(auto) wq_dispatch(int, F &&f) { return f(std::integral_constant<int, DEFAULT>{}); }
template <int DEFAULT, int W0, int... WS, class F> inline decltype(auto) wq_dispatch(int w, F &&f) {
    if (w == W0) return f(std::integral_constant<int, W0>{});
    return wq_dispatch<DEFAULT, WS...>(w, static_cast<F &&>(f));
}

// lanes per row of the word kernels (k_rot_analyze, the chain kernels): the power of two >= Wq, at most 64
static inline int row_lanes(int Wq) {
    int G = 1;
    while (G < Wq && G < 64) G <<= 1;
    return G;
}

constexpr i64 JOIN_MAX_T = ((i64)1 << 22) - 1;   // rows a join table takes: 22-bit row index + 1 per entry (and <= 4096 scan blocks)
constexpr i64 SCAN_MAX_T = (i64)1 << 22;         // rows of the two-launch scan (k_rotf_scan3): <= 4096 blocks of 1024

// runs of Clifford rotations (symgpu_rotate_clifford_chain_dev, rotate_chain_forms.hip)
constexpr int CHAIN_TMAX = 8192;               // rows the single-workgroup kernel can hold: 8 per thread of the slot scan
constexpr int CHAIN_LOCAL_T = 128;             // ... and up to where it beats the multi-workgroup kernels: 3.5 us per rotation at 1 row, 5.0 at
                                               // 64, 6.6 at 128, 9.9 at 256, 29 at 1,000, against 6.7-7 us of the two-launch form (below)
constexpr int CHAIN_TWO_T = 262144;            // two launches per rotation (k_cchain_flags / k_cchain_move) up to here (256 group counts): 6.7 us at
                                               // 64-384 rows, 7.1 at 1,000, 10.4 at 8,000, 13.4 / 20.8 / 26.7 at 16,384 / 65,536 / 131,072 against 15.6
                                               // us (launch-rate bound) up to 8,000 rows and 17.3 / 24.0 / 32.4 us of the four-launch form
constexpr int CHAIN_LDS_T = 128;               // rows of the LDS-resident kernel

// Every switch the rotation reads, read at the top of each entry point (read_rotate_switches: a single rotation reads its own,
// a Clifford run its own): tests flip them between calls of one process.
// (SYMGPU_RES_SLOTS and SYMGPU_RES_TRACE, tuning knobs of the one-launch kernel, are read where it is launched.)
struct RotateSwitches {
    bool general = false;            // SYMGPU_ROTATE_GENERAL (set): the merging multi-launch path only
    int resident = 1;                // SYMGPU_ROT_RESIDENT: 0 off, 2 on again after a failure, 3 tests: the kernel reports a failed verification
    int hbm = 1;                     // SYMGPU_ROT_HBM: 0 off, 2 tests: rows left in memory whatever the size
    bool chain_reg = true;           // SYMGPU_CHAIN_REG=0: runs without the register chain
    bool local_t_set = false;        // SYMGPU_CHAIN_LOCAL_T (tests): the single-workgroup kernels up to local_t, the register chain above
    i64 local_t = CHAIN_LOCAL_T;
    // tuning knobs (SG_TUNE: compiled out of the default build)
    bool chain_lds = true;           // SYMGPU_CHAIN_LDS=0: no LDS-resident chain kernel
    bool chain_two = true;           // SYMGPU_CHAIN_TWO=0: no two-launch chain form
    i64 chain_two_t = CHAIN_TWO_T;   // SYMGPU_CHAIN_TWO_T: its term limit
    bool chunks = true;              // SYMGPU_ROT_CHUNKS=0: the word analysis kernel for every row length
    i64 analyze_cap = 1024;          // SYMGPU_ROT_ANALYZE_CAP: grid cap of the word analysis kernel
};

// counts of one rotation; dup: a duplicate input row was seen by this call's join-table insert (multi-launch path); the resident
// kernel reports a failed row verification or a barrier time-out there (2 / 3).
struct RotCounts { u32 nC, nA, nN, nAnti, dup; };

// scratch of the per-row fast paths (k_rotf_match2 / k_rotc_classify -> k_rotf_scan3 -> k_rotf_write)
struct RotScratch {
    Scratch selfc, prodc, cls, pself, pnew, cnt, blk;      // coefficients (own row / product row), classes, output slots, counts, block counts
    int n_blk = 0;                                         // 1024-row blocks
    int alloc(i64 T);
};

// One single rotation (symgpu_rotate_single_dev): arguments, and what its stages hand on to each other.
struct RotationRun {
    symgpu_op_t in;
    const u64 *q_host;
    double cos_t, sin_t, thr;
    int k;                                                 // clifford_k: -1 non-Clifford, else the multiple of pi/2 (not reduced mod 4)
    const RotateSwitches &sw;
    symgpu_op_t *out;
    int *all_commute;
    Scratch q, anti, ph;                                   // Q on the device, anticommutation flags, phase exponents (from the analysis)
    bool has_dup = false;                                  // the duplicate check found two equal rows (or could not run)
};

// rotate_analyze.hip
int host_counts(RotCounts **host, RotCounts **dev);          // pinned, device-mapped host copy of the counts (one per context)
int join_table_for(i64 T, JoinTable *jt);                     // the persistent join table with a fresh generation
// flags + phase exponents of every row; with `jt` also the join-table insert (row hashes taken from the handle or computed now and
// cached on it).  q_host_arg: Q reaches q_dev with this launch (in its kernel arguments when the row has <= 64 words).
int analyze_rows(symgpu_op_t in, u64 *q_dev, u32 *anti, uint8_t *ph, const JoinTable *jt, const RotateSwitches &sw, const u64 *q_host_arg = nullptr);
int rotate_dup_check(RotationRun &r);                         // analysis + join-table insert: r.has_dup; sets in->dup_free if there is none

// rotate_fast.hip
void launch_rotf_write(const u64 *rows, const u64 *q, i64 T, int Wq, const RotScratch &s, u64 *out_rows, double *out_coeff, int clifford,
                       const u64 *hin, u64 hq, u64 *hout);
void clifford_classify_scan_write(const u64 *rows, const double *coeff, const u64 *q, const u32 *anti, const uint8_t *ph, i64 T, int Wq, int k,
                                  double thr, const RotScratch &s, RotCounts *host_cnt, u64 *out_rows, double *out_coeff, const u64 *hin, u64 hq,
                                  u64 *hout);
int rotate_join(RotationRun &r, int *done);                   // non-Clifford hash join; *done = 0: duplicate rows (rows analysed)
int rotate_clifford_fast(RotationRun &r);                     // Clifford, rows analysed, no merge possible

// rotate_general.hip: stacked operator + cleanup, rows analysed
int rotate_general(RotationRun &r);

// rotate_resident.hip: the whole rotation as ONE persistent launch, each workgroup keeping its block of R rows on the chip.
// Where the rows of a block stay between the one read and the write: in LDS; in LDS but for two 1,024-chunk rounds of the load that stay in
// registers; or in memory, read a second time when they are written out (only the 26 bytes of per-row state are in LDS then).
enum class ResidentForm { Lds, Registers, RowsInMemory };
constexpr symgpu_counter counter_of(ResidentForm f) { return (symgpu_counter)(SYMGPU_CTR_RESIDENT_LDS + (int)f); }   // launches by form
static_assert(counter_of(ResidentForm::Lds) == SYMGPU_CTR_RESIDENT_LDS && counter_of(ResidentForm::Registers) == SYMGPU_CTR_RESIDENT_REGISTERS &&
              counter_of(ResidentForm::RowsInMemory) == SYMGPU_CTR_RESIDENT_ROWS_IN_MEMORY, "ResidentForm and its counters are in one order");
struct ResidentPlan {
    bool applicable = false;                               // the operator qualifies (what the process state may still veto: rotate_resident_try)
    ResidentForm form = ResidentForm::Lds;
    int G = 0, R = 0;                                      // workgroups, rows of each
    int nreg = 0, hbm = 0, lds_bytes = 0;                  // res_layout's arguments for the form, and its total
    int GA = 1;                                            // lanes per row where rows are analysed from LDS or memory
};
// pure: no HIP call, no context.  dup_free: symgpu_op_s::dup_free; num_cu: compute units of the device
ResidentPlan plan_resident(i64 T, int Wq, bool dup_free, int clifford_k, int num_cu, const RotateSwitches &sw);
// *done = 0: switched off, disabled in this process, or the launch reported a failed verification or a time-out — take the other paths.
int rotate_resident_try(symgpu_op_t in, const u64 *q_host, double cos_t, double sin_t, int clifford_k, double thr, const RotateSwitches &sw,
                        const ResidentPlan &plan, symgpu_op_t *out, int *all_commute, int *done);
int rotate_resident_trace(u64 *out, int max_wgs, int *n_wgs);   // phase stamps of the last traced launch (SYMGPU_RES_TRACE=1)

// A run of Clifford rotations of a clean operator (symgpu_rotate_clifford_chain_dev): `a` holds a copy of the input, `b` is a second operator
// of the same capacity.  Every form has the same signature; *in_b: the result is in `b`.
struct ChainRun {
    symgpu_op_t in, a, b;
    i64 T, K;
    int Wq;
    u64 *qs;                                               // [K][2 Wq] Q rows, device
    const int *ks;                                         // [K] k of every rotation (0..3), device
    const int *ks_host;                                    // ... and host
    const RotateSwitches &sw;
};
// rotate_chain.hip: rows in registers
bool clifford_chain_registers_applicable(i64 T, int Wq, bool chain_reg);
int chain_registers(const ChainRun &c, int *in_b);
// rotate_chain_forms.hip
bool chain_lds_attr_ok();                                    // k_clifford_chain_lds may use 128 KiB of LDS (once per device)
int chain_lds(const ChainRun &c, int *in_b);
int chain_single_workgroup(const ChainRun &c, int *in_b);
int chain_two_launch(const ChainRun &c, int *in_b);
int chain_four_launch(const ChainRun &c, int *in_b);

}  // namespace symgpu
