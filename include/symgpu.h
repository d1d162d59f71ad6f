/* symgpu.h — C ABI of libsymgpu.so: the MI355X (gfx950) implementation of Symmer's symplectic hot path.
 *
 * The reference (UCL-CCS/symmer) is pure Python and has NO FFI for this path; the seam it offers is the
 * set of NumPy-level functions below (file:line relative to the reference checkout).  Each entry point
 * here replaces one of them; `INTEGRATION.md` shows the ctypes stub a Symmer maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns SYMGPU_OK (0) or a negative error code and
 *    never throws or exits; `symgpu_last_error()` gives the text of the last failure on this thread.
 *  - host buffers are caller-owned, C-contiguous, and are not retained past the call.
 *  - packed symplectic row: 2*Wq uint64 words, X words first then Z words, Wq = max(1, ceil(n/64));
 *    bit j (LSB = 0) of word w <-> qubit 64*w + j; padding bits MUST be zero.
 *    == np.packbits(block, axis=1, bitorder='little') viewed as '<u8' after zero-padding to 64*Wq columns.
 *  - GF(2) matrices: R rows of Wc uint64 words, same bit rule; "leftmost column" = lowest set bit of the
 *    first non-zero word.
 *  - coefficients: complex128 as interleaved double[2] (re, im).
 *  - one context per DEVICE, with a lock: calls on one device are serialised WHOLE (host work, read-backs and kernels of one
 *    call do not interleave with another thread's call on that device); calls on different devices run concurrently.  Any thread
 *    may make them.  A handle belongs to the device it was created on and has one owner: several threads may pass the same handle
 *    to calls that only read it, but freeing or writing a handle while another thread may still pass it is the caller's error.
 *    Exceptions: the symgpu_comm_* calls take no lock (a collective that never returns must not block the device's other calls);
 *    symgpu_init* and symgpu_shutdown run before the threads start and after they end, never concurrently with another call.
 *    Multi-GPU = one process per device (symgpu_init + symgpu_comm_*, RCCL over xGMI) or one
 *    process driving several devices (symgpu_init_all + symgpu_set_device + symgpu_comm_init_all).
 */
#ifndef SYMGPU_H
#define SYMGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYMGPU_OK 0
#define SYMGPU_E_INVALID (-1)   /* bad argument (null pointer, negative size, Wq mismatch, T >= 2^32 for cleanup ...) */
#define SYMGPU_E_HIP (-2)       /* a HIP runtime call failed; see symgpu_last_error() */
#define SYMGPU_E_NOMEM (-3)     /* device allocation failed */
#define SYMGPU_E_CAPACITY (-4)  /* caller-supplied output capacity too small; *n_out (*k) holds the required row count and the output
                                 * buffers are untouched: call with capacity 0 to ask, allocate, call again */
#define SYMGPU_E_NODEVICE (-5)  /* no HIP device / symgpu_init not called */
#define SYMGPU_E_COLLISION (-6) /* row-hash collision survived every reseed (never observed; exactness guard) */
#define SYMGPU_E_RCCL (-7)      /* RCCL could not be loaded or a collective failed */

typedef struct symgpu_op_s *symgpu_op_t; /* device-resident operator: packed rows (+ optional coefficients) */

/* ---- context -------------------------------------------------------------------------------- */
#define SYMGPU_MAX_DEVICES 16
int symgpu_init(int device);              /* create the device's context (stream, allocator) if needed and make it the calling thread's current device */
/* Single-process multi-device mode ("one host process ... driving <= 8 devices — no MPI launcher needed"): contexts for devices
 * 0 .. n-1 (n <= 0: all visible), peer access between them.  A host thread has a CURRENT device (symgpu_set_device; initially the first
 * device initialised): uploads, allocations and every call without a handle go there.  A call that takes handles runs on the handles'
 * device whatever the current one is, and refuses handles of different devices (SYMGPU_E_INVALID) — symgpu_op_copy_rows is the one call
 * that crosses devices (peer copy over xGMI).  Each device has its own stream; calls on different devices overlap, so one thread can
 * launch a block of an all-pairs kernel on every device and then collect the results. */
int symgpu_init_all(int n_devices);
int symgpu_set_device(int device);
int symgpu_current_device(int *device);
int symgpu_n_initialised(int *n);          /* number of devices with a context in this process */
int symgpu_shutdown(void);                 /* all devices */
const char *symgpu_last_error(void);
int symgpu_device_count(int *n);          /* does not initialise a device */
int symgpu_sync(void);                    /* wait for the library stream */
int symgpu_device_sync(void);             /* hipDeviceSynchronize on the library's device (all streams) */
int symgpu_device_name(char *buf, int len);
int symgpu_mem_info(int64_t *free_bytes, int64_t *total_bytes);
/* HIP-event timer on the library stream (used by bench.py for per-kernel durations) */
int symgpu_timer_start(void);
int symgpu_timer_stop(float *ms);
/* per-launch HIP-event timing of the dominant kernel of a class (0 = product row stream k_mul_rows, 1 = commutation k_commutes,
 * 2 = GF(2) sweep k_sweep_m4r (main launches), 3 = cleanup output stage k_emit_fused (k_emit_stream with SYMGPU_EMIT_FUSED=0), 4 = one-launch rotation k_rot_resident,
 * 5 = register-resident run of Clifford rotations k_cchain_reg): enable, run, then read {launch count, total ms}. */
#define SYMGPU_PROF_CLASSES 6
int symgpu_prof_enable(int kernel_class, int on);
int symgpu_prof_read(int kernel_class, int64_t *n_launches, double *total_ms);
/* Statistics for tests: the counters of symgpu_debug_counter, each exactly once, as X(NAME, id, "what it counts").  The ids are part of
 * the ABI and never change; the enum below, the library's array and symgpu_debug_counter_name are generated from this list.
 * All counts are per process, since load. */
#define SYMGPU_COUNTER_LIST(X) \
    X(HASH_RESEEDS, 0, "number of row-hash collisions that forced the cleanup to reseed its hash and retry (the exactness guard behind " \
      "symplectic_cleanup, operators/utils.py:230-279; expected 0 outside the tests, which weaken the hash on purpose)") \
    X(RESIDENT_DONE, 1, "rotations completed by the one-launch LDS-resident kernel") \
    X(RESIDENT_FAILED, 2, "calls of that kernel that reported a failed row verification or a barrier time-out (the multi-launch path then " \
      "recomputes)") \
    X(DEV_MALLOC_CALLS, 3, "device allocations that were not served from the allocator's arena") \
    X(RESIDENT_NS_PREPARE, 4, "host nanoseconds spent by the one-launch rotation in preparation") \
    X(RESIDENT_NS_LAUNCH, 5, "host nanoseconds spent by the one-launch rotation in the launch call") \
    X(RESIDENT_NS_WAIT, 6, "host nanoseconds spent by the one-launch rotation waiting for the kernel's status word") \
    /* The drop-in classes keep their operands on the device between calls; the tests assert through 7-10 that a multi-step workflow
     * (symmer/projection/base.py:44-124, rotate -> project -> cleanup) moves its operator once in and once out. */ \
    X(H2D_BYTES, 7, "payload bytes copied host -> device by this library (operators, coefficients, index arrays, result matrices; not the " \
      "few-byte counts and flags a call reads back)") \
    X(D2H_BYTES, 8, "payload bytes copied device -> host by this library (as 7)") \
    X(OP_UPLOADS, 9, "operator uploads (calls that moved a whole operator or its coefficients)") \
    X(OP_DOWNLOADS, 10, "operator downloads (calls that moved a whole operator or its coefficients)") \
    X(CANARY_HITS, 11, "device blocks whose guard bytes were overwritten (tuning build, SYMGPU_ALLOC_CANARY)") \
    X(CTX_MAX_THREADS, 12, "the most threads seen using one device's context at once since load, counted where a call uses the context's " \
      "state, whichever lock it took (1 while the per-device lock holds)") \
    X(CTX_WAITS, 13, "calls that found their device busy with another thread's call and waited") \
    X(CTX_UNLOCKED_USES, 14, "uses of a device's context by a call that did not hold that context's lock (0 while the lock is taken on the " \
      "right device)") \
    /* 15-17: a reduction that is redone after an in-launch time-out counts both runs.  tests/test_gpu_gf2_structure.py asserts through
     * them which panel a matrix family took. */ \
    X(GF2_BLOCKS_PANELLED, 15, "blocks (of up to 64 rows) panelled by the blocked GF(2) elimination since load - the one-workgroup path for " \
      "matrices of at most 64 rows and 64 words counts none") \
    X(GF2_PANEL_FULL_ROWS, 16, "of 15, the blocks whose panel ran on the full rows in LDS") \
    X(GF2_PANEL_WINDOW, 17, "of 15, the blocks whose panel ran on the two-word window (the rest took the four-word window, or held zero " \
      "rows only)") \
    /* 18-21: a call with no rows on either side counts nothing.  tests/test_gpu_commute_families.py asserts through them which kernel a
     * call took. */ \
    X(COMMUTE_REGISTER_TILE, 18, "commutation calls (symgpu_commutes, symgpu_commutes_dev, symgpu_commutes_bits_dev and what is built on " \
      "them) served by the register-tile kernel") \
    X(COMMUTE_WIDE_ROWS, 19, "commutation calls served by the wide-row kernel") \
    X(COMMUTE_M4R_TILE, 20, "launches of the Four-Russians commutation kernel with one tile per workgroup (a stream-K request with fewer " \
      "tiles than compute units counts here)") \
    X(COMMUTE_M4R_STREAMK, 21, "launches of the Four-Russians commutation kernel as stream-K (persistent workgroups over the (tile, step) " \
      "space)") \
    /* 22-32: tests/test_gpu_rotation_families.py asserts through them which form and stage ran.  Rotations completed by the one-launch
     * kernel are counted by 1 alone. */ \
    X(CHAIN_REGISTERS, 22, "runs of Clifford rotations (symgpu_rotate_clifford_chain_dev with at least one row and one rotation, and the " \
      "runs that symgpu_perform_rotations_dev hands to it) served by the register chain") \
    X(CHAIN_LDS, 23, "runs of Clifford rotations served by the LDS-resident kernel") \
    X(CHAIN_SINGLE_WORKGROUP, 24, "runs of Clifford rotations served by the single-workgroup kernel") \
    X(CHAIN_TWO_LAUNCHES, 25, "runs of Clifford rotations served by the two-launch form") \
    X(CHAIN_FOUR_LAUNCHES, 26, "runs of Clifford rotations served by the four-launch form") \
    X(CHAIN_SORT_ONE_LAUNCH, 27, "segments (of up to 40 rotations) of the register chain whose keys were sorted by the one-launch sort (a " \
      "run that is redone after a time-out of the one-launch sort counts 27 and 28)") \
    X(CHAIN_SORT_LAUNCHES, 28, "segments (of up to 40 rotations) of the register chain whose keys were sorted by the multi-launch sort") \
    X(ROTATE_HASH_JOIN, 29, "single rotations (symgpu_rotate_single_dev) completed by the hash join") \
    X(ROTATE_CLIFFORD_FAST, 30, "single rotations completed by the Clifford fast path") \
    X(ROTATE_GENERAL, 31, "single rotations completed by the general path (stack + cleanup)") \
    X(ROTATE_GENERAL_BY_DUP_CHECK, 32, "of 31, odd-k Clifford rotations whose duplicate check found two equal rows") \
    /* 33-35: tests/test_gpu_rotate_resident.py and the full-size tests assert through them which form a shape took. */ \
    X(RESIDENT_LDS, 33, "one-launch rotations LAUNCHED (completed or not) with each block's rows in LDS") \
    X(RESIDENT_REGISTERS, 34, "one-launch rotations LAUNCHED (completed or not) with each block's rows in LDS and registers") \
    X(RESIDENT_ROWS_IN_MEMORY, 35, "one-launch rotations LAUNCHED (completed or not) with each block's rows left in memory") \
    /* 36-47: the fused product + cleanup (symgpu_mul_cleanup*, and what is built on them), counted once per ATTEMPT of a call (a call
     * that reseeds the row hash or repeats with the full sort counts every attempt).  Calls on 64-bit keys with an index sort (plain
     * cleanups, SYMGPU_CLEANUP_UNPACKED=1, index fields over 32 bits) count none of 36-46.  tests/test_gpu_pair_flows.py and
     * tests/test_gpu_product_coeff_stage.py assert through 36-52 which flow and path a call took. */ \
    X(FLOW_COMPLETE_SORT, 36, "the packed pair keys were ordered by the complete sort, no flag pass") \
    X(FLOW_FLAGS_HASH_TABLES, 37, "the flag pass was launched from the bucketed operand hash tables") \
    X(FLOW_FLAGS_PARTIAL_SORT, 38, "the flag pass was launched behind the partial sort") \
    X(FLOW_FLAGS_GAVE_UP, 39, "a flag pass came back with its give-up word set") \
    X(GIVEUP_PRODUCT_BUCKET, 40, "of 39, the hash-table pass by reason (one each for every reason it reported): a product bucket of more " \
      "than 16,384 pairs") \
    X(GIVEUP_COUNTER_SATURATED, 41, "of 39, the hash-table pass by reason: a saturated 4-bit counter") \
    X(GIVEUP_LIST_OVERFLOW, 42, "of 39, the hash-table pass by reason: an overflowing list") \
    X(GIVEUP_OPERAND_BUCKET, 43, "of 39, the hash-table pass by reason: an operand bucket of more than 255 terms") \
    X(FLOW_SORTED_WHOLE, 44, "the sort was finished on the whole array after the flag pass (most keys flagged, a give-up, or " \
      "SYMGPU_CLEANUP_SUSPECTS=2)") \
    X(FLOW_SORTED_FLAGGED, 45, "the flagged keys were sorted alone") \
    X(FLOW_MARKED_FROM_BYTES, 46, "the single terms were marked from one byte per pair") \
    X(FLOW_FULL_SORT_REPEAT, 47, "the attempt was repeated with the full 64-bit sort (a long run of equal key prefixes that holds " \
      "different keys)") \
    /* 48-52: calls of symgpu_mul_allpairs_dev (and of symgpu_mul_allpairs) with at least one pair to form (counted before the path runs,
     * whether or not it succeeds), by path. */ \
    X(PRODUCT_ROWS_ONLY, 48, "all-pairs products by path: rows only") \
    X(PRODUCT_PHASE_STREAM, 49, "all-pairs products by path: phase-byte row stream") \
    X(PRODUCT_WIDE_COEFF_THEN_ROWS, 50, "all-pairs products by path: wide coefficient kernel, then rows") \
    X(PRODUCT_WORD_MAJOR_THEN_ROWS, 51, "all-pairs products by path: word-major coefficient kernel, then rows") \
    X(PRODUCT_WORD_MAJOR_BESIDE_ROWS, 52, "all-pairs products by path: the same beside the rows on a second stream") \
    /* 53 / 54: one per call in LDS, one per chunk of workgroups whose slots fit the scratch limit otherwise.
     * tests/test_gpu_csr_families.py asserts through them which form a shape took and in how many launches. */ \
    X(CSR_FILL_LDS, 53, "launches of the fill kernel of symgpu_to_csr_fill (k_csr_fill) with its slots in LDS") \
    X(CSR_FILL_SCRATCH, 54, "launches of the fill kernel of symgpu_to_csr_fill (k_csr_fill) with its slots in global scratch") \
    /* 55 / 56: the cached device allocator (alloc.hip).  tests/test_gpu_handle_balance.py asserts through them that a call returns every
     * block it took: 55 is the same before and after, 56 does not move. */ \
    X(DEV_BLOCKS_LIVE, 55, "a GAUGE, not a count: device blocks handed out by the allocator and not yet returned to it (operators, their " \
      "caches, scratch, what the contexts keep); never below 0") \
    X(DEV_FREE_UNKNOWN, 56, "blocks returned to the allocator that it did not hold (a double free, a pointer from elsewhere); the call " \
      "fails with SYMGPU_E_INVALID and nothing is released") \
    /* 57-60: builds of what a handle caches between calls (symgpu_op_s, csrc/common.h), bumped where the build happens and nowhere else: a
     * call that finds its cache valid counts nothing.  tests/test_gpu_handle_state.py asserts through them that a cache is hit while the
     * rows stay and rebuilt once after every change of rows. */ \
    X(OP_WORD_MAJOR_BUILDS, 57, "word-major copies of an operator's rows built into its handle (op_wordmajor, layout.hip)") \
    X(OP_BIT_MAJOR_BUILDS, 58, "bit-major copies of an operator's rows built into its handle for the Four-Russians commutation kernel " \
      "(m4r_bit_major, commute_m4r.hip; a copy built into the call's scratch counts nothing)") \
    X(OP_YCOUNT_BUILDS, 59, "Y-count arrays built into an operator's handle (op_ycount, layout.hip)") \
    X(OP_ROW_HASH_BUILDS, 60, "row-hash arrays computed from an operand's rows into its handle (analyze_rows, rotate_analyze.hip; " \
      "ensure_row_hashes, rotate_resident.hip); hashes a rotation hands on to its result count nothing")
#define SYMGPU_COUNTER_ENUM_ENTRY(name, id, text) SYMGPU_CTR_##name = id,
typedef enum symgpu_counter { SYMGPU_COUNTER_LIST(SYMGPU_COUNTER_ENUM_ENTRY) SYMGPU_CTR_COUNT = 61 } symgpu_counter;
#undef SYMGPU_COUNTER_ENUM_ENTRY
/* *value = the counter `which` (an id of the list above; SYMGPU_E_INVALID outside it).  Needs no device and no context. */
int symgpu_debug_counter(int which, int64_t *value);
/* The name of counter `which` as spelled in the list ("HASH_RESEEDS", ...), NULL outside 0 .. 60: a binder builds its name -> id map from
 * it instead of copying numbers.  Needs no device and no context. */
const char *symgpu_debug_counter_name(int which);
/* The radix sort and the two scans that everything else stands on, run directly on device buffers of the caller's (symgpu_dev_alloc /
 * symgpu_dev_upload), for tests/test_gpu_sort.py.  All three return after a stream synchronisation.
 *  debug_sort       sorts keys[0..n) (and vals[0..n) with them, if not NULL) in place by key bits [begin_bit, end_bit) (a multiple of 8
 *                   wide), stable.  form 0: one launch per step of every pass; 1: all passes in one launch if the keys fit it (up to 2^19),
 *                   else as 0; 2: one launch where the library's thresholds choose it (up to 48 tiles of 4,096 keys, 32 with values), else
 *                   as 0.  with_first_hist != 0: the entry forms the tile histograms of the first pass itself and hands them in, as a caller
 *                   does whose own kernel reads the keys anyway; the sort then takes a launch per step whatever `form` says.
 *                   *form_ran = 1 if the one launch ran, 0 if the launches per step.  If the one launch gave up at a barrier (its
 *                   workgroups were not co-resident) the call returns SYMGPU_E_HIP, the buffers hold no sorted data, and the form is off
 *                   for the rest of the process (symgpu_degraded).
 *  debug_scan       out[i] = in[0] + .. + in[i - 1] (mod 2^32) for i < n, *total (may be NULL; device) = the sum of all; out may equal in.
 *                   SYMGPU_SCAN_RECURSIVE=1 forces the form of inputs over 2^23 elements.
 *  debug_popc_scan  out[w] = set bits in words [0, w) of a bitmap of 1 .. 8,192 64-bit words, *total (may be NULL; device) = all of them, in
 *                   one launch.  n32 = -1, or the number of 32-bit words the bitmap was written in (2 n_words or 2 n_words - 1): if odd, the
 *                   upper half of the last 64-bit word is unwritten and is not counted. */
int symgpu_debug_sort(uint64_t *keys, uint32_t *vals, int64_t n, int begin_bit, int end_bit, int form, int with_first_hist, int *form_ran);
int symgpu_debug_scan(const uint32_t *in, uint32_t *out, int64_t n, uint32_t *total);
int symgpu_debug_popc_scan(const uint64_t *bits, int64_t n_words, int64_t n32, uint32_t *out, uint32_t *total);
/* Fast paths that gave up in this process and were replaced by a slower, equally exact form — the one-launch rotation, the one-launch
 * radix sort, the fused selector launch of the GF(2) elimination: their in-kernel waits assume co-resident workgroups and are bounded, so
 * a shared or partitioned GPU turns them off.  Each is announced once on stderr; this returns the list ("" = nothing degraded). */
int symgpu_degraded(char *buf, int len);
/* tuning aid (library built with `make TUNING=1`): with SYMGPU_RES_TRACE=1 every workgroup of the one-launch rotation kernel stamps the 100 MHz wall clock at its phase
 * boundaries; this copies the stamps of the last traced launch, 16 words per workgroup */
int symgpu_debug_rotation_trace(uint64_t *out, int max_workgroups, int *n_workgroups);

/* measured on-box HBM ceilings for the roofline: one-shot 16-byte-per-thread fill (GB/s written) and copy (GB/s read+written)
 * over scratch buffers of `bytes` each (best of 3). */
int symgpu_membw_probe(int64_t bytes, double *fill_GBps, double *copy_GBps);

/* ---- device-resident operators -------------------------------------------------------------- */
int symgpu_op_upload(const uint64_t *rows, const double *coeff /* may be NULL */, int64_t T, int Wq, symgpu_op_t *out);
int symgpu_op_alloc(int64_t capacity_rows, int Wq, int with_coeff, symgpu_op_t *out);
int symgpu_op_download(symgpu_op_t op, uint64_t *rows, double *coeff /* may be NULL */, int64_t capacity_rows);
int symgpu_op_info(symgpu_op_t op, int64_t *T, int *Wq, int64_t *capacity_rows);
int symgpu_op_free(symgpu_op_t op);
int symgpu_op_set_rows(symgpu_op_t op, int64_t T);   /* trim (T <= capacity), e.g. after an all-gather with padding */
/* host rows (+ coefficients if both sides have them) -> rows [row_offset, row_offset + count) of an existing operator
 * (within its capacity; T grows to cover them).  Used by the host-staged all-gather. */
int symgpu_op_write(symgpu_op_t op, int64_t row_offset, const uint64_t *rows, const double *coeff /* may be NULL */, int64_t count);
/* device-to-device: rows (and coefficients, if both have them) src[src_offset .. +count) -> dst[dst_offset ..); stream ordered */
int symgpu_op_copy_rows(symgpu_op_t dst, int64_t dst_offset, symgpu_op_t src, int64_t src_offset, int64_t count);
int symgpu_op_random(int64_t T, int n_qubits, double density, uint64_t seed, symgpu_op_t *out); /* synthetic input, generated on device */
/* Handle-level primitives behind the device-resident drop-in classes (no reference counterpart: the reference keeps NumPy arrays):
 *  clone       rows (+ coefficients) copied device to device into a new handle
 *  set_coeff   the T coefficients replaced from a host array (allocated if the operator had none); rows and their cached layouts stay
 *  scale       in place c <- (conjugate_first ? conj(c) : c) * (re + i im)   (multiply_by_constant base.py:750-762, dagger :1366-1376)
 *  ycount      PauliwordOp.Y_count (base.py:604-615) of a resident operator -> int64[T] on the host
 *  upload_bool / download_bool   the reference layout itself (np.bool_ [T][2n], X columns then Z columns, base.py:42-74) <-> packed rows,
 *              packed / unpacked ON THE DEVICE: np.packbits on the host runs at ~1.5 GB/s of bools, PCIe + a ballot kernel at >10 GB/s */
int symgpu_op_clone(symgpu_op_t in, symgpu_op_t *out);
int symgpu_op_set_coeff(symgpu_op_t op, const double *coeff_host);
int symgpu_op_scale(symgpu_op_t op, double re, double im, int conjugate_first);
int symgpu_op_ycount(symgpu_op_t op, int64_t *out_host);
int symgpu_op_upload_bool(const uint8_t *symp /* [T][2n] */, const double *coeff /* may be NULL */, int64_t T, int n_qubits, symgpu_op_t *out);
int symgpu_op_download_bool(symgpu_op_t op, int n_qubits, uint8_t *symp_out /* [capacity_rows][2n] */, int64_t capacity_rows);
/* XOR-fold of all packed rows (2*Wq words) and plain sum of coefficients: size-independent checksums.  Either output may be NULL; an
 * operator without coefficients (or without rows) gives a zero sum.  The fold is defined for rows of up to 8,192 words (Wq <= 4,096: one
 * word per column in 64 KiB of LDS); wider rows are refused with SYMGPU_E_INVALID when xor_words is asked for. */
int symgpu_op_checksum(symgpu_op_t op, uint64_t *xor_words /* [2*Wq] */, double *coeff_sum /* [2] */);
/* number of set bits in all packed rows: sum_{i,o} |a_i ^ b_o| of a product slab follows from the operands' bit-column counts in O(N + M) */
int symgpu_op_popcount(symgpu_op_t op, uint64_t *sum);

/* ---- a2: PauliwordOp.Y_count  (symmer/operators/base.py:604-615) ----------------------------- */
int symgpu_ycount(const uint64_t *rows, int64_t T, int Wq, int64_t *out);

/* ---- a6: commutes_termwise / adjacency_matrix (base.py:938-971, 1054-1062; utils.py:9-78) ------
 * out[i*M + j] = 1 iff A[i] commutes with B[j] (np.bool_ layout of the reference's return value). */
int symgpu_commutes(const uint64_t *A, int64_t N, const uint64_t *B, int64_t M, int Wq, uint8_t *out);
/* device-resident; out_dev is a DEVICE pointer obtained from symgpu_dev_alloc (N*M bytes) */
int symgpu_commutes_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint8_t *out_dev);
/* bit-packed variant: out_bits[i*ceil(M/64) + j/64] bit (j%64); 1/8 byte per pair */
int symgpu_commutes_bits_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint64_t *out_bits_dev);
int symgpu_dev_alloc(int64_t bytes, void **ptr);
int symgpu_dev_free(void *ptr);
int symgpu_dev_download(const void *dev, void *host, int64_t bytes);
int symgpu_dev_upload(void *dev, const void *host, int64_t bytes);
/* number of 1 bytes among n bytes that must each be 0 or 1 (a commutation table: the number of commuting pairs); dev 16-byte aligned.
 * Other byte values are not summed: whole 16-byte groups are counted by their set bits. */
int symgpu_dev_checksum_u8(const uint8_t *dev, int64_t n, uint64_t *sum);
int symgpu_dev_popcount_u64(const uint64_t *dev, int64_t n_words, uint64_t *sum);

/* ---- a3/a4: all-pairs product  (base.py:764-794 `_multiply_by_operator`, :821-859 `__mul__`) ----
 * Output row o*Ni + i = inner[i] xor outer[o]; coefficient = c_inner[i]*c_outer[o]*i^e with
 * e = (3(Y_i+Y_o) + Y_out + 2|x_left & z_right|) mod 4, left = inner if inner_is_left else outer
 * (the reference's dagger-swap for N < M, base.py:847-849, folded into one exponent).  No cleanup. */
int symgpu_mul_allpairs(const uint64_t *inner, const double *ci, int64_t Ni,
                        const uint64_t *outer, const double *co, int64_t No, int Wq, int inner_is_left,
                        uint64_t *out_rows, double *out_coeff);
/* device-resident slab: outer rows [o_begin, o_end) -> out (capacity >= (o_end-o_begin)*Ni rows).  out must be a third handle: out == inner
 * or out == outer is refused with SYMGPU_E_INVALID (the rows would be read out of the buffer being written). */
int symgpu_mul_allpairs_dev(symgpu_op_t inner, symgpu_op_t outer, int64_t o_begin, int64_t o_end,
                            int inner_is_left, symgpu_op_t out);

/* ---- a5: symplectic_cleanup / PauliwordOp.cleanup (utils.py:230-279, base.py:617-638) ------------
 * Merge duplicate rows (sequential sum in input order), keep |c| > thr (strict) if use_thr, output in
 * first-occurrence order.  W = words per row (2*Wq).  n_out always receives the row count, also with SYMGPU_E_CAPACITY (the output
 * buffers are then untouched; they may be NULL when capacity is 0). */
int symgpu_cleanup(const uint64_t *rows, const double *coeff, int64_t T, int W, double thr, int use_thr,
                   uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out);
int symgpu_cleanup_dev(symgpu_op_t in, double thr, int use_thr, symgpu_op_t *out);
/* product + cleanup fused: product rows are never materialised (linear row hash of pairs) */
int symgpu_mul_cleanup(const uint64_t *inner, const double *ci, int64_t Ni,
                       const uint64_t *outer, const double *co, int64_t No, int Wq, int inner_is_left,
                       double thr, int use_thr,
                       uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out);
int symgpu_mul_cleanup_dev(symgpu_op_t inner, symgpu_op_t outer, int inner_is_left, double thr, int use_thr,
                           symgpu_op_t *out);
/* The same two device calls with the FIRST-OCCURRENCE INDEX of every output term kept on the result (read it with symgpu_op_first_index):
 * the position of the first input row of a plain cleanup, (o << 32) | i of a product's first pair (o: outer index, i: inner index; the
 * reference's pair index is o * Ni + i, base.py:783-792).  A caller that cleans ONE product in parts — symmer_amd/parallel.py, the
 * hash-partitioned multi-GPU cleanup — merges the parts in the reference's first-occurrence order with it (utils.py:271). */
int symgpu_cleanup_indexed_dev(symgpu_op_t in, double thr, int use_thr, symgpu_op_t *out);
int symgpu_mul_cleanup_indexed_dev(symgpu_op_t inner, symgpu_op_t outer, int inner_is_left, double thr, int use_thr, symgpu_op_t *out);
int symgpu_op_first_index(symgpu_op_t op, uint64_t *first_host, int64_t capacity_rows);
/* Device side of the hash-partitioned multi-GPU cleanup (symmer_amd/parallel.py): out = op[idx] (rows + coefficients); the indices of an
 * indexed product of two gathered sub-operands rewritten to pair indices of the complete operands (o_global * Ni_global + i_global); an index
 * array attached to an operator (the shares received from other ranks); and the merge of indexed operators: concatenated, ordered by index
 * (keys below 2^key_bits; 0 = 64), then — do_cleanup — rows that several parts share merged at their smallest index with the cleanup's
 * semantics and threshold.  The result carries its indices again (ascending). */
int symgpu_op_gather(symgpu_op_t op, const int64_t *idx_host, int64_t n, symgpu_op_t *out);
int symgpu_part_global_index(symgpu_op_t part, const int64_t *inner_idx_host, int64_t n_inner, const int64_t *outer_idx_host, int64_t n_outer,
                             int64_t Ni_global);
int symgpu_op_set_first_index(symgpu_op_t op, const uint64_t *first_host);
int symgpu_merge_indexed_dev(const symgpu_op_t *parts, int n_parts, int key_bits, int do_cleanup, double thr, int use_thr, symgpu_op_t *out);

/* ---- a7: _rotate_by_single_Pword (base.py:1090-1161), one fused pass ------------------------------
 * clifford_k < 0: non-Clifford: cleanup([commuting, cos*anticommuting, -i*sin*(anticommuting*Q)], thr)
 * clifford_k >= 0 (= round(2*angle/pi)): [rotated anticommuting rows, commuting rows], no merge;
 *   odd k: c*i^e*(-i); k in {2,3}: negated (not reduced mod 4, base.py:1148).
 * *all_commute = 1 (and out untouched / *out = NULL) when every row commutes with Q — also when there is no row (N = 0); the host-array
 * call then sets *n_out = N: the result is the input, which the caller still holds.  Otherwise *n_out is the result's row count, also
 * when the call returns SYMGPU_E_CAPACITY (out untouched). */
int symgpu_rotate_single(const uint64_t *rows, const double *coeff, int64_t N, int Wq, const uint64_t *q_row,
                         double cos_t, double sin_t, int clifford_k, double thr,
                         uint64_t *out_rows, double *out_coeff, int64_t capacity, int64_t *n_out, int *all_commute);
int symgpu_rotate_single_dev(symgpu_op_t in, const uint64_t *q_row_host, double cos_t, double sin_t, int clifford_k,
                             double thr, symgpu_op_t *out, int *all_commute);
/* The same call, also returning the result's term count (0 when *out == NULL): the drop-in class needs it for every rotation
 * (base.py:1159-1161: a rotation that leaves no term returns 0 * I) and saves a symgpu_op_info round trip per call. */
int symgpu_rotate_single_dev_n(symgpu_op_t in, const uint64_t *q_row_host, double cos_t, double sin_t, int clifford_k,
                               double thr, symgpu_op_t *out, int *all_commute, int64_t *n_out);

/* A run of K Clifford rotations (perform_rotations, base.py:1163-1186, on pi/2-multiples; CircuitSymmerlator) of a CLEAN
 * operator: `in` must come from a cleanup (no duplicate rows, every |c| > 1e-15) — then every step is a stable partition
 * [anticommuting | commuting] + row ^= Q + exact phase, exactly what the reference's rotation followed by cleanup() returns, the
 * term count never changes and nothing has to come back to the host between the steps.  Up to 1,536 rows the whole run is ONE
 * single-workgroup launch; larger operators (<= 2^22 rows) run the per-rotation kernels back to back without a read-back.
 * q_rows: K packed rows; ks: clifford_k per rotation, 0..3 as for symgpu_rotate_single (k = round(2*angle/pi) mapped as
 * symmer_amd.kernels.rotation_args). */
int symgpu_rotate_clifford_chain_dev(symgpu_op_t in, const uint64_t *q_rows_host, const int *ks_host, int64_t K, symgpu_op_t *out);
/* perform_rotations (base.py:1163-1186) on a device-resident operator in ONE call: rotations r = 0 .. K-1 (q_rows[r][2*Wq], cos_t[r], sin_t[r],
 * ks[r] = clifford_k as for symgpu_rotate_single_dev) applied in order, each followed by the reference's cleanup() — which is the identity once the
 * operator is clean (`clean` != 0 on entry says it already is), so it runs once; runs of Clifford rotations of a clean operator go through the chain
 * entry point.  acted[r] (may be NULL; zeroed by the caller) is set where a single rotation changed the operator.  The call always processes all K
 * rotations (*n_done == K on success): an operator that loses all its terms is taken through the reference's alternation between "no terms" and
 * 0 * I (cleanup() of an empty operator, base.py:631-632, utils.py:275-278) INSIDE the call — the caller must not apply it again — and *clean_out
 * reflects the state after the last rotation.  *out = NULL: nothing changed, keep using `in` (which is never freed here). */
int symgpu_perform_rotations_dev(symgpu_op_t in, const uint64_t *q_rows_host, const double *cos_t, const double *sin_t, const int *ks_host, int64_t K,
                                 double thr, int clean, symgpu_op_t *out, uint8_t *acted, int64_t *n_done, int *clean_out);

/* ---- a8: _rref_binary (utils.py:292-315): in place, no row swaps, leftmost pivot, eliminate above and
 * below.  xor_count (may be NULL) = sum_i |update_set_i| as the reference loop performs them.
 * pivots (may be NULL) = pivot column per row or -1. */
int symgpu_rref(uint64_t *rows, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots);
int symgpu_rref_dev(uint64_t *rows_dev, int64_t R, int64_t Wc, int64_t *xor_count, int64_t *pivots_host);

/* ---- a9: IndependentOp.symmetry_generators (independent_op.py:124-126) ----------------------------
 * H: M packed rows over n qubits.  out: generators as packed rows in the reference's order; *k = count.
 * capacity in rows (2n always suffices). */
int symgpu_symmetry_kernel(const uint64_t *H, int64_t M, int n_qubits, int Wq,
                           uint64_t *out, int64_t capacity, int64_t *k, int64_t *xor_count);
int symgpu_symmetry_kernel_dev(symgpu_op_t H, int n_qubits, uint64_t *out, int64_t capacity, int64_t *k,
                               int64_t *xor_count);

/* ---- f2: generator routines on packed rows, device side (csrc/genrec.hip) ------------------------------------------------
 * symgpu_op_gf2_rank   rank over GF(2) of the operator's symplectic rows = number of non-zero rows of _rref_binary(symp_matrix)
 *   (utils.py:292-315); check_independent (utils.py:504-519) is `rank == T`.
 * symgpu_generators_dev   PauliwordOp.generators (base.py:1436-1456): the non-zero rows of _rref_binary(symp_matrix), in row order, with
 *   coefficient 1 — a new resident operator.
 * symgpu_generator_reconstruction_dev   PauliwordOp.generator_reconstruction (base.py:523-560): reduced = cref_binary(vstack([G, M]))
 *   (utils.py:349-359); recon_host int64 [T][g] = reduced[g:, :g] (the reference returns .astype(int)), mask_host uint8 [T] =
 *   all(~reduced[g:, g:], axis=1).  g = G's terms (1 <= g <= 2n), T = M's terms (>= 1).  The transposed stack is built bit-packed on the
 *   device, reduced by the blocked elimination and read out in pivot order: no one-byte-per-bit matrix on either side. */
int symgpu_op_gf2_rank(symgpu_op_t op, int64_t *rank);
int symgpu_generators_dev(symgpu_op_t op, symgpu_op_t *out);
int symgpu_generator_reconstruction_dev(symgpu_op_t G, symgpu_op_t M, int n_qubits, int64_t *recon_host, uint8_t *mask_host);

/* ---- f3 / f4: the callers next to the hot path, device side -----------------------------------------------------------
 * symgpu_project_dev   S3Projection._perform_projection (symmer/projection/base.py:44-84) on an operator that has already been taken
 *   through the stabiliser rotations: terms that anticommute with any of the k fixed (single-qubit) stabiliser rows vanish; the others
 *   are multiplied by (-1)^|row & neg_mask| (neg_mask: the symplectic positions of the stabilisers with eigenvalue -1, i.e. the product
 *   of eigenvalues over the occupied stabilised positions, :68-71); the qubits not listed in keep_qubits (ascending) are deleted and equal
 *   terms merged with the cleanup's semantics (:82).  stab_rows [k][2*Wq], neg_mask [2*Wq], keep_qubits [n_keep >= 1]: host arrays.
 * symgpu_noncontextual_dev   PauliwordOp.is_noncontextual (base.py:1074-1088, check_adjmat_noncontextual utils.py:567-589): 1 iff the
 *   terms that do not commute with every term split into disjoint cliques of the commutation graph.
 * symgpu_state_inner_dev   QuantumState bra * ket (base.py:1808-1815): sum over the basis rows present in both CLEANED states of
 *   c_a * c_b, added in the order of a's rows (pass the state with fewer terms as a, as the reference does).  out: double[2]. */
int symgpu_project_dev(symgpu_op_t op, const uint64_t *stab_rows, int k, const uint64_t *neg_mask, const int *keep_qubits, int n_keep,
                       int n_qubits, double thr, int use_thr, symgpu_op_t *out, int64_t *n_survived /* may be NULL: terms that commute with every stabiliser */);
int symgpu_noncontextual_dev(symgpu_op_t op, int *is_noncontextual);
int symgpu_state_inner_dev(symgpu_op_t a, symgpu_op_t b, double *out);

/* ---- f3, batched: every term of <phi|H|psi> in one call (PauliwordOp.expval / single_term_expval, base.py:796-819, 2438-2471;
 * csrc/expval.hip).  For term k of op with symplectic row (x, z) and Y count y = |x & z|
 *   <phi|P_k|psi> = i^y  sum over b in supp psi with b ^ x in supp phi of  conj(phi[b ^ x]) psi[b] (-1)^{|z & b|}
 * phi and psi are CLEANED state operators (results of a cleanup, with coefficients, the Wq of op; SYMGPU_E_INVALID otherwise); only their
 * X halves (the basis strings) and coefficients enter the sums, the Z halves (~X below n, zero above) only the hash.  phi == psi (the same
 * handle) is the expectation value and builds one table.  op needs coefficients and is NOT cleaned: a repeated term has its own entry.
 *   out_terms (may be NULL) double [T][2]: <phi|P_k|psi> as (re, im), without the term's coefficient
 *   out_total double [2]: 0 + c_0 e_0 + c_1 e_1 + ..., plain IEEE complex products added in term order by one wavefront
 * T = 0 or a state without terms: zeros, *form = 0.  Fewer than 2^31 basis states per state.
 * Summation order (every run and both forms give the same bits): the states of psi in chunks of C = max(64, the power of two at or above
 * S_psi / 64) consecutive rows; within a chunk the products conj(phi) psi, negated where |z & b| is odd, are added to 0 in row order;
 * the chunk sums are added to 0 in ascending order; then i^y as a component swap.
 * *form (may be NULL) = SYMGPU_EXPVAL_LDS: the look-up table over phi's rows, phi's coefficients and X halves were staged into LDS once per
 * workgroup, taken when  S_phi (16 + 8 Wq) + 4 cap <= 65536,  cap = the power of two at or above max(64, 2 S_phi)  (Wq = 1: S_phi <= 2048);
 * or SYMGPU_EXPVAL_GLOBAL: they stayed in memory.  SYMGPU_EXPVAL_FORM=global (read on every call) forces the second form.
 * Every device scratch buffer is freed before the call returns, also on failure; one read-back, at the end. */
#define SYMGPU_EXPVAL_LDS 1
#define SYMGPU_EXPVAL_GLOBAL 2
int symgpu_expval_terms_dev(symgpu_op_t op, symgpu_op_t phi, symgpu_op_t psi, double *out_terms /* [T][2] or NULL */, double *out_total /* [2] */,
                            int *form /* or NULL */);

/* ---- f5: PauliwordOp.to_sparse_matrix (base.py:1458-1507) of a resident operator, n_qubits 1 .. 31, as CSR (csrc/sparse_matrix.hip) -------
 * Entry (b, b ^ x_k) = sum over terms k, in operator order, of c_k (-i)^{Y_k} (-1)^{|b & z_k|}; qubit 0 is the MOST significant bit of
 * b and of x_k, z_k.  Duplicate terms are summed, the operator is not cleaned first; entries whose two components are both +-0 are not
 * stored, NaN / inf ones are.  Columns ascend within a row.
 * symgpu_to_csr_count   groups the terms by X-part, counts the kept entries of every row and scans them into a 64-bit indptr, all on the
 *   operator's device; *nnz = the exact entry count, *fill_scratch_bytes = the device scratch the fill will allocate besides its output
 *   (data, indices, and an int32 indptr when index_bytes = 4).  The grouped terms and indptr stay on the device in *plan (the operator is
 *   not referenced again).
 * symgpu_to_csr_fill    consumes the plan: data (complex128 [nnz]), indices ([nnz]) and indptr ([2^n + 1]), both of index_bytes = 4
 *   (int32) or 8 (int64), written into host buffers; every device buffer of the plan is freed before it returns, also on failure.
 *   All three buffers NULL: the plan is only freed (a caller that cannot hold the output).  SYMGPU_CSR_SCRATCH=1 forces the fill's
 *   global-scratch form (taken by itself when a row's groups do not fit the LDS).  SYMGPU_CSR_SCRATCH_MIB=m replaces the 512 MiB limit
 *   of that scratch per launch by m MiB (the floor of four workgroups per compute unit per launch stays): the fill then takes several
 *   launches at a small size, as it does by itself when the slots of all rows exceed 512 MiB. */
typedef struct symgpu_csr_s *symgpu_csr_t;
int symgpu_to_csr_count(symgpu_op_t op, int n_qubits, int64_t *nnz, int64_t *fill_scratch_bytes, symgpu_csr_t *plan);
int symgpu_to_csr_fill(symgpu_csr_t plan, double *data, void *indices, void *indptr, int index_bytes);

/* ---- f7: H x on a dense statevector without the matrix, and the vector kernels of exact_gs_energy (symmer/utils.py:14-76;
 * csrc/matvec.hip, csrc/lanczos.hip).  Conventions of f5: qubit 0 is the MOST significant bit of a basis index b; for term k, x_k and z_k
 * are its X and Z parts as n-bit integers, Y_k = |x_k & z_k|, c'_k = c_k (-i)^{Y_k} (an exact component swap), and
 *   (H v)[b] = sum_k c'_k (-1)^{|b & z_k|} v[b ^ x_k]
 * The operator is not cleaned: repeated terms each count.  Vectors are complex128 [2^n] device buffers of symgpu_dev_alloc.
 * symgpu_matvec_plan   groups the terms of a resident operator (with coefficients, Wq = 1) by X-part on its device and keeps c', z and the
 *   group table resident in *plan; the operator is not referenced afterwards.  n_qubits 1 .. 32, anything else SYMGPU_E_INVALID before
 *   anything is allocated.  T = 0 is a valid plan (H = 0).  symgpu_matvec_free frees it; symgpu_matvec_info reports its sizes (any output
 *   may be NULL): n_groups = the distinct X-parts G, device_bytes = what the plan holds, 20 T + 8 G + 4 (0 for T = 0).
 * symgpu_matvec_apply   y = H x, x != y.  Summation order, the same on every run (no floating-point atomics; two calls give the same
 *   bits): row b is  D_0(b) x[b ^ x_0] + D_1(b) x[b ^ x_1] + ...  over the groups in ascending x, the sum started from the first product,
 *   every product a plain IEEE complex product (re = D.re x.re - D.im x.im, im = D.re x.im + D.im x.re, each operation rounded);
 *   D_g(b) = sum_{k in g} c'_k (-1)^{|b & z_k|}, the terms of a group in operator order, started from the first term.  T = 0: zeros.
 *   *form (may be NULL) = SYMGPU_MATVEC_DIRECT: one thread per row, the gathered element read straight from memory (a wavefront's 64 rows
 *   read 64 consecutive elements); 0 when no kernel ran (T = 0).  It is the only form: none other has been measured to pay, so
 *   there is no switch.  A workgroup takes 2^8 consecutive rows.
 * symgpu_matvec_sector_mask   plan_N must have no term with x != 0 (SYMGPU_E_INVALID otherwise); keep_dev uint8 [2^n]: keep[b] = 1 iff
 *   the nearest integer to Re D_0(b) equals n_particles, else 0; *n_kept = the number of kept states.
 * symgpu_lanczos_step   basis_dev complex128 [capacity][2^n], slots 0 .. j hold orthonormal vectors, 0 <= j < capacity < 65536.
 *   w = keep o (H v_j) (keep_dev uint8 [2^n] or NULL); h_i = <v_i, w> for i <= j; *alpha = Re h_j; w <- w - h_0 v_0 - ... - h_j v_j in
 *   that order; the same again (classical Gram-Schmidt done twice; the second pass does not change alpha); *beta = |w|; if
 *   j + 1 < capacity and beta > 0, v_{j+1} = w / beta.  All j + 1 inner products of a pass come from one launch over the basis and all
 *   subtractions from one.  Nothing but the two scalars returns to the host.
 *   Reductions run in a fixed two-level order: chunks of C = max(256, 2^n / 1024) consecutive elements; within a chunk thread t of 256
 *   adds the products conj(v[b]) w[b] of elements t, t + 256, ... to 0 in ascending order, and the 256 thread sums are folded by
 *   halving (s[t] += s[t + 128], then 64, ... 1); one workgroup then adds the chunk sums to 0 in ascending chunk order.
 * symgpu_vec_combine   out = s_0 v_0 + ... + s_{m-1} v_{m-1} over the first m vectors of basis_dev ([m][2^n]), s_host double [m], the sum
 *   started from the first product; normalise != 0: then out / |out| (the norm in the order above; a zero vector stays zero).  out may
 *   be slot 0 of the basis: the restart of the iteration.  The call takes no plan, so it runs on the calling thread's CURRENT device: the
 *   basis and out must live there.
 * The device memory is checked before it is allocated (SYMGPU_E_NOMEM); every scratch buffer is freed before a call returns, also on
 * failure. */
#define SYMGPU_MATVEC_DIRECT 1
struct symgpu_matvec_s;   /* a plan: opaque, owned by the caller between symgpu_matvec_plan and symgpu_matvec_free */
int symgpu_matvec_plan(symgpu_op_t op, int n_qubits, struct symgpu_matvec_s **plan);
int symgpu_matvec_free(struct symgpu_matvec_s *plan);
int symgpu_matvec_info(struct symgpu_matvec_s *plan, int *n_qubits, int64_t *n_terms, int64_t *n_groups, int64_t *device_bytes);
int symgpu_matvec_apply(struct symgpu_matvec_s *plan, const double *x_dev, double *y_dev, int *form /* or NULL */);
int symgpu_matvec_sector_mask(struct symgpu_matvec_s *plan_N, int64_t n_particles, uint8_t *keep_dev, int64_t *n_kept);
int symgpu_lanczos_step(struct symgpu_matvec_s *plan, const uint8_t *keep_dev /* or NULL */, double *basis_dev, int64_t capacity, int64_t j,
                        double *alpha, double *beta);
int symgpu_vec_combine(const double *basis_dev, int64_t m, int n_qubits, const double *s_host, double *out_dev, int normalise);

/* ---- f8: variational states on a dense statevector (symmer/evolution/variational_optimization.py VQE_Driver, ADAPT_VQE; csrc/ansatz.hip):
 * |psi(theta)> = U_{K-1} ... U_0 |ref>, U_k = exp(i theta_k P_k) = cos theta_k + i sin theta_k P_k, the energy <psi|H|psi>, its gradient
 * by one reverse sweep, and the gradient of a whole operator pool.  Conventions of f5 / f7: qubit 0 is the MOST significant bit of a basis
 * index b; for a generator with X part x, Z part z (n-bit integers) and Y = |x & z|:  (P v)[b] = (-i)^Y (-1)^{|b & z|} v[b ^ x].
 * Vectors are complex128 [2^n] device buffers of symgpu_dev_alloc; n_qubits 1 .. 32, anything else SYMGPU_E_INVALID before anything is
 * allocated; the rows of gens / pool have Wq = 1, their coefficients are not read.
 * symgpu_ansatz_plan   takes the K rows of a resident operator in operator order, not cleaned (a repeated generator is its own parameter;
 *   an identity row is a valid generator, a global phase) and keeps x, z and Y mod 4 of each resident in *plan (16 bytes each); the
 *   operator is not referenced afterwards.  K = 0 is a valid plan.  symgpu_ansatz_free frees it; symgpu_ansatz_info reports n, K, the
 *   number of tiled runs (below) and the device bytes (16 K, 32 K when there is a tiled run); any output may be NULL.
 * symgpu_ansatz_apply   applies U_k for k = k_begin .. k_end-1 to psi_dev in place, in that order, or with reverse != 0 from k_end-1 down
 *   to k_begin.  cos_t / sin_t: host double [K], indexed by k, the caller's cos theta_k and sin theta_k (the device arithmetic does not
 *   depend on a libm); pass -sin for the inverse rotations.  Per amplitude, with a = psi[b], p = psi[b ^ x] (p = a for x = 0),
 *   c = cos_t[k], s' = +-sin_t[k] with the sign (-1)^{|b & z| + (Y >> 1)} (an exact sign change):
 *     odd Y:   psi'[b] = (c a.re + s' p.re, c a.im + s' p.im)          even Y:   psi'[b] = (c a.re + (-(s' p.im)), c a.im + s' p.re)
 *   every product and every sum rounded once to IEEE double, nothing contracted: a NumPy restatement gives the same bits.  One launch per
 *   rotation over the 2^(n-1) SLOTS: slot t owns, for x != 0, the pair (b0, b0 ^ x) where b0 is t with a clear bit inserted at the top set
 *   bit of x, and for x = 0 the elements t and t + 2^(n-1); its thread reads both and writes both (64-bit indices).
 *   That is the DIRECT form.  The TILED form gives the same bits with one pass over the vector per RUN of rotations.  The plan cuts the
 *   sequence greedily: a run's tile bits S start as the 4 lowest index bits (contiguous pieces of 256 bytes) and grow by each generator's
 *   X-part while |S| <= min(n, 12) (2^12 amplitudes = 64 KiB of LDS); x = 0 joins any open run; a generator that does not fit closes the
 *   run and opens the next, or, when its own X-part with the 4 low bits exceeds the budget, takes a direct pass; a closed run of fewer
 *   than min(n, 10) tile bits takes the lowest free bits up to that number.  A workgroup loads the 2^|S| amplitudes that agree outside S,
 *   applies the run's rotations (those of the requested range) in LDS with a barrier between them — the same arithmetic, the sign of the
 *   bits outside S uniform to the workgroup — and writes them back.  Runs are planned on the whole sequence; a range clips them.
 *   *form (may be NULL) = SYMGPU_ANSATZ_DIRECT | SYMGPU_ANSATZ_TILED, the forms that ran; 0 when no rotation ran.
 *   SYMGPU_ANSATZ_FORM=direct (read on every call) forces direct passes, also in the forward half of symgpu_ansatz_energy_grad; the
 *   reverse sweep is always direct.
 * symgpu_ansatz_energy_grad   psi = a copy of ref_dev, all K rotations applied; phi = H psi (symgpu_matvec_apply's kernel and order);
 *   *energy = Re<psi, phi> in the two-level order of symgpu_lanczos_step (the same kernels).  psi_out_dev (or NULL) gets psi, the bits of
 *   symgpu_ansatz_apply.  grad_host (double [K] or NULL) gets dE/dtheta_k from one reverse sweep with lambda = phi: for k = K-1 .. 0 one
 *   launch forms t_k = sum_b Im conj(lambda[b]) (P_k psi)[b] from the values before the update and applies U_k^+ (c, -s) to psi and lambda
 *   in place (a slot's thread reads four amplitudes and writes four); g_k = -2 t_k.  For a Pauli generator g_k equals the parameter shift
 *   E(theta + pi/4 e_k) - E(theta - pi/4 e_k).  Order of t_k: the slots are cut into chunks of C = max(256, 2^(n-1) / 1024) consecutive
 *   slots; thread t of 256 adds (term of b0 + term of b1) of slots t, t + 256, ... of its chunk to 0 in ascending order, a term being
 *   lambda.re q.im - lambda.im q.re for q = (P_k psi)[b]; the 256 thread sums are folded by halving (s[t] += s[t + 128], then 64, ... 1);
 *   after the sweep one launch adds the chunk sums of every k to 0 in ascending chunk order and multiplies by -2.  Only K + 1 doubles
 *   return to the host, in one read-back.  Scratch: two vectors, the [K][chunks] chunk sums when a gradient is asked for.
 * symgpu_pool_gradient   phi = H psi once; grad_host[j] = -2 sum_b Im conj(phi[b]) (P_j psi)[b] = <psi| i [H, P_j] |psi> for every row j of
 *   `pool` (on the plan's device); *energy (or NULL) = Re<psi, phi> as above.  Order: the 2^n elements are cut into chunks of
 *   C = max(256, 2^n / 1024); workgroup (chunk, j): thread t adds the terms of elements t, t + 256, ... of the chunk to 0 in ascending
 *   order, the thread sums folded by halving; one launch adds the chunk sums in ascending chunk order and multiplies by -2.  M = 0 with
 *   energy NULL returns at once.  One read-back of M + 1 doubles.
 * No floating-point atomics anywhere: two calls with the same input give the same bits.  The device memory is checked before it is
 * allocated (SYMGPU_E_NOMEM); every scratch buffer is freed before a call returns, also on failure. */
#define SYMGPU_ANSATZ_DIRECT 1
#define SYMGPU_ANSATZ_TILED 2
struct symgpu_ansatz_s;   /* a plan: opaque, owned by the caller between symgpu_ansatz_plan and symgpu_ansatz_free */
int symgpu_ansatz_plan(symgpu_op_t gens, int n_qubits, struct symgpu_ansatz_s **plan);
int symgpu_ansatz_free(struct symgpu_ansatz_s *plan);
int symgpu_ansatz_info(struct symgpu_ansatz_s *plan, int *n_qubits, int64_t *n_generators, int64_t *n_runs, int64_t *device_bytes);
int symgpu_ansatz_apply(struct symgpu_ansatz_s *plan, const double *cos_t, const double *sin_t, int64_t k_begin, int64_t k_end, int reverse,
                        double *psi_dev, int *form /* or NULL */);
int symgpu_ansatz_energy_grad(struct symgpu_ansatz_s *plan, struct symgpu_matvec_s *plan_H, const double *cos_t, const double *sin_t,
                              const double *ref_dev, double *psi_out_dev /* or NULL */, double *energy, double *grad_host /* [K] or NULL */);
int symgpu_pool_gradient(struct symgpu_matvec_s *plan_H, symgpu_op_t pool, const double *psi_dev, double *energy /* or NULL */,
                         double *grad_host /* [M] */);

/* ---- f9: the reduced density matrix of a dense statevector (symmer/operators/base.py:2025-2054 QuantumState.partial_trace_over_qubits,
 * get_rdm; symmer/utils.py:78-94 get_entanglement_entropy; csrc/rdm.hip).  Conventions of f7 / f8: qubit q is bit n-1-q of a basis index
 * b.  kept_host: the k kept qubits, strictly ascending.  The row index a of rho carries the kept qubits with the lowest qubit number as
 * its most significant bit, e carries the traced qubits the same way, b(a, e) is the index with both in place, and
 *   rho[a][a'] = sum_e psi[b(a, e)] conj psi[b(a', e)]
 * psi_dev: complex128 [2^n] (symgpu_dev_alloc), not normalised by the call and not written.  rho_dev: complex128 [2^k][2^k], row-major.
 * n_qubits 1 .. 32, k 0 .. min(n_qubits, 12) — a refusal bound that keeps the matrix to 256 MiB and a host eigensolve possible, not a
 * performance claim.  k = 0 gives the 1 x 1 matrix <psi|psi>, k = n gives psi psi^+.  SYMGPU_E_INVALID, before anything is allocated and
 * with psi and rho untouched: n_qubits or k outside the range, kept_host not strictly ascending or outside 0 .. n-1, a null psi_dev,
 * rho_dev or kept_host (kept_host may be NULL when k = 0), rho_dev overlapping psi_dev.
 * Result: only a <= a' is summed and rho[a'][a] is written as the exact conjugate of rho[a][a'], so rho is Hermitian to the bit; the
 * diagonal is sum_e (re^2 + im^2) with imaginary part +0.0.  One multiply-add, with p = psi[b(a, e)], q = psi[b(a', e)]:
 *   re <- fma(p.im, q.im, fma(p.re, q.re, re)),  im <- fma(-p.re, q.im, fma(p.im, q.re, im))      (the diagonal: re only)
 * No floating-point atomics; every sum runs in an order fixed by (n, kept) and the form: two calls give the same bytes.
 * Two forms, chosen once per call from (n, k); global reads go in index order in both (pieces of at least 2^4 amplitudes = 256 bytes
 * whatever the kept set is), the kept / traced split is applied when LDS is indexed:
 *   SYMGPU_RDM_STREAM (k <= KS = 3): one pass over psi.  The tile bits are the kept bits and the min(8, n-k) lowest traced index bits; a
 *     workgroup stages a tile in LDS and thread t takes e = tile 2^min(8, n-k) + t, its 2^k amplitudes and the upper triangle in
 *     registers.  The tiles are cut into C = min(tiles, 1024) chunks of consecutive tiles, one workgroup each, tiles ascending; the 256
 *     thread sums of an entry are folded by halving (s[t] += s[t + 128], then 64, ... 1); one last launch adds the chunk sums to 0 in
 *     ascending chunk order.  Scratch: C 2^k (2^k + 1) / 2 entries of 16 bytes.
 *   SYMGPU_RDM_TILED (every other k): a Hermitian rank update on tiles of 64 x 64 entries, only the tile pairs I <= J.  e goes in blocks
 *     of 2^min(4, n-k) values, the blocks in C chunks of consecutive blocks, C = min(blocks, the largest power of two <=
 *     max(1, 1024 / pairs)) — a function of (n, k) only.  Workgroup (pair, chunk): per block the 64 x 2^4 panel of the row tile and of the
 *     column tile (one panel on the diagonal) is staged in LDS, thread (ty, tx) of 16 x 16 adds to its 4 x 4 entries (rows ty + 16 i,
 *     columns tx + 16 j), e ascending, from 0 (on a diagonal tile only to those with i <= j: the others lie below the diagonal for
 *     every thread).  Chunk tiles go to scratch [C][2^k][2^k] (C 4^k 16 bytes, at most 256 MiB); one launch adds
 *     them to 0 in ascending chunk order and writes both triangles.
 * SYMGPU_RDM_FORM=stream|tiled (read on every call) forces a form where it is legal: tiled accepts every k, stream beyond KS is ignored.
 * info (int64 [6] or NULL): [0] the form that ran, [1] KS, [2] C, [3] the tile edge (64; 0 for STREAM), [4] the workgroups of the
 * accumulating launch, [5] the scratch bytes.  The device memory is checked before it is allocated (SYMGPU_E_NOMEM); the scratch is freed
 * before the call returns, also on failure.  The call runs on the calling thread's CURRENT device. */
#define SYMGPU_RDM_STREAM 1
#define SYMGPU_RDM_TILED 2
int symgpu_rdm(const double *psi_dev, int n_qubits, const int *kept_host, int k, double *rho_dev /* complex128 [2^k][2^k], row-major */,
               int64_t *info /* [6] or NULL */);

/* ---- f10: measuring a statevector (symmer/operators/base.py:2070-2096 QuantumState.sample_state, :2188-2212
 * measure_state_in_computational_basis, :2474 ff. change_of_basis_XY_to_Z; csrc/sample.hip, csrc/basis.hip).  Conventions of f7 - f9:
 * qubit q is bit n-1-q of a basis index, amplitudes are complex128, no floating-point atomics, every sum in the order stated here, two
 * calls with the same input give the same bytes.  Every call runs on the calling thread's CURRENT device (a plan: on the plan's).
 *
 * Uniforms.  symgpu_philox_uniform writes draws first_draw .. first_draw + count - 1 of the stream of `seed` to out_dev (double [count]).
 *   Draw s (counted from 0) is word s mod 4 of the Philox4x64-10 block with key (seed, 0) and counter (s div 4 + 1, 0, 0, 0); the double
 *   is (word >> 11) * 2^-53.  Philox4x64-10: ten rounds (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
 *   with the multipliers M0 = 0xD2E7470EE14C6C93, M1 = 0xCA5A826395121157 (hi / lo: the halves of the 128-bit product), the key advanced
 *   between rounds by the Weyl constants k0 += 0x9E3779B97F4A7C15, k1 += 0xBB67AE8584CAA73B.  This is, bit for bit, the stream of
 *   numpy.random.Generator(numpy.random.Philox(key=seed, counter=0)).random(): a draw is a pure function of (seed, s), so launches,
 *   batches and the offset carry no state.  SYMGPU_E_INVALID: a null out_dev, a negative first_draw or count, first_draw + count >= 2^63.
 *
 * Plan.  symgpu_sample_plan takes m >= 1 amplitudes (any m up to 2^40, not only a power of two) at amp_dev, which the plan REFERENCES
 *   and never writes: the caller keeps them alive and unchanged until symgpu_sample_free.  The weight is w[i] = re re + im im: two
 *   products and one sum, each rounded once, nothing contracted.  Above the weights sits a radix-16 tree: an entry of level j+1 is the sum
 *   of its (up to 16) consecutive children of level j, added to 0 in ascending order; level 0 is the weights, the levels repeat until one
 *   entry, the total, remains (m = 1: one level above the weight).  Levels >= 1 are stored (about m / 15 doubles, 1/30 of the vector's
 *   bytes); the weights are recomputed from the amplitudes.  The plan is built with ONE read of the vector (a workgroup reads 4,096
 *   amplitudes and writes their entries of levels 1, 2, 3; each further level is formed from the one below).  A total that is zero,
 *   negative or not finite (an all-zero vector, a NaN or an infinite amplitude) is SYMGPU_E_INVALID, as are a null pointer and m < 1; the
 *   tree is freed before the refusal returns.  symgpu_sample_info: *total (or NULL) the root; info (int64 [6] or NULL): [0] m, [1] the tree
 *   depth (stored levels), [2] the plan's device bytes, [3] the launches that built it, [4] the counting form of the last draw
 *   (SYMGPU_SAMPLE_HIST | SYMGPU_SAMPLE_SORT, 0: none), [5] the launches of the last draw in csrc/sample.hip (the scan and the sort add theirs).
 *
 * Draw.  With the uniform u of a draw, r = u * total (one rounding); walk down from the root.  At a node with children c_0 .. c_15 form
 *   acc_0 = c_0, acc_k = acc_{k-1} + c_k — the partial sums of the construction, in its order — and take the first k with r < acc_k; then
 *   r <- r - acc_{k-1} (r unchanged for k = 0).  FALLBACK: if no k qualifies (rounding at the right edge, or a parent's rounded partial sum
 *   admitted slightly more than the child holds) take the last child with c_k > 0 and apply the same subtraction.  At level 0 the child
 *   index is the sample.  A sample always has w > 0.  Against the exact inverse CDF the scheme is biased by the order of 2^-53 relative
 *   per boundary (each boundary is a rounded partial sum).  symgpu_sample_draw: n_samples draws, 0 <= n_samples < 2^31; draw i uses
 *   u_dev[i] (caller's uniforms in [0, 1), double [n_samples]) when u_dev is not NULL, else draw first_draw + i of the Philox stream of
 *   `seed`.  order_dev (int64 [n_samples] or NULL) receives the sample of every draw in draw order.  idx_dev / count_dev (int64, capacity
 *   min(m, n_samples) each) receive the distinct samples, ascending, with their counts; *n_distinct their number.  Two counting forms
 *   give identical bytes: SYMGPU_SAMPLE_HIST (integer atomics into m 32-bit counters, then a compaction with the library's scan; m < 2^31)
 *   and SYMGPU_SAMPLE_SORT (the library's radix sort of the draws, keys only, then run lengths).  The rule, in one place, compares bytes
 *   moved — HIST where 28 m + 8 n_samples <= 24 P n_samples, P = the bytes of m - 1 —; SYMGPU_SAMPLE_COUNT=hist|sort (read on every call)
 *   forces a form where it is legal.  SYMGPU_E_INVALID before anything is allocated: a null plan, idx_dev, count_dev or n_distinct,
 *   n_samples outside the range, a negative first_draw, first_draw + n_samples >= 2^63.  n_samples = 0 launches nothing, *n_distinct = 0.
 *
 * Basis.  symgpu_basis_change applies, in place on psi_dev (complex128 [2^n], n_qubits 1 .. 32), H on the qubits of x_mask and H S^+ on
 *   those of y_mask (bit q of a mask = qubit q; the masks disjoint and within n qubits, else SYMGPU_E_INVALID), so that U P U^+ = +Z on
 *   every measured qubit of P (H X H = Z, H S^+ Y S H = Z); other qubits are untouched.  On the pair (a0, a1) of a measured index bit (a1:
 *   the bit set): on a Y-qubit first a1 <- (a1.im, -a1.re) (S^+, exact); then a0' = (a0 + a1) r, a1' = (a0 - a1) r per component, each
 *   sum and product rounded once, r = 0x3FE6A09E667F3BCD (0x1.6a09e667f3bcdp-1), the double nearest 1/sqrt 2.  ORDER (it changes the bits):
 *   the measured qubits in descending qubit number, which is ascending index bit.  SYMGPU_BASIS_DIRECT: one launch per measured qubit over
 *   the 2^(n-1) pairs.  SYMGPU_BASIS_TILED (the default): the measured bits go, ascending, into groups, one pass over the vector per group;
 *   the tile rule of symgpu_ansatz_apply: a group's tile bits are the 4 lowest index bits and its measured bits while the tile holds
 *   <= 2^12 amplitudes (64 KiB of LDS), filled with the lowest free bits up to min(n, 10); the butterflies run in LDS in the same order
 *   with a barrier between them.  Both forms give the same bits.  SYMGPU_BASIS_FORM=direct (read on every call) forces direct passes.
 *   *form (or NULL): the form that ran, 0 when both masks are empty.
 *
 * Estimates.  symgpu_counts_signed_sums: out_host[k] = sum_j count_j (-1)^{|z_k & b_j|} (int64, exact, independent of order) for every
 *   row k of a resident operator (Wq = 1, n_qubits 1 .. 32) over the n_distinct basis indices b_j = idx_dev[j] with counts count_dev[j];
 *   packed rows carry qubit q at bit q, basis indices at bit n-1-q: the call reverses z_k.  A row with a non-empty X-part is
 *   SYMGPU_E_INVALID (out_host untouched).  One read-back of T integers (and the X flag).
 * The device memory is checked before it is allocated (SYMGPU_E_NOMEM); scratch is freed before a call returns, also on failure. */
#define SYMGPU_SAMPLE_HIST 1
#define SYMGPU_SAMPLE_SORT 2
#define SYMGPU_BASIS_DIRECT 1
#define SYMGPU_BASIS_TILED 2
struct symgpu_sample_s;   /* a plan: opaque, owned by the caller between symgpu_sample_plan and symgpu_sample_free */
int symgpu_philox_uniform(uint64_t seed, int64_t first_draw, int64_t count, double *out_dev);
int symgpu_sample_plan(const double *amp_dev, int64_t m, struct symgpu_sample_s **plan);
int symgpu_sample_free(struct symgpu_sample_s *plan);
int symgpu_sample_info(struct symgpu_sample_s *plan, double *total /* or NULL */, int64_t *info /* [6] or NULL */);
int symgpu_sample_draw(struct symgpu_sample_s *plan, int64_t n_samples, uint64_t seed, int64_t first_draw, const double *u_dev /* or NULL */,
                       int64_t *order_dev /* [n_samples] or NULL */, int64_t *idx_dev, int64_t *count_dev, int64_t *n_distinct);
int symgpu_basis_change(double *psi_dev, int n_qubits, uint64_t x_mask, uint64_t y_mask, int *form /* or NULL */);
int symgpu_counts_signed_sums(symgpu_op_t op, int n_qubits, const int64_t *idx_dev, const int64_t *count_dev, int64_t n_distinct,
                              int64_t *out_host /* [T] */);

/* ---- f11: a polynomial of H on a dense statevector, in the Chebyshev basis (symmer_amd/evolution/time_evolution.py evolve_state:
 * exp(-i H t) psi and exp(-tau H) psi by the Chebyshev expansion; csrc/evolve.hip).  Conventions and the plan of f7.
 * symgpu_cheb_apply   out = sum_{k=0..K} c_k T_k(H~) psi,  H~ = (H - centre) / half_width,  T_0 = 1, T_1 = x, T_k = 2 x T_{k-1} - T_{k-2}.
 *   coef_host: double [K + 1][2] on the host, (re, im) of c_k.  psi_dev, out_dev: complex128 [2^n] device buffers, not the same one; psi
 *   is never written.  SYMGPU_E_INVALID before anything is allocated: a null plan, coef_host, psi_dev or out_dev, psi_dev == out_dev,
 *   K < 0, half_width not finite or <= 0, centre not finite.  The spectrum of H is the caller's business: outside
 *   [centre - half_width, centre + half_width] the T_k grow exponentially in k.
 *   Arithmetic — every operation below is one IEEE double operation rounded to nearest, nothing contracted, so that a NumPy restatement
 *   on separate real and imaginary parts gives the same bits, and two calls give the same bytes.  h(v)[b] is the row sum that
 *   symgpu_matvec_apply computes, in its order (groups in ascending x, D_g from its first term, the sum started from the first product;
 *   +0.0 in both components for a plan without groups).  A complex product c v is the plain one of f7 with the coefficient in the place
 *   of D:  (c.re v.re - c.im v.im,  c.re v.im + c.im v.re).  inv = 1.0 / half_width (one division, on the host), s_1 = inv, s_k = 2 inv.
 *     T_0 = psi;                                        out[b] = c_0 psi[b]
 *     t[b]   = h(T_{k-1})[b] - centre T_{k-1}[b]        per component: sub(h, mul(centre, v))
 *     T_1[b] = s_1 t[b]                                 per component: mul(s_1, t)
 *     T_k[b] = s_k t[b] - T_{k-2}[b]   (k >= 2)         per component: sub(mul(s_k, t), u)
 *     out[b] = out[b] + c_k T_k[b]                      the complex product, then a componentwise add
 *   Launches: one thread per row, 2^8 rows a workgroup, one launch per order k >= 1 (order 0 is folded into the first; K = 0 is one launch
 *   of its own), all on the context's stream with one synchronise at the end.  Row b's thread alone reads and writes element b of
 *   T_{k-2}, T_k and out, so T_k overwrites T_{k-2} in place except at k = 2, where T_0 is the caller's psi: two scratch vectors of
 *   2^n complex128 for any K.  No atomics, no barrier across workgroups.  Beyond the G gathered reads of T_{k-1} an order moves one read
 *   of T_{k-1}[b] and T_{k-2}[b], one write of T_k[b], one read and one write of out[b]: 16 (G + 4) bytes per row and order beyond the
 *   cached re-read.  *form (may be NULL) = SYMGPU_CHEB_DIRECT; it is the only form (a plan without terms still runs the kernels, with
 *   h = 0).  The device memory is checked before it is allocated (SYMGPU_E_NOMEM); the scratch is freed before the call returns, also
 *   on failure. */
#define SYMGPU_CHEB_DIRECT 1
int symgpu_cheb_apply(struct symgpu_matvec_s *plan, double centre, double half_width, const double *coef_host /* [K+1][2] (re, im) */, int64_t K,
                      const double *psi_dev, double *out_dev, int *form /* or NULL */);

/* ---- f6: PauliwordOp.from_matrix (base.py:239-425), the inverse of f5: the Pauli decomposition of a 2^n x 2^n matrix M, n_qubits 1 .. 31
 * (csrc/pauli_decomp.hip).  With the conventions of f5 (qubit 0 the MOST significant bit of b, x, z):
 *   c(x, z) = i^{|x & z| mod 4} 2^-n sum_b (-1)^{|b & z|} M[b, b ^ x]
 * The sum is the radix-2 butterfly on the XOR-diagonal d_x[b] = M[b, b ^ x]: stage s = 0 .. n-1 combines the two elements whose indices
 * differ in bit s, a' = a + b, b' = a - b (a: bit clear), per component in IEEE double; then one multiplication by 2^-n and i^k as a
 * component swap: every form of the transform, and any restatement with these additions, agrees bit for bit.
 * symgpu_from_matrix_dense   matrix: complex128 [2^n][2^n], C order (n_qubits <= 16).
 * symgpu_from_matrix_csr     data complex128 [nnz], indices [nnz], indptr [2^n + 1], both of index_bytes = 4 (int32) or 8 (int64); no entry
 *   may be stored twice (canonical CSR); only the diagonals x = row ^ col of stored entries are transformed, absent entries are +0.0.
 * Basis (optional): basis_x / basis_z uint64 [K], the X and Z parts of K terms as n-bit integers; K = 0 means all 4^n terms.
 *   K = 0: *out = a new resident operator (Wq = 1, marked duplicate-free) holding every coefficient whose two components are not both
 *     +-0 (NaN and inf are kept), in ascending (x, z) order, x the high part; *n_out = its term count; coeff_out is not used.
 *   K > 0: coeff_out complex128 [K] on the host = c(basis_x[k], basis_z[k]) in basis order, zeros included; out / n_out are not used.
 * *form (may be NULL) = SYMGPU_PAULI_ONE_PASS: every diagonal (2^n <= 2^13 elements = 128 KiB) was transformed in LDS in one launch, or
 * SYMGPU_PAULI_TWO_PASS: the low tile bits in LDS tiles, the bits above them across the tiles in further launches.
 * SYMGPU_PAULI_TILE_BITS=t (3 .. 13, read on every call) sets the tile size, so that a small matrix takes the two-pass form.
 * (number of diagonals) x 2^n must stay below 2^31 slots of 16 bytes (SYMGPU_E_INVALID); the device memory is checked before it is
 * allocated (SYMGPU_E_NOMEM).  Every device scratch buffer is freed before the call returns, also on failure. */
#define SYMGPU_PAULI_ONE_PASS 1
#define SYMGPU_PAULI_TWO_PASS 2
int symgpu_from_matrix_dense(const double *matrix, int n_qubits, const uint64_t *basis_x, const uint64_t *basis_z, int64_t K, symgpu_op_t *out,
                             int64_t *n_out, double *coeff_out, int *form);
int symgpu_from_matrix_csr(const double *data, const void *indices, const void *indptr, int index_bytes, int64_t nnz, int n_qubits,
                           const uint64_t *basis_x, const uint64_t *basis_z, int64_t K, symgpu_op_t *out, int64_t *n_out, double *coeff_out, int *form);

/* ---- g: measurement grouping (qubitwise_commutes_termwise base.py:985-1009, clique_cover base.py:1266-1364; csrc/clique.hip) ----------
 * Relations of two packed rows a = (xa | za), b = (xb | zb):
 *   SYMGPU_REL_C    related iff the parity of popcount(xa & zb ^ za & xb) over the row is even (the terms commute)
 *   SYMGPU_REL_AC   related iff that parity is odd
 *   SYMGPU_REL_QWC  related iff no word has (xa | za) & (xb | zb) & ((xa ^ xb) | (za ^ zb)) != 0 (they commute qubit by qubit)
 * In the degrees and in the colouring a term is never related to (and never conflicts with) itself: itself is the same INDEX, an equal
 * row at another index is a term like any other.
 * symgpu_qwc_dev   as symgpu_commutes_dev for QWC: out_dev[i * M + j] = 1 iff A[a_begin + i] qubit-wise commutes with B[j] (np.bool_ layout,
 *   N * M bytes from symgpu_dev_alloc); a term qubit-wise commutes with itself.
 * symgpu_relation_degrees_dev   deg_host[t] = the number of terms u != t related to t: an all-pairs pass with integer row sums, 8 T bytes of
 *   device scratch, no table.
 * symgpu_clique_colour_dev   first-fit colouring of the CONFLICT graph (terms that are not related) in the order given: for s = 0 .. T-1 term
 *   order_host[s] takes the lowest colour none of whose members it conflicts with, a new one if there is none.  Every colour class is a
 *   clique of the relation; this is `sorted_insertion` for order = argsort(-|c|) and networkx's greedy_color(complement, 'largest_first')
 *   for order = stable argsort of -(T - 1 - degree).  colour_host[t] (by term index) in 0 .. *n_colours - 1, colours opened in order.
 *   order_host must be a permutation of 0 .. T-1 (checked on the host before the device is touched).  T = 0: nothing is written but
 *   *n_colours = 0.  Coefficients are not read.
 *   info (may be NULL) int64 [4]: [0] the form that ran — SYMGPU_CLIQUE_PAIRS (relations C and AC): every term met every term coloured before
 *   it, T^2 / 2 pair predicates; SYMGPU_CLIQUE_UNIONS (QWC): every term met the merged Pauli string of every clique open before its block,
 *   T K predicates for K colours — [1] the blocks of the order that were resolved (ceil(T / [2])), [2] the terms a block, [3] the 32-bit words of
 *   a term's forbidden-colour bitmap (T / 32 + 2: as wide as colours can become).
 *   Device memory: 16 Wq T bytes (rows in colouring order; as much again for SYMGPU_CLIQUE_UNIONS) + 12 T + 4 (order, colours) +
 *   256 (T / 32 + 2) 4 (the bitmaps of ONE block) — O(T Wq + T), no T x T table.  Two launches a block, no read-back before the last.
 * Every device scratch buffer is freed before a call returns, also on failure. */
#define SYMGPU_REL_C 0
#define SYMGPU_REL_AC 1
#define SYMGPU_REL_QWC 2
#define SYMGPU_CLIQUE_PAIRS 1
#define SYMGPU_CLIQUE_UNIONS 2
int symgpu_qwc_dev(symgpu_op_t A, int64_t a_begin, int64_t a_end, symgpu_op_t B, uint8_t *out_dev);
int symgpu_relation_degrees_dev(symgpu_op_t op, int relation, int64_t *deg_host /* [T] */);
int symgpu_clique_colour_dev(symgpu_op_t op, int relation, const int64_t *order_host /* [T], a permutation */,
                             int32_t *colour_host /* [T], by term index */, int64_t *n_colours, int64_t *info /* [4] or NULL */);

/* ---- h: noncontextual operators (noncontextual_op.py:502-531 noncontextual_reconstruction, :533-554 get_energy, :686-704
 * energy_via_brute_force; csrc/noncon.hip) ------------------------------------------------------------------------------------------
 * symgpu_noncon_signs_dev   signs[k] for every term k of `terms`: the generators of `gens` that row k of `sel` selects (bit j % 64 of word
 *   sel[k * sel_words + j / 64] selects generator j; bits at or above the generator count are not read) are multiplied in generator order,
 *   starting from the identity, under the phase rule of symgpu_mul_allpairs.  +1 or -1 if the product is + or - the term's own Pauli
 *   string; 0 if its row differs from the term's or its phase is +-i.  sel and signs are host arrays; coefficients are not read.
 * symgpu_noncon_search   the minimum over all 2^n_free assignments m of
 *       E(m) = sum_{clique[k] = -1} coeff[k] s_k(m) - sqrt( sum_{i < n_cliques} ( sum_{clique[k] = i} coeff[k] s_k(m) )^2 ),
 *       s_k(m) = (-1)^popcount(mask[k] & m),
 *   as Walsh-Hadamard transforms blocked in LDS: O(n_free 2^n_free) work, nothing but the T terms read from memory.  Bit b of m set means
 *   that free generator number n_free-1-b (in generator order) is assigned -1; mask[k] has bit b set iff term k's reconstruction uses that
 *   generator.  coeff, mask, clique: host arrays [T]; clique[k] = -1 for a term outside the cliques, else 0 .. n_cliques-1.
 *   *best_energy, *best_mask: the minimum and its assignment; among assignments whose computed energies compare equal the LARGEST m wins
 *   (the reference's `min` over itertools.product([-1, 1], ...) keeps the first minimum and -1 sorts first) — for T = 0 every energy is 0.
 *   energies (may be NULL; ignored for n_free > 24): double [2^n_free], E(m) at index m.  Two calls with equal input return identical
 *   bytes: every sum is taken in an order that depends on the input alone (no floating-point atomics).
 *   SYMGPU_E_INVALID: n_free outside 0 .. 40 (a refusal bound, not a performance claim), n_cliques < 0, T < 0, a clique number outside
 *   -1 .. n_cliques-1, a mask bit at or above n_free, a coefficient that is not finite, coefficients whose magnitudes sum beyond 1e154 (below that no
 *   sum or square overflows: every energy is a finite number), a null best_energy or best_mask.
 *   info (may be NULL) int64 [4]: [0] L, the assignment bits a workgroup holds in LDS (three double[2^L] vectors); [1] the blocks of 2^min(n_free, L)
 *   assignments, 2^(n_free - min(n_free, L)); [2] the entries folded per block (T); [3] the workgroups launched. */
int symgpu_noncon_signs_dev(symgpu_op_t terms, symgpu_op_t gens, const uint64_t *sel /* [T][sel_words] */, int sel_words, int8_t *signs /* [T] */);
int symgpu_noncon_search(const double *coeff, const uint64_t *mask, const int32_t *clique, int64_t T, int n_free, int64_t n_cliques,
                         double *best_energy, uint64_t *best_mask, double *energies /* [2^n_free] or NULL */, int64_t *info /* [4] or NULL */);

/* ---- h2: noncontextual sweeps (utils.py:592-616 perform_noncontextual_sweep; noncontextual_op.py:126-226 the three constructors on it;
 * csrc/noncon_sweep.hip) ----------------------------------------------------------------------------------------------------------------
 * symgpu_noncon_sweep_dev   n_starts sweeps over the T terms of op.  Sweep s visits the terms order[(starts[s] + i) % T], i = 0 .. T-1, and
 *   keeps a term whenever the kept terms stay noncontextual (the first visited term is always kept).  order: a host permutation of
 *   0 .. T-1, NULL = the identity; starts: host [n_starts], each in [0, T).  Coefficients are not read.
 *   kept_bits: host [n_starts][ceil(T/64)]; bit p % 64 of word p / 64 of row s is set iff the term at POSITION p of order (not of the
 *   rolled visit) was kept by sweep s; the bits at or above T are zero.
 *   labels (may be NULL): host int32 [n_starts][T] by position: -2 rejected, -1 kept and commuting with every kept term, c >= 0 kept in
 *   the clique numbered c in order of creation (two kept terms with labels >= 0 commute iff their labels are equal).
 *   info (may be NULL) int64 [4]: [0] bytes of the commutation table, [1] workgroups launched, [2] sweeps a workgroup ran at most,
 *   ceil(n_starts / [1]), [3] the largest clique count a sweep ended with.  All zero when nothing was launched.
 *   The T x T commutation bits are computed once, on the rows permuted into order (a roll is an offset into that table); one workgroup
 *   runs one sweep, a persistent grid strides over the sweeps.  The output is integers: equal inputs give identical bytes, and a batch
 *   gives what its sweeps give one call each.  T = 0, T = 1 and n_starts = 0 return without a launch (T = 1: the term is kept, label -1).
 *   SYMGPU_E_INVALID, before anything is allocated: a null handle; T above SYMGPU_NONCON_SWEEP_MAX_T (the table takes T^2 / 8 bytes, 2 GiB
 *   at the cap, and the three masks of a sweep 3 T / 8 bytes of LDS, 48 KiB at the cap); n_starts < 0; a start outside [0, T); an order
 *   that is not a permutation; null starts or kept_bits with sweeps to run.  Scratch is freed before the call returns, also on failure. */
#define SYMGPU_NONCON_SWEEP_MAX_T 131072
int symgpu_noncon_sweep_dev(symgpu_op_t op, const int64_t *order /* [T] or NULL */, int64_t n_starts, const int64_t *starts /* [n_starts] */,
                            uint64_t *kept_bits /* [n_starts][ceil(T/64)] */, int32_t *labels /* [n_starts][T] or NULL */, int64_t *info /* [4] or NULL */);

/* ---- e: multi-GPU (one process per GPU; RCCL over xGMI) ------------------------------------------- */
#define SYMGPU_UNIQUE_ID_BYTES 128
int symgpu_comm_available(void);                                                /* librccl loadable? (no device, no collective) */
int symgpu_comm_unique_id(uint8_t id[SYMGPU_UNIQUE_ID_BYTES]);                 /* rank 0 */
int symgpu_comm_init(const uint8_t id[SYMGPU_UNIQUE_ID_BYTES], int rank, int nranks);
int symgpu_comm_destroy(void);
/* A caller whose watchdog gave up on a symgpu_comm_init that has not returned calls this: should ncclCommInitRank come back later,
 * its communicator is destroyed instead of installed (the ranks have agreed on the host-staged data plane by then). */
int symgpu_comm_abandon(void);
/* all-gather equal-sized shards of packed rows (+coefficients if both have them) into `full`
 * (capacity >= nranks * shard rows); rank r's rows land at [r*T_shard, (r+1)*T_shard). */
int symgpu_comm_allgather_op(symgpu_op_t shard, symgpu_op_t full);
int symgpu_comm_barrier(void);
/* The same all-gather for ONE process that drives n devices (symgpu_init_all): one communicator per device (ncclCommInitAll); shards[d] and
 * fulls[d] live on device d, every shard has the same capacity Ts, device d's rows land at [d * Ts, (d + 1) * Ts) of every full operator.
 * The n all-gathers are enqueued from the calling thread as one RCCL group (ncclGroupStart / ncclGroupEnd), each on its device's stream. */
int symgpu_comm_init_all(int n_devices);
int symgpu_comm_allgather_ops(const symgpu_op_t *shards, const symgpu_op_t *fulls, int n);

#ifdef __cplusplus
}
#endif
#endif /* SYMGPU_H */
