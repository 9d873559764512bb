/*
 * k16.h -- C ABI of libk16.so: the MI355X (gfx950) device shim under the Groth16 prover.
 *
 * This is the "thin extern-C shim" between the C++ prover host code and the HIP kernels.
 * Plain pointers and sizes only; every function returns an int status (K16_OK = 0), never
 * throws, and never falls back to a CPU implementation: without a usable HIP device the
 * context cannot be created and every entry point fails with K16_ERR_NO_DEVICE.
 *
 * What each entry point replaces in the reference (paths relative to
 * rust-rapidsnark/rapidsnark/src/ of aptos-labs/keyless-zk-proofs):
 *
 *   k16_msm*            Curve<F>::multiMulByScalar -> ParallelMultiexp::multiexp
 *                       (curve.hpp:209-215, multiexp.cpp:183-245), G1 and G2
 *   k16_ntt             FFT<RawFr>::fft / ::ifft (fft.cpp:192-246)
 *   k16_prover_*        Groth16::makeProver / Prover::prove (groth16.cpp:18-39, 41-360) and the
 *                       FullProverImpl ctor / prove around them (fullprover.cpp:136-250)
 *   k16_field_op_vec,
 *   k16_point_op_vec    RawFq/RawFr raw ops and Curve<F>::add/dbl (fq_raw_generic.cpp:12-233,
 *                       curve.cpp:91-458) exposed as batch kernels for parity tests
 *
 * Data formats are the reference's own: field elements are 32 bytes,
 * little-endian; Fq/Fr values in Montgomery form (R = 2^256) unless stated; G1 affine = x|y
 * (64 B), G2 affine = x.a|x.b|y.a|y.b (128 B), affine infinity = all zero; XYZZ = x|y|zz|zzz
 * (128 B / 256 B), infinity <=> zz == 0; MSM scalars = 32 B standard (non-Montgomery) form.
 */
#ifndef K16_H
#define K16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    K16_OK             = 0,
    K16_ERR_NO_DEVICE  = -1, /* no HIP device / runtime failure at context creation */
    K16_ERR_HIP        = -2, /* a HIP call or kernel failed; see k16_last_error */
    K16_ERR_ARG        = -3,
    K16_ERR_IO         = -4, /* file open / mmap failure         (-> ZKEY_FILE_LOAD_ERROR) */
    K16_ERR_FORMAT     = -5, /* malformed zkey / wtns            (-> INVALID_INPUT) */
    K16_ERR_CURVE      = -6, /* prime is not BN254 r             (-> UNSUPPORTED_ZKEY_CURVE /
                                                                     WITNESS_GENERATION_INVALID_CURVE) */
    K16_ERR_BUFFER     = -7,
    K16_ERR_NOMEM      = -8  /* a host allocation failed inside the library (-> PROVER_NOT_READY) */
};

enum { K16_G1 = 0, K16_G2 = 1 };
enum { K16_FQ = 0, K16_FR = 1 };
/* Selectors for k16_field_op_vec / k16_point_op_vec only: the SAME inputs and outputs (the reference's canonical
 * Montgomery form), but the operation runs on the representation the hot kernels use -- the unsaturated radix-2^29
 * field of bn254_fq9.h (Fq9 for G1, Fr9 for the NTT chain, Fq2n = Fq2 over Fq9 for G2; elements of K16_FQ2N are 64 B:
 * a | b) and the Eng9 / Eng2n point formulas of the MSM kernels.  Values are converted at the edges, exactly.
 * For these selectors bits 8-11 / 12-15 of `op` add that many multiples of the modulus to operand a / b after the
 * conversion (operands at the documented bounds: X < 8p, Y < 4p, ZZ < 2p ...); the result must not change. */
enum { K16_FQ9 = 2, K16_FR9 = 3, K16_FQ2N = 4,
       K16_FQ2H = 5 /* Fq2 on a LANE PAIR (bn254_fq2pair.h: real part on the even lane, imaginary part on the odd one) -- what
                       the G2 accumulation, fold and weighted-sum kernels execute since round 5; elements as for K16_FQ2N */ };
enum { K16_G1_ENG9 = 2, K16_G2_ENG2N = 3, K16_G2_PAIR = 4 /* the XYZZ formulas instantiated on K16_FQ2H */ };
#define K16_OP_BOUND_A(k) ((k) << 8)
#define K16_OP_BOUND_B(k) ((k) << 12)
enum { K16_OP_ADD = 0, K16_OP_SUB, K16_OP_NEG, K16_OP_MUL, K16_OP_SQR, K16_OP_TOMONT, K16_OP_FROMMONT,
       /* K16_FQ9 / K16_FR9 only: the NTT butterflies' lazy-limb forms (bn254_fq9.h fadd9_lazy, fsub9_lazy4_t) followed by the
        * multiplication that consumes them: (a + b) * b and (a - b) * b; K16_OP_BOUND_A counts in steps of 2 moduli here
        * (up to a + 30 p), b stays below 2 p as in the kernels */
       K16_OP_LAZY_ADDMUL, K16_OP_LAZY_SUBMUL };
enum { K16_PT_ADD = 0, K16_PT_MADD, K16_PT_DBL,
       /* K16_G1_ENG9 only: the bucket accumulation's own mixed addition (bn254_fq9.h acc9_madd: the accumulator keeps
        * W = +-Y with a flag, the entry's sign goes into the addition, lazy subtractions).  p1 XYZZ, p2 affine as for
        * K16_PT_MADD; K16_OP_BOUND_B bit 0: the entry is negative (result p1 - p2), bit 1: the accumulator arrives with
        * W = -Y.  Result: the XYZZ representation of curve.cpp:185-250 for p1 + (+-p2). */
       K16_PT_MADD_ACC };

typedef struct k16_ctx    k16_ctx;
typedef struct k16_prover k16_prover;

/* ---- process set-up (optional) ----
 * ROCm multiplexes a process's HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4); one prover uses four
 * streams, so a pool of provers on one GPU, or a prover beside RCCL, wants more.  This sets the
 * variable to n unless the environment already has it.  Call it from the host program's start-up, BEFORE the process's
 * first HIP call and before it starts threads (the library itself never touches the environment). */
int         k16_runtime_hw_queues(int n);
/* number of HIP devices this process can use (0 without a device or runtime; never an error code) */
int         k16_device_count(void);
/* Host worker threads of the library: ONE pool per process, shared by all contexts and provers (the reference has one TBB
 * arena per process, multiexp.cpp:46) -- K16_HOST_THREADS, default 3/4 of the CPUs the process may use, at most 12, counting
 * the calling thread.  Returns the number of workers started so far (0 before the first prover is created). */
int         k16_host_threads(void);

/* ---- context: one per GPU (one process per GPU in multi-GPU runs) ----
 * THREADING: a context (and every prover / key / classes object created from it) is for ONE caller thread at a time.  Two
 * exceptions the library itself relies on: one thread may k16_msm_enqueue* while another k16_msm_finish*es (bench.py), and
 * k16_verify_batch may be called from several threads -- its latency path (n <= 64) shares the context's staging area and is
 * serialised inside the call.  Callers that want proofs in parallel use one context per prover (FullProver's K16_DEVICES
 * pool does); all contexts of a process share one host-thread pool (k16_host_threads). */
int         k16_ctx_create(int device, k16_ctx** out);
/* The same, behind `stream_offset` (0..7) placeholder streams that the context creates first and keeps until it is destroyed.
 * ROCm hands hardware queues to streams in creation order and the queues share four dispatch pipes, so the offset decides WHICH
 * streams of two contexts that work on one GPU take turns on a pipe: with the second prover of a device one stream behind the
 * first (what FullProver does for K16_DEVICES=0,0) two provers reach 198 instead of 189 proofs/s through the facade (8 of 8
 * alternating runs, profiles/r06/ab_facade_pool_stream_offset.log); a context that works ALONE wants offset 0.
 * Results are identical for every offset. */
int         k16_ctx_create_ex(int device, int stream_offset, k16_ctx** out);
void        k16_ctx_destroy(k16_ctx* ctx);
const char* k16_last_error(const k16_ctx* ctx);
/* Tuning.  K16_OPT_PIPELINED_MSM (value 0/1, default 0): the caller keeps several MSMs in flight on different lanes
 * (k16_msm_set_lane) and cares about MSMs per second rather than the latency of one: the weighted bucket sum uses 16
 * instead of 8 slots per lane (12 % less work, chains twice as long) and consecutive bucket accumulations of different
 * lanes are fenced one behind the other (they never overlap anyway; the per-kernel HIP-event statistics then time
 * execution only).  Results are identical either way.
 * K16_OPT_GRAPHS (0/1, default 0): the ~50 launches of an MSM's sort and of its fold + reduction are captured into HIP
 * graphs (per lane, shape and staging slot) after their second use and replayed with one call each -- for hosts whose
 * kernel launches are slow.  The per-stage statistics then cover the bucket accumulation only.
 * K16_OPT_SHARED_GPU (0/1, default 0): other contexts prove on the same GPU at the same time (FullProver sets it for the
 * entries of K16_DEVICES that name a device more than once): kernels leave room for the other provers' (the NTT passes
 * keep three workgroups per CU instead of four) -- more proofs per second, up to 0.3 ms more for a proof alone.  Results
 * are identical either way.
 * K16_OPT_YIELDING_WAITS (0/1, default 0; round 6): the host waits of k16_msm_finish* and of the prove calls poll the device
 * (hipEventQuery) with short sleeps instead of spinning inside the runtime: a caller that waits for its proof costs next to no CPU
 * (a proof otherwise keeps one core busy for its whole 5 ms) at up to ~50 us per wait -- for hosts that run many provers (FullProver
 * sets it for every pool with more than one prover).  Results are identical either way. */
enum { K16_OPT_PIPELINED_MSM = 1, K16_OPT_GRAPHS = 2, K16_OPT_SHARED_GPU = 3, K16_OPT_YIELDING_WAITS = 4 };
int         k16_ctx_set_option(k16_ctx* ctx, int option, int value);
int         k16_sync(k16_ctx* ctx);
/* the HIP stream every kernel of this context is launched on (hipStream_t as void*) */
void*       k16_stream(k16_ctx* ctx);

/* ---- device memory (so callers need no HIP of their own) ---- */
int k16_dev_alloc(k16_ctx* ctx, size_t bytes, void** dptr);
int k16_dev_free(k16_ctx* ctx, void* dptr);
int k16_h2d(k16_ctx* ctx, void* dptr, const void* hptr, size_t bytes);
int k16_d2h(k16_ctx* ctx, void* hptr, const void* dptr, size_t bytes);
/* Page-lock a host buffer the caller owns (hipHostRegister) -- e.g. the scalar array Curve::multiMulByScalar (curve.hpp:209-215)
 * receives by pointer on every call -- so that k16_h2d / k16_msm_host / k16_msm_sharded_run copy from
 * it by DMA instead of through the runtime's staging buffer (a 2^24-row scalar array: 24 instead of 27 ms per upload, and
 * the copy no longer occupies a host core).  The buffer must stay mapped until k16_host_unregister.  Not needed for
 * correctness anywhere. */
int k16_host_register(k16_ctx* ctx, void* hptr, size_t bytes);
int k16_host_unregister(k16_ctx* ctx, void* hptr);

/* ---- timing on the context's stream with HIP events ---- */
int k16_timer_start(k16_ctx* ctx);
int k16_timer_stop(k16_ctx* ctx, float* elapsed_ms); /* synchronises */
/* per-kernel statistics: when enabled, the named hot kernels are bracketed by HIP events.
 * name: "msm_accumulate", "msm_sort", "msm_reduce", "ntt".  total_ms / launches since reset. */
int k16_kernel_stats_enable(k16_ctx* ctx, int on); /* 0 off, 1 all stages, 2 only "msm_accumulate" (+ the host_* timers) */
int k16_kernel_stats_reset(k16_ctx* ctx);
int k16_kernel_stats_get(k16_ctx* ctx, const char* name, uint64_t* launches, double* total_ms);

/* ---- multi-scalar multiplication  (multiexp.cpp:183-245) ----
 * d_bases: n affine points on the device; d_scalars: n x 32 B on the device.
 * Result: XYZZ point (host memory, 128 B for G1 / 256 B for G2), and/or its affine form.
 * Any 256-bit scalar is accepted; (0,0) bases contribute nothing; n == 0 gives infinity.
 * k16_msm / k16_msm_host take any n that fits the device: above 2^24 points they run contiguous chunks of 2^24 on two
 * lanes and fold the chunk results (the in-time version of the multi-GPU sharding).  k16_msm_enqueue* is one device
 * pass and refuses n >= 2^32 / 80. */
int k16_msm(k16_ctx* ctx, int group, const void* d_bases, const void* d_scalars, uint64_t n, void* h_out_xyzz,
            void* h_out_affine);
/* same with host buffers (uploads, runs, downloads) */
int k16_msm_host(k16_ctx* ctx, int group, const void* h_bases, const void* h_scalars, uint64_t n, void* h_out_xyzz,
                 void* h_out_affine);
/* Enqueue only (no host synchronisation): leaves the per-window sums in the context's workspace.
 * k16_msm_finish() synchronises, downloads them and does the final Horner combine on the host. */
int k16_msm_enqueue(k16_ctx* ctx, int group, const void* d_bases, const void* d_scalars, uint64_t n);
int k16_msm_finish(k16_ctx* ctx, void* h_out_xyzz, void* h_out_affine);
/* k16_msm_finish for a caller that knows which group the oldest MSM in flight belongs to: fails with K16_ERR_ARG and
 * consumes nothing when it is the other one (a G2 result is 256 bytes; it must never land in a 128-byte G1 buffer). */
int k16_msm_finish_group(k16_ctx* ctx, int group, void* h_out_xyzz, void* h_out_affine);
/* number of MSMs enqueued and not yet finished (0 .. 8), negative on error */
int k16_msm_pending(k16_ctx* ctx);
/* error recovery: waits for and drops every MSM in flight, clears sort-reuse / lane state (the prover does this on
 * every failed prove so that a later prove never pops a stale result) */
int k16_msm_abort_all(k16_ctx* ctx);
/* Static point tables (the zkey's sections 5-9) can be prepared once: d_out (same size as d_bases)
 * receives the rows in the layout the accumulate kernel gathers from (G1: x*2^261, y*2^261 mod p packed
 * in 2 x 32 B -- the Montgomery form of the kernels' radix-2^29 field; G2: the same per Fq2 component).  A prepared
 * table is passed to k16_msm_enqueue_prepared instead of the zkey-format one. */
int k16_msm_bases_prepare(k16_ctx* ctx, int group, const void* d_bases, uint64_t n, void* d_out);
int k16_msm_enqueue_prepared(k16_ctx* ctx, int group, const void* d_prepared, const void* d_scalars, uint64_t n);
/* Fixed-base MSM for a static G1 table: W = ceil(257/c) precomputed window tables (row w*n + i =
 * 2^(c*w) * P_i) let all digit positions share ONE bucket set, so c can be 20 instead of 16 and a 254-bit scalar costs 13
 * bucket additions instead of 16.  k16_msm_fixed_base_info gives the window size chosen for n (0: not available -- n below
 * 2^13 or n*W >= 2^25 -- use the ordinary MSM) and the table size in 64-byte rows; k16_msm_fixed_base_prepare fills the
 * caller's d_table from a zkey-format table (once; ~W*n*(c + 400) field multiplications); k16_msm_enqueue_fixed_base is
 * k16_msm_enqueue_prepared for such a table (results through k16_msm_finish, same values). */
int k16_msm_fixed_base_info(uint64_t n, unsigned* c, uint64_t* table_rows);
int k16_msm_fixed_base_prepare(k16_ctx* ctx, int group, const void* d_bases, uint64_t n, void* d_table);
int k16_msm_enqueue_fixed_base(k16_ctx* ctx, int group, const void* d_table, const void* d_scalars, uint64_t n);
/* Scalar-class MSM: for scalar vectors that are mostly small -- the wire values of a circom witness: zeros, ones, bytes, a
 * few field elements.  Replaces what the zero-digit skip of the reference's bucket loop (multiexp.cpp:59-65, `if
 * (chunkValue)`) does for its four witness MSMs (groth16.cpp:88-112).  One classification of the scalars serves every
 * table indexed by the same wires:
 *     sum_i s_i P_i  =  sum_{b<8} 2^b (sum of the P_i with s_i < 256 and bit b of s_i set)  +  MSM over the s_i >= 256
 * k16_msm_zero_row_mask:     bit i of d_mask ((n + 63) / 64 x 8 bytes) = row i of the table is (0,0); such rows are left out
 *                            of that table's lists (they add nothing: curve.cpp:185-250).  Works on zkey-format and prepared
 *                            tables alike ((0,0) stays (0,0)).
 * k16_scalar_classes_create: workspace for up to max_n scalars and max_sets (1..4) tables with different zero rows.
 * k16_scalar_classes_build:  classifies d_scalars[0..n) on the current lane's stream; d_zero_masks[s] (may be NULL) is the
 *                            mask of set s.  n_wide_bound < 0: waits and reads the number of scalars >= 256 back; >= 0: the
 *                            caller's upper bound on it (nothing waits; a larger actual count makes k16_msm_finish of every
 *                            MSM enqueued from these classes fail with K16_ERR_ARG instead of returning a wrong sum).
 * k16_msm_enqueue_classified: the MSM of one PREPARED table (k16_msm_bases_prepare) with the classified scalars, on the
 *                            current lane; result through k16_msm_finish*, same value as k16_msm_enqueue_prepared with the
 *                            original scalars.  The classes must not be rebuilt while such an MSM is in flight.
 * k16_scalar_classes_counts: list lengths of the last build, out[s * 8 + b], then the wide count (tests). */
typedef struct k16_scalar_classes k16_scalar_classes;
int  k16_msm_zero_row_mask(k16_ctx* ctx, int group, const void* d_rows, uint64_t n, void* d_mask);
int  k16_scalar_classes_create(k16_ctx* ctx, uint64_t max_n, int max_sets, k16_scalar_classes** out);
void k16_scalar_classes_destroy(k16_scalar_classes* cls);
int  k16_scalar_classes_build(k16_ctx* ctx, k16_scalar_classes* cls, const void* d_scalars, uint64_t n,
                              const void* const* d_zero_masks, int n_sets, int64_t n_wide_bound);
int  k16_scalar_classes_counts(k16_ctx* ctx, const k16_scalar_classes* cls, uint32_t* out);
int  k16_msm_enqueue_classified(k16_ctx* ctx, int group, const void* d_prepared, const k16_scalar_classes* cls, int set);
/* The next k16_msm_enqueue / _prepared leaves the points whose bit is set in d_mask (k16_msm_zero_row_mask of its table, or
 * the AND of the masks of several tables that will share the sort) out of its bucket sort: (0,0) rows add nothing, but as
 * sorted entries they cost a lane of every addition they sit beside.  Covers one enqueue; n <= 2^24. */
int  k16_msm_set_zero_row_mask(k16_ctx* ctx, const void* d_mask);
/* The next k16_msm_enqueue_prepared on the current lane reads the bucket sort that `lane` has made of the SAME scalar
 * array (same device pointer, n and window size; groth16.cpp:88-112: four MSMs over one witness) instead of sorting.
 *   derive = 0  that lane's lists as they are (the zero-row mask named for this enqueue must be the one they were made with);
 *   derive = 1  lists of the current lane's own, built from that lane's partition without the rows of this enqueue's
 *               zero-row mask (a superset of the owner's): for a table with many (0,0) rows of its own.  Other lanes may
 *               share the derived lists with derive = 0.  K16_ERR_ARG when that lane holds no matching sort. */
int  k16_msm_sort_from_lane(k16_ctx* ctx, int lane, int derive);
/* A context has K16_MSM_LANES independent MSM lanes (HIP stream + workspace).  The next k16_msm_enqueue* uses the
 * selected lane; MSMs on different lanes may overlap on the GPU (their inputs must already be complete: uploads
 * through k16_h2d are).  k16_msm_finish still returns results in enqueue order.  Default lane 0. */
#define K16_MSM_LANES 4
int k16_msm_set_lane(k16_ctx* ctx, int lane);
/* override the window size chosen for the next MSMs (0 = automatic) */
int k16_msm_set_window_bits(k16_ctx* ctx, unsigned c);

/* ---- ONE MSM sharded over several GPUs (BASELINE config 5: "MSMs above ~2^24 points shard the scalar / point
 * array across the GPUs of a node") -- the multi-device form of Curve::multiMulByScalar -> ParallelMultiexp::multiexp
 * (curve.hpp:209-215, multiexp.cpp:183-245).  Shard r owns the contiguous rows [lo_r, hi_r) (the first n % shards shards
 * get one more row) of the point table and of the scalars; every shard runs the whole device pipeline on its rows; the only
 * thing that leaves a device is the shard's partial result, ONE XYZZ point (128 / 256 B), and the results are folded with
 * EC additions.
 *
 * (1) One process, several devices: one context per entry of `devices` (entries may repeat: two shards on one GPU is how
 * one-GPU boxes test it).  The point table is placed once (static tables: k16_msm_sharded_set_bases* converts each slice to
 * the kernels' row layout on its device); every run uploads / reads the scalars per shard on one host thread per shard and
 * folds the partials on the host -- they arrive there anyway for the Horner combine, so no collective is needed.
 * k16_msm_sharded_ctx gives the shard's context, e.g. to fill its slice with k16_synth_points. */
typedef struct k16_msm_shards k16_msm_shards;
int         k16_msm_sharded_create(const int* devices, int n_devices, int group, uint64_t n, k16_msm_shards** out);
void        k16_msm_sharded_destroy(k16_msm_shards* s);
int         k16_msm_sharded_count(const k16_msm_shards* s);
int         k16_msm_sharded_range(const k16_msm_shards* s, int shard, uint64_t* lo, uint64_t* hi);
k16_ctx*    k16_msm_sharded_ctx(k16_msm_shards* s, int shard);
const char* k16_msm_sharded_last_error(const k16_msm_shards* s);
/* h_bases: all n rows on the host, the reference's format (affine, Montgomery, LE) */
int         k16_msm_sharded_set_bases(k16_msm_shards* s, const void* h_bases);
/* ... or shard `shard`'s rows [lo, hi) already on that shard's device, same format */
int         k16_msm_sharded_set_bases_device(k16_msm_shards* s, int shard, const void* d_slice);
/* h_scalars: n x 32 B on the host (any 256-bit values).  Result as for k16_msm. */
int         k16_msm_sharded_run(k16_msm_shards* s, const void* h_scalars, void* h_out_xyzz, void* h_out_affine);
/* d_scalars[r]: shard r's (hi_r - lo_r) x 32 B already on shard r's device */
int         k16_msm_sharded_run_device(k16_msm_shards* s, const void* const* d_scalars, void* h_out_xyzz, void* h_out_affine);
/* Rows per device pass inside a shard (same result for any value): scalars from host memory are uploaded and enqueued in
 * pieces of host_rows (default 2^22 = 128 MB: piece i + 1 crosses PCIe while piece i is sorted and accumulated, two MSMs and
 * one upload in flight), resident scalars in passes of device_rows (default and maximum 2^24).  0 keeps / restores the
 * default; K16_ERR_ARG below 64 or above 2^24. */
int         k16_msm_sharded_set_piece_rows(k16_msm_shards* s, uint64_t host_rows, uint64_t device_rows);
/* wall time of the last run: all shards (upload + device work + per-shard combine, in parallel), the fold, the total */
int         k16_msm_sharded_last_ms(const k16_msm_shards* s, double* shards_ms, double* fold_ms, double* total_ms);
/* (2) One PROCESS per GPU (a launcher starts the ranks; each rank has its own context and its shard): the ranks exchange
 * their partial results with ONE ncclAllGather over xGMI and every rank folds them in rank order (RCCL has no elliptic-curve
 * reduction operator).  RCCL is dlopen'ed at the first call -- libk16.so does not link it; K16_ERR_NO_DEVICE (and
 * k16_rank_comm_load_error) when it cannot be loaded.  Rank 0 makes the 128-byte id and hands it to all ranks by whatever
 * the launcher offers (a file, MPI, a TCP store); k16_rank_comm_create is collective (ncclCommInitRank).
 * K16_RCCL_LIB (environment, read once per process at the first k16_rank_comm_* call) names the RCCL library file outright,
 * for installations outside the loader's search path.  A gather is waited for at most K16_RANK_COMM_TIMEOUT_MS (read by
 * k16_rank_comm_create; default 60 000): when a rank does not arrive in time the communicator is aborted, the call and every
 * later one on it return K16_ERR_HIP -- a dead rank never hangs the others. */
typedef struct k16_rank_comm k16_rank_comm;
int         k16_rank_comm_unique_id(void* out128);
const char* k16_rank_comm_load_error(void);
int         k16_rank_comm_create(k16_ctx* ctx, int rank, int world, const void* unique_id128, k16_rank_comm** out);
void        k16_rank_comm_destroy(k16_rank_comm* c);
int         k16_rank_comm_allgather_fold(k16_rank_comm* c, int group, const void* h_partial_xyzz, void* h_out_xyzz,
                                         void* h_out_affine);
/* The same exchange split in two, for a caller that keeps the GPU busy with the next MSM meanwhile: _start enqueues the
 * upload of this rank's partial, the ncclAllGather and the download on the communicator's stream and returns at once (up to
 * 4 exchanges in flight, K16_ERR_ARG beyond); _finish completes the OLDEST one (bounded wait) and folds it.  Every rank must
 * start its exchanges in the same order. */
int         k16_rank_comm_allgather_start(k16_rank_comm* c, int group, const void* h_partial_xyzz);
int         k16_rank_comm_allgather_finish(k16_rank_comm* c, void* h_out_xyzz, void* h_out_affine);

/* combine partial MSM results from several shards/GPUs: out = sum_i parts[i] (XYZZ, host) */
int k16_points_sum(int group, const void* h_parts_xyzz, uint64_t count, void* h_out_xyzz, void* h_out_affine);

/* ---- NTT over Fr (fft.cpp:192-246), in place on the device, Montgomery form ----
 * max_domain selects the root table (the reference builds it for 2*domainSize, groth16.hpp:96);
 * n must be a power of two <= max_domain. inverse != 0 -> FFT::ifft. */
int k16_ntt(k16_ctx* ctx, void* d_a, uint64_t n, uint64_t max_domain, int inverse);
int k16_ntt_host(k16_ctx* ctx, void* h_a, uint64_t n, uint64_t max_domain, int inverse);

/* ---- synthetic inputs: d_out[i] = (start + i + 1) * G, affine Montgomery (the point family of the
 * reference's own MSM test, alt_bn128_test.cpp:183-190); used by bench.py and the full-size tests ---- */
int k16_synth_points(k16_ctx* ctx, int group, uint64_t start, uint64_t n, void* d_out_affine);
/* d_out[i] = scalar_i * G for n arbitrary 256-bit scalars (device, 32 B little-endian standard form): lets a test build a
 * Groth16 key from a known trapdoor, i.e. a synthetic key of any size whose proofs verify (tests/valid_key_builder.py) */
int k16_synth_points_scalars(k16_ctx* ctx, int group, const void* d_scalars, uint64_t n, void* d_out_affine);

/* ---- batch primitives, for parity tests of the device arithmetic ---- */
int k16_field_op_vec(k16_ctx* ctx, int field, int op, const void* h_a, const void* h_b, void* h_r, uint64_t n);
int k16_point_op_vec(k16_ctx* ctx, int group, int op, const void* h_p1, const void* h_p2, void* h_r, uint64_t n);
/* A TEST PRIMITIVE, not part of the service's interface: runs a caller's program through the wave-cooperative verifier's
 * interpreter -- the kernel k16_verify_batch_folded launches for its final exponentiation, unchanged -- one block per set
 * of 12 inputs.  Program format: csrc/verify_script.h (CoopProgram: a class per step, 64 instruction words per step, term
 * words of the linear steps); slots [0, n_const) are constants, given as n_const x 9 raw radix-2^29 limbs in the R' = 2^261
 * domain (slot 0 = 0, slot 1 = R' mod p; any representative below 5p elsewhere), slots [n_const, n_const + 12) the inputs
 * (h_inputs: n x 12 x 32 B canonical Montgomery Fq), and h_out receives the 12 slots out_slot names, canonical (n x 12 x
 * 32 B).  Every argument is validated on the host before anything is launched: K16_ERR_ARG names the rule that failed
 * (k16_last_error).  Not for concurrent use with k16_vk_create or a folded verification on another thread (it adjusts the
 * kernel's dynamic-LDS attribute, which the process shares).  tests/coop_asm.py assembles such programs; tests/test_gpu_coop_exec.py uses them. */
int k16_coop_exec(k16_ctx* ctx, const uint8_t* step_class, uint64_t n_steps, const uint64_t* words /* 64 per step */,
                  const uint32_t* terms, uint64_t n_terms, uint32_t n_const, uint32_t n_slots, const uint32_t* out_slot /* [12] */,
                  const uint32_t* const9, const void* h_inputs, uint64_t n, void* h_out);

/* ---- Groth16 prover (groth16.cpp:41-360 behind fullprover.cpp:136-250) ----
 * k16_prover_create parses the zkey (iden3 binfile, sections 1,2,4-9), checks r, and uploads
 * coefficients and point tables to HBM once.  k16_prover_prove_* run the whole proof on the GPU
 * and write the compact snarkjs JSON (same bytes as Proof::toJson().dump()).
 * r_std / s_std: blinding scalars, 32 B standard form, < r.  NULL => drawn from the OS CSPRNG
 * exactly as groth16.cpp:296-316 does (254-bit candidates, rejection). */
int  k16_prover_create(k16_ctx* ctx, const char* zkey_path, k16_prover** out);
int  k16_prover_create_mem(k16_ctx* ctx, const void* zkey_bytes, size_t zkey_size, k16_prover** out);
/* A further prover of the SAME key on the SAME device as `other` (throughput mode: several provers sharing one GPU, what
 * FullProver builds for K16_DEVICES=0,0; replaces the per-instance zkey mapping + section walk of fullprover.cpp:136-181): it shares other's read-only device data -- point tables, H window tables,
 * coefficients, masks, 2.7 GB at the Keyless shape -- by reference count instead of parsing, uploading and preparing the key
 * again (0.1 s instead of 1.1 s), and owns only what a proof writes.  ctx must be a context of its own on that device.  The
 * shared part is freed with the last prover that uses it; `other` may be destroyed first.  Same proofs as a prover made by
 * k16_prover_create. */
int  k16_prover_create_shared(k16_ctx* ctx, const k16_prover* other, k16_prover** out);
void k16_prover_destroy(k16_prover* p);
int  k16_prover_info(const k16_prover* p, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain_size,
                     uint64_t* n_coefs);
int  k16_prover_prove_file(k16_prover* p, const char* wtns_path, const uint8_t* r_std, const uint8_t* s_std,
                           char* out_json, size_t cap, float* device_ms);
/* the same, also reporting the host wall time of the proof proper (witness file already opened, mapped and checked):
 * the interval the reference's `prover_time` metric covers (fullprover.cpp:226-244) */
int  k16_prover_prove_file_timed(k16_prover* p, const char* wtns_path, const uint8_t* r_std, const uint8_t* s_std,
                                 char* out_json, size_t cap, float* device_ms, float* prove_wall_ms);
/* witness already in memory: n_vars x 32 B standard form (the payload of wtns section 2) */
int  k16_prover_prove_mem(k16_prover* p, const void* h_wtns, uint64_t n_vars, const uint8_t* r_std,
                          const uint8_t* s_std, char* out_json, size_t cap, float* device_ms);
/* Compact witness hand-off (round 5; SURVEY 8(f).1, the step after k16_prover_prove_mem; replaces the file hand-off of
 * fullprover.cpp:212-224 for a caller that owns its witness calculator).  k16_prover_prove_mem spends its first 0.24 ms scanning
 * the n_vars x 32-byte witness into the form that crosses PCIe: one byte per wire -- the value when it is below 256, 0
 * otherwise -- plus the list of the wires that hold larger values (wire number, 32-byte standard-form value; any order, every
 * such wire exactly once).  A witness calculator produces that form for free while it computes the wires:
 *   k16_prover_compact_buffers   the prover's pinned, device-mapped upload buffers (valid for the prover's lifetime; written
 *                                by the caller before every k16_prover_prove_compact): narrow[n_vars], wide_idx[*wide_cap],
 *                                wide_val[*wide_cap][32].  K16_ERR_ARG for a prover without them (circuits below 2^16 wires).
 *   k16_prover_prove_compact     proves the witness the buffers hold, n_wide entries of the list being valid: the proof's
 *                                first kernel starts at once.  Same result, outputs and errors as k16_prover_prove_mem for
 *                                the same witness; K16_ERR_ARG when n_wide exceeds the list (such a witness goes through
 *                                k16_prover_prove_mem), K16_ERR_FORMAT for a wire number out of range, a listed wire whose
 *                                narrow byte is not 0, or a wire listed twice (checked on the device by the kernel that reads
 *                                the list: the entry is skipped, the call fails when its device work has been joined).
 * One proof at a time per prover, as for every prove call; k16_prover_prove_mem / _prove_file overwrite the same buffers. */
int  k16_prover_compact_buffers(k16_prover* p, uint8_t** narrow, uint32_t** wide_idx, uint8_t** wide_val, uint64_t* wide_cap);
int  k16_prover_prove_compact(k16_prover* p, uint64_t n_wide, const uint8_t* r_std, const uint8_t* s_std, char* out_json,
                              size_t cap, float* device_ms);
/* The drop-in FullProver (include/k16_fullprover.hpp) with the witness in memory: `fullprover` points to a FullProver object
 * (the one the Rust crate holds; its pool of provers -- K16_DEVICES -- serves concurrent callers), wtns_values is the payload
 * of the .wtns file's section 2.  FullProver::prove(path) maps and parses a 43 MB file inside every call; a service that
 * keeps several GPUs busy binds this instead.  Returns the JSON's length, or K16_ERR_NO_DEVICE (the reference's
 * PROVER_NOT_READY: not constructed, or every device retired), K16_ERR_HIP (device fault: the slot was rebuilt, retry),
 * K16_ERR_FORMAT / K16_ERR_ARG / K16_ERR_BUFFER / K16_ERR_NOMEM.  prover_time_ms: wall time of the call (may be NULL). */
int  k16_fullprover_prove_mem(const void* fullprover, const void* wtns_values, uint64_t n_values, char* out_json, size_t cap,
                              int* prover_time_ms);
/* The compact hand-off (k16_prover_compact_buffers / k16_prover_prove_compact above) THROUGH THE POOL: the buffers belong to
 * one prover, so the caller leases a slot first, writes the witness into that slot's buffers, and proves on it:
 *   k16_fullprover_compact_lease     waits for a free prover like prove() does and hands out its upload buffers (same meaning
 *                                    as k16_prover_compact_buffers) and the circuit's wire count; *lease names the slot.
 *                                    K16_ERR_NO_DEVICE: not ready / every device retired; K16_ERR_ARG: the key's provers upload
 *                                    plainly (below 2^16 wires) -- nothing is leased then.
 *   k16_fullprover_prove_compact     proves the witness the leased buffers hold and gives the slot back WHATEVER the outcome
 *                                    (results and error classes as k16_fullprover_prove_mem; a device fault rebuilds the slot).
 *   k16_fullprover_compact_cancel    gives the slot back without proving (the witness calculator failed).
 * A lease is for one proof and one thread; a service bounds how long it holds one (the slot serves nobody else meanwhile).
 * Replaces the temp-file hand-off of fullprover.cpp:204-250 / prover_handler.rs:511-527 for a pooled multi-GPU service. */
int  k16_fullprover_compact_lease(const void* fullprover, void** lease, uint8_t** narrow, uint32_t** wide_idx,
                                  uint8_t** wide_val, uint64_t* wide_cap, uint32_t* n_vars);
int  k16_fullprover_prove_compact(const void* fullprover, void* lease, uint64_t n_wide, char* out_json, size_t cap,
                                  int* prover_time_ms);
int  k16_fullprover_compact_cancel(const void* fullprover, void* lease);
/* debugging / parity: H scalars of the last proof (domain_size x 32 B, standard form) */
int  k16_prover_last_h(k16_prover* p, void* h_out);
/* status of the discarded warm-up proof k16_prover_create runs (K16_OK, or the error it ended with: a prover whose device
 * cannot prove reports it here instead of on the first real request) */
int  k16_prover_warmup_status(const k16_prover* p);

/* ---- batched Groth16 verification ----
 * Replaces the CPU check the service runs on every proof before it is released
 * (prover-service/src/request_handler/prover_handler.rs:329-336: Groth16Proof::verify_proof(public_inputs_hash, &pvk), i.e.
 * ark-groth16 0.4.0 prepare_inputs + verify_proof_with_prepared_inputs over ark-ec 0.4.2 / ark-bn254 0.4.0 -- third-party
 * crates, Cargo.lock:501-639; types.rs:141-196 prepared_vk builds the key from the decimal strings of the vkey file):
 *     e(A, B) * e(vk_x, -gamma) * e(C, -delta) == e(alpha, beta),     vk_x = IC[0] + sum_i x_i * IC[i + 1]
 * Points are affine, Montgomery form, little-endian -- the zkey's own point format: G1 64 B, G2 128 B.
 * k16_vk_create uploads the key and computes e(alpha, beta) once (PreparedVerifyingKey::alpha_g1_beta_g2).
 * k16_verify_batch: h_proofs = n x 256 B (A | B | C), h_inputs = n x (n_ic - 1) x 32 B standard-form integers (any 256-bit
 * value; they act modulo r, as Fr::from_le_bytes_mod_order), out_ok[i] = 1 accept / 0 reject.  3n Miller loops and n final
 * exponentiations, one GPU lane each: a throughput path for batches (BASELINE config 4 releases 64 proofs per wave).
 * Input validation: a proof whose A / B / C has a coordinate >= p (a non-canonical encoding: A, A + p, A + 2p would
 * otherwise be interchangeable) or does not lie on the curve (A, C) / the twist (B) is REJECTED (flag 0), as ark's
 * deserialisation refuses it before verify_proof runs.  Membership of B in the r-torsion subgroup is NOT tested (the
 * service verifies its own prover's output; aptos-types validates foreign points when it deserialises them): a caller that
 * verifies proofs from elsewhere calls k16_verify_batch_checked below, which adds that test.  Points with a zero
 * coordinate pair count as the point at infinity (the pair then contributes 1, as ark-ec's multi_miller_loop skips it). */
typedef struct k16_vk k16_vk;
int  k16_vk_create(k16_ctx* ctx, const void* alpha1_g1, const void* beta2_g2, const void* gamma2_g2, const void* delta2_g2,
                   const void* ic_g1, uint32_t n_ic, k16_vk** out);
void k16_vk_destroy(k16_vk* vk);
int  k16_verify_batch(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n,
                      uint8_t* h_out_ok);
/* Small batches (n <= K16_VERIFY_COOP_MAX, default 2048) of k16_verify_batch run ONE WAVEFRONT PER PROOF (a static program
 * of ~2000 steps of <= 64 independent field operations, csrc/verify_script.h): 1-2 ms for one proof or for a wave of 64,
 * where one lane per pairing needs ~45 ms -- the latency the per-proof check of prover_handler.rs:329-336 needs.  Same
 * flags.  parity tests: the GT value that path computes for every proof, e(A,B) e(vk_x,-gamma) e(C,-delta), 12 x 32 B per proof */
int  k16_verify_coop_gt(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n, void* h_out_gt);
/* parity tests: out[i] = e(P_i, Q_i) exactly as ark-ec's Bn::pairing gives it, 12 x 32 B per value (Fq12 = Fq6[w]/(w^2 - v),
 * Fq6 = Fq2[v]/(v^3 - 9 - u): c0.c0.a, c0.c0.b, c0.c1.a, ...), Montgomery form */
int  k16_pairing_vec(k16_ctx* ctx, const void* h_g1, const void* h_g2, uint64_t n, void* h_out_gt);

/* ---- point validation on the GPU: what ark-serialize's validated deserialisation checks ----
 * Status of a point: its coordinates are canonical (< p), checked first; then it lies on the curve (G1) or the twist (G2);
 * then, for G2 only, it lies in the order-r subgroup (the twist's cofactor is 2p - r = 10069 x a 241-bit prime; G1's is 1).
 * The G2 test is the endomorphism test of eprint 2022/348 section 5.1, one lane pair per point (csrc/bn254_points.h). */
enum { K16_PT_OK = 0, K16_PT_NONCANONICAL = 1, K16_PT_OFF_CURVE = 2, K16_PT_NOT_IN_SUBGROUP = 3 };
enum { K16_VERIFY_PAIRING_MISMATCH = 4 };
/* status per point, affine Montgomery LE as everywhere (G1 64 B, G2 128 B); all-zero = infinity = K16_PT_OK.  group is
 * K16_G1 or K16_G2; the points stream through bounded device buffers, so n is not limited by device memory. */
int  k16_points_check(k16_ctx* ctx, int group, const void* h_points, uint64_t n, uint8_t* h_status);
/* k16_verify_batch plus ark's validated deserialisation: out_ok[i] == (k16_verify_batch's flag && B_i in G2).
 * out_reason (may be NULL): 0 accepted, 1..3 the first failing point's status (A, then B, then C),
 * 4 = K16_VERIFY_PAIRING_MISMATCH.  The subgroup test of the batch is one launch on a stream of the key's own, running
 * beside the pairing (the wave-cooperative path for small batches as well as the general one). */
int  k16_verify_batch_checked(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n,
                              uint8_t* h_out_ok, uint8_t* h_out_reason);
/* Folded batch verification: ONE final exponentiation for n proofs -- the small-exponent batch test of Bellare, Garay and
 * Rabin (the form bellman ships as verify_proofs_batch).  Same inputs and the same out_ok / out_reason as
 * k16_verify_batch_checked, for bulk verification where nearly every proof is expected to be valid: waves a service
 * produced itself, re-verification of history under one key.  Single proofs and small waves belong on
 * k16_verify_batch[_checked]: below K16_VERIFY_FOLD_MIN proofs this call only forwards to k16_verify_batch_checked.
 *   Per proof (GPU): canonical coordinates, A and C on the curve, B on the twist AND in G2 (not optional: the fold relies on
 *   e(w A, B) = e(A, B)^w, which the ate Miller loop only promises for B in G2).  A proof that fails gets its reason
 *   (1..3) and takes no part in the fold; a proof with a zero point takes no part either and is settled by
 *   k16_verify_batch_checked.
 *   The fold: a 128-bit weight w_i per proof from the operating system's CSPRNG (getrandom), drawn after the proofs have
 *   been handed over, never zero; nothing fixes or disables them.  One equation is checked,
 *       prod_i e(w_i A_i, B_i) * e(S_x, -gamma) * e(S_C, -delta) * e(-s alpha, beta) == 1
 *       s = sum w_i mod r,  S_C = sum w_i C_i,  S_x = s IC[0] + sum_j (sum_i w_i x_ij mod r) IC[j+1]:
 *   n + 3 Miller loops, one final exponentiation (on 64 lanes: the wave-cooperative interpreter), one 128-bit G1 scalar
 *   multiplication per proof and one G1 MSM.  If it holds, every proof that took part is accepted and *out_folded = 1.
 *   Acceptance is PROBABILISTIC: a batch holding a wrong proof passes with probability about 2^-128.
 *   If it does not hold, some proof is wrong: the whole batch is verified again by k16_verify_batch_checked for exact flags
 *   (*out_folded = 0).  A batch with one bad proof therefore costs the fold PLUS k16_verify_batch_checked's time; there is
 *   no bisection.
 * A key whose wave-cooperative program is not on the device (K16_VERIFY_NO_COOP, or no room in LDS) forwards every batch
 * to k16_verify_batch_checked as well: *out_folded tells.
 * out_reason and out_folded may be NULL.  The call uses the context's MSM queue and stream: same threading rule as k16_msm
 * on that context, K16_ERR_ARG when k16_msm_pending(ctx) != 0 on entry; lane, window bits and the one-shot MSM settings of
 * the context are left as they were found. */
/* Smallest batch that is folded: the smallest measured n from which the fold's p50 stays below k16_verify_batch_checked's for
 * every larger measured n (tools/bench_verify_fold.py on one MI355X, profiles/verify_fold/bench_verify_fold.json: the fold
 * takes 26-28 ms whatever n is up to 16 384; the checked call takes 16.1 ms at n = 2048, the last size of its
 * wave-cooperative path, and 45.8 ms or more from n = 2049 on).  A compile-time constant, not a switch. */
#define K16_VERIFY_FOLD_MIN 2049
int  k16_verify_batch_folded(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n,
                             uint8_t* h_out_ok, uint8_t* h_out_reason, uint8_t* out_folded);
/* parity tests: the fold at ANY n >= 1 under the caller's weights (n x 16 B little-endian; a zero weight drops that proof):
 * the value V of the left-hand side above after the final exponentiation, 12 x 32 B in the format of k16_pairing_vec.  No
 * fallback; K16_ERR_ARG when a proof fails the point checks or has a zero point, or when MSMs are pending. */
int  k16_verify_fold_gt(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n,
                        const void* h_weights, void* h_out_gt);
/* ---- verified proving: every proof checked on the GPU before it is released (prover_handler.rs:329-336 in one call) ----
 * The verification key a proving key carries: alpha1, beta2, gamma2, delta2 from section 2 and IC from section 3 of the zkey
 * (no separate vkey file, no decimal parsing).  Container / curve errors as k16_prover_create_mem; K16_ERR_FORMAT when
 * section 3 is absent (synthetic keys omit it) or does not hold exactly nPublic + 1 points.  The result is an ordinary k16_vk. */
int  k16_vk_create_from_zkey(k16_ctx* ctx, const void* zkey, size_t size, k16_vk** out);
int  k16_vk_create_from_zkey_file(k16_ctx* ctx, const char* zkey_path, k16_vk** out);
/* Attaches the key the _verified calls check against (NULL detaches; the prover does not own it: destroy it after the
 * prover, or detach first).  K16_ERR_ARG unless vk belongs to the prover's context and has nPublic + 1 IC points. */
int  k16_prover_set_vk(k16_prover* p, const k16_vk* vk);
/* k16_prover_prove_mem / _prove_compact plus the check.  JSON and return value are exactly the plain call's for the same
 * witness and (r, s).  out_proof (256 B: A | B | C, affine Montgomery LE -- k16_verify_batch's proof format; may be NULL).
 * *out_ok: the flag k16_verify_batch gives for that proof with the public inputs taken from the witness (rows 1..nPublic of
 * the mem call's witness; the same wires read from `narrow` or the wide list for the compact call).  A rejected proof is
 * still written out, with *out_ok = 0 (the witness does not satisfy the circuit): the caller decides.  K16_ERR_ARG when no
 * key is attached.  On every error path nothing of the call is left in flight.
 * The check is SPLIT where the prover's data arrive (csrc/verify_script.h): A and B are final while the GPU still works on the
 * H MSM, so e(A,B) and e(vk_x,-gamma) -- two of the three Miller loops -- run on a stream of the key's own under it; only
 * e(C,-delta), one Fp12 product and the final exponentiation wait for C.  A case the programs do not decide (a zero point,
 * vk_x at infinity) is settled by k16_verify_batch after the proof: same flag.  One verified prove at a time per key. */
int  k16_prover_prove_mem_verified(k16_prover* p, const void* h_wtns, uint64_t n_vars, const uint8_t* r_std, const uint8_t* s_std,
                                   char* out_json, size_t cap, float* device_ms, uint8_t* out_proof, uint8_t* out_ok);
int  k16_prover_prove_compact_verified(k16_prover* p, uint64_t n_wide, const uint8_t* r_std, const uint8_t* s_std, char* out_json,
                                       size_t cap, float* device_ms, uint8_t* out_proof, uint8_t* out_ok);
/* k16_prover_prove_file_timed with the same check (what FullProver::prove runs once k16_fullprover_set_verify is on) */
int  k16_prover_prove_file_verified(k16_prover* p, const char* wtns_path, const uint8_t* r_std, const uint8_t* s_std,
                                    char* out_json, size_t cap, float* device_ms, float* prove_wall_ms, uint8_t* out_proof,
                                    uint8_t* out_ok);
/* Verified proving behind the drop-in FullProver (`fullprover` as for k16_fullprover_prove_mem).  on != 0: every pool slot builds
 * its verification key from the zkey and attaches it (a slot rebuilt after a device fault gets its key again); from then on
 * FullProver::prove, k16_fullprover_prove_mem and k16_fullprover_prove_compact answer a proof the check rejects with
 * ProverError::INVALID_INPUT (K16_ERR_FORMAT from the C entry points): the witness does not satisfy the circuit.  on == 0
 * detaches.  Call it after construction and before the first proof (K16_ERR_ARG while a slot is proving).  K16_ERR_FORMAT: the
 * zkey has no usable section 3 -- the reason goes to stderr, verification stays off, the provers keep working unverified.
 * K16_ERR_NO_DEVICE: the object is not ready.  Without the call nothing changes.  (A call, not an environment variable: which
 * variables the production library reads is a fixed list, tests/test_boundary.py.) */
int  k16_fullprover_set_verify(const void* fullprover, int on);
/* parity tests: the split check with no prover involved, n <= 64 proofs: out_early = the multi-Miller value of (A,B) and
 * (vk_x,-gamma) before any final exponentiation (not canonical: an Fq factor rides on it), out_gt = the GT value, byte-equal
 * to k16_verify_coop_gt's; n x 12 x 32 B each.  No fallback: K16_ERR_ARG when a proof fails the point checks, has a zero
 * point, or its vk_x is the point at infinity. */
int  k16_verify_split_gt(k16_ctx* ctx, const k16_vk* vk, const void* h_proofs, const void* h_inputs, uint64_t n,
                         void* h_out_early, void* h_out_gt);
/* every point of a Groth16 zkey, in the sections that are present: 2 (alpha1, beta1, beta2, gamma2, delta1, delta2 =
 * indices 0..5), 3 (IC; the prover does not need it and synthetic keys omit it), 5 (A), 6 (B1), 7 (B2), 8 (C), 9 (H).
 * K16_OK with *n_bad = 0 when all pass; otherwise the first failure in (section, index) order and the number of failing
 * points.  Container / curve errors as k16_prover_create_mem (K16_ERR_FORMAT, K16_ERR_CURVE).  The key streams through
 * bounded device buffers (two 32 MB chunks): it is never held on the device whole.  Not run by k16_prover_create: the
 * caller decides when to pay for it. */
int  k16_zkey_check(k16_ctx* ctx, const void* zkey, size_t size, uint32_t* bad_section, uint64_t* bad_index,
                    uint8_t* bad_status, uint64_t* n_bad);
int  k16_zkey_check_file(k16_ctx* ctx, const char* zkey_path, uint32_t* bad_section, uint64_t* bad_index,
                         uint8_t* bad_status, uint64_t* n_bad);

/* ---- R1CS witness check: WHICH constraints does a witness break? ----
 * A verified prove (above) can only say that a proof was rejected; a zkey cannot say more, its section 4 holds A and B alone.
 * With the circuit's .r1cs file (iden3 container: header section 1, constraints section 2, coefficients in standard form;
 * csrc/r1cs_file.h) the check is (A.w) o (B.w) - C.w = 0, evaluated on the GPU in the prover's own field code: three sparse
 * matrix-vector products in one launch and one pointwise pass (csrc/r1cs_check.hip).
 * k16_r1cs_create* parse and upload a circuit once: K16_ERR_FORMAT for a malformed file (truncation, a count that runs past its
 * section, a wire >= nWires, a coefficient >= r, bytes left over, a header with nWires = 0 or nPubOut + nPubIn >= nWires),
 * K16_ERR_CURVE when the field is not BN254's Fr, K16_ERR_ARG for
 * 2^32 / 3 constraints or more, or 2^32 or more (padded) terms.  A wire listed twice in a combination is legal: its coefficients add.
 * The check calls: *n_failed = number of broken constraints (0: the witness satisfies the circuit); h_failed (may be NULL) receives
 * the lowest min(*n_failed, cap) constraint numbers, ascending -- the same list for every run.
 *   k16_r1cs_check_mem             h_wtns: n_wires x 32 B standard form (the payload of wtns section 2); K16_ERR_ARG unless
 *                                  n_wires is the circuit's
 *   k16_r1cs_check_file            a .wtns file, under the container and curve checks of k16_prover_prove_file; K16_ERR_FORMAT
 *                                  when it does not hold exactly the circuit's number of values
 *   k16_r1cs_check_prover_witness  the witness of the prover's LAST prove call, read where it lies on the device -- no upload.
 *                                  K16_ERR_ARG unless that call succeeded (k16_prover_prove_mem / _file / _compact and their
 *                                  _verified forms alike: an accepted and a rejected proof both leave the whole witness; a
 *                                  failed or aborted call does not, nor does the warm-up of k16_prover_create), unless the
 *                                  R1CS object lives on the prover's context and unless its nWires is the key's nVars.
 * A witness is REFUSED with K16_ERR_FORMAT, whatever its constraints say, when a wire value is >= r (checked on the device) or
 * when wire 0 is not 1: every constraint can hold for such an assignment, yet no proof of it verifies.
 * THREADING: one check at a time per object, on the context's stream, under the context's one-caller rule.  Every error leaves
 * nothing in flight. */
typedef struct k16_r1cs k16_r1cs;
int  k16_r1cs_create(k16_ctx* ctx, const char* path, k16_r1cs** out);
int  k16_r1cs_create_mem(k16_ctx* ctx, const void* r1cs, size_t size, k16_r1cs** out);
void k16_r1cs_destroy(k16_r1cs* r);
int  k16_r1cs_info(const k16_r1cs* r, uint32_t* n_wires, uint32_t* n_public, uint32_t* n_constraints, uint64_t* n_terms);
int  k16_r1cs_check_mem(k16_ctx* ctx, k16_r1cs* r, const void* h_wtns, uint64_t n_wires, uint64_t* n_failed, uint32_t* h_failed,
                        uint32_t cap);
int  k16_r1cs_check_file(k16_ctx* ctx, k16_r1cs* r, const char* wtns_path, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap);
int  k16_r1cs_check_prover_witness(k16_prover* p, k16_r1cs* r, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap);
/* A.w | B.w | C.w of one constraint as the LAST completed check computed them, 3 x 32 B standard form, canonical.  K16_ERR_ARG
 * when no check has completed on the object (a refused witness completes none) or the constraint number is out of range. */
int  k16_r1cs_last_values(k16_r1cs* r, uint32_t constraint, void* h_out96);
/* Do this circuit and this proving key belong together?  Host only.  Section 4 of a snarkjs Groth16 zkey is derived from the
 * circuit: per term of A and B a record { matrix, constraint, wire, coefficient * 2^512 mod r } plus one row per public wire
 * (and the constant) behind the last constraint.  *mismatch = 0: the zkey's section 4 and header (nVars, nPublic, a power-of-two
 * domain that holds the rows) are this circuit's; else the kind of the first difference -- 1 header, 2 matrix A, 3 matrix B,
 * 4 public rows -- with its constraint and wire in k16_last_error.  K16_ERR_FORMAT / K16_ERR_CURVE for an unreadable zkey. */
int  k16_r1cs_match_zkey(k16_ctx* ctx, const k16_r1cs* r, const void* zkey, size_t size, uint32_t* mismatch);

/* ---- unbound-wire scan: WHICH wires does the circuit leave free under this witness? ----
 * The dual of the check: not "does w satisfy the circuit" but "does the circuit pin w".  With a_c, b_c, c_c the sums A.w, B.w, C.w
 * of constraint c as the LAST completed check left them on the device, and A^, B^, C^ the MERGED coefficients of wire i in
 * constraint c (a wire listed twice adds, as in the check), changing wire i alone by d moves the residual a_c b_c - c_c by
 * d lin + d^2 quad,  lin = A^ b_c + B^ a_c - C^,  quad = A^ B^  (mod r).  Every wire 1 .. nWires - 1 gets a class:
 *   K16_WIRE_BOUND    some constraint has lin != 0 or quad != 0
 *   K16_WIRE_ABSENT   A^ = B^ = C^ = 0 in every constraint: the wire is in no term, or its coefficients cancel.  Structural, the
 *                     same for every witness
 *   K16_WIRE_UNBOUND  some merged coefficient is non-zero, yet lin = 0 and quad = 0 everywhere: under THIS witness every value
 *                     of the wire leaves every residual as it is
 * Wire 0 is the constant 1: reported BOUND, never listed.  Zero is zero modulo r (canonical form, as in the check); the scan is
 * exact and deterministic.  It is defined for any witness a check completed on, and meant for a satisfying one.  It judges
 * nothing: a mux input behind a zero selector is UNBOUND and legitimate.
 *   k16_r1cs_unbound_wires     one launch over the circuit's incidences (csrc/r1cs_check.hip) on the sums of the last completed
 *                              check: K16_ERR_ARG when none has completed on r (a refused witness completes none), exactly as
 *                              k16_r1cs_last_values.  *n_absent / *n_unbound: how many wires of each class.  h_wires / h_class
 *                              (either may be NULL): the lowest min(*n_absent + *n_unbound, cap) wires that are not BOUND,
 *                              ascending, with their class -- the same list on every run.  Public wires are 1 .. nPublic, so they
 *                              come FIRST: an unbound public wire is the finding to look at first.  h_status (may be NULL):
 *                              n_wires bytes, the class of every wire.
 *   k16_r1cs_wire_constraints  the constraints `wire` appears in with a non-zero merged coefficient: *n = how many, h_constraints
 *                              (may be NULL) the lowest min(*n, cap), ascending.  Host only; needs no check.  K16_ERR_ARG for a
 *                              wire >= nWires.
 *   k16_r1cs_incidences        the number of (wire, constraint) pairs with a non-zero merged coefficient: what the scan walks
 *                              (all but the column of wire 0, which is no variable).  Host only.
 * The incidence list is built by the first of these calls and its device copy by the first scan; both stay with the object.  A
 * circuit that is never scanned pays nothing.  K16_ERR_ARG for 2^32 incidences or more; K16_ERR_NOMEM / K16_ERR_HIP as elsewhere.
 * THREADING: as k16_r1cs_check_*: one call at a time per object, on the context's stream.  On an object attached to a prover
 * the scan is legal BETWEEN prove calls (the sums are the last prove's), not while one runs.  Every error leaves nothing in
 * flight. */
enum { K16_WIRE_BOUND = 0, K16_WIRE_ABSENT = 1, K16_WIRE_UNBOUND = 2 };
int  k16_r1cs_unbound_wires(k16_r1cs* r, uint64_t* n_absent, uint64_t* n_unbound, uint32_t* h_wires, uint8_t* h_class, uint32_t cap,
                            uint8_t* h_status);
int  k16_r1cs_wire_constraints(k16_r1cs* r, uint32_t wire, uint64_t* n, uint32_t* h_constraints, uint32_t cap);
int  k16_r1cs_incidences(k16_r1cs* r, uint64_t* n_pairs);

/* ---- second-value scan: WHICH wires could take exactly one other value? ----
 * The unbound-wire scan finds the wires that may take ANY value.  This one finds the wires that may take ONE other value with
 * every other wire held fixed -- the two roots of a square, a boolean that nothing but b (b - 1) = 0 uses.  Such a wire is BOUND
 * above, yet a second witness satisfies every constraint and its proof verifies.  With lin and quad as above, changing wire i
 * alone by d moves the residual of constraint c by d lin + d^2 quad, and each (wire, constraint) incidence is
 *   FREE  lin = 0 and quad = 0: every d leaves the residual as it is
 *   PIN   exactly one of lin, quad is zero: no d != 0 leaves it (the linear case, and the double root x x = y at x = 0)
 *   ROOT  lin != 0 and quad != 0: exactly one d != 0 leaves it, d = -lin / quad
 * A wire is K16_WIRE_TWO_VALUED when it has no PIN incidence, at least one ROOT incidence, and all its ROOT incidences give the
 * same d: the wire's SHIFT; w_i + d is the second value.  Every other wire keeps its class of the unbound-wire scan, BOUND now
 * reading "single-valued with respect to changes of one wire".  Wire 0 is BOUND and never listed.  Zero is zero modulo r
 * (canonical form); the scan is exact and deterministic.  It is a statement about the CHANGE of the residuals: defined for any
 * witness a check completed on, meant for a satisfying one.  It judges nothing: both roots may be meant.
 *   k16_r1cs_second_values  on the sums of the last completed check, over the incidence list of the unbound-wire scan (made and
 *                           uploaded by whichever of the two scans comes first; this scan's own per-wire buffers by its first
 *                           call).  *n_two_valued: how many wires are two-valued.  h_wires / h_shift (either may be NULL): the
 *                           lowest min(*n_two_valued, cap) of them, ascending, and their shifts, 32 bytes each: standard form,
 *                           little-endian, canonical, never zero -- the same bytes on every run.  h_status (may be NULL): n_wires
 *                           bytes, the class 0 .. 3 of every wire; with 3 read as K16_WIRE_BOUND these are the bytes
 *                           k16_r1cs_unbound_wires writes for the same sums.
 * Preconditions, errors and THREADING as k16_r1cs_unbound_wires: K16_ERR_ARG when no check has completed on r or a prove call is
 * running on it; every error leaves nothing in flight. */
enum { K16_WIRE_TWO_VALUED = 3 };
int  k16_r1cs_second_values(k16_r1cs* r, uint64_t* n_two_valued, uint32_t* h_wires, uint8_t* h_shift /* 32 B each */, uint32_t cap,
                            uint8_t* h_status /* n_wires bytes, may be NULL */);

/* ---- determinism closure: WHICH wires do the inputs leave open? ----
 * Both scans above move ONE wire with every other wire held fixed.  This call asks the question of an audit: given the values of
 * the SEED wires (by default the circuit's inputs), is every other wire forced?  With FREE / PIN / ROOT of an incidence as
 * above, the closure K is the least set of wires that holds the seed S (wire 0 always) and satisfies
 *     constraint c was not found broken by the last check, exactly one wire x with a non-zero merged coefficient in c lies
 *     outside K, and the incidence (x, c) is a PIN   ==>   x is in K
 * taken level by level: K_0 = S, K_k+1 = K_k and every x the rule gives with respect to K_k.  The ROUND of a derived wire is the
 * first k with x in K_k, its BY constraint the lowest c the rule holds for with respect to K_(round - 1).  Both are functions of
 * circuit, witness and seed alone; the call is exact and deterministic.
 * SOUND: a witness that satisfies the circuit and agrees with this one on S agrees with it on K (in c all wires but x are equal,
 * the residuals differ by t lin + t^2 quad, both are 0, a PIN leaves t = 0).  Hence: a broken constraint derives nothing; a FREE
 * incidence of a second outside wire still counts (two outside wires have a cross term neither's lin or quad shows); a ROOT
 * derives nothing (the two-valued case).  NOT COMPLETE: an OPEN wire may still be forced by an argument over several constraints.
 *   K16_DET_SEED     in S
 *   K16_DET_DERIVED  in K, not in S
 *   K16_DET_ABSENT   not in K and in no term (structural, as K16_WIRE_ABSENT)
 *   K16_DET_OPEN     not in K and in some term
 * It judges nothing: an OPEN wire behind a zero selector is legitimate; an OPEN public output is the finding to look at first.
 * Defined for any witness a check completed on, meant for a satisfying one.
 *   h_seed / n_seed   the seed wires; duplicates are legal, wire 0 is added, a wire >= nWires is K16_ERR_ARG before anything is
 *                     launched.  NULL: wire 0 and the wires nPubOut + 1 .. nPubOut + nPubIn + nPrvIn of the .r1cs header (iden3
 *                     wire order); K16_ERR_ARG when the header's counts reach beyond nWires.
 *   *n_derived, *n_absent, *n_open   wires per class;  *n_rounds   the highest round used
 *   h_wires (may be NULL)   the lowest min(*n_open, cap) OPEN wires, ascending
 *   h_status (may be NULL)  n_wires bytes, the class of every wire
 *   h_round (may be NULL)   n_wires words: 0 for a seed wire, k >= 1 for a derived one, 0xffffffff otherwise
 *   h_by (may be NULL)      n_wires words: the deriving constraint, 0xffffffff where there is none
 * One pair of launches and one host synchronise per round (csrc/r1cs_check.hip): a circuit of depth D costs D of them.  The
 * incidence list is the scans' (made and uploaded by whichever call comes first), this call's own buffers are made by its first
 * call and stay with the object.  Preconditions, errors and THREADING as k16_r1cs_unbound_wires: K16_ERR_ARG when no check has
 * completed on r or a prove call is running on it; legal between prove calls on an attached object; every error leaves nothing
 * in flight. */
enum { K16_DET_SEED = 0, K16_DET_DERIVED = 1, K16_DET_ABSENT = 2, K16_DET_OPEN = 3 };
int  k16_r1cs_determined_wires(k16_r1cs* r, const uint32_t* h_seed, uint32_t n_seed, uint64_t* n_derived, uint64_t* n_absent,
                               uint64_t* n_open, uint32_t* n_rounds, uint32_t* h_wires, uint32_t cap, uint8_t* h_status,
                               uint32_t* h_round, uint32_t* h_by);

/* ---- witness completion: WHICH VALUES do the given wires force? ----
 * The closure above names the wires a seed forces; this call computes them.  It takes the circuit, the GIVEN wires G and their
 * values (wire 0 is always given and must be 1), K_0 = G + {0}, and applies, level by level,
 *     in constraint c exactly one wire x with a non-zero merged coefficient (A^, B^, C^ as in the scans) lies outside K_k; with
 *     a0, b0, c0 the sums of c's three combinations over its wires in K_k, the residual of c as a polynomial in x is
 *     quad x^2 + lin x + k0,  quad = A^ B^,  lin = A^ b0 + B^ a0 - C^,  k0 = a0 b0 - c0  (mod r);
 *     quad = 0 and lin != 0   ==>   x joins K_k+1 with the value -k0 / lin
 * Otherwise c gives nothing: quad != 0 leaves a quadratic (no square root is taken), lin = 0 means c does not depend on x.
 * round[x] = k + 1; by[x] is the LOWEST c the rule holds for with respect to K_k, and the value is that constraint's.  The result
 * is a function of circuit, givens and their values alone: exact, deterministic, the same bytes on every run.
 *   K16_SOLVE_GIVEN   in G (or wire 0)
 *   K16_SOLVE_SOLVED  in K, not given
 *   K16_SOLVE_ABSENT  not in K and in no term
 *   K16_SOLVE_OPEN    not in K and in some term
 * numbered as K16_DET_*: the two maps compare directly.
 * RETURNED ASSIGNMENT (h_wtns, n_wires x 32 B standard form, in and out): given wires keep their values, solved wires get
 * theirs in canonical standard form, ABSENT and OPEN wires are written as 0.  What the caller had in the positions outside G is
 * ignored: any bytes, values >= r included.
 * VERDICT: a constraint with no wire outside the final K is CLOSED and is judged on the returned assignment.  *n_failed = the
 * number of closed constraints that are broken, h_failed (may be NULL) the lowest min(*n_failed, cap_failed) of them, ascending;
 * a constraint that would have given an already solved wire a different value shows up here.  *n_open_constraints counts the
 * rest; they are not judged.
 * SOUND: every satisfying witness that agrees with the givens agrees with every solved value (with quad = 0 and lin != 0 the
 * root is unique).  *n_failed > 0 proves that NO satisfying witness has these given values.  *n_open == 0 && *n_failed == 0:
 * the returned bytes are a satisfying witness, and the only one with these givens.
 * NOT COMPLETE, in two ways, and the call judges nothing beyond this: an OPEN wire may still be forced by an argument over
 * several constraints, or by a quadratic; and a constraint with lin = 0, k0 != 0 whose one wire is never solved stays unjudged,
 * although nothing satisfies it.
 *   h_given / n_given   the given wires; duplicates are legal, wire 0 is added.  NULL: the default seed of
 *                       k16_r1cs_determined_wires (wire 0 and the header's inputs), K16_ERR_ARG when the header's counts reach
 *                       beyond nWires
 *   *n_solved, *n_absent, *n_open, *n_rounds, *n_failed, *n_open_constraints   required; zeroed on entry
 *   h_wires (may be NULL)   the lowest min(*n_open, cap) OPEN wires, ascending
 *   h_status, h_round, h_by (may be NULL)   as k16_r1cs_determined_wires: class, round (0 for a given wire) and solving
 *                       constraint of every wire, 0xffffffff where there is none
 * ERRORS: K16_ERR_ARG when a given wire is >= nWires (nothing is launched, no list, map or witness byte is written);
 * K16_ERR_FORMAT when a GIVEN value is >= r or wire 0's value is not 1, as in k16_r1cs_check_* (h_wtns, lists and maps stay
 * untouched); K16_ERR_ARG while a prove call runs on an attached object -- the call is legal between prove calls.  Every error
 * leaves nothing in flight.  THREADING as k16_r1cs_check_*.
 * STATE: the call needs no completed check and ends with one: after K16_OK the object is in the state k16_r1cs_check_mem on the
 * returned h_wtns would leave -- k16_r1cs_last_values, both scans and the closure read the sums of the returned assignment.
 * After an error the object holds no completed check.
 * One host synchronise per round, as the closure; the row view of the circuit (8 bytes a term) is uploaded by the first call and
 * stays with the object, the incidence list is the scans' (csrc/r1cs_scan.hip). */
enum { K16_SOLVE_GIVEN = 0, K16_SOLVE_SOLVED = 1, K16_SOLVE_ABSENT = 2, K16_SOLVE_OPEN = 3 };
int  k16_r1cs_complete_witness(k16_r1cs* r, void* h_wtns /* n_wires x 32 B standard form, in and out */, const uint32_t* h_given,
                               uint32_t n_given, uint64_t* n_solved, uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds,
                               uint64_t* n_failed, uint32_t* h_failed, uint32_t cap_failed, uint64_t* n_open_constraints,
                               uint32_t* h_wires /* lowest min(*n_open, cap) OPEN wires, ascending */, uint32_t cap, uint8_t* h_status,
                               uint32_t* h_round, uint32_t* h_by);

/* ---- witness completion, second rule: the bit decompositions the booleans force ----
 * The linear rule stops at a constraint with two unknown wires.  The commonest such constraint of a circom circuit is
 * Num2Bits: ONE linear constraint sum 2^i b_i = x over wires that each carry their own b (b - 1) = 0.
 * BOOLEAN: a wire x >= 1 is BOOLEAN when some constraint has a non-zero merged coefficient on no wire other than x and wire 0
 * and, with wire 0 = 1 and A = a1 x + a0, B = b1 x + b0, C = c1 x + c0, its residual quad x^2 + lin x + k has quad = a1 b1 != 0,
 * k = a0 b0 - c0 = 0 and lin + quad = 0 (lin = a1 b0 + a0 b1 - c1): the roots are exactly 0 and 1.  A function of the circuit
 * alone; b (b - 1) = 0, b (1 - b) = 0, b b = b and their scaled forms qualify.
 *   k16_r1cs_boolean_wires   *n_boolean = how many wires are BOOLEAN; h_mark (may be NULL): n_wires bytes, 1 for a BOOLEAN wire.
 *                            Needs no completed check; the marks are made by the first call that needs them and stay with the
 *                            object.  THREADING and errors as k16_r1cs_incidences.
 * THE BIT RULE, with respect to a set K of known wires: constraint c has k unknown wires x_1 .. x_k (merged coefficient
 * non-zero, outside K), 2 <= k <= 253; a0, b0, c0 are the sums of its combinations over its wires in K.  The rule applies when
 *   (a) every x_j is BOOLEAN;
 *   (b) every unknown has A^ = 0, or every unknown has B^ = 0: the residual is sum lin_j x_j + k0 with
 *       lin_j = A^_j b0 + B^_j a0 - C^_j, k0 = a0 b0 - c0;
 *   (c) there is a lambda != 0 with lin_j / lambda = 2^(e_j) as canonical integers, the e_j pairwise distinct, 0 <= e_j <= 252.
 *       lambda is tried as the lin of the LOWEST-numbered unknown wire, then as that of the HIGHEST-numbered (a lin of 0 is no
 *       lambda); where neither serves, c gives nothing.  This is part of the definition.
 * With v = -k0 / lambda as a canonical integer: v < 2^253 and every set bit of v among the e_j -> c is FEASIBLE and every x_j
 * joins K with the value bit e_j of v; otherwise c is INFEASIBLE: it gives nothing, its wires stay as they are.
 * LEVELS: the linear rule runs to its fixed point as in k16_r1cs_complete_witness; then ONE bit level examines every constraint
 * with respect to that K.  The wires it solves get the next round number, by[x] = the LOWEST feasible c that names x, and the
 * value is that constraint's; the linear rule resumes.  The call ends when a bit level solves nothing.
 * SOUND: a satisfying witness that agrees on K has x_j in {0, 1} by the wires' own constraints, and sum 2^(e_j) x_j < 2^253 < r:
 * distinct 0/1 vectors give distinct residuals, so the solution is unique where it exists -- whichever lambda was found.
 * *n_infeasible > 0 proves that NO satisfying witness has these givens, exactly as *n_failed > 0 does; *n_open == 0 &&
 * *n_failed == 0 still means the returned bytes are the only satisfying witness with these givens.
 *   rules            K16_SOLVE_RULE_LINEAR, or K16_SOLVE_RULE_LINEAR | K16_SOLVE_RULE_BITS; anything else is K16_ERR_ARG (the
 *                    object keeps the check it had)
 *   *n_by_bits       required: the wires the bit rule solved
 *   *n_infeasible    required: the INFEASIBLE constraints of the FINAL state; h_infeasible (may be NULL) the lowest
 *                    min(*n_infeasible, cap_infeasible) of them, ascending
 *   h_rule (may be NULL)   n_wires bytes: 0 for a wire that is given or not solved, 1 for the linear rule, 2 for the bit rule
 * Every other argument, the returned assignment, STATE, errors and THREADING are k16_r1cs_complete_witness's.  With
 * rules = K16_SOLVE_RULE_LINEAR every output byte is that call's and *n_by_bits = *n_infeasible = 0.  The result is a function
 * of circuit, givens, values and rules alone: the same bytes on every run.  One host synchronise per bit level on top of the
 * linear rounds; a constraint-side index of the incidence list (4 bytes an incidence) is uploaded by the first call that asks
 * for the bit rule (csrc/r1cs_scan.hip, csrc/r1cs_bools.h). */
enum { K16_SOLVE_RULE_LINEAR = 1, K16_SOLVE_RULE_BITS = 2 };
int  k16_r1cs_boolean_wires(k16_r1cs* r, uint64_t* n_boolean, uint8_t* h_mark /* n_wires bytes, may be NULL */);
int  k16_r1cs_complete_witness_ex(k16_r1cs* r, void* h_wtns, const uint32_t* h_given, uint32_t n_given, uint32_t rules,
                                  uint64_t* n_solved, uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint64_t* n_failed,
                                  uint32_t* h_failed, uint32_t cap_failed, uint64_t* n_open_constraints, uint32_t* h_wires, uint32_t cap,
                                  uint8_t* h_status, uint32_t* h_round, uint32_t* h_by, uint64_t* n_by_bits, uint64_t* n_infeasible,
                                  uint32_t* h_infeasible, uint32_t cap_infeasible, uint8_t* h_rule /* n_wires bytes, may be NULL */);

/* ---- determinism closure, second rule: the bit decompositions the held booleans force ----
 * k16_r1cs_determined_wires stops at every constraint with two outside wires, Num2Bits among them, so it calls OPEN what the
 * completion above proves unique.  k16_r1cs_determined_wires_ex adds the bit rule to the closure.  The closure reads the sums and
 * the verdicts of the last completed check, never the witness; that a wire holds 0 or 1 in this witness comes from there too:
 * HELD: a wire x >= 1 is HELD under the last completed check when some constraint that marks x BOOLEAN (above) was not found
 * broken by it.  Such a row's residual is quad x (x - 1) = 0 with quad != 0: x is 0 or 1 in this witness.  HELD is a subset of
 * BOOLEAN, and all of it on a satisfying witness.
 *   k16_r1cs_held_wires   *n_held = how many wires are HELD; h_mark (may be NULL): n_wires bytes, 1 for a HELD wire.  Needs a
 *                         completed check, like the scans (K16_ERR_ARG without one); its buffers are made by its first call or
 *                         by the first k16_r1cs_determined_wires_ex call that asks for the bit rule.
 * THE BIT RULE OF THE CLOSURE, with respect to K: constraint c was not found broken by the last check and has k outside wires
 * x_1 .. x_k (merged coefficient non-zero, outside K), 2 <= k <= 253.  It applies when
 *   (a) every x_j is HELD;
 *   (b) every outside incidence has no A^, or every outside incidence has no B^ (one wire on both sides counts as both): the sum
 *       of the check that multiplies an unknown is then a sum over K, and lin_j = A^_j b0 + B^_j a0 - C^_j depends on K alone;
 *   (c) as (c) of the completion's bit rule: lambda is the lin of the LOWEST outside wire, then of the HIGHEST; a lin of 0 is no
 *       lambda; every lin_j / lambda is 2^(e_j) as a canonical integer, the e_j pairwise distinct and <= 252.  Where neither end
 *       serves, c gives nothing: part of the definition.
 * Then every x_j joins K.  There is no feasibility test and no INFEASIBLE class: c is unbroken and the x_j are 0 / 1 in this
 * witness, so the witness is the expansion.
 * SOUND: let w' satisfy the circuit and agree with this witness w on K.  w'_j is 0 or 1 by the static marks, w_j by HELD.  Both
 * residuals of c are 0 and the lin_j depend on K alone, so sum 2^(e_j) (w_j - w'_j) = 0 modulo r; every difference is -1, 0 or
 * 1 and the sum is below 2^253 < r in absolute value, so it is 0 as an integer, and two 0/1 vectors with the same sum over
 * distinct powers of two are equal.  Three things the argument needs, none an inefficiency: a BROKEN c derives nothing; a
 * BOOLEAN wire whose marking rows are all broken is not HELD; a FREE outside incidence (lin_j = 0) fails (c) and keeps the row out.
 * LEVELS: the PIN rule runs to its fixed point as in k16_r1cs_determined_wires; then ONE bit level examines every constraint with
 * respect to that K.  The wires it derives get the next round number and by[x] = the LOWEST qualifying c; the PIN rule resumes.
 * The call ends when a bit level derives nothing.
 *   rules          K16_DET_RULE_PIN, or K16_DET_RULE_PIN | K16_DET_RULE_BITS; anything else is K16_ERR_ARG before anything is
 *                  launched (the object keeps the check it had)
 *   *n_by_bits     required: the wires the bit rule derived
 *   h_rule (may be NULL)   n_wires bytes: 0 for a seed or underived wire, 1 for the PIN rule, 2 for the bit rule
 * Every other argument, preconditions, errors, THREADING and state are k16_r1cs_determined_wires's.  With rules =
 * K16_DET_RULE_PIN the call runs that call's code, allocates nothing beyond it, every output byte is that call's and
 * *n_by_bits = 0.  One host synchronise per bit level on top of the PIN rounds, at most n_wires - 1 levels.  The constraint-side
 * index (shared with the completion's bit rule, made by whichever comes first), the marking rows, the HELD mask, the bit
 * candidates and the rule bytes are made by the first call that asks for the bit rule; the row view of the completion is not
 * built (csrc/r1cs_scan.hip, csrc/r1cs_bools.h). */
enum { K16_DET_RULE_PIN = 1, K16_DET_RULE_BITS = 2 };
int  k16_r1cs_determined_wires_ex(k16_r1cs* r, const uint32_t* h_seed, uint32_t n_seed, uint32_t rules, uint64_t* n_derived,
                                  uint64_t* n_absent, uint64_t* n_open, uint32_t* n_rounds, uint32_t* h_wires, uint32_t cap,
                                  uint8_t* h_status, uint32_t* h_round, uint32_t* h_by, uint64_t* n_by_bits,
                                  uint8_t* h_rule /* n_wires bytes, may be NULL */);
int  k16_r1cs_held_wires(k16_r1cs* r, uint64_t* n_held, uint8_t* h_mark /* n_wires bytes, may be NULL */);

/* ---- the open-set solve: rank and null space of what a closure leaves open ----
 * The closure derives a wire only when ONE constraint pins it.  x + y = s1, x - y = s2 force both wires, yet every constraint
 * has two outside wires: both stay OPEN.  Wherever the constraints are LINEAR in the open wires the question "forced, or what
 * is the second witness?" has an exact answer, by linear algebra over Fr on the Jacobian of the residuals at this witness.
 * Reads the sums and the verdicts of the last completed check, as the scans do.
 *   h_fixed     n_wires bytes, non-zero = the wire is held FIXED; wire 0 always is.  Typically status != K16_DET_OPEN of a
 *               closure; any mask is legal.  An OUTSIDE wire is one that is not fixed.
 *   DROPPED     a constraint the last check found broken gives no equation and no connectivity (the closure's rule)
 *   LINEAR / CROSS   an unbroken constraint with an outside incidence is LINEAR when its outside wires with A^ != 0 or its outside
 *               wires with B^ != 0 are none, CROSS otherwise (x * x = y with x outside is CROSS: two-valued, never forced).
 *               Moving the outside wires by t moves the residual of a LINEAR constraint by exactly sum_x lin(x, c) t_x,
 *               lin = A^ b_c + B^ a_c - C^ as in the scans.
 *   COMPONENTS  of the bipartite graph of outside wires and unbroken constraints, LINEAR and CROSS alike; a component's id is its
 *               lowest wire; EXACT: it has no CROSS constraint.  An outside wire whose incidences all lie in broken constraints
 *               is a component of one wire and no rows.
 *   J, R, rank  J: rows = the component's LINEAR constraints, columns = its wires ascending, entries lin mod r.  R: its reduced
 *               row echelon form for that column order (unique, whatever the row order); rank: its pivots.
 * One byte per wire:
 *   K16_OPEN_FIXED      in h_fixed, or wire 0
 *   K16_OPEN_ABSENT     outside and in no term of any constraint (structural, as K16_WIRE_ABSENT)
 *   K16_OPEN_FORCED     e_x lies in the row space of J: x is a pivot column whose row of R is zero in every non-pivot column
 *   K16_OPEN_FREE       not FORCED, component EXACT
 *   K16_OPEN_UNDECIDED  not FORCED, the component has a CROSS constraint
 *   K16_OPEN_SKIPPED    the component has more than K16_OPEN_MAX_WIRES wires: not eliminated
 * SOUND: any witness that satisfies the circuit and agrees with this one on the fixed wires agrees with it on every FORCED wire
 * (in EXACT components and others alike: only LINEAR rows are used).  EXACT on EXACT components: every FREE wire x has a direction
 * d with d_x != 0, supported on its component, such that w + d leaves the residual of every unbroken constraint at zero.  The
 * call judges nothing: a FREE mux input behind a zero selector is legitimate.
 * The CANONICAL direction of a FREE wire x: F = the non-pivot columns; for f in F, v_f[f] = 1, v_f[f'] = 0 for the other free
 * columns, v_f[p] = -R[row(p)][f] for pivot columns.  x in F: d = v_x; else f = the lowest free column with R[row(x)][f] != 0 and
 * d = v_f / v_f[x].  So d_x = 1; the bytes are the same on every run and for every order of the constraints in the file.
 *   k16_r1cs_open_system     *n_forced .. *n_absent: wires of each class; *n_components: all components, SKIPPED ones included;
 *                            *n_dims: the sum of (wires - rank) over the EXACT components that were eliminated.  h_wires /
 *                            h_class (may be NULL): the lowest min(cap, n_forced + n_free + n_undecided + n_skipped) wires that
 *                            are neither FIXED nor ABSENT, ascending, with their class.  h_status (may be NULL): n_wires
 *                            bytes, the class of every wire.  h_comp (may be NULL): n_wires words, the lowest wire of the
 *                            wire's component, 0xffffffff for FIXED / ABSENT.
 *   k16_r1cs_open_direction  stateless: finds `wire`'s component on the host from h_fixed and eliminates that one component.
 *                            *cls: the wire's class; *comp_wires / *comp_rows / *comp_cross (may be NULL): the component's wires,
 *                            LINEAR rows and CROSS constraints (0 for FIXED / ABSENT); *rank (may be NULL; 0 for SKIPPED);
 *                            *n: the non-zeros of d, 0 unless the wire is FREE; h_wires / h_vals (may be NULL): the lowest
 *                            min(*n, cap) wires with d != 0, ascending, and their values, 32 bytes each, standard form,
 *                            little-endian, canonical.  Add d to the witness and k16_r1cs_check_mem finds what it found.
 * Preconditions, errors and THREADING as k16_r1cs_unbound_wires: K16_ERR_ARG when no check has completed on r, while a prove call
 * runs on an attached object, for h_fixed == NULL and for wire >= nWires; every error leaves nothing in flight.  The components
 * are found on the host (one walk over the outside wires' incidences); the elimination is k_r1cs_open_rref, one wave per
 * component, one launch per size class (<= 16, <= 32, <= 64 wires).  The constraint-side index and every buffer are made by the
 * first call and stay with the object (csrc/r1cs_open.h, csrc/r1cs_scan.hip). */
#define K16_OPEN_MAX_WIRES 64
enum { K16_OPEN_FIXED = 0, K16_OPEN_ABSENT = 1, K16_OPEN_FORCED = 2, K16_OPEN_FREE = 3, K16_OPEN_UNDECIDED = 4, K16_OPEN_SKIPPED = 5 };
int  k16_r1cs_open_system(k16_r1cs* r, const uint8_t* h_fixed, uint64_t* n_forced, uint64_t* n_free, uint64_t* n_undecided,
                          uint64_t* n_skipped, uint64_t* n_absent, uint64_t* n_components, uint64_t* n_dims, uint32_t* h_wires,
                          uint8_t* h_class, uint32_t cap, uint8_t* h_status /* n_wires bytes, may be NULL */,
                          uint32_t* h_comp /* n_wires words, may be NULL */);
int  k16_r1cs_open_direction(k16_r1cs* r, const uint8_t* h_fixed, uint32_t wire, uint8_t* cls, uint32_t* comp_wires,
                             uint32_t* comp_rows, uint32_t* comp_cross, uint32_t* rank, uint64_t* n, uint32_t* h_wires,
                             uint8_t* h_vals /* 32 B each */, uint32_t cap);

/* ---- the open-set solve with a wider cap: components of up to K16_OPEN_MAX_WIRES_EX wires ----
 * One multiplication between two hints glues their components together, and a component of more than K16_OPEN_MAX_WIRES wires is
 * SKIPPED by the calls above whatever its FORCED wires would be.  The _ex calls take the cap as an argument:
 *   max_wires   64 .. K16_OPEN_MAX_WIRES_EX.  Anything else is K16_ERR_ARG before anything is launched or written: every output
 *               keeps its bytes and the object keeps its check.  A component of more than max_wires wires is SKIPPED.
 * Definitions, classes, the canonical direction, preconditions, errors and threading are those of k16_r1cs_open_system and
 * k16_r1cs_open_direction, with "K16_OPEN_MAX_WIRES" read as max_wires; the remaining arguments are theirs, in their order.
 * max_wires == 64 runs their code and allocates nothing beyond it: every output byte is theirs (the convention of
 * k16_r1cs_determined_wires_ex).  k16_r1cs_open_direction_ex returns up to *comp_wires <= max_wires non-zeros; cap works as above.
 * The first call with max_wires > 64 adds, once per object, an arena of 144 MiB on the device (K16_ERR_NOMEM when the device has
 * not got it, as every other stage; the object and the 64-wire calls stay usable).  Components of 65 .. 128 and 129 .. 256 wires
 * are two more size classes, eliminated by k_r1cs_open_rref_wide: one workgroup of 128 / 256 threads per component, thread j
 * owning column j, the basis in a slab of the arena per workgroup (256 / 64 workgroups a launch, striding the components), a
 * fraction-free elimination -- no field inversion in k16_r1cs_open_system_ex; in k16_r1cs_open_direction_ex every pivot's thread
 * inverts its own pivot value at the same time (csrc/r1cs_scan.hip). */
#define K16_OPEN_MAX_WIRES_EX 256
int  k16_r1cs_open_system_ex(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint64_t* n_forced, uint64_t* n_free,
                             uint64_t* n_undecided, uint64_t* n_skipped, uint64_t* n_absent, uint64_t* n_components, uint64_t* n_dims,
                             uint32_t* h_wires, uint8_t* h_class, uint32_t cap, uint8_t* h_status /* n_wires bytes, may be NULL */,
                             uint32_t* h_comp /* n_wires words, may be NULL */);
int  k16_r1cs_open_direction_ex(k16_r1cs* r, const uint8_t* h_fixed, uint32_t max_wires, uint32_t wire, uint8_t* cls,
                                uint32_t* comp_wires, uint32_t* comp_rows, uint32_t* comp_cross, uint32_t* rank, uint64_t* n,
                                uint32_t* h_wires, uint8_t* h_vals /* 32 B each */, uint32_t cap);

/* ---- checked proving: every prove call carries the list of the constraints its witness breaks ----
 * k16_prover_set_r1cs attaches a circuit to a prover (NULL detaches; not owned, as k16_prover_set_vk: destroy it after the
 * prover, or detach first).  K16_ERR_ARG unless r lives on the prover's context, its nWires is the key's nVars and its number of
 * public wires the key's nPublic; k16_r1cs_match_zkey is the caller's to run.  From then on EVERY prove call (_mem, _compact,
 * _file, _file_timed and their _verified forms) runs the check of k16_r1cs_check_* on its own witness where it lies on the device,
 * on a stream the prover already has, behind the proof's last kernels (no stream is created); the call joins it before it
 * returns, on every path.  JSON, return value, *out_ok and out_proof are what they are without a circuit: a proof is still written for a
 * broken witness, the caller decides.  While attached, the object's per-check buffers are the prover's: no other check on it
 * while a prove call runs.  A prover without a circuit executes nothing of this.
 * k16_prover_last_check reports the check of the LAST prove call: *status = K16_CHECK_NONE after a call that failed, with
 * nothing attached, after attaching or detaching, or after the create-time warm-up; K16_CHECK_SATISFIED; K16_CHECK_BROKEN with the exact
 * *n_failed and, in h_failed (may be NULL), the lowest min(*n_failed, cap, K16_R1CS_REPORT_MAX) constraint numbers, ascending,
 * the same on every run; K16_CHECK_WITNESS_REFUSED where k16_r1cs_check_* answer K16_ERR_FORMAT (a value >= r, wire 0 != 1).
 * After SATISFIED or BROKEN, k16_r1cs_last_values on the attached object reads the sums of that call's witness; for more
 * than K16_R1CS_REPORT_MAX numbers call k16_r1cs_check_prover_witness. */
#define K16_R1CS_REPORT_MAX 64
enum { K16_CHECK_NONE = 0, K16_CHECK_SATISFIED = 1, K16_CHECK_BROKEN = 2, K16_CHECK_WITNESS_REFUSED = 3 };
int  k16_prover_set_r1cs(k16_prover* p, k16_r1cs* r);
int  k16_prover_last_check(const k16_prover* p, int* status, uint64_t* n_failed, uint32_t* h_failed, uint32_t cap);
/* Checked proving behind the drop-in FullProver.  r1cs_path: every pool slot parses the file into an R1CS object on its own
 * context and attaches it (a slot rebuilt after a device fault gets it again); NULL detaches.  The circuit is compared with the
 * zkey once (k16_r1cs_match_zkey): K16_ERR_FORMAT on a mismatch or an unreadable file, with the reason on stderr and nothing
 * attached -- the provers keep working unchecked.  K16_ERR_ARG while a slot is proving, K16_ERR_NO_DEVICE when the object is not
 * ready.  Once set, FullProver::prove, k16_fullprover_prove_mem and k16_fullprover_prove_compact answer a witness whose check is
 * BROKEN or WITNESS_REFUSED with ProverError::INVALID_INPUT / K16_ERR_FORMAT, with or without k16_fullprover_set_verify (with
 * both on, either one rejecting is enough).
 * k16_fullprover_last_rejection: what the CALLING THREAD's last prove through a FullProver was rejected for by the check --
 * copied out of the slot before it went back to the pool, kept per thread.  *status = K16_CHECK_NONE when that prove was not
 * rejected by the check (or the thread never proved); else BROKEN / WITNESS_REFUSED, *n_failed the exact count, h_failed (may be
 * NULL) the lowest min(*n_failed, cap, K16_R1CS_REPORT_MAX) numbers.  With K16_LOG=1 the same goes out as one JSON log line. */
int  k16_fullprover_set_r1cs(const void* fullprover, const char* r1cs_path);
int  k16_fullprover_last_rejection(uint64_t* n_failed, uint32_t* h_failed, uint32_t cap, int* status);

/* ---- set-up from a trapdoor: a valid proving key for any .r1cs, made on the GPU ----
 * WARNING: the key is DEVELOPMENT AND TEST MATERIAL.  Whoever holds the trapdoor can forge proofs.  A key whose trapdoor was
 * passed in, or drawn here and held in this process's memory, must never guard anything of value: production keys come from a
 * multi-party ceremony in which nobody ever knows tau, alpha, beta, gamma or delta.
 * k16_r1cs_setup* evaluate the circuit's QAP at tau on the device and write the snarkjs Groth16 zkey the prover reads (sections
 * 1 .. 10 in order; formulas and layout: csrc/setup_plan.h).  Section 10 carries a zero circuit hash and no
 * contribution; nothing in this project can test whether snarkjs itself loads the file.
 * trapdoor160: tau | alpha | beta | gamma | delta, 5 x 32 B little-endian standard form, each in [1, r).  NULL: the five values
 * are drawn from the OS CSPRNG the way a proof's r and s are.
 *   k16_r1cs_setup_size  the exact size of the key in bytes
 *   k16_r1cs_setup       into out_zkey[0 .. cap); *out_size = the key's size, also when K16_ERR_BUFFER says that cap is too small
 *   k16_r1cs_setup_file  into a file, written under a temporary name and renamed: an error leaves no partial file behind
 * K16_ERR_ARG: a trapdoor value of 0 or >= r; tau with tau^(2N) = 1 (tau lies in the evaluation domain or in its odd coset: a
 * Lagrange denominator or Z(tau) vanishes); a circuit with 0 constraints; an R1CS object of another context; 3 * nWires >= 2^32;
 * a domain above 2^27.  K16_ERR_IO: the file cannot be written, or the OS gives no random bytes.
 * k16_generator_mul: d_out[i] = scalar_i * G, the contract and the bytes of k16_synth_points_scalars (any 256-bit scalar, 32 B
 * little-endian standard form, on the device; affine Montgomery out, the all-zero point for a multiple of r), through a window
 * table of the generator that is built on the device on first use and freed with the context: ceil(256 / w) complete mixed
 * additions per point instead of a double-and-add walk, and one inversion per batch of points.  k16_generator_mul_info: w and
 * the number of windows of a group (K16_G1 / K16_G2).
 * THREADING: as k16_r1cs_check_*: one call at a time per object, on the context's stream, under the context's one-caller rule.
 * k16_r1cs_setup* return when the key is complete; k16_generator_mul enqueues (k16_sync waits).  Every error leaves nothing in
 * flight. */
int k16_r1cs_setup_size(const k16_r1cs* r, uint64_t* zkey_bytes);
int k16_r1cs_setup(k16_ctx* ctx, k16_r1cs* r, const uint8_t* trapdoor160, void* out_zkey, size_t cap, size_t* out_size);
int k16_r1cs_setup_file(k16_ctx* ctx, k16_r1cs* r, const uint8_t* trapdoor160, const char* zkey_path);
int k16_generator_mul(k16_ctx* ctx, int group, const void* d_scalars, uint64_t n, void* d_out_affine);
int k16_generator_mul_info(int group, unsigned* window_bits, unsigned* n_windows);

#ifdef __cplusplus
}
#endif
#endif
