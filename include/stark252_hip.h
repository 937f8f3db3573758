/* stark252_hip.h — C ABI of the MI355X (gfx950) STARK proving hot path for the lambdaworks Cairo prover.
 *
 * The reference (lambdaclass/lambdaworks_cairo_prover) has no FFI: `prove` (src/starks/prover.rs:532-766) calls
 * the lambdaworks-math / lambdaworks-crypto traits directly.  This header is what a Rust `extern "C"` block in
 * src/starks/prover.rs (or a replacement lambdaworks backend, like the existing `metal` feature, Cargo.toml:39)
 * binds; INTEGRATION.md shows the binding.  Each entry point cites the reference code it replaces.
 *
 * Conventions
 *   - return 0 (SP_OK) on success, a negative SP_E_* code otherwise; nothing aborts or throws across the ABI
 *     (the reference `unwrap()`s; a shim maps non-zero to ProvingError::WrongParameter, prover.rs:40-43).
 *   - field elements are contiguous 32-byte records in one of two encodings (sp_fe_encoding):
 *       SP_FE_MONT_LIMBS  4 x u64, limb 0 MOST significant, Montgomery form R = 2^256 — the in-memory layout of
 *                         lambdaworks `FieldElement<Stark252PrimeField>` (zero-copy from a Rust `&[FE]`);
 *       SP_FE_CANON_BE    canonical 32-byte big-endian (`to_bytes_be`, the proof wire format).
 *   - the caller owns every input/output buffer; a context owns its device memory; calls on one context are
 *     serial (the round structure is sequential); different contexts may be used from different threads.
 *   - host pointers unless a parameter is named *_dev.
 */
#ifndef STARK252_HIP_H
#define STARK252_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SP_OK = 0,
    SP_E_INVALID_ARG = -1,   /* null pointer, non power-of-two size, unknown enum */
    SP_E_NO_DEVICE = -2,     /* no gfx950 device visible / HIP runtime unusable */
    SP_E_HIP = -3,           /* a HIP call failed; see sp_last_error() */
    SP_E_ALLOC = -4,
    SP_E_STATE = -5,         /* round called out of order */
    SP_E_ZERO_INVERSE = -6,  /* batch inverse of a zero element (lambdaworks panics) */
    SP_E_UNSUPPORTED = -7,
    SP_E_PROGRAM = -8        /* Cairo front-end: undecodable instruction, missing memory cell, step limit */
};

typedef enum { SP_FE_MONT_LIMBS = 0, SP_FE_CANON_BE = 1 } sp_fe_encoding;

/* ProofOptions — reference src/starks/proof/options.rs:21-26 */
typedef struct {
    uint8_t blowup_factor;            /* a power of two, 2 .. 128 (the reference's u8); n x blowup <= 2^30 */
    uint64_t fri_number_of_queries;
    uint64_t coset_offset;
    uint8_t grinding_factor;
} sp_proof_options;
/* The presets and checked constructors of the same file (host arithmetic, no device): SecurityLevel (options.rs:5-12),
 * ProofOptions::new_secure (:35-75; every level: blowup 4, grinding 20, queries 31 / 41 / 55 conjecturable, 80 / 104 / 140 provable),
 * new_with_checked_security (:78-102) and new_with_checked_provable_security (:107-129) - restated as the reference computes them,
 * including the latter's use of the u8's LEADING zeros - for a field of `field_bits` bits (252 for Stark252; the reference is generic
 * over the field: F::field_bit_size()).  InsecureOptionError (errors.rs) comes back as SP_E_INVALID_ARG with sp_last_error() =
 * "InsecureOptionError::FieldSize" (field_bits <= security_target + 40) or "InsecureOptionError::SecurityBits". */
typedef enum { SP_SEC_CONJECTURABLE_80 = 0, SP_SEC_CONJECTURABLE_100 = 1, SP_SEC_CONJECTURABLE_128 = 2,
               SP_SEC_PROVABLE_80 = 3, SP_SEC_PROVABLE_100 = 4, SP_SEC_PROVABLE_128 = 5 } sp_security_level;
int sp_proof_options_new_secure(int security_level, uint64_t coset_offset, sp_proof_options* out);
int sp_proof_options_checked(uint8_t blowup_factor, uint64_t fri_number_of_queries, uint64_t coset_offset, uint8_t grinding_factor,
                             uint8_t security_target, int provable, uint32_t field_bits, sp_proof_options* out);

typedef struct {
    int device;        /* HIP device ordinal */
    int fe_encoding;   /* sp_fe_encoding of every field-element buffer crossing the ABI on this context */
} sp_config;

typedef struct sp_ctx sp_ctx;

/* Blocking all-gather hook for coset sharding across GPUs: every rank contributes `bytes_per_rank` bytes at send_dev
 * (device memory) and receives world*bytes_per_rank bytes at recv_dev, rank-major. Must have completed when it returns. */
typedef int (*sp_allgather_fn)(void* user, const void* send_dev, void* recv_dev, uint64_t bytes_per_rank);

const char* sp_version(void);
/* Version of this header: bumped whenever a structure (sp_air_desc, sp_openings, sp_cairo_public_inputs, sp_proof_options) changes
 * layout, an entry point or option key is added, or a call changes meaning (4: round 5's sp_comm_measure / sp_comm_time_ms /
 * sp_proof_options_* / sp_proof_file_verify / SP_OPT_HOST_RANKS family and sp_set_collective keeping the prover across re-installs
 * of the same world; 5: sp_fe_mul; 6: sp_air_limits, sp_air_prove beyond 64 columns and 3 boundary rows; 7: sp_air_prove_aux, sp_air_aux_desc,
 * sp_air_aux_desc_size, sp_air_prove_periodic, sp_air_verify_periodic, sp_air_periodic_desc_size, sp_air_periodic_limits,
 * sp_air_periodic_eval, sp_air_periodic_lde; sp_air_check_trace and sp_air_violation_size joined under 7 - they change no structure
 * and no call, and a binding finds a build without them by probing the symbols; so did sp_air_prove_ext, sp_air_verify_ext, sp_air_check_trace_ext,
 * sp_air_stride_size, sp_air_stride_desc_size, sp_air_ext_size, sp_air_stride_limits, sp_air_stride_eval and sp_air_stride_table, and after them sp_air_prove_pub, sp_air_verify_pub,
 * sp_air_check_trace_pub, sp_air_boundary_desc_size and sp_air_boundary_resolve, and then sp_air_prove_main, sp_air_check_trace_main,
 * sp_air_main_trace, sp_air_main_check and sp_air_main_desc_size, then sp_air_prove_rec, sp_air_check_trace_rec, sp_air_main_trace_rec,
 * sp_air_main_check_rec and sp_air_main_chain_limits, then sp_air_prove_lk, sp_air_check_trace_lk, sp_air_main_trace_lk, sp_air_main_check_lk
 * and sp_air_main_count_limits, then sp_air_prove_link, sp_air_check_trace_link, sp_air_main_trace_link, sp_air_main_check_link and
 * sp_air_main_link_limits, then sp_air_prove_div, sp_air_check_trace_div, sp_air_main_trace_div and sp_air_main_check_div, then
 * sp_air_prove_fetch, sp_air_check_trace_fetch, sp_air_main_trace_fetch, sp_air_main_check_fetch and sp_air_main_fetch_limits, and last
 * sp_air_prove_word, sp_air_check_trace_word, sp_air_main_trace_word, sp_air_main_check_word and sp_air_main_word_limits, and after them
 * sp_air_prove_int, sp_air_check_trace_int, sp_air_main_trace_int, sp_air_main_check_int and sp_air_main_int_limits, and last
 * sp_air_prove_multi, sp_air_check_trace_multi, sp_air_main_trace_multi, sp_air_main_check_multi and sp_air_main_multi_limits, and after them sp_lde_dev,
 * sp_intt_bitrev_dev and sp_ntt_plan).  A binding compares it (and sp_air_desc_size against its own idea of the struct) when it loads the library, so
 * a stale build fails at load time with "rebuild the library" instead of with a missing symbol or shifted fields later. */
#define SP_ABI_VERSION 7
int sp_abi_version(void);
uint64_t sp_air_desc_size(void);
const char* sp_last_error(void);          /* thread-local description of the last failure */
int sp_device_count(int* count_out);      /* number of visible HIP devices (0 without a GPU) */
/* CPUs the host side of the library may really use: hardware threads cut down by the affinity mask and the cgroup CPU quota
 * (what sizes the gather threads of sp_cairo_prove and the front-end's trace builder). */
int sp_host_cpus(int* count_out);
/* This process' share of them: sp_host_cpus / the ranks sharing the host (SP_OPT_HOST_RANKS, see sp_set_option), at least 1 - the
 * figure every host-side thread count is derived from.  ranks_out (optional): the rank count in force. */
int sp_host_cpu_budget(int* budget_out, int* ranks_out);
/* NUMA placement on multi-socket hosts: restricts the CALLING THREAD - and every thread it creates afterwards - to the CPUs of the
 * NUMA node the device hangs off (within the affinity mask it already has), so that the tables a prover process builds are
 * first-touched on that node: the page-locked staging of the host-buffer entry points lives there, and a table on the other node
 * crosses the socket link on its way in (sp_cairo_prove from a far table: 37 - 43 GB/s instead of 52 - 56).  The equivalent of
 * `numactl --cpunodebind=<node of the GPU>`; call it first thing in a one-process-per-GPU prover.  *node_out (nullable): the node,
 * -1 when it is unknown (single-node host, no sysfs, no device) - nothing is changed then.  Touches the HIP runtime (the device's PCI
 * address), creates no context. */
int sp_host_bind_to_device(int device, int* node_out);

int sp_ctx_create(sp_ctx** ctx_out, const sp_config* cfg);
void sp_ctx_destroy(sp_ctx* ctx);

/* ---- multi-GPU: one process and one context per GPU; the LDE cosets are sharded over `world` ranks
 * (world a power of two; beyond the blowup factor the surplus ranks are replicas). Every rank calls the same sequence (sp_cairo_prove or the round-level calls)
 * with the same inputs and obtains the same roots / proof bytes. The data-path exchanges are all-gathers of 32-byte leaf
 * digests, composition evaluations and DEEP evaluations; everything else is local. Either install a hook ... */
int sp_set_collective(sp_ctx* ctx, int world, int rank, sp_allgather_fn fn, void* user);
/* (Re-installing with the SAME world - another rank, other hooks - keeps the prover's device arena: the next proof re-carves it for the new
 * rank; a different world releases it.  Every installation resets the optional hooks below: install them again afterwards.) */
/* ... or let the library own an RCCL communicator (ncclAllGather on the context stream over xGMI): rank 0 obtains a 128-byte
 * id with sp_comm_unique_id and distributes it out of band (e.g. torch.distributed broadcast); every rank then calls
 * sp_comm_init_rccl with it. */
int sp_comm_unique_id(uint8_t id_out[128]);
int sp_comm_init_rccl(sp_ctx* ctx, const uint8_t id[128], int world, int rank);
/* Optional stream-ordered all-gather (same layout as sp_allgather_fn): enqueue the exchange on `hip_stream` (a hipStream_t) and
 * return without waiting.  With it the sharded prover splits the coefficient all-gather of a trace segment into column blocks on a
 * stream of its own, so that the exchange of one block runs beside the inverse transforms of the next and the LDE of the one
 * before (prover.rs:161-185 has no such dependency between columns).  sp_comm_init_rccl installs it (ncclAllGather on that
 * stream); the blocking hook stays in use for every other exchange.  Call after sp_set_collective. */
typedef int (*sp_allgather_async_fn)(void* user, const void* send_dev, void* recv_dev, uint64_t bytes_per_rank, void* hip_stream);
int sp_set_collective_async(sp_ctx* ctx, sp_allgather_async_fn fn);
/* Timing-only transport for projections on fewer GPUs than ranks (bench.py --project-ranks): nothing is exchanged - the own block
 * lands where a collective would put it, the other ranks' blocks are zero-filled (the HBM writes a receive costs) - so ONE rank's
 * share of a sharded proof runs at its real kernel sizes.  The proof bytes that come out are meaningless; never use it to prove. */
int sp_comm_init_null(sp_ctx* ctx, int world, int rank);
/* Optional second hook ("Merkle combine"): blocking all-to-all of equal blocks, send_dev =
 * [world][bytes_per_pair] (block d goes to rank d), recv_dev = [world][bytes_per_pair] (block s came from rank s).  With it
 * the 32-byte leaf digests of a commitment travel once (each rank receives only the contiguous 1/world of the leaves whose
 * subtree it reduces); without it the prover falls back to an all-gather of the digests.  sp_comm_init_rccl installs both
 * (grouped ncclSend/ncclRecv on the context stream).  Call after sp_set_collective. */
typedef int (*sp_alltoall_fn)(void* user, const void* send_dev, void* recv_dev, uint64_t bytes_per_pair);
int sp_set_alltoall(sp_ctx* ctx, sp_alltoall_fn fn);
/* Stream-ordered form of the all-to-all (same layout as sp_alltoall_fn), optional: with it AND sp_set_collective_async the digest
 * exchange and the root all-gather of a commitment are enqueued on the prover's compute stream between the kernels that produce and
 * consume them instead of each costing a host round trip, and the FRI commit phase runs through its sharded layers without any - the
 * launch that finishes a layer's top tree takes the transcript step on the device (fri/mod.rs:37-67 is one dependent chain).
 * sp_comm_init_rccl installs it (grouped ncclSend / ncclRecv on the stream it is given).  Call after sp_set_collective. */
typedef int (*sp_alltoall_async_fn)(void* user, const void* send_dev, void* recv_dev, uint64_t bytes_per_pair, void* hip_stream);
int sp_set_alltoall_async(sp_ctx* ctx, sp_alltoall_async_fn fn);
/* Collective traffic of this context since creation: out = {world, all-gather calls, bytes contributed to all-gathers,
 * all-to-all calls, bytes sent in all-to-alls, bytes received in all collectives}. */
int sp_comm_stats(sp_ctx* ctx, uint64_t out[6]);
/* ... and how long they took, in ms since creation: out = {stream-ordered collectives - an event pair around each on the stream it was
 * enqueued on, i.e. what the exchange occupied that stream for, the wait for the slowest peer included -, blocking collectives - wall
 * clock around the hook}.  Synchronizes the device. */
int sp_comm_time_ms(sp_ctx* ctx, double out[2]);
/* Checks the installed transport (RCCL or hooks): one all-gather and, if installed, one all-to-all of rank-stamped blocks of
 * bytes_per_block bytes (a multiple of 8); every rank must call it.  0 = both deliver the layout documented above. */
int sp_comm_selftest(sp_ctx* ctx, uint64_t bytes_per_block);
/* Times the installed transport - every rank must call it: all-gathers and (if installed) all-to-alls of bytes_per_rank bytes per
 * rank, one untimed of each and then three timed ones whose MEDIAN counts.  out = {all-gather ms, its GB/s per link and direction,
 * all-to-all ms, its GB/s per link and direction, bytes per rank, world}: what a rank received from the others / time / (world - 1)
 * links - the unit of SP_OPT_LINK_GBS - as the MINIMUM over the ranks, so every rank holds the same figures.
 * SP_OPT_SHARD_INTERPOLATION = 2 decides from the all-gather's rate DIVIDED BY SP_LINK_MEASURED_MARGIN (a measured figure near the
 * threshold must not flip the mode from run to run) unless the caller stated SP_OPT_LINK_GBS.  sp_comm_init_rccl runs it once
 * (64 MB per rank; environment SP_COMM_MEASURE_MB, 0 = not at all).  bytes_per_rank = 0: only read the stored figures back (zeros
 * when nothing was measured).  The outcome is agreed between the ranks: everything local (payload buffers, events) is prepared
 * before the first collective, a status word per rank goes round on every path, and a rank that could not prepare or could not time
 * its collectives makes EVERY rank drop the figures and return non-zero - the ranks never end up with different rates, hence never
 * with different interpolation modes. */
#define SP_LINK_MEASURED_MARGIN 1.25
int sp_comm_measure(sp_ctx* ctx, uint64_t bytes_per_rank, double out[6]);
/* The decision rule of SP_OPT_SHARD_INTERPOLATION = 2 as a pure function: 1 when interpolating a trace segment by column (+ an
 * all-gather of the coefficients) beats interpolating every column on every rank - 64 x 1.35e11 < (groups - 1) x link x log2(rows):
 * the butterfly rate of one MI355X against what groups - 1 links deliver. */
int sp_model_shard_interpolation(double link_gbs_per_direction, uint32_t groups, uint32_t log2_rows);
/* Tuning knobs of the sharded prover (defaults in parentheses):
 *   SP_OPT_FRI_SHARD_MIN_LOG (16)  FRI layers with at least 2^value leaves keep their evaluations and trees sharded; smaller
 *                                  layers are all-gathered once and continue replicated (fri/mod.rs:20-72 is sequential in the layers);
 *   SP_OPT_SHARD_INTERPOLATION (2) 1: the size-n inverse transforms of a trace segment are split by column over the ranks and the
 *                                  coefficients all-gathered (prover.rs:161-185, trace.rs:104-110); 0: every rank interpolates all columns;
 *                                  2: whichever is faster for the shape on the link model - a rank saves (1 - 1/G) of the inverse transforms
 *                                  and receives (1 - 1/G) of the coefficients, which pays when (G - 1) x link rate x log2 n > 64 x 1.35e11.
 *   SP_OPT_LINK_GBS (46)           GB/s one xGMI link delivers per direction, for that decision.  Unset: the rate sp_comm_measure found
 *                                  (sp_comm_init_rccl measures once per communicator), else 46 (76.8 GB/s x an assumed 0.6).
 *   SP_OPT_UPLOAD_THREADS (24)     host threads that gather the column groups of a row-major host trace into pinned memory
 *                                  (sp_cairo_prove / sp_commit_trace from host buffers above 64 MB).
 *   SP_OPT_HOST_RANKS (env)        how many ranks (processes, one context and GPU each) share this HOST.  Process-wide.  Every host thread
 *                                  count of the library is a share of the CPUs the process may use (affinity mask, cgroup quota) divided by
 *                                  this: the gather pool is min(SP_OPT_UPLOAD_THREADS, 2 x CPUs / ranks), the front-end's loops CPUs / ranks;
 *                                  with more ranks than CPUs the Fiat-Shamir waits block instead of polling.  Default: the environment -
 *                                  SP_HOST_RANKS, else LOCAL_WORLD_SIZE (what torch.distributed.run exports), else 1.  0 = back to that.
 *   SP_OPT_MERKLE_BACKEND (SP_MERKLE_KECCAK256)  the hash of every commitment of the context (trace, composition and FRI trees,
 *                                  sp_merkle_build*).  SP_MERKLE_KECCAK256 is the reference's configuration (src/starks/config.rs:10-20)
 *                                  and the only one whose proofs the reference verifies.  SP_MERKLE_POSEIDON (BASELINE.json configs[4]; NO
 *                                  reference counterpart at the pinned revision) is Starknet's Poseidon over Stark252 as later lambdaworks
 *                                  versions configure it: digest = the canonical 32-byte big-endian element, node = hash(left, right),
 *                                  leaf of a row of columns = hash_many(row), leaf of a single-element tree (FRI layers) =
 *                                  hash_single(x).  Transcript and grinding stay Keccak; the proof layout does not change.
 *                                  Such proofs are checked with sp_cairo_verify_backend / sp_air_verify_backend.
 *   SP_OPT_DEVICE_TRACE (1)        sp_cairo_prove_run builds the main trace ON THE DEVICE from the run's register states and memory
 *                                  (build_main_trace, src/cairo/execution_trace.rs:57-87: 24 B per step + 32 B per memory cell cross
 *                                  PCIe instead of the n x cols table); 0: the run's host table goes up column group by column group.
 *   SP_OPT_MERKLE_ONE_COLUMN_ROWS (0)  which Poseidon tree sp_merkle_build / sp_merkle_build_dev build for fe_per_leaf == 1: 0 the
 *                                  single-element tree of a FRI layer (leaf = hash_single(x), fri_commitment.rs:39), 1 the tree over
 *                                  rows of ONE column (leaf = hash_many over one element) - what the prover commits a one-column trace
 *                                  segment with (prover.rs:96-104 batch_commit).  Keccak256 trees have one leaf form; no effect there. */
enum { SP_OPT_FRI_SHARD_MIN_LOG = 1, SP_OPT_SHARD_INTERPOLATION = 2, SP_OPT_UPLOAD_THREADS = 3, SP_OPT_MERKLE_BACKEND = 4, SP_OPT_MERKLE_ONE_COLUMN_ROWS = 5,
       SP_OPT_DEVICE_TRACE = 6, SP_OPT_LINK_GBS = 7, SP_OPT_HOST_RANKS = 8 };
enum { SP_MERKLE_KECCAK256 = 0, SP_MERKLE_POSEIDON = 1 };
int sp_set_option(sp_ctx* ctx, int key, int64_t value);

/* ---- fine-grained layer: the lambdaworks seam the reference calls ------------------------ */

/* Natural-order DFT of n = 2^k elements, in place.
 *   inverse == 0, coset == NULL : Polynomial::evaluate_fft                           (data = coefficients)
 *   inverse == 0, coset != NULL : evaluate_offset_fft(1, None, coset)  (prover.rs:117, fri_commitment.rs:36)
 *   inverse != 0, coset == NULL : Polynomial::interpolate_fft                         (trace.rs:107)
 *   inverse != 0, coset != NULL : Polynomial::interpolate_offset_fft  (constraints/evaluation_table.rs:32)
 * `coset` is one field element in the context's encoding. */
int sp_ntt(sp_ctx* ctx, uint8_t* data, uint64_t n, int inverse, const uint8_t* coset);

/* Batched variant on device memory: `batch` vectors of n elements each, vector v at data_dev + v*n*32,
 * elements in the DEVICE layout (8 x u32 little-endian Montgomery, see sp_fe_to_device). Used by bench.py so the
 * timed region starts with inputs resident in HBM. Asynchronous on the context stream; sp_sync() to wait. */
int sp_ntt_dev(sp_ctx* ctx, void* data_dev, uint64_t n, uint32_t batch, int inverse, const uint8_t* coset);

/* evaluate_polynomial_on_lde_domain (prover.rs:106-123) for `cols` polynomials of n coefficients each
 * (column-major: column j at coeffs + j*n*32): out column j holds n*blowup evaluations p_j(coset * w_N^i). */
int sp_lde(sp_ctx* ctx, const uint8_t* coeffs, uint64_t n, uint32_t cols, uint32_t blowup, const uint8_t* coset,
           uint8_t* out);

/* ---- the transform drivers as the prover itself calls them, on device memory (tests compare them element by element) ----
 * All three are asynchronous on the context stream like sp_ntt_dev, take buffers in the DEVICE layout and strides in ELEMENTS, and
 * validate every argument before the first launch: SP_E_INVALID_ARG for a size that is no power of two, n * blowup beyond 2^30,
 * shard_log > log2(blowup), shard_rank >= 2^shard_log, a stride shorter than the array it separates, a null buffer, cols / batch of 0
 * or beyond what one launch holds, and source and destination extents that overlap (src == data included).  Nothing is launched then.
 *
 * sp_lde_dev: the low-degree extension of `cols` polynomials from their bit-reversed, h-scaled coefficients - entry pos of column v, at
 * coeffs_dev + (v * src_stride + pos) * 32, holds c_rev(pos) * h^rev(pos) (rev over log2 n bits), what sp_intt_bitrev_dev leaves with
 * post_table[pos] = h^rev(pos) / n.  With b_loc = blowup >> shard_log the rank computes the cosets c = c_loc * 2^shard_log + shard_rank,
 * c_loc < b_loc, and column v of the output starts at out_dev + v * dst_stride * 32 (dst_stride >= n * b_loc):
 *   order SP_LDE_NATURAL (NttEngine::lde_from_bitrev):      element q * b_loc + c_loc = p_v(h w_N^(q * blowup + c)), q < n;
 *   order SP_LDE_COSET_MAJOR (NttEngine::lde_coset_major):  element c_loc * n + m     = p_v(h w_N^(m * blowup + c)), m < n.
 * sp_intt_bitrev_dev (NttEngine::dif_natural_to_bitrev_inverse): `batch` vectors of n natural-order evaluations at data_dev + v * stride
 * * 32, in place: position pos receives post_table_dev[pos] * n * c_rev(pos), c = the interpolating coefficients (the transform is
 * unscaled; post_table_dev - n entries, shared by the vectors - usually carries the 1 / n), canonical.  post_table_dev NULL: no
 * factor.  src_dev non-NULL: read the evaluations from that array (same stride) and leave it untouched. */
enum { SP_LDE_NATURAL = 0, SP_LDE_COSET_MAJOR = 1 };
int sp_lde_dev(sp_ctx* ctx, const void* coeffs_dev, void* out_dev, uint64_t n, uint32_t blowup, uint32_t cols, uint64_t src_stride,
               uint64_t dst_stride, int order, uint32_t shard_log, uint32_t shard_rank);
int sp_intt_bitrev_dev(sp_ctx* ctx, void* data_dev, uint64_t n, uint32_t batch, uint64_t stride, const void* post_table_dev,
                       const void* src_dev);
/* The pass list a transform driver launches, from the code that launches it (csrc/ntt.hip ntt_plan), without a context or a GPU:
 * driver = SP_NTT_DRIVER_*, 2^k elements per vector, blowup 2^logb and 2^shard_log shards (both 0 unless the driver is one of the two
 * LDEs), `batch` vectors.  Up to `cap` passes are written to out (nullable) in execution order, *count_out (required) receives how
 * many the driver launches; SP_E_INVALID_ARG for an unknown driver, k + logb > 30, shard_log > logb, batch 0 and cap < count. */
enum { SP_NTT_DRIVER_FORWARD_NATURAL = 0, SP_NTT_DRIVER_INVERSE_NATURAL = 1, SP_NTT_DRIVER_DIT_BITREV_TO_NATURAL = 2,
       SP_NTT_DRIVER_INTT_BITREV = 3, SP_NTT_DRIVER_LDE_NATURAL = 4, SP_NTT_DRIVER_LDE_COSET_MAJOR = 5 };
typedef struct {
    uint32_t dif;          /* 1: decimation in frequency with inverse roots, 0: decimation in time */
    uint32_t load, store;  /* load: 0 in place, 1 bit-reversal gather, 2 expand (replicated LDE input); store: 0 in place, 1 bit-reversal scatter */
    uint32_t contig, gtw;  /* contiguous tile; twiddles from the transform's table (0: the pass-local table) */
    uint32_t s, r, g;      /* LOCAL stride 2^s, 2^r rows, 2^g adjacent elements per row */
    uint32_t radix4;       /* stages run in pairs (1024-element tiles with r >= 2) */
    uint32_t xcd_map;      /* work-groups dealt to the XCDs by tile */
    uint32_t weak_out;     /* stores values below 2p (every pass but the last) */
    uint32_t stage_tw;     /* reads per-stage twiddle tables where the context could allocate them */
    uint32_t log_len;      /* log2 of the array the pass addresses */
    uint32_t tiles;        /* work-groups per vector */
    uint32_t vectors;      /* vectors per launch (columns x local cosets in the coset-major LDE) */
    uint32_t coset_count;  /* coset-major LDE: local cosets per column, else 0 */
} sp_ntt_pass;
int sp_ntt_plan(int driver, uint32_t k, uint32_t logb, uint32_t shard_log, uint32_t batch, sp_ntt_pass* out, uint32_t cap, uint32_t* count_out);

/* MerkleTree::<BatchKeccak256Tree|Keccak256Tree>::build (prover.rs:96-104, fri_commitment.rs:39; backends
 * config.rs:10-20): n_leaves rows of fe_per_leaf elements (row-major); leaf = Keccak256(row as 32-byte BE
 * elements), parent = Keccak256(left || right). nodes_out (nullable) receives all 2n-1 nodes, root first,
 * children of i at 2i+1 and 2i+2 (the lambdaworks node order).
 * With SP_OPT_MERKLE_BACKEND = SP_MERKLE_POSEIDON: fe_per_leaf = 1 builds the single-element tree (leaf = hash_single),
 * fe_per_leaf > 1 the tree over rows (leaf = hash_many); the same holds for sp_merkle_build_dev. */
int sp_merkle_build(sp_ctx* ctx, const uint8_t* leaves, uint64_t n_leaves, uint32_t fe_per_leaf,
                    uint8_t root_out[32], uint8_t* nodes_out);

/* MerkleTree::build (prover.rs:96-104 batch_commit, fri_commitment.rs:39) on device memory, for bench.py and callers that
 * already hold the evaluations in HBM: `fe_per_leaf` columns in the DEVICE layout, column j at cols_dev + j*col_stride*32,
 * leaf i = Keccak-256 of the canonical big-endian encodings of column 0..fe_per_leaf-1 at row i.  nodes_dev receives the
 * 2*n_leaves - 1 digests in lambdaworks order (root first).  Asynchronous on the context stream; sp_sync() to wait. */
int sp_merkle_build_dev(sp_ctx* ctx, const void* cols_dev, uint64_t n_leaves, uint32_t fe_per_leaf, uint64_t col_stride,
                        void* nodes_dev);

/* FieldElement::inplace_batch_inverse (constraints/evaluator.rs:69,171; cairo/air.rs:540,561). */
int sp_batch_inverse(sp_ctx* ctx, uint8_t* data, uint64_t n);
/* FieldElement<Stark252PrimeField> Mul / square on the device (src/lib.rs:12-13; every product of the path, e.g. cairo/air.rs:525-572,
 * constraints/evaluator.rs:142-154): out[i] = a[i] * b[i] for n elements in the context's encoding; b == NULL squares a.  The kernels'
 * own Montgomery product and square (csrc/fp.h) on caller-chosen operands - what the parity tests drive with adversarial limbs (with
 * SP_FE_MONT_LIMBS the limbs go to the multiplier as they are). */
int sp_fe_mul(sp_ctx* ctx, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out);

/* Encoding helpers between the ABI encodings and the device layout (host side, no GPU needed). */
int sp_fe_to_device(int fe_encoding, const uint8_t* in, uint64_t n, uint8_t* out_device_layout);
int sp_fe_from_device(int fe_encoding, const uint8_t* in_device_layout, uint64_t n, uint8_t* out);

int sp_sync(sp_ctx* ctx);
/* Duration in milliseconds of the kernels launched by the last sp_*_dev call, measured with HIP events on the context
 * stream; waits for that call to finish. */
int sp_last_kernel_ms(sp_ctx* ctx, float* ms_out);
/* HIP-event timer on the context stream around any sequence of asynchronous calls: sp_timer_start records an event,
 * sp_timer_stop records a second one, waits for it and returns the elapsed device time in milliseconds. bench.py
 * brackets its timed region with these, so the per-launch figure contains no host round trips. */
int sp_timer_start(sp_ctx* ctx);
int sp_timer_stop(sp_ctx* ctx, float* ms_out);

/* PublicInputs — reference src/cairo/air.rs:163-181 (HashMaps flattened to arrays). Field elements in
 * SP_FE_CANON_BE regardless of the context encoding. */
typedef struct {
    uint8_t pc_init[32], ap_init[32], fp_init[32], pc_final[32], ap_final[32];
    uint16_t range_check_min, range_check_max;
    uint32_t n_segments;
    const uint8_t* segment_types;      /* 0 = RangeCheck, 1 = Output */
    const uint64_t* segment_ranges;    /* (start, end) pairs */
    uint64_t n_public_memory;
    const uint8_t* public_memory;      /* (address, value) pairs, 64 bytes each */
    uint64_t num_steps;
} sp_cairo_public_inputs;

/* ---- round-level layer: one call per prover round; the Fiat-Shamir transcript stays with the
 * caller (it is sequential Keccak over < 10 KB): roots go out, challenges come in. Field elements in the context
 * encoding. Call order: sp_prove_setup, sp_commit_trace(0), [sp_commit_trace(1)], sp_composition, sp_ood,
 * sp_deep_fri_commit_begin, sp_fri_fold_commit x log2(n), sp_grind, sp_open; out-of-order calls return SP_E_STATE. */

/* A::new + Domain::new (reference src/starks/prover.rs:549-551, src/starks/domain.rs:20-56): sizes the device buffers
 * for a trace of n rows (power of two), main_cols + aux_cols columns. has_rc_builtin selects the 61-column Cairo layout. */
int sp_prove_setup(sp_ctx* ctx, uint64_t n, uint32_t main_cols, uint32_t aux_cols, int has_rc_builtin, const sp_proof_options* opt);

/* Pre-warm for the reference's one-proof-per-process shape (src/main.rs:85-108: run the VM, prove once, exit): call it - on a
 * thread of its own, or before the VM starts - while the trace does not exist yet, with the shape the proof will have.  It does
 * sp_prove_setup's work and everything else a first proof would otherwise pay on its critical path:
 *   SP_PREWARM_KERNELS    a small valid Cairo proof (2^13 rows) from a device-built trace and the commitment of the same trace through
 *                         the three other input forms, on this context: the first launch of every kernel family, the side streams, the
 *                         auxiliary-trace workspace;
 *   SP_PREWARM_CLOCKS     round 1's kernels at the REAL shape on the arena's contents, column slice by column slice: the size-specific
 *                         kernel variants, and the device at its clocks when the trace arrives (sp_prewarm_cancel ends it early);
 *   SP_PREWARM_HOST_ROWS  the page-locked ring and the parked gather threads of the row-major entry points (sp_cairo_prove,
 *                         sp_commit_trace from host tables above 64 MB).
 * flags = 0 means all of them.  The proof that follows (any entry point, same n / columns / blowup / coset offset) then costs what a
 * warm one does; its bytes are not affected.  With several ranks every rank calls it (the small proofs are sharded proofs). */
enum { SP_PREWARM_KERNELS = 1, SP_PREWARM_CLOCKS = 2, SP_PREWARM_HOST_ROWS = 4, SP_PREWARM_ALL = 7 };
int sp_prewarm(sp_ctx* ctx, uint64_t n, uint32_t main_cols, uint32_t aux_cols, int has_rc_builtin, const sp_proof_options* opt, uint32_t flags);
/* Callable from ANY thread: asks the sp_prewarm that runs on this context - or the next one, if none does yet - to return as soon as it
 * can.  Everything a first proof needs (arena, plumbing, first launches) is still done; the clock ramp (SP_PREWARM_CLOCKS: round 1 at the
 * real shape, column slice by column slice) stops behind the slice in flight.  The intended use: start sp_prewarm on a thread, run the VM,
 * call sp_prewarm_cancel when the trace exists, join the thread, prove - the ramp then lasts exactly as long as the VM did.  A request
 * that finds no prewarm to stop is dropped by the next proof on the context. */
int sp_prewarm_cancel(sp_ctx* ctx);

/* interpolate_and_commit (prover.rs:126-159): rows = row-major n x cols trace segment (0 main, 1 auxiliary).
 * iNTT + LDE + batched Keccak Merkle tree; keeps polynomials, LDE and tree on the device. */
int sp_commit_trace(sp_ctx* ctx, int segment, const uint8_t* rows, uint64_t n, uint32_t cols, uint8_t root_out[32]);

/* The same from host COLUMNS - what interpolate_and_commit itself starts from (`trace.cols()`, prover.rs:130, trace.rs:23-31):
 * column j of the segment at cols + j*col_stride*32 (col_stride in elements, 0 = n); device_layout != 0: elements in the DEVICE
 * layout, 0: context encoding.  One DMA per column group, no host-side gather (see sp_cairo_prove_columns, sp_host_alloc). */
int sp_commit_trace_columns(sp_ctx* ctx, int segment, const uint8_t* cols, uint64_t n, uint32_t n_cols, uint64_t col_stride,
                            int device_layout, uint8_t root_out[32]);

/* CairoAIR::build_auxiliary_trace + interpolate_and_commit of the auxiliary segment, entirely on the device
 * (reference src/cairo/air.rs:660-729, src/starks/prover.rs:199-213): rap = alpha_memory, z_memory, z_range_check
 * sampled by the caller after the main root. Requires sp_commit_trace(0) of a Cairo main trace (34|43 columns). */
int sp_cairo_commit_aux(sp_ctx* ctx, const uint8_t* rap, const sp_cairo_public_inputs* pub, uint8_t root_out[32]);

/* BoundaryConstraint (reference src/starks/constraints/boundary.rs:13-17) */
typedef struct { uint32_t col; uint64_t step; uint8_t value[32]; } sp_boundary_constraint;

/* round_2_compute_composition_polynomial (prover.rs:226-286) for the Cairo AIR: rap = 3 RAP challenges (alpha_memory,
 * z_memory, z_range_check); coeffs = alpha^B (n_boundary), beta^B (n_boundary), alpha^T (n_transitions),
 * beta^T (n_transitions), in the order prover.rs:597-615 samples them. Returns the [H1],[H2] root. */
int sp_composition(sp_ctx* ctx, const uint8_t* rap, const sp_boundary_constraint* boundary, uint32_t n_boundary,
                   const uint8_t* coeffs, uint32_t n_transitions, uint8_t root_out[32]);

/* round_3 (prover.rs:288-325): out = H1(z^2), H2(z^2), then t_j(z g^k) row-major [k][j], k = 0,1: (2 + 2C) elements. */
int sp_ood(sp_ctx* ctx, const uint8_t z[32], uint8_t* out);

/* compute_deep_composition_poly + first FRI layer (prover.rs:347-378, fri/mod.rs:27-33): gammas = gamma, gamma',
 * then the 2C trace gammas (index j*2 + k). */
int sp_deep_fri_commit_begin(sp_ctx* ctx, const uint8_t* gammas, uint8_t root0_out[32]);

/* One FRI fold + commitment (fri/mod.rs:37-67). While *is_last == 0 the output is the next layer's Merkle root; the
 * log2(n)-th call sets *is_last = 1 and outputs fri_last_value (one field element) instead. */
int sp_fri_fold_commit(sp_ctx* ctx, const uint8_t zeta[32], uint8_t root_or_last_out[32], int* is_last);

/* generate_nonce_with_grinding (reference src/starks/grinding.rs:40-48): the smallest qualifying nonce. */
int sp_grind(sp_ctx* ctx, const uint8_t challenge[32], uint8_t factor, uint64_t* nonce_out);

/* fri_query_phase + open_deep_composition_poly (fri/mod.rs:74-127, prover.rs:484-529). All arrays are host memory
 * owned by the context until the next call on it; digests are 32 bytes; field elements in the context encoding. */
typedef struct {
    uint32_t n_queries, n_layers, n_cols, depth0;  /* tree depth of FRI layer k is depth0 - k */
    const uint8_t* trace_evals;     /* [q][n_cols]  trace LDE row at iota                      */
    const uint8_t* comp_evals;      /* [q][2]       H1, H2 at iota                             */
    const uint8_t* main_paths;      /* [q][depth0]  authentication paths, bottom-up            */
    const uint8_t* aux_paths;       /* [q][depth0]                                              */
    const uint8_t* comp_paths;      /* [q][depth0]                                              */
    const uint8_t* fri_evals;       /* [q][n_layers]      layer value at iota mod |D_k|        */
    const uint8_t* fri_evals_sym;   /* [q][n_layers]      value at the symmetric index         */
    const uint8_t* fri_paths;       /* [q][sum_k (depth0 - k)], layers concatenated            */
    const uint8_t* fri_paths_sym;
} sp_openings;
int sp_open(sp_ctx* ctx, const uint64_t* iotas, uint32_t q, sp_openings* out);

/* ---- whole proof: generate_cairo_proof (reference src/cairo/air.rs:1165-1171) + StarkProof::serialize
 * (src/starks/proof/stark.rs:161-218). main_trace = row-major n x cols (34, or 43 with the range-check builtin) in the
 * context encoding. *proof_out is malloc'd; release it with sp_free. The bytes equal the reference prover's. */
int sp_cairo_prove(sp_ctx* ctx, const uint8_t* main_trace, uint64_t n, uint32_t cols, const sp_cairo_public_inputs* pub,
                   const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
/* Same with the main trace already resident in device memory (row-major, context encoding): the timed region of bench.py
 * starts with its input in HBM; sp_cairo_prove additionally pays the PCIe copy of n*cols*32 bytes. */
int sp_cairo_prove_dev(sp_ctx* ctx, const void* main_trace_dev, uint64_t n, uint32_t cols, const sp_cairo_public_inputs* pub,
                       const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
/* Same from host COLUMNS: column j of the main trace at main_trace_cols + j*col_stride*32 (col_stride in elements, 0 = n),
 * the layout `TraceTable::cols()` produces (reference src/starks/trace.rs:23-31, the input of compute_trace_polys, :104-110).
 * device_layout != 0: elements in the DEVICE layout (sp_fe_to_device); 0: in the context encoding.  No host-side gather: every
 * column group is one DMA overlapped with the transforms of the group before it.  Allocate the buffer with sp_host_alloc and
 * the DMA runs at PCIe speed; ordinary (pageable) memory works too, through the runtime's staging copy. */
int sp_cairo_prove_columns(sp_ctx* ctx, const uint8_t* main_trace_cols, uint64_t n, uint32_t cols, uint64_t col_stride, int device_layout,
                           const sp_cairo_public_inputs* pub, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
/* Page-locked host memory for trace tables (hipHostMalloc): SP_E_ALLOC when the runtime cannot provide it. */
int sp_host_alloc(uint64_t bytes, void** out);
void sp_host_free(void* p);
void sp_free(void* p);
/* How the main trace of the last proof reached the device: out = {kind (0: one copy / resident, 1: row-major host buffer gathered
 * into column groups by host threads, 2: DMA of page-locked host columns, 3: host columns in pageable memory, 4: register states +
 * memory of a run from page-locked memory, trace built on the device, 5: the same from pageable memory), column groups, bytes, host ms until the last chunk had been gathered and sent (kind 1), bytes over that time in GB/s, DMA ms
 * (sum over the groups), DMA GB/s, exposed ms (how long the compute stream waited for column groups in total), longest wait
 * for one group ms, host wall ms of the upload loop}. */
int sp_last_upload_stats(sp_ctx* ctx, double out[10]);
/* Device time (ms, HIP events on the context stream) of rounds 0..4 of the last sp_cairo_prove. */
/* What the last proof on this context did: out[0] = composition path (1: 2n-point evaluation after a clean trace check,
 * 2: whole LDE domain, deg H < 2n, 3: whole domain, deg H >= 2n - a constraint-violating trace), out[1] = FRI layers kept
 * sharded, out[2] = groups the LDE is sharded over, out[3] = 1 when the trace interpolation was split by column. */
int sp_last_proof_info(sp_ctx* ctx, uint32_t out[4]);
/* Device memory the prover of this context holds (trace, coefficients, LDE, trees, FRI layers, staging), in bytes: linear in
 * the trace length for a given column count, blowup factor and world size. */
int sp_prover_device_bytes(sp_ctx* ctx, uint64_t* bytes_out);
int sp_last_round_ms(sp_ctx* ctx, float out[5]);

/* ---- AIRs other than Cairo ------------------------------------------------------------------ */

/* What an implementor of the reference's `AIR` trait provides (src/starks/traits.rs:15-119, context.rs:4-18), with
 * `compute_transition` as a straight-line program over frame cells:
 *   op 0 LOAD  a = frame row (index into `offsets`), b = column of main||aux      -> value
 *   op 1 CONST a = index into consts; indices >= n_consts are the RAP challenges   -> value
 *   op 2 ADD, 3 SUB, 4 MUL   a, b = indices of earlier ops                          -> value
 *   op 5 OUT   a = constraint index, b = index of the op holding its value
 *   op 6 PERIODIC  a = frame row, b = periodic column                                -> value  (sp_air_prove_periodic only, see below)
 * The reference's examples (src/starks/example/{simple_fibonacci,fibonacci_2_columns,quadratic_air,fibonacci_rap,
 * dummy_air}.rs) are given in this form by lambdaworks_cairo_prover_amd/air.py. */
typedef struct { uint8_t op; uint8_t pad; uint16_t a; uint16_t b; uint16_t pad2; } sp_air_op;
typedef struct { uint32_t col; uint32_t pad; uint64_t step; uint8_t value[32]; /* canonical BE */ } sp_air_boundary;
/* build_auxiliary_trace(main_trace, rap_challenges) of the caller's AIR (traits.rs:25-29), for aux_kind 2: called once, after
 * the main commitment, with the n_rap challenges (32 bytes each, context encoding); must write the row-major n x aux_cols
 * auxiliary trace (context encoding) to aux_rows_out and return 0. */
typedef int (*sp_aux_trace_fn)(void* user, const uint8_t* rap, uint32_t n_rap, uint8_t* aux_rows_out);
typedef struct {
    uint32_t main_cols, aux_cols;            /* AirContext::trace_columns = main_cols + aux_cols (<= 1024) */
    uint32_t n_offsets; uint32_t offsets[8]; /* transition_offsets */
    uint32_t n_transitions; uint32_t degrees[64]; uint32_t exemptions[64]; /* transition_degrees / transition_exemptions */
    uint32_t num_transition_exemptions;      /* AirContext::num_transition_exemptions */
    uint32_t degree_bound_factor;            /* composition_poly_degree_bound() / trace_length (1 or 2) */
    uint32_t n_ops; const sp_air_op* ops;    /* <= 65535 ops, <= 64 values alive at any point of the program */
    uint32_t n_consts; const uint8_t* consts; /* <= 4096, canonical BE */
    uint32_t n_rap;                          /* build_rap_challenges: this many transcript_to_field samples */
    uint32_t aux_kind;                       /* build_auxiliary_trace: 0 none, 1 fibonacci_rap permutation column, 2 aux_fn,
                                              * 3 (SP_AIR_AUX_PROGRAM) an sp_air_aux_desc given to sp_air_prove_aux */
    uint32_t n_boundary; const sp_air_boundary* boundary;   /* <= 4096, on any rows (several per column allowed) */
    sp_aux_trace_fn aux_fn; void* aux_user;  /* aux_kind 2 */
} sp_air_desc;

/* prove::<Stark252PrimeField, A> (reference src/starks/prover.rs:532-766) + Serializable::serialize for the AIR `air`.
 * main_trace: row-major n x air->main_cols, context encoding, host memory.  *proof_out is malloc'd (sp_free). */
int sp_air_prove(sp_ctx* ctx, const sp_air_desc* air, const uint8_t* main_trace, uint64_t n, const sp_proof_options* opt,
                 uint8_t** proof_out, uint64_t* proof_len);
/* The bounds sp_air_prove accepts, in order: columns (main + aux), transition constraints, frame rows, boundary constraints,
 * constants, ops, values alive at once, 0 (reserved).  A binding can refuse a descriptor before proving. */
int sp_air_limits(uint32_t out[8]);

/* Auxiliary (RAP) columns built on the device from a straight-line program over the main-trace row and the RAP challenges
 * (permutation arguments, multiset checks, LogUp lookups).  The program runs once per row i; its ops use the sp_air_op encoding:
 *   op 0 LOAD  a = row shift s (0 .. 7): main column b of row (i + s) mod n
 *   op 1 CONST a = index into the aux program's consts; indices >= n_consts are the RAP challenges
 *   op 2 ADD, 3 SUB, 4 MUL   a, b = indices of earlier ops          (no OUT)
 * Auxiliary column k (trace column main_cols + k) takes N = value of op num_op and D = value of op den_op (D = 1 for
 * SP_AIR_AUX_NO_DEN) on every row:
 *   SP_AIR_AUX_PRODUCT  z_0 = 1, z_i = z_(i-1) N(i-1) / D(i-1)
 *   SP_AIR_AUX_SUM      z_0 = 0, z_i = z_(i-1) + N(i-1) / D(i-1)
 * A zero D on any row is SP_E_ZERO_INVERSE.  Bounds: those of the constraint program (sp_air_limits: 65535 ops, 4096 constants,
 * 64 values alive at once).
 *   SP_AIR_AUX_SORTED   a sorted copy of values of the main-trace row (Cairo's memory and range-check arguments).  num_op is the op whose
 *                       value the column carries, den_op the op that is the KEY of its sort group (SP_AIR_AUX_NO_DEN is refused), pad
 *                       the key's bits (1 .. 64; 0 means 64, above 64 is refused; kinds 0 and 1 ignore pad).  Columns with one den_op
 *                       form a group and must agree on pad; at most SP_AIR_AUX_MAX_SORT_GROUPS groups.  With key_i the canonical
 *                       integer of the key on row i and pi the stable ascending order of the rows by key_i (ties stay in row order),
 *                       row i of the column holds the value of num_op on row pi(i).  A key >= 2^bits on any row - every "negative"
 *                       element such as p - 1 included - is SP_E_INVALID_ARG ("a sort key is out of range").
 * A LOAD with b = main_cols + k reads auxiliary column k of row (i + s) mod n; k must be a SORTED column.  The ops behind a sorted
 * column's key or value must not contain such a LOAD, directly or through earlier ops (SP_E_INVALID_ARG).  All sort groups are built
 * before any product or sum, whatever the order of the columns. */
#define SP_AIR_AUX_PROGRAM 3
#define SP_AIR_AUX_PRODUCT 0
#define SP_AIR_AUX_SUM 1
#define SP_AIR_AUX_SORTED 2
#define SP_AIR_AUX_NO_DEN 0xFFFFFFFFu
#define SP_AIR_AUX_MAX_SORT_GROUPS 16
typedef struct { uint32_t kind, num_op, den_op, pad; } sp_air_aux_column;
typedef struct {
    uint32_t n_ops; const sp_air_op* ops;
    uint32_t n_consts; const uint8_t* consts;   /* canonical BE */
    uint32_t n_cols; const sp_air_aux_column* cols;
} sp_air_aux_desc;
/* sp_air_prove for an AIR with air->aux_kind == SP_AIR_AUX_PROGRAM and aux->n_cols == air->aux_cols >= 1: the same transcript,
 * rounds and proof bytes as sp_air_prove of the same trace columns, with the auxiliary segment built and committed on the device
 * (every rank of a sharded context builds all of it from its whole copy of the main trace). */
int sp_air_prove_aux(sp_ctx* ctx, const sp_air_desc* air, const sp_air_aux_desc* aux, const uint8_t* main_trace, uint64_t n,
                     const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
uint64_t sp_air_aux_desc_size(void);

/* Periodic columns (NO reference counterpart: the reference's `AIR` trait has none): public sequences of `period` values that repeat
 * down the trace - round constants, every-k-th-row selectors, builtin schedules.  period is a power of two, 1 <= period <= n.  With g
 * the trace-domain generator and w_p = g^(n/period), q is the polynomial of degree < period with q(w_p^j) = values[j]; the column's
 * polynomial is P(x) = q(x^(n/period)), so P(g^i) = values[i mod period] and deg P < n.  A constraint program reads it with
 *   op 6 PERIODIC  a = frame row (index into `offsets`), b = periodic column index   -> value  P at that frame row's point
 * In a constraint's declared degree a periodic value counts as a trace cell does (one factor of degree < n): the degree adjustments of
 * the composition polynomial do not change.  The columns are NOT committed and do not enter the transcript, the proof format is
 * unchanged: like the program's constants they are part of the statement prover and verifier both hold.  sp_air_prove,
 * sp_air_prove_aux, sp_air_verify and sp_air_verify_backend answer a program that contains op 6 as they answer any unknown op
 * (SP_E_INVALID_ARG / 0); an auxiliary program (sp_air_aux_desc) cannot read periodic columns and is refused the same way (only
 * sp_air_prove_pub and its siblings below let it). */
#define SP_AIR_OP_PERIODIC 6
typedef struct { uint32_t period, pad; const uint8_t* values; /* period x 32, canonical BE */ } sp_air_periodic_column;
typedef struct { uint32_t n_cols, pad; const sp_air_periodic_column* cols; } sp_air_periodic_desc;
uint64_t sp_air_periodic_desc_size(void);
/* out = {periodic columns at most (64), 0, 0, 0 (reserved)}; a period is a power of two with 1 <= period <= n. */
int sp_air_periodic_limits(uint32_t out[4]);
/* sp_air_prove (aux == NULL) or sp_air_prove_aux (aux != NULL, air->aux_kind == SP_AIR_AUX_PROGRAM) for an AIR whose constraint
 * program reads the periodic columns of `periodic` (n_cols 0 .. 64).  The device holds period x blowup evaluations per column (every
 * rank of a sharded context all of them).  SP_E_INVALID_ARG for a period that is no power of two or exceeds n, null values, more
 * than 64 columns, an op 6 naming a column >= n_cols. */
int sp_air_prove_periodic(sp_ctx* ctx, const sp_air_desc* air, const sp_air_aux_desc* aux, const sp_air_periodic_desc* periodic,
                          const uint8_t* main_trace, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
/* sp_air_verify_backend for such an AIR: 1 accept, 0 reject (also for the malformed descriptors above).  The verifier evaluates
 * P_k(z g^offsets[r]) itself (sp_air_periodic_eval's routine). */
int sp_air_verify_periodic(const uint8_t* proof, uint64_t proof_len, const sp_air_desc* air, const sp_air_periodic_desc* periodic,
                           const sp_proof_options* opt, int merkle_backend);
/* Test seams.  sp_air_periodic_eval (host): out = P(point) for a trace of n rows, canonical BE in and out - q interpolated from the
 * values, evaluated at point^(n/period).  sp_air_periodic_lde (device): the table the composition kernel reads, in natural order:
 * out[k] = P(coset w_N^k) for k < period x blowup (N = n x blowup; the evaluations repeat with that period), canonical BE.  n, blowup and
 * the period are powers of two with blowup >= 2, n x blowup <= 2^30 and 1 <= period <= n (SP_E_INVALID_ARG otherwise), as a proof's are. */
int sp_air_periodic_eval(const sp_air_periodic_column* col, uint64_t n, const uint8_t point[32], uint8_t out[32]);
int sp_air_periodic_lde(sp_ctx* ctx, const sp_air_periodic_column* col, uint64_t n, uint32_t blowup, const uint8_t coset[32], uint8_t* out);

/* Which constraints of a program AIR a trace breaks, and where (reference validate_trace, src/starks/debug.rs:13-104, which logs the
 * constraint, the step and the value).  sp_air_prove proves a constraint-violating trace anyway, as the reference does; the only
 * signal there is the 3 in sp_last_proof_info and a proof the verifier rejects.  This call produces no proof.
 *   air, aux (nullable), periodic (nullable), main_trace, n: what sp_air_prove_periodic takes, with its argument checks and error codes.
 *   rap: air->n_rap x 32 bytes in the context encoding - the auxiliary columns (aux_kind 1, 2 or 3) are built from these challenges -
 *        or NULL: the challenges a proof under `opt` would sample (round 1's main commitment, then n_rap transcript samples).
 *   opt: required when rap == NULL (SP_E_INVALID_ARG without both); with rap it only sizes the commitments, and may be NULL.
 * The trace checked is main || aux as the prover holds it before round 2, reached through the prover's own ingest and auxiliary
 * builders (round 1 runs, commitments included).  Constraint k is enforced on rows 0 .. n - 1 - e_k, frame rows wrapping modulo n;
 * e_k is the exemption count the composition uses for it: exemptions[k], or - with num_transition_exemptions == 1 - the first
 * non-zero entry of exemptions[] for every constraint that has one.
 * out receives the violated constraints, transitions first by index, then boundary constraints by index - at most `cap` records;
 * *n_out is their total number and may exceed cap (0: the trace satisfies the AIR).  out may be NULL with cap == 0.  SP_OK whether
 * or not anything is violated; a zero denominator in an aux program stays SP_E_ZERO_INVERSE; SP_E_UNSUPPORTED on a context with
 * world > 1.  A later proof on the context is not affected. */
typedef struct {
    uint32_t kind;        /* 0 transition constraint, 1 boundary constraint */
    uint32_t index;       /* transition: constraint index (OUT's a); boundary: index into air->boundary */
    uint64_t rows;        /* enforced rows on which it is non-zero (boundary: 1) */
    uint64_t first_row;   /* lowest such row (boundary: its step) */
    uint64_t last_row;    /* highest such row (boundary: its step) */
    uint8_t  value[32];   /* canonical BE.  transition: the evaluation on first_row; boundary: the cell found */
} sp_air_violation;
uint64_t sp_air_violation_size(void);
int sp_air_check_trace(sp_ctx* ctx, const sp_air_desc* air, const sp_air_aux_desc* aux, const sp_air_periodic_desc* periodic,
                       const uint8_t* main_trace, uint64_t n, const sp_proof_options* opt, const uint8_t* rap,
                       sp_air_violation* out, uint32_t cap, uint32_t* n_out);

/* Strided transition constraints (NO reference counterpart, like periodic columns): constraint k is enforced on the rows
 * i = offset_k (mod period_k) only - "every 8th row starts a hash invocation", "rows = 3 (mod 4) carry the range-check cell".  period
 * is a power of two with 1 <= period <= n and 0 <= offset < period; (1, 0) is sp_air_prove's behaviour.  With s = period, o = offset,
 * e = exemptions[k], g the trace-domain generator, f = degree_bound_factor and d = degrees[k]:
 *   enforced rows   i = o (mod s) except the last e rows OF THAT PROGRESSION, o + s (n/s - 1 - t) for t < e; a stride with s > 1
 *                   needs e < n/s and always uses its own e (the num_transition_exemptions == 1 rule stays with the (1, 0) constraints)
 *   zerofier        Z(x) = x^(n/s) - g^(o n/s)
 *   exemptions      E(x) = prod_{t < e} (x - g^(o + s (n/s - 1 - t)))
 *   composition     (alpha_k x^adj + beta_k) C_k(x) E(x) / Z(x),  adj = n (f - d) + n/s   (s = 1: sp_air_prove's n (f - d + 1))
 * The term has f n - d + e + 1 coefficients whatever the stride.  A stride with s > 1 needs d <= f: the quotient C_k / Z divides by n/s
 * roots only and has degree d n - n/s, so adj would be negative for d = f + 1 (which a (1, 0) constraint may have).  Constraints with
 * the same (s, o), s > 1, form a stride class: at most 4 classes per AIR, at most 4 distinct (class, e > 0) exemption products
 * (sp_air_stride_limits).  Nothing of this enters the transcript or the proof format. */
typedef struct { uint32_t period, offset; } sp_air_stride;
typedef struct { uint32_t n; uint32_t pad; const sp_air_stride* strides; /* n == air->n_transitions */ } sp_air_stride_desc;
/* The extensions of a program AIR in one block, each nullable: size = sizeof(sp_air_ext) as the caller compiled it. */
typedef struct {
    uint32_t size, pad;
    const sp_air_aux_desc* aux;              /* as sp_air_prove_aux takes it */
    const sp_air_periodic_desc* periodic;    /* as sp_air_prove_periodic takes it */
    const sp_air_stride_desc* strides;
} sp_air_ext;
uint64_t sp_air_stride_size(void);
uint64_t sp_air_stride_desc_size(void);
uint64_t sp_air_ext_size(void);
/* out = {stride classes at most (4), distinct (class, e > 0) exemption products at most (4), 0, 0 (reserved)} */
int sp_air_stride_limits(uint32_t out[4]);
/* sp_air_prove / _aux / _periodic, sp_air_verify_periodic and sp_air_check_trace with the extensions of `ext` (NULL, or all members
 * NULL: sp_air_prove, sp_air_verify_backend, sp_air_check_trace without extensions - the same bytes, verdicts and error codes).  A
 * malformed stride descriptor - n != air->n_transitions, null strides, a period that is zero, no power of two or above the trace
 * length, offset >= period, exemptions[k] >= n/period or degrees[k] > degree_bound_factor for a period > 1, more classes or exemption products than
 * sp_air_stride_limits, ext->size other than sizeof(sp_air_ext) - is SP_E_INVALID_ARG from the prover and the trace check and 0 from
 * the verifier, before anything is sized from it.  sp_air_check_trace_ext follows the enforced-row rule above: rows outside a
 * constraint's progression are neither flagged nor counted. */
int sp_air_prove_ext(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const uint8_t* main_trace, uint64_t n,
                     const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_verify_ext(const uint8_t* proof, uint64_t proof_len, const sp_air_desc* air, const sp_air_ext* ext,
                      const sp_proof_options* opt, int merkle_backend);
int sp_air_check_trace_ext(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const uint8_t* main_trace, uint64_t n,
                           const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap, uint32_t* n_out);
/* Test seams.  sp_air_stride_eval (host, the verifier's routine): out_z = Z(point), out_e = E(point) for a stride (period, offset)
 * with `exemptions` exempted rows on a trace of n rows, canonical BE in and out; period 1 gives x^n - 1 and the last rows of the
 * trace.  sp_air_stride_table (device): one period of 1 / Z as the composition kernel reads it, in natural order: out[k] =
 * 1 / Z(coset w_N^k) for k < period x blowup (N = n x blowup), canonical BE.  n, blowup, period powers of two, blowup >= 2,
 * n x blowup <= 2^30, 1 <= period <= n, offset < period, exemptions <= n / period and <= 65536 (one host product each) (SP_E_INVALID_ARG otherwise); SP_E_ZERO_INVERSE when
 * Z vanishes on the coset. */
int sp_air_stride_eval(uint32_t period, uint32_t offset, uint32_t exemptions, uint64_t n, const uint8_t point[32], uint8_t out_z[32],
                       uint8_t out_e[32]);
int sp_air_stride_table(sp_ctx* ctx, uint32_t period, uint32_t offset, uint64_t n, uint32_t blowup, const uint8_t coset[32], uint8_t* out);

/* Public data inside a randomized (RAP) argument, through the three _pub calls below only.
 *
 * (1) The auxiliary program of ext->aux may read the periodic columns of ext->periodic - a LogUp lookup against a public table, an
 *     S-box, an opcode table:
 *   op 6 PERIODIC  a = row shift s (0 .. 7), b = periodic column of ext->periodic: values[(i + s) mod period] on row i
 * An op 6 with b >= ext->periodic->n_cols, or without ext->periodic, is malformed.  sp_air_prove_aux / _periodic / _ext keep refusing
 * op 6 in an auxiliary program.
 *
 * (2) Boundary values computed from the RAP challenges (reference traits.rs:44-47, `boundary_constraints(&self, rap_challenges)`).  A
 *     straight-line program in the sp_air_op encoding: CONST (indices >= n_consts are the RAP challenges), ADD, SUB, MUL only.  Entry j
 *     replaces air->boundary[values[j].boundary].value by N / D (D = 1 for SP_AIR_AUX_NO_DEN) once the challenges exist.
 * Bounds: those of sp_air_limits (65535 ops, 4096 constants, constants + RAP challenges <= 65535).  Malformed - null members, an op
 * other than 1 .. 4, an operand that is not an earlier op, boundary >= air->n_boundary, the same boundary named twice, num_op / den_op
 * beyond the program - is SP_E_INVALID_ARG from the prover and the trace check and 0 from the verifier, before anything is sized from
 * it.  A D that evaluates to zero is SP_E_ZERO_INVERSE from the prover and the trace check and 0 from the verifier.  Nothing of this
 * enters the transcript; the proof format is unchanged.
 *
 * With bvals == NULL and an auxiliary program without op 6 the three calls are sp_air_prove_ext / _verify_ext / _check_trace_ext: the
 * same bytes, verdicts and error codes. */
typedef struct { uint32_t boundary, num_op, den_op, pad; } sp_air_boundary_value;
typedef struct {
    uint32_t n_ops; const sp_air_op* ops;
    uint32_t n_consts; const uint8_t* consts;   /* canonical BE */
    uint32_t n_values; const sp_air_boundary_value* values;
} sp_air_boundary_desc;
uint64_t sp_air_boundary_desc_size(void);
int sp_air_prove_pub(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const uint8_t* main_trace,
                     uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_verify_pub(const uint8_t* proof, uint64_t proof_len, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals,
                      const sp_proof_options* opt, int merkle_backend);
int sp_air_check_trace_pub(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const uint8_t* main_trace,
                           uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap, uint32_t* n_out);
/* Test seam (host): out[j] = the resolved value of values[j], canonical BE; rap = n_rap x 32 bytes, canonical BE.  The `boundary` members
 * are only held against each other here (no AIR to hold them against). */
int sp_air_boundary_resolve(const sp_air_boundary_desc* bvals, const uint8_t* rap, uint32_t n_rap, uint8_t* out);

/* ---- A program for the MAIN segment: the caller supplies the first input_cols main columns, the device derives the other n_cols as
 * row-local functions of columns that exist already (bit decompositions, is-zero inverses, intermediate products, counters), then
 * commits the main segment as ever.  The proof is that of sp_air_prove_pub given the whole table: same bytes, same verifier calls
 * (there is no verifier entry point for it - how a trace was made is no part of the statement).
 *
 * The program runs once per row i (the sp_air_op encoding): LOAD a = row shift 0 .. 7 (row (i + a) mod n), b = main column; CONST
 * a = constant; ADD, SUB, MUL over earlier ops.  No OUT, no op 6, no RAP challenges (there are none yet).  Derived column k (main
 * column input_cols + k) names its ops N = num_op and D = den_op (SP_AIR_AUX_NO_DEN: D = 1) and a kind: */
#define SP_AIR_MAIN_VALUE       0  /* z_i = N(i) / D(i)   (D = 1 for SP_AIR_AUX_NO_DEN); a zero D on any row: SP_E_ZERO_INVERSE */
#define SP_AIR_MAIN_INV_OR_ZERO 1  /* z_i = 0 where N(i) = 0, else 1 / N(i); den_op must be SP_AIR_AUX_NO_DEN; never an error    */
#define SP_AIR_MAIN_BIT         2  /* z_i = bit `pad` (0 .. 251) of the canonical integer of N(i); den_op must be NO_DEN          */
#define SP_AIR_MAIN_SUM         3  /* z_0 = 0, z_i = z_(i-1) + N(i-1) / D(i-1)   (as SP_AIR_AUX_SUM, without challenges)           */
#define SP_AIR_MAIN_PRODUCT     4  /* z_0 = 1, z_i = z_(i-1) N(i-1) / D(i-1)                                                       */
/* A LOAD of b < input_cols reads an input; a LOAD of input_cols + k reads derived column k and may stand only behind (the N or D of)
 * a derived column j > k: columns are built in index order, and a column is complete before anything reads it (shifts wrap).  A column
 * whose evolution is a true recurrence - z_(i+1) a non-linear function of z_i, such as the state of a hash chain - cannot be written
 * with these five kinds; it is an SP_AIR_MAIN_CHAIN column of the _rec entry points below.  With a main program air->aux_kind must be 0 or SP_AIR_AUX_PROGRAM (kinds 1 and 2 read a host table of
 * the main segment, which no longer exists: SP_E_UNSUPPORTED).  Bounds: those of sp_air_limits (65535 ops, 4096 constants, 64 live
 * values).  Malformed - size other than sizeof(sp_air_main_desc), null members, input_cols == 0 or input_cols + n_cols !=
 * air->main_cols, input_location above 1, an unknown kind, pad > 251 on a BIT, a denominator on INV_OR_ZERO or BIT, an op outside
 * 0 .. 4, an operand that is no earlier op, a LOAD of a derived column that is not earlier, num_op / den_op beyond the program - is
 * SP_E_INVALID_ARG before anything is sized from it. */
typedef struct { uint32_t kind, num_op, den_op, pad; } sp_air_main_column;
typedef struct {
    uint32_t size, input_cols;          /* size = sizeof as compiled; the first input_cols main columns come from the caller */
    uint32_t input_location, pad;       /* 0: host memory, 1: device memory of the context's device; both row-major n x input_cols, context encoding */
    uint32_t n_ops;    const sp_air_op* ops;
    uint32_t n_consts; const uint8_t* consts;     /* canonical BE */
    uint32_t n_cols;   const sp_air_main_column* cols;   /* input_cols + n_cols == air->main_cols, input_cols >= 1 */
} sp_air_main_desc;
uint64_t sp_air_main_desc_size(void);
/* sp_air_prove_pub / sp_air_check_trace_pub (ext and bvals nullable, as there) with `inputs` in place of the main trace. */
int sp_air_prove_main(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                      const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_main(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                            const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                            uint32_t* n_out);
/* Test seam (device): rows_out = the whole n x air->main_cols table the prover would commit, row-major, context encoding, host memory;
 * nothing is committed.  sp_air_main_check (host only): SP_OK, or the decoder's refusal of this program for this AIR and n rows. */
int sp_air_main_trace(sp_ctx* ctx, const sp_air_desc* air, const sp_air_main_desc* main, const void* inputs, uint64_t n, uint8_t* rows_out);
int sp_air_main_check(const sp_air_desc* air, const sp_air_main_desc* main, uint64_t n);

/* ---- Block recurrences in a main program: the states of many independent permutations (MiMC, Poseidon, Rescue rounds; Merkle paths;
 * hash-based signatures), each a block of s = 2^l consecutive rows seeded on its first row.  Through the _rec entry points - and only
 * through them: everywhere else kind 5 stays an unknown kind and op 6 a malformed op - a main program may hold columns of kind */
#define SP_AIR_MAIN_CHAIN       5  /* z(B s) = Seed(B s);  z(i + 1) = Step(i) for (i + 1) mod s != 0   (rows i = B s + t)                  */
/* and read the periodic columns of ext->periodic with op 6: a = row shift 0 .. 7, b = periodic column k, the value values[(i + a) mod
 * period_k] - the raw values, as the auxiliary program's table read; behind columns of every kind.
 * A chain group is a run of w consecutive CHAIN columns, 1 <= w <= 16: pad = l + 256 j with s = 2^l the block length (1 <= l <= log2 n)
 * and j the column's position in its group - j = 0 opens a group, the columns after it carry j = 1, 2, .. and the same l.  den_op names
 * the column's SEED op (SP_AIR_AUX_NO_DEN is refused: a chain needs a seed), num_op its STEP op.  The seeds are evaluated on the block's
 * first row and may read inputs, derived columns before the group and periodic columns - nothing of the group.  The steps are evaluated
 * on the row they leave from: a LOAD of a column of the group must have shift 0 and is the state on row i; inputs and derived columns
 * before the group at shifts 0 .. 7, wrapping modulo n; periodic columns.  The w next values are assigned together, after the whole
 * step program has run.  Columns after the group read its columns as any earlier derived column.  No denominators: seeds and steps are
 * polynomial (CONST, ADD, SUB, MUL) - an inverse S-box (x^(1/d)) is out of scope, a division inside a seed or a step is op 7 of the
 * _div entry points below.  A block seeded from the
 * block before it (a multi-block sponge, a Merkle path) is a linked group of the _link entry points below; through these every block
 * stands alone, and bits of pad at or above 16 count as part of j.  Refused with SP_E_INVALID_ARG and a message that names the
 * column, before anything is sized: j out of sequence or a group longer than 16, l = 0 or 2^l > n, members of a group that differ in l,
 * a step that loads its group at a shift other than 0, a seed that loads its group, any load of a later column, a chain without a seed,
 * op 6 naming a periodic column the statement does not have (or without ext->periodic).  Argument lists as sp_air_prove_main /
 * sp_air_check_trace_main / sp_air_main_trace / sp_air_main_check; the last two also take the sp_air_ext (nullable) that carries the
 * periodic columns. */
int sp_air_prove_rec(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                     const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_rec(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                           const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                           uint32_t* n_out);
int sp_air_main_trace_rec(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                          uint8_t* rows_out);
int sp_air_main_check_rec(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most columns of a chain group (16), out[1] = the highest row shift of a LOAD or an op 6 (7) */
int sp_air_main_chain_limits(uint32_t out[2]);

/* ---- Lookup multiplicities in a main program: the column m of a LogUp lookup into a table ("how often is the table entry of row i
 * looked up"), which is a join of the looked-up column against the table and so no row-local kind.  Through the _lk entry points - and
 * only through them: everywhere else kind 6 stays an unknown kind - a main program may hold columns of kind */
#define SP_AIR_MAIN_COUNT       6  /* z_i = #{ j in [0, n) : X(j) = T(i) } if no row i' < i has T(i') = T(i), else 0                         */
/* num_op names the looked-up value X, den_op the table value T (SP_AIR_AUX_NO_DEN is refused: a COUNT needs a table), pad = key_bits,
 * 1 .. 64.  X and T are ordinary values of the program, evaluated on every row: inputs, earlier derived columns at shifts 0 .. 7 and
 * periodic columns (op 6).  Each distinct table value's multiplicity sits on the first row that holds it; values of X that no T holds
 * are counted nowhere, which is no error (the LogUp sum then does not close and the proof is rejected as for any violating trace).
 * The canonical integers of X(j) and T(i) must be below 2^key_bits on every row: otherwise SP_E_INVALID_ARG with "a lookup key is out
 * of range on some row", which is reported before a zero denominator of the same program when both occur.  A tuple is looked up by
 * packing it on both sides (a + 2^w b + 2^(2w) c): X and T are expressions.  n < 2^32.  The _lk entry points accept everything the
 * _rec ones do; they refuse, with SP_E_INVALID_ARG and a message that names the column, before anything is sized: a COUNT column
 * without a table, key_bits 0 or above 64, X or T reading a column that is not an earlier one, ops beyond the program, more than 16
 * COUNT columns in one program.  Argument lists as the _rec entry points. */
int sp_air_prove_lk(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                    const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_lk(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                          const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                          uint32_t* n_out);
int sp_air_main_trace_lk(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                         uint8_t* rows_out);
int sp_air_main_check_lk(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most key bits of a COUNT column (64), out[1] = the most COUNT columns of one main program (16) */
int sp_air_main_count_limits(uint32_t out[2]);

/* ---- Linked chain groups: blocks seeded from the block before (a sponge that absorbs several blocks, a Merkle path whose level
 * k + 1 hashes level k's digest with a sibling).  Through the _link entry points - and only through them - the pad of a CHAIN column
 * is l + 256 j + 65536 k: l = pad & 255 and j = (pad >> 8) & 255 as above, and k = pad >> 16 links 2^k consecutive blocks into a RUN of
 * 2^(l + k) rows, aligned.  k = 0 is the group of the _rec entry points, bit for bit.  For k >= 1: l + k <= log2 n, all columns of a
 * group carry the same k, and the seed programs may LOAD columns of their own group at shift 0.  Such a LOAD reads the CARRY: for a
 * block whose first row is i, the state of that group column on row i - 1 (the last row of the block before) when the block is not the
 * first of its run, and zero when it is.  A seed may read the carry of any column of its group; every other LOAD and every op 6 of a
 * seed is evaluated on row i, as ever; the w seeds are assigned together after the whole seed program has run.  Steps are unchanged,
 * and so is the proof: the same table gives the same bytes, and sp_air_verify* take these proofs as they are.  One lane builds one run,
 * so a program wants n / 2^(l + k) runs in the thousands to fill the device.  The _link entry points accept everything the _lk ones do;
 * they refuse, with SP_E_INVALID_ARG and a message that names the column, before anything is sized: k above the limit, l + k > log2 n,
 * members of a group that differ in k, a seed that loads its group at a shift other than 0, and - with k = 0 - a seed that loads its
 * group at all.  Argument lists as the _lk entry points. */
int sp_air_prove_link(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                      const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_link(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                            const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                            uint32_t* n_out);
int sp_air_main_trace_link(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                           uint8_t* rows_out);
int sp_air_main_check_link(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the highest k of a linked group (62), out[1] = the most columns of a linked group (16) */
int sp_air_main_link_limits(uint32_t out[2]);

/* ---- Quotients in chain steps: a recurrence whose next state needs a division by something the state decides - the slope
 * lambda = (y - y_P) / (x - x_P) of an elliptic-curve addition chain (Pedersen, EC-op, ECDSA), itself a trace column because the AIR
 * constrains lambda (x - x_P) = y - y_P.  Through the _div entry points - and only through them: everywhere else op 7 stays the malformed
 * op it was - a main program may hold */
#define SP_AIR_OP_DIV 7            /* op 7 DIV  a, b = earlier ops  -> value(a) / value(b)                                        */
/* behind the SEED or the STEP op of an SP_AIR_MAIN_CHAIN column, that is: reachable through operands from a CHAIN column's den_op or
 * num_op.  A quotient is an ordinary intermediate value: it may feed further arithmetic and another DIV, and several next values may
 * share it.  Only the ops a group's seeds or steps reach are evaluated, so a zero under a DIV that nothing reaches is no error.  A
 * reachable denominator that is zero on any row its group evaluates fails the call with SP_E_ZERO_INVERSE - the verdict of a zero D
 * of a VALUE column, at the same moment: once the root (or the table) is back; nothing is returned and the context goes on.  Every
 * other kind stays as it is: a VALUE, INV_OR_ZERO, BIT, SUM, PRODUCT or COUNT column whose N, D, X or T depends on an op 7 is refused
 * with SP_E_INVALID_ARG and a message that names the column - a row-local quotient is a VALUE column's N / D, which shares one batched
 * inversion with its whole chunk, where a DIV costs one inversion per lane (tens of microseconds: a DIV step is dominated by them, and
 * a group's time is about rows-per-block x DIVs-per-step x that, whatever the number of blocks up to the device's width).  Constraint
 * programs, auxiliary programs and boundary programs know no op 7.  The _div entry points accept everything the _link ones do; the
 * proof is unchanged: the same table gives the same bytes.  Argument lists as the _link entry points. */
int sp_air_prove_div(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                     const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_div(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                           const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                           uint32_t* n_out);
int sp_air_main_trace_div(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                          uint8_t* rows_out);
int sp_air_main_check_div(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);

/* ---- Looked-up values in a main program: the result of a lookup - c = a xor b as "the third field of the table row whose first two
 * are a, b", the word at a program counter, a read from read-only memory - is a join of the looked-up key against the table, as the
 * multiplicity of the same lookup is, and so no row-local kind.  Through the _fetch entry points - and only through them: everywhere
 * else kind 7 stays an unknown kind - a main program may hold columns of kind */
#define SP_AIR_MAIN_FETCH       7  /* z_i = V(j*), j* the lowest row j with T(j) = X(i)                                                     */
/* num_op names the looked-up key X, den_op the table key T (SP_AIR_AUX_NO_DEN is refused: a FETCH needs a table key), and pad =
 * key_bits + 256 v_op: key_bits (bits 0 - 7) in 1 .. 64, v_op (bits 8 - 23) the op whose value is the table value V; a bit at or above
 * 24 is refused.  X, T and V are ordinary values of the program, evaluated on every row: inputs, earlier derived columns at shifts
 * 0 .. 7 (wrapping) and periodic columns (op 6).  The canonical integers of X(i) and T(j) must be below 2^key_bits on every row -
 * otherwise SP_E_INVALID_ARG with the COUNT columns' "a lookup key is out of range on some row", reported first -; V is a full field
 * element.  Equal table keys: the lowest row wins, the row a COUNT column puts the key's multiplicity on.  A key X(i) that no row of T
 * holds fails the call with SP_E_INVALID_ARG, "a fetched key is in no table row" (a COUNT column lets such a value pass and the proof
 * fail; a FETCH has no value to write): nothing is returned and the context goes on, and a caller with idle rows points them at a key
 * the table holds.  It is reported behind the key range and before a zero denominator of the same program.  n < 2^32.  Consecutive
 * FETCH columns with one X, one T and one key_bits that read nothing of each other - the fields of an instruction word, several
 * outputs of one table - share one sort of the table and one search (at most 16 columns at a time); the values are those of the
 * columns taken one by one.  A tuple key is packed on both sides.  The _fetch entry points accept everything the _div ones do; they
 * refuse, with SP_E_INVALID_ARG and a message that names the column, before anything is sized: a pad with a bit at or above 24, a
 * FETCH column without a table key, key_bits 0 or above 64, X, T or v_op beyond the program, X, T or V behind an op 7 or reading a
 * column that is not an earlier one, more than 64 FETCH columns in one program.  The proof is unchanged: the same table gives the same
 * bytes.  Argument lists as the _div entry points. */
int sp_air_prove_fetch(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                       const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_fetch(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                             const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                             uint32_t* n_out);
int sp_air_main_trace_fetch(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                            uint8_t* rows_out);
int sp_air_main_check_fetch(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most key bits of a FETCH column (64), out[1] = the most FETCH columns that share one sort and one search (16), out[2] =
 * the most FETCH columns of one main program (64) */
int sp_air_main_fetch_limits(uint32_t out[3]);

/* ---- Limbs and bitwise words in a main program: the 16-bit limbs of a range check, the fields of an instruction word, AND, XOR and OR
 * of two words are row-local functions of a value's CANONICAL INTEGER int(v), 0 <= int(v) < p - the one thing the field ops of a program
 * cannot express; a BIT column is the one-bit case.  Through the _word entry points - and only through them: everywhere else kinds 8
 * and 9 stay unknown kinds - a main program may hold columns of kind */
#define SP_AIR_MAIN_LIMB        8  /* z_i = (int(N(i)) >> lo) mod 2^width                                                                  */
#define SP_AIR_MAIN_WORD        9  /* z_i = int(N(i)) AND / OR / XOR int(D(i))                                                             */
/* LIMB: num_op names N, den_op must be SP_AIR_AUX_NO_DEN (as for a BIT column), and pad = lo + 256 width with 1 <= width and lo + width
 * <= 252 (so lo <= 251); a bit at or above 16 is refused.  width = 1 gives the cells of BIT lo, lo = 0 and width = 252 gives N.  Every
 * canonical integer has limbs: there is no run-time error.
 * WORD: num_op names N, den_op names D (SP_AIR_AUX_NO_DEN is refused), and pad = fn + 256 bits: fn (bits 0 - 7) 0 AND, 1 OR, 2 XOR, bits
 * (bits 8 - 15) in 1 .. 251; a bit at or above 16 is refused.  2^251 < p, so every result is a canonical integer.  An operand at or above
 * 2^bits on any row fails the call with SP_E_INVALID_ARG, "a word operand is out of range on some row (both operands of a WORD column
 * must be below 2^bits as canonical integers)": nothing is returned and the context goes on.  It is reported behind a key out of range
 * and a fetched key in no table row, and before a zero denominator of the same program.
 * Both kinds are row-local: N and D follow the rules of a VALUE column's operands - earlier columns only, at shifts 0 .. 7 (wrapping),
 * periodic columns (op 6), behind no op 7 - and any later column of any kind may read them: the X of a COUNT or FETCH column, a chain
 * seed, a scan.  LIMB columns with one N share one pass out of Montgomery form, WORD columns with one N, D and bits two.  Shifts,
 * rotations, NOT, add-with-carry and comparisons are a LIMB and a VALUE column - rotl(x, r) over w bits = limb(x, 0, w - r) 2^r +
 * limb(x, w - r, r) - and have no kind of their own.  The _word entry points accept everything the _fetch ones do; they refuse, with
 * SP_E_INVALID_ARG and a message that names the column, before anything is sized: a pad with a bit at or above 16, a LIMB with width 0,
 * with lo + width > 252 or with a denominator, a WORD without a second operand, with fn > 2 or with bits 0 or above 251, an operand
 * beyond the program, behind an op 7 or reading a column that is not an earlier one.  The proof is unchanged: the same table gives the
 * same bytes.  Argument lists as the _fetch entry points. */
int sp_air_prove_word(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                      const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_word(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                            const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                            uint32_t* n_out);
int sp_air_main_trace_word(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                           uint8_t* rows_out);
int sp_air_main_check_word(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most lo + width of a LIMB column (252), out[1] = the most bits of a WORD column (251), out[2] = the number of WORD
 * functions (3: fn 0 .. 2), out[3] = 0 */
int sp_air_main_word_limits(uint32_t out[4]);

/* ---- Integer ops in chain steps: a recurrence whose next state is an integer function of the state - the rotations, additions
 * modulo 2^w, XORs, ANDs and ORs of a round of an ARX cipher, of SHA-2 or of Blake.  A LIMB or WORD column is row-local and may not
 * read its own group, so it cannot stand inside a step.  Through the _int entry points - and only through them: everywhere else ops
 * 8 .. 11 stay the malformed ops they were - a main program may hold */
#define SP_AIR_OP_LIMB 8           /* op 8  LIMB a = earlier op, b = lo + 256 width (an immediate)  -> (int(value(a)) >> lo) mod 2^width */
#define SP_AIR_OP_AND  9           /* op 9  AND  a, b = earlier ops  -> int(value(a)) AND int(value(b))                            */
#define SP_AIR_OP_OR   10          /* op 10 OR   a, b = earlier ops  -> int(value(a)) OR  int(value(b))                            */
#define SP_AIR_OP_XOR  11          /* op 11 XOR  a, b = earlier ops  -> int(value(a)) XOR int(value(b))                            */
/* behind the SEED or the STEP op of an SP_AIR_MAIN_CHAIN column, exactly where op 7 may stand.  int(v) is the canonical integer,
 * 0 <= int(v) < p, as for kinds 8 and 9.  LIMB: 1 <= width and lo + width <= 252, the limits of a LIMB column; every canonical integer
 * has limbs, so it has no run-time error.  AND, OR and XOR take no `bits`: both operands must be below 2^251 as canonical integers, and
 * since 2^251 < p every result is canonical.  An operand at or above 2^251 on any row its group evaluates fails the call with
 * SP_E_INVALID_ARG, "an integer op's operand is out of range on some row (both operands of an AND, OR or XOR op must be below 2^251 as
 * canonical integers)": nothing is returned and the context goes on.  It is reported behind a key out of range and a fetched key in no
 * table row, and before a zero denominator of the same program - a WORD column's place, and where a WORD column of the same program is
 * out of range too, either of the two messages may come back.  Only the ops a group's seeds or steps reach are evaluated.  Rotation,
 * shift, NOT and addition or subtraction modulo 2^w have no op: rotl(x, r) over w bits = limb(x, 0, w - r) 2^r + limb(x, w - r, r), and
 * (x + y) mod 2^w = limb(x + y, 0, w).  Each integer op takes its operands out of Montgomery form and its result back: the cost of two
 * to three field products.  Every other kind stays as it is: a VALUE, INV_OR_ZERO, BIT, SUM, PRODUCT, COUNT, FETCH, LIMB or WORD
 * column whose operand depends on an op 8 .. 11 is refused with SP_E_INVALID_ARG and a message that names the column - a row-local
 * limb or word is a LIMB or WORD column.  The decoder also refuses, naming the op: a LIMB op with width 0 or with lo + width > 252, and
 * operands that are not earlier values.  Constraint programs, auxiliary programs and boundary programs know no op 8 .. 11.  The _int
 * entry points accept everything the _word ones do; the proof is unchanged: the same table gives the same bytes.  Argument lists as
 * the _word entry points. */
int sp_air_prove_int(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                     const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_int(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                           const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                           uint32_t* n_out);
int sp_air_main_trace_int(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                          uint8_t* rows_out);
int sp_air_main_check_int(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most lo + width of a LIMB op (252), out[1] = the bits an AND / OR / XOR operand must stay below 2^ of (251), out[2] = the
 * number of integer ops (4: ops 8 .. 11), out[3] = 0 */
int sp_air_main_int_limits(uint32_t out[4]);

/* ---- One multiplicity column for several looked-up columns: the usual shape of a lookup argument - the limbs of a range check, the
 * bytes of a word, a dozen cells in one 16-bit table - under ONE multiplicity column.  Through the _multi entry points - and only
 * through them: everywhere else op 12 stays a malformed op and such a pad a key_bits out of range - an SP_AIR_MAIN_COUNT column may be
 * a joint column: bit 8 of its pad is set (pad = key_bits + 256, key_bits 1 .. 64), den_op names the table value T as before, and
 * num_op names a list of 1 .. 16 looked-up values X_0 .. X_(L-1), made of cells of */
#define SP_AIR_OP_ALSO 12          /* op 12 ALSO a = an earlier value op (one X_k), b = an earlier op 12 (the rest of the list) or 0xFFFF (its end) */
#define SP_AIR_MAIN_COUNT_LIST 256 /* bit 8 of a COUNT column's pad: num_op names a list */
#define SP_AIR_LIST_END 0xFFFF
/* X_0 is the a of the cell num_op names, X_1 the a of the cell its b names, and so on.  The column is
 *   z_i = sum_k #{ j in [0, n) : X_k(j) = T(i) } if no row i' < i has T(i') = T(i), else 0,
 * and everything else is a COUNT column's rule: X_k and T are ordinary values over the inputs, earlier derived columns at shifts 0 .. 7
 * and periodic columns; a value of some X_k that no T holds is counted nowhere; a canonical integer of any X_k(j) or T(i) at or above
 * 2^key_bits fails the call with SP_E_INVALID_ARG and the COUNT columns' own words ("a lookup key is out of range on some row"), in
 * their place in the order of verdicts; n < 2^32.  A cell has no value: it is never an operand of a value op, takes none of the 64
 * live values and is never sent to the device.  Joint and plain COUNT columns count together against the 16 a program may hold.  The
 * decoder refuses, naming the column (or the op): a pad with a bit above 8; bit 8 with a num_op that is no cell, and a cell as the
 * num_op of a column without it; a cell whose a is no earlier value op, or whose b is neither 0xFFFF nor an earlier cell; a list of
 * more than 16 cells; a cell as an operand, as a den_op, as a FETCH column's v_op or behind a column of any other kind; an X_k behind an
 * op 7 or an op 8 .. 11, or one that reads a column that is not an earlier one; key_bits 0 or above 64; a joint column without a
 * table.  A COUNT column without bit 8 is the column it was, bit for bit and launch for launch.  The device sorts the table once,
 * searches it from every looked-up key and adds into one 64-bit counter per table position.  The _multi entry points accept everything
 * the _int ones do; the proof is unchanged: the same table gives the same bytes.  Argument lists as the _int entry points. */
int sp_air_prove_multi(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                       const void* inputs, uint64_t n, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
int sp_air_check_trace_multi(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_boundary_desc* bvals, const sp_air_main_desc* main,
                             const void* inputs, uint64_t n, const sp_proof_options* opt, const uint8_t* rap, sp_air_violation* out, uint32_t cap,
                             uint32_t* n_out);
int sp_air_main_trace_multi(sp_ctx* ctx, const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, const void* inputs, uint64_t n,
                            uint8_t* rows_out);
int sp_air_main_check_multi(const sp_air_desc* air, const sp_air_ext* ext, const sp_air_main_desc* main, uint64_t n);
/* out[0] = the most looked-up values of a joint COUNT column (16), out[1] = the most key bits (64), out[2] = the most COUNT columns of
 * one main program, joint and plain together (16), out[3] = 0 */
int sp_air_main_multi_limits(uint32_t out[4]);

/* verify::<Stark252PrimeField, A> (reference src/starks/verifier.rs:559-657) on the host CPU: 1 accept, 0 reject (also for
 * malformed proofs or descriptors). */
int sp_air_verify(const uint8_t* proof, uint64_t proof_len, const sp_air_desc* air, const sp_proof_options* opt);

/* ---- Cairo front-end on the host --------------------------------------------------- */

typedef struct sp_cairo_run sp_cairo_run;  /* register trace + memory + public inputs + main trace */

/* run_program + PublicInputs::from_regs_and_mem + build_main_trace for a hint-free, builtin-free program given as
 * `n_words` canonical-BE field elements (reference src/cairo/runner/run.rs:242-263). */
int sp_cairo_run_program(const uint8_t* program_words, uint64_t n_words, uint64_t max_steps, sp_cairo_run** out);
/* Same with main's entry point at address `entry_pc` (1-based; the compiled program's "main" identifier pc + 1). */
int sp_cairo_run_program_at(const uint8_t* program_words, uint64_t n_words, uint64_t entry_pc, uint64_t max_steps, sp_cairo_run** out);
/* Same for a hint-free program that declares builtins (reference tests/integration_tests.rs:151-172 `rc_program`,
 * `signed_div_rem`; run.rs:211-222): builtins_mask bit 0 = output, bit 1 = range_check.  The builtin base pointers are main's
 * implicit arguments, main returns the advanced pointers; the used range of each builtin segment becomes a memory segment of
 * the public inputs (the range-check segment switches the AIR to its 43 + 18 column layout, cairo/air.rs:623-629; the output
 * cells join the public memory, air.rs:200-206).  Range-checked values must lie in [0, 2^128). */
int sp_cairo_run_program_builtins(const uint8_t* program_words, uint64_t n_words, uint64_t entry_pc, uint64_t max_steps,
                                  uint32_t builtins_mask, sp_cairo_run** out);
/* The 22-word fibonacci program of benches/proofs/fibonacci_70000.proof with index `fib_index`. */
int sp_cairo_run_fibonacci(uint64_t fib_index, sp_cairo_run** out);
/* From cairo-run's binary dumps: .trace (24 B/row LE, register_states.rs:51-78) and .memory (8+32 B/row LE,
 * cairo_mem.rs:35-61), program occupying addresses 1..program_size. */
int sp_cairo_run_from_dumps(const uint8_t* trace, uint64_t trace_len, const uint8_t* memory, uint64_t memory_len,
                            uint64_t program_size, sp_cairo_run** out);
/* The same from what cairo-vm hands the reference IN MEMORY (run_program, reference src/cairo/runner/run.rs:64-240): regs = steps x
 * (ap, fp, pc) relocated register states, (addrs[k], values[k]) = the n_cells relocated memory cells (values 32 bytes each in
 * `fe_encoding`), and the builtin segments run.rs:211-222 reads back (seg_types: 0 = RangeCheck, 1 = Output; seg_ranges: (start, end)
 * pairs) - generate_prover_args (run.rs:242-263) without the binary dump files.  For a shim that keeps cairo-vm (hints, Cairo 1). */
int sp_cairo_run_from_arrays(const uint64_t* regs, uint64_t steps, const uint64_t* addrs, const uint8_t* values, int fe_encoding, uint64_t n_cells,
                             uint64_t program_size, const uint8_t* seg_types, const uint64_t* seg_ranges, uint32_t n_segments, sp_cairo_run** out);
/* The register states and the memory of a run in that form (cells in increasing address order): call with null buffers for the
 * two counts, then with buffers of steps x 3 words, n_cells words and n_cells x 32 bytes. */
int sp_cairo_run_export(const sp_cairo_run* run, int fe_encoding, uint64_t* steps_out, uint64_t* n_cells_out, uint64_t* regs_out, uint64_t* addrs_out,
                        uint8_t* values_out);
void sp_cairo_run_free(sp_cairo_run* run);
/* Where the front-end's time went, in ms: out = {the VM (0 for runs read from dumps), the shape pass of build_main_trace (addresses,
 * offsets, range-check and memory holes, every validity check), the upload image for the device-side trace builder, the n x cols
 * host table (0 until something asks for it: sp_cairo_run_main_trace / _columns, or a proof with SP_OPT_DEVICE_TRACE off)}. */
int sp_cairo_run_timings(const sp_cairo_run* run, double out[4]);
/* Shape of the main trace: n rows (power of two) x cols (34, or 43 with the range-check builtin). */
int sp_cairo_run_shape(const sp_cairo_run* run, uint64_t* n_rows, uint32_t* n_cols, uint64_t* num_steps);
/* Copies the row-major main trace in `fe_encoding` (n*cols*32 bytes). */
int sp_cairo_run_main_trace(const sp_cairo_run* run, int fe_encoding, uint8_t* out);
/* Fills `pi`; the pointers inside stay valid until sp_cairo_run_free(run). */
int sp_cairo_run_public_inputs(const sp_cairo_run* run, sp_cairo_public_inputs* pi);
/* The main trace as the run keeps it: column-major [cols][n_rows] in the DEVICE layout, page-locked when *pinned_out = 1 (the
 * HIP runtime was usable when the run was built).  The pointer lives as long as the run. */
int sp_cairo_run_columns(const sp_cairo_run* run, const void** cols_out, uint64_t* n_rows, uint32_t* n_cols, int* pinned_out);
/* generate_prover_args + generate_cairo_proof (reference src/cairo/runner/run.rs:242-263, src/cairo/air.rs:1165-1171) for a run
 * of this front-end.  By default the register states and the memory of the run go up and the device writes the main trace itself
 * (SP_OPT_DEVICE_TRACE; the host never builds the table); with the option off - or for a run whose memory is not one flat array -
 * the run's own column-major page-locked table goes up by DMA, column group by column group, behind the transforms of the groups
 * before it (sp_cairo_prove_columns on sp_cairo_run_columns + sp_cairo_run_public_inputs). */
int sp_cairo_prove_run(sp_ctx* ctx, const sp_cairo_run* run, const sp_proof_options* opt, uint8_t** proof_out, uint64_t* proof_len);
/* build_main_trace (reference src/cairo/execution_trace.rs:57-87) on the device: the table sp_cairo_prove_run proves (SP_OPT_DEVICE_TRACE),
 * downloaded as sp_cairo_run_main_trace would return it (row-major n x cols, `fe_encoding`) - for callers that want the table, and
 * for the parity tests of the device builder. */
int sp_cairo_run_main_trace_dev(sp_ctx* ctx, const sp_cairo_run* run, int fe_encoding, uint8_t* out);

/* verify_cairo_proof (reference src/cairo/air.rs:1176-1182, src/starks/verifier.rs:559-657) on the host CPU: returns 1 when the
 * proof is accepted, 0 when it is rejected or malformed. Ships with the library so that proofs of shapes without a golden
 * file can be checked where they are produced.
 * STRICTER THAN THE REFERENCE'S PARSER, on purpose: StarkProof::deserialize (src/starks/proof/stark.rs:225-440) reads each part inside
 * the slice its length prefix announces and the nonce from the last eight bytes, so it tolerates padding inside and behind the parts;
 * this verifier accepts only the bytes StarkProof::serialize writes (every prefix equals its part, element length 32, nothing behind the
 * nonce, Poseidon path digests below p) - a proof the reference accepts can be refused here if someone re-framed it.  After a 0,
 * sp_last_error() says which it was by its first word: "rejected:" a well-formed proof failed a verification step; "malformed:" neither
 * parser could read it; "non-canonical framing:" only this strict parser refuses it (re-serialize the proof and try again). */
int sp_cairo_verify(const uint8_t* proof, uint64_t proof_len, const sp_cairo_public_inputs* pub, const sp_proof_options* opt);
/* The same two verifiers for proofs whose commitments use another hash (SP_OPT_MERKLE_BACKEND): merkle_backend = SP_MERKLE_*.
 * With SP_MERKLE_KECCAK256 they are sp_cairo_verify / sp_air_verify. */
int sp_cairo_verify_backend(const uint8_t* proof, uint64_t proof_len, const sp_cairo_public_inputs* pub, const sp_proof_options* opt,
                            int merkle_backend);
int sp_air_verify_backend(const uint8_t* proof, uint64_t proof_len, const sp_air_desc* air, const sp_proof_options* opt, int merkle_backend);
/* Starknet Poseidon over Stark252 on the host (csrc/poseidon.h), for known-answer tests of the Poseidon backend: in = n elements in
 * the given encoding; mode 0: hash_many(in[0..n)), 1: hash(in[0], in[1]) (n = 2), 2: hash_single(in[0]) (n = 1),
 * 3: the Hades permutation of in[0..3) (n = 3; out receives three elements).  out: 32 bytes (96 for mode 3), same encoding. */
int sp_poseidon_host(int fe_encoding, int mode, const uint8_t* in, uint64_t n, uint8_t* out);
/* The reference CLI's `verify` command (src/main.rs:113-143) on the bytes of a proof file - u64_be(len(proof)) || StarkProof::serialize ||
 * PublicInputs::serialize (src/cairo/air.rs:223-276), read back as PublicInputs::deserialize does (:278-450; bytes behind num_steps are
 * ignored, public-memory addresses must fit 64 bits): 1 accepted, 0 rejected or malformed, sp_last_error() as for sp_cairo_verify.
 * benches/proofs/fibonacci_70000.proof - written by the reference itself - is accepted as it is. */
int sp_proof_file_verify(const uint8_t* file, uint64_t file_len, const sp_proof_options* opt);
int sp_proof_file_verify_backend(const uint8_t* file, uint64_t file_len, const sp_proof_options* opt, int merkle_backend);
/* CLI proof file of the reference (src/main.rs:98-102): u64_be(len(proof)) || proof || PublicInputs::serialize
 * (src/cairo/air.rs:223-276). *out is malloc'd; release with sp_free. */
int sp_proof_file_encode(const uint8_t* proof, uint64_t proof_len, const sp_cairo_run* run, uint8_t** out, uint64_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* STARK252_HIP_H */
