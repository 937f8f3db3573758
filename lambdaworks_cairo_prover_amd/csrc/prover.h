// Device-resident STARK prover state: one object per proof, driven round by round (the transcript stays on the
// host; roots go out, challenges come in).  Mirrors the round structure of reference src/starks/prover.rs:532-766.
#pragma once
#include "ctx.h"
#include "stark_kernels.h"
#include "air_desc.h"
#include "aux_kernels.h"
#include "air_aux_kernels.h"
#include "air_main_kernels.h"
#include "trace_kernels.h"
#include "cairo_host.h"
#include <vector>
#include <memory>
#include <array>
#include <initializer_list>
#include <utility>
#include <algorithm>

namespace sp {

// the bounds a statement is decoded under (air_desc.h) are the kernels'
static_assert(AIR_LIMIT_COLS == AIR_MAX_COLS && AIR_LIMIT_BOUNDARY == AIR_MAX_BOUNDARY && AIR_LIMIT_CONSTS == AIR_MAX_CONSTS && AIR_LIMIT_OPS == AIR_MAX_OPS &&
              AIR_LIMIT_AUX_SHIFT == AIR_AUX_MAX_SHIFT && AIR_MAX_STRIDE_CLASSES == AIR_MAX_STRIDE_CLASSES_DEV && AIR_MAX_STRIDE_EXEMPT_KINDS == AIR_MAX_STRIDE_KINDS_DEV &&
              AIR_MAIN_CHAIN_MAX_WIDTH == AIR_MAIN_CHAIN_WIDTH,
              "air_desc.h and the kernel headers disagree about a bound");
// Value slots of a straight-line program (ops 0 - 4 produce a value, op 5 OUT consumes op b): values that no OUT reads, directly
// or through other values, are dropped; every other value gets one of AIR_MAX_LIVE slots, released after its last use.  The ops
// must already be validated.  SP_E_UNSUPPORTED with `live_error` as sp_last_error() when more than AIR_MAX_LIVE are alive at once.
int air_assign_slots(const std::vector<AirOpHost>& ops, std::vector<AirOpDev>& out, const char* live_error);
// Tables of `cnt` periodic columns of one period p = 2^logp on a trace of 2^logn rows: vals = [cnt][p] values (overwritten),
// tab = [cnt][b][p] coset-major evaluations, entry (c, j) = P(h w_N^(j b + c)) = q(h^(n/p) w_(p b)^(j b + c)); ws: cnt * p elements.
// Periods up to AIR_PERIODIC_DIRECT_MAX by the direct kernels, longer ones by the transform plans (an inverse transform whose post
// factors scale by h^(n/p) and 1/p, then the coset-major LDE every trace column goes through).
int air_periodic_tables(hipStream_t st, NttEngine& ntt, fe* vals, fe* ws, fe* tab, uint32_t cnt, uint32_t logp, uint32_t logn, uint32_t logb, const fe& h);
// The tables of the stride class (s = 2^logs, offset) on a trace of 2^logn rows, coset-major [b][s]: u = U = x^(n/s), z = U - g^(offset n/s)
// at x = h w_N^(j b + c) (air_stride_tables with its constants).  The caller inverts z.  What composition_air calls per class and what
// sp_air_stride_table hands out.
int air_stride_class_tables(hipStream_t st, NttEngine& ntt, fe* u, fe* z, uint32_t logs, uint32_t offset, uint32_t logn, uint32_t logb, const fe& h);

struct Openings {
    uint32_t n_queries = 0, n_layers = 0, n_cols = 0, depth0 = 0;
    bool values_canonical_be = false;                            // the four value arrays hold wire-format bytes, not Montgomery limbs
    std::vector<fe> trace_evals, comp_evals;                     // [q][C], [q][2]
    std::vector<digest32> main_paths, aux_paths, comp_paths;     // [q][depth0]
    std::vector<fe> fri_evals, fri_evals_sym;                    // [q][L]
    std::vector<digest32> fri_paths, fri_paths_sym;              // [q][sum_k (depth0-k)]
};

// One violated constraint of a program AIR (sp_air_violation): kind 0 a transition constraint (index = OUT's a), 1 a boundary
// constraint (index into the descriptor's list; rows = 1, first_row = last_row = its step, value = the cell found).
struct AirViolationHost { uint32_t kind, index; uint64_t rows, first_row, last_row; fe value; };

class HostPool;   // prover.cpp: parked host threads for the upload pipeline

// Device memory that setup() does not carve: allocated on first use or grown on demand by StarkProver::grow, `cap` elements of T.
template <class T> struct DevBuf { T* p = nullptr; uint64_t cap = 0; };
// Page-locked host memory, kept until the prover goes.  ensure() sets "<what>: allocation failed" and returns SP_E_ALLOC.
struct PinnedBuf {
    void* p = nullptr; size_t bytes = 0;
    PinnedBuf() = default; PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int ensure(size_t need, const char* what, size_t headroom = 0) {   // (headroom: extra bytes when it has to be allocated anew)
        if (need <= bytes) return SP_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        if (hipHostMalloc(&p, need + headroom, hipHostMallocDefault) != hipSuccess) { p = nullptr; (void)hipGetLastError(); sp_set_error(std::string(what) + ": allocation failed"); return SP_E_ALLOC; }
        bytes = need + headroom;
        return SP_OK;
    }
};
// A staging buffer of one call outside the arena (plain hipMalloc); freed once `st` has finished with it.
struct ScopedDevAlloc {
    void* p = nullptr; hipStream_t st;
    explicit ScopedDevAlloc(hipStream_t stream) : st(stream) {}   ScopedDevAlloc(const ScopedDevAlloc&) = delete;
    ~ScopedDevAlloc() { if (p) { (void)hipStreamSynchronize(st); (void)hipFree(p); } }
    int alloc(size_t bytes, const char* who) {
        if (hipMalloc(&p, bytes) == hipSuccess) return SP_OK;
        p = nullptr; (void)hipGetLastError(); sp_set_error(std::string(who) + ": staging allocation failed"); return SP_E_ALLOC;
    }
};
// The pinned flag slot (64 bytes): flags that ride to the host behind the work they belong to.  presort_malformed and presort_wide_key
// stay adjacent and in the order of SIDE_PRESORT_MALFORMED, SIDE_PRESORT_WIDE_KEY: launch_aux_presort fills both with one copy.
struct HostFlags { int presort_malformed, presort_wide_key, _pad[2], trace_build_oob, auxp_zero_den, auxp_bad_key, auxp_missing_key, auxp_bad_word; };
// flags of the side-stream work (device): DEEP inverses, boundary inverses, the presort's malformed input / key beyond its bits
enum SideFlag { SIDE_DEEP_INV = 0, SIDE_BND_INV, SIDE_PRESORT_MALFORMED, SIDE_PRESORT_WIDE_KEY, SIDE_FLAGS };

class StarkProver : public sp_deletable {
  public:
    StarkProver(sp_ctx* ctx) : c_(ctx) {}
    ~StarkProver() override;

    int setup(uint64_t n, uint32_t main_cols, uint32_t aux_cols, bool has_rc_builtin, const ProofOptionsHost& opt);
    // round 1: interpolate + LDE + Merkle of one trace segment (0 = main, 1 = aux); rows = row-major n x cols, ABI encoding
    // rows_on_device: `rows` is device memory (same row-major ABI encoding) — no PCIe copy inside the round
    // src = TRACE_HOST_COLUMNS: column-major [cols][n] host memory (column j at src + j * col_stride * 32; col_stride 0 = n), in the
    // DEVICE layout (col_enc < 0) or an ABI encoding (col_enc = sp_fe_encoding): every column group is one DMA, no host gather
    // src = TRACE_DEVICE_BUILD: `rows` points at a TraceBuildInput - the register states and the memory of a run go up (24 B per step,
    // 32 B per cell) and the table is written by the device (trace_kernels.h)
    enum TraceSource { TRACE_HOST_ROWS = 0, TRACE_DEVICE_ROWS = 1, TRACE_HOST_COLUMNS = 2, TRACE_DEVICE_BUILD = 3 };
    struct TraceBuildInput { const TracePlan* plan; TraceImage* image; };
    int commit_trace(int segment, const uint8_t* rows, uint32_t cols, uint8_t root_out[32], TraceSource src = TRACE_HOST_ROWS,
                     int col_enc = -1, uint64_t col_stride = 0);
    // round 1, Cairo auxiliary segment built on the device from the resident main trace (reference cairo/air.rs:660-729)
    int commit_aux_cairo(const PublicInputs& pub, const fe rap[3], uint8_t root_out[32]);
    // (the column builders of a program AIR, commit_aux_program to main_program_table, are in prover_programs.cpp)
    // round 1, auxiliary segment of a program AIR built on the device from the statement's auxiliary program (st.aux, present and
    // validated: air_statement_from_c) and the RAP challenges: the sorted columns first (key pass, radix sort, gather; a key beyond its
    // bits is SP_E_INVALID_ARG), then per-row N and D, one batch inversion, an exclusive product / sum scan per column,
    // commit_segment_resident.  The columns the program may read with op 6 (a = row shift, b = column:
    // values[(i + a) mod period]) are st.aux_periodic().
    int commit_aux_program(const AirStatement& st, const std::vector<fe>& rap, uint8_t root_out[32]);
    // round 1, main segment of a program AIR with a main-trace program (st.main, present and validated: air_statement_from_c) in place
    // of commit_trace(0, ..): `inputs` - row-major n x input_cols in the context encoding, host or device memory by
    // st.main->input_location - become columns [0, input_cols); the derived columns follow in index order, in chunks that end where
    // the workspace does or before a column that reads one of the chunk's own (a shifted read needs the whole column): per chunk one
    // pass of the interpreter, one batch inversion (behind the zero guard of the INV_OR_ZERO columns), the bits, the scans; then
    // commit_segment_resident.  A zero denominator is SP_E_ZERO_INVERSE once the root is back.  Every rank builds every column.
    // From st.main_level Rec on a chain group (SP_AIR_MAIN_CHAIN) is a chunk of its own, built by one launch of air_main_chain, and op 6
    // reads st.periodic, whose raw values go up with the program; at Link a group whose columns carry k >= 1 is that launch with a lane
    // per run.  From Lk on a COUNT column (SP_AIR_MAIN_COUNT) is a chunk of its own as well: two key passes, two radix sorts and
    // air_main_count; a key out of range is SP_E_INVALID_ARG once the root is back, ahead of a zero denominator.  At Div a chain group
    // whose slotted seed or step program still holds an op 7 launches the kernel's DIV instantiation with the context's flag word - a
    // zero under a quotient is the same SP_E_ZERO_INVERSE -, every other group the instantiation it always launched.  At Fetch a run of
    // FETCH columns (SP_AIR_MAIN_FETCH) that share X, T and key_bits is a chunk of its own too: two key passes, V's terms, one radix sort
    // of the table's pairs and air_main_fetch; a key in no table row is SP_E_INVALID_ARG once the root is back, behind the key range and
    // ahead of a zero denominator.  At Word LIMB and WORD columns (SP_AIR_MAIN_LIMB, SP_AIR_MAIN_WORD) are members of a row-local chunk,
    // grouped by their operands as BIT columns are: air_main_limbs and air_main_words behind the chunk's one pass of terms; a WORD
    // operand at or above 2^bits is SP_E_INVALID_ARG once the root is back, behind a missing key and ahead of a zero denominator.
    // At Int a chain group whose slotted seed or step program still holds an op 8 .. 11 launches the kernel's INT instantiation with
    // the WORD columns' verdict word - an AND, OR or XOR operand at or above 2^251 is the same SP_E_INVALID_ARG, under a value of its
    // own -, every other group the instantiation it always launched.
    // At Multi a joint COUNT column (bit 8 of its pad, a list of op 12 cells behind num_op) is a chunk of its own: the table's key pass
    // and its sort - the only one -, one key pass for all looked-up values, and air_main_count_many, which searches the sorted table
    // from every looked-up key and adds into counters zeroed on the stream on every run; a key out of range is the COUNT columns'
    // verdict.  A COUNT column without bit 8 launches what it always launched.
    int commit_main_program(const AirStatement& st, const uint8_t* inputs, uint8_t root_out[32]);
    // the same table without the commitment, to host memory: row-major n x main_cols, context encoding (sp_air_main_trace)
    int main_program_table(const AirStatement& st, const uint8_t* inputs, uint8_t* rows_out);
    // round 2: constraint composition, H1/H2 split, LDE and commitment
    int composition(const fe rap[3], const std::vector<BoundaryConstraint>& bcs, const std::vector<fe>& b_alpha,
                    const std::vector<fe>& b_beta, const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta,
                    const std::vector<uint32_t>& degrees, const std::vector<uint32_t>& exemptions, uint8_t root_out[32]);
    // Optional, before composition() of the Cairo AIR: the exact constraint check on the trace (what decides between the 2n-point
    // and the whole-domain evaluation) needs the RAP challenges and the boundary constraints but none of the alpha / beta
    // coefficients - queued here it runs while the caller samples those ~110 challenges and composition() builds its tables.
    int composition_precheck(const fe rap[3], const std::vector<BoundaryConstraint>& bcs, uint32_t n_transitions);
    // round 2 for an AIR given as a constraint program (reference traits.rs:15-119 + evaluator.rs:38-260); rap = its RAP
    // challenges (appended to the program's constants); also sets the frame offsets used by rounds 3 and 4.
    // air: st.air as everything behind round 1 sees it (its boundary values resolved); the tables of st.periodic, the columns the
    // program reads with op 6, are built here (od_.periodic)
    int composition_air(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, const std::vector<fe>& b_alpha, const std::vector<fe>& b_beta,
                        const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta, uint8_t root_out[32]);
    // Instead of round 2, for an AIR given as a constraint program: which constraints the trace held since round 1 (d_trace_,
    // main || aux) breaks, and where - the transition constraints by index, then the boundary constraints by index (sp_air_check_trace).
    // Leaves the stage where it was: composition_air may follow.
    int check_trace_air(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, std::vector<AirViolationHost>& out);
    // round 3: H1(z^2), H2(z^2), t_j(z g^ofs_k) for every frame row k (row-major [k][j])
    int ood(const fe& z, fe* h1_z2, fe* h2_z2, std::vector<fe>& trace_ood);
    // round 4
    int deep_fri_begin(const fe& gamma, const fe& gamma_p, const std::vector<fe>& trace_gammas /*[j*2+k]*/, uint8_t root0_out[32]);
    int fri_fold_commit(const fe& zeta, uint8_t root_out[32], fe* last_value, int* is_last);
    // The whole commit phase after layer 0 without a host round trip per layer (one GPU): the launch that produces a layer's
    // root also takes the transcript step (append root, sample zeta - merkle.h FriChallenge) and leaves zeta's fold constant
    // in device memory for the next layer.  state32 = the transcript buffer after that zeta was sampled (32 bytes); roots_out =
    // the roots of the layers committed here (those after the last one committed before the call), which the caller feeds to its
    // own transcript afterwards.
    // Several ranks: with a stream-ordered transport the sharded layers are part of the chain (their digest exchange and root
    // all-gather sit on the compute stream); with blocking hooks it is available from the first layer every rank holds whole (the
    // sharded layers in front of it go through fri_fold_commit, one exchange each).  The caller passes the zeta of the layer to fold next.
    bool fri_chain_available() const { return stage_ == Stage::FriRunning && logn_ >= 2 && fri_layer_ >= 1 && (!fri_sharded(fri_layer_ - 1) || comm_async()); }
    int fri_commit_chain(const fe& zeta0, const uint8_t state32[32], std::vector<std::array<uint8_t, 32>>& roots_out, fe* last_value);
    int grind(const uint8_t challenge[32], uint8_t factor, uint64_t* nonce_out);
    // values_canonical_be: the opened field elements come back as their canonical 32-byte big-endian encodings (the proof's wire format,
    // written by the gather's launch-mate on the device) in the same `fe`-sized slots - for the whole-proof drivers, whose serializer
    // then copies bytes instead of converting 7 - 8 thousand elements on one host thread.  The round-level ABI keeps Montgomery values.
    int open(const std::vector<uint64_t>& iotas, Openings& out, bool values_canonical_be = false);

    // sp_prewarm (capi_prove.cpp): host-side plumbing of a first proof, and round 1's kernels at the real shape on arena contents
    int warm_plumbing(bool host_rows);
    int warm_round1();
    // AIRs other than Cairo: frame rows of the transition constraints (reset to {0, 1} by setup)
    void set_frame_offsets(const std::vector<uint32_t>& ofs) { offsets_ = ofs; }
    uint32_t frame_rows() const { return (uint32_t)offsets_.size(); }
    bool ready() const { return ready_; }
    uint64_t n() const { return n_; }
    uint64_t N() const { return N_; }
    uint32_t cols() const { return C_; }
    uint32_t fri_layers() const { return logn_; }
    // per-round device time of the last proof (ms, hipEvent)
    float round_ms[5] = {0, 0, 0, 0, 0};

  private:
    // One commitment tree.  Single GPU: `sub` is the whole tree (lambdaworks node order, 2 leaves - 1 nodes), top == sub.
    // Sharded: `sub` is the subtree over this rank's CONTIGUOUS 1/G of the leaves, `top` the replicated tree over the G
    // subtree roots; root = top[0].
    struct TreeBuf { digest32* sub = nullptr; digest32* top = nullptr; uint64_t sub_leaves = 0; };
    void free_all();
    // what the calls of one proof leave for each other: cleared by every setup()
    void reset_proof_flags() { bpre_valid_ = deep_pref_ = check_pending_ = presorted_ = h_full_ = false; presort_pub_ = nullptr; }
    // small device -> host read-back on the compute stream through a pinned slot, waiting by polling the stream (a blocking
    // synchronisation costs ~20 us of wake-up per Fiat-Shamir round trip; a proof has ~35 of them)
    int readback(void* dst_host, const void* src_dev, size_t bytes);
    int wait_stream();
    int alloc(void** p, size_t bytes);
    void release(void* p, size_t bytes);
    // The one grow path of the on-demand buffers: nothing to do while `elems` fit, otherwise the old block is released (release() waits
    // for its readers; a first allocation waits for nothing) and a new one allocated.  *moved: what pointed into the old block is gone.
    template <class T> int grow(DevBuf<T>& b, uint64_t elems, bool* moved = nullptr) {
        if (moved) *moved = elems > b.cap;
        if (elems <= b.cap) return SP_OK;
        release(b.p, sizeof(T) * b.cap);   b = {};
        SP_TRY(alloc(reinterpret_cast<void**>(&b.p), sizeof(T) * elems));
        b.cap = elems;
        return SP_OK;
    }
    std::vector<uint8_t> h_up_fri_, h_up_open_;   // host sides of small asynchronous uploads (fri_commit_chain, open)
    std::vector<uint64_t> h_idx_open_;
    int alloc_tree(TreeBuf& t, uint64_t leaves_total, bool sharded);
    int setup_impl(uint64_t n, uint32_t main_cols, uint32_t aux_cols, bool has_rc_builtin, const ProofOptionsHost& opt);
    bool ready_ = false;   // setup() completed: every buffer below exists
    // Commitment over `L` leaves this rank holds in local natural order (leaf l = global leaf (l << logG) | rank): hash,
    // exchange the digests so that every rank owns a contiguous range, reduce the subtree, combine the G roots.
    // ch (FRI commit chain): the launch that produces the root also takes the transcript step (merkle.h, FriChallenge); nothing is read
    // back, root_out is not written
    int commit_local(const fe* cols_dev, uint64_t stride, uint32_t ncols, uint64_t L, LdeOrder order, TreeBuf& tree, uint8_t root_out[32],
                     bool single_element_tree = false, const FriChallenge* ch = nullptr);
    // the hash of the commitments (sp_set_option SP_OPT_MERKLE_BACKEND): rows of columns, or the single elements of a FRI layer
    MerkleHash merkle_hash(bool single_element_tree) const {
        return c_->opt_merkle_backend == SP_MERKLE_POSEIDON ? (single_element_tree ? MerkleHash::POSEIDON_SINGLE : MerkleHash::POSEIDON_BATCH)
                                                            : MerkleHash::KECCAK256;
    }
    int commit_columns(const fe* cols_dev, uint64_t stride, uint32_t ncols, TreeBuf& tree, uint8_t root_out[32]) {
        return commit_local(cols_dev, stride, ncols, Nl_, lde_order(), tree, root_out);
    }
    // Round 1 of `cols` columns: interpolate_fft (natural-order trace -> bit-reversed coefficients, n^-1 h^j folded in through d_t1_),
    // then evaluate_offset_fft onto this rank's cosets, coset-major (reference trace.rs:104-110, prover.rs:161-185).  Every array
    // holds its columns back to back: n_ elements apart in trace and coeffs, Nl_ apart in lde.
    int interpolate_extend(const fe* trace, fe* coeffs, fe* lde, uint32_t cols) {
        SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(coeffs, (int)logn_, cols, n_, d_t1_, trace));
        return c_->ntt->lde_coset_major(coeffs, lde, (int)logn_, (int)logb_, cols, n_, Nl_, (int)logG_, (int)rank_);
    }
    int commit_segment_resident(int segment, uint32_t cols, uint8_t root_out[32]);
    // the ingest and the derived columns of commit_main_program, queued on the compute stream; the zero-denominator flag is on its way
    // to host_flags().auxp_zero_den behind them (prover_programs.cpp: a plan made without a HIP call, then the launches)
    int build_main_program(const AirStatement& st, const uint8_t* inputs);
    int commit_trace_pipelined(int segment, const uint8_t* rows_host, uint32_t table_cols, uint8_t root_out[32], uint32_t c_begin = 0, uint32_t c_count = 0,
                               bool window_only = false, uint32_t binary_cols = 0);
    // The first `binary_cols` columns of the main segment hold only 0 and 1 (the sixteen instruction flags of a Cairo trace, reference
    // src/cairo/air.rs:29-46: 47 % of the table): the row-major upload sends them as one bit per cell.  A hint, checked cell by cell by
    // the gather threads - a table that breaks it (an invalid trace) is uploaded again in full, so the bytes never depend on it.
    uint32_t binary_cols_hint_ = 0;
    static constexpr int SP_RETRY_RAW_UPLOAD = 1000;   // internal: the packed upload met a cell that is neither 0 nor 1
    // several ranks, row-major host table: every rank uploads the columns of its role only, the trace columns are all-gathered
    int commit_trace_rows_sharded(int segment, const uint8_t* rows_host, uint32_t cols, uint8_t root_out[32], uint32_t binary_cols = 0);
    uint32_t pending_up_groups_ = 0; uint64_t pending_up_bytes_ = 0; double pending_up_gather_ms_ = 0, pending_up_host_ms_ = 0;
    int shard_mode_ = 2;
    bool shard_interp_ = false;    // this shape interpolates by column and all-gathers coefficients (SP_OPT_SHARD_INTERPOLATION, setup())
    int commit_trace_columns(int segment, const uint8_t* cols_host, uint32_t cols, int col_enc, uint64_t col_stride, uint8_t root_out[32]);
    int commit_trace_built(const TraceBuildInput& in, uint8_t root_out[32]);
    // upload pipeline bookkeeping (sp_last_upload_stats): per column group the DMA interval on the copy stream, the moment the
    // group is usable and the moment the compute stream is done with it
    static constexpr int UPLOAD_MAX_GROUPS = 48;
    struct UploadTimers { hipEvent_t dma0 = nullptr, dma1 = nullptr, ready = nullptr, done = nullptr; };
    UploadTimers up_ev_[UPLOAD_MAX_GROUPS];
    hipEvent_t up_start_ = nullptr;
    int ensure_upload(uint32_t groups);
    int ensure_ring_and_pool();   // page-locked ring slots + parked gather threads of the row-major upload
    int finish_upload_stats(uint32_t groups, uint64_t bytes, double gather_ms, double host_ms, int kind);
    hipStream_t copy_stream_ = nullptr;                       // host-buffer uploads (commit_trace_pipelined)
    static constexpr int UPLOAD_SLOTS = 4;                    // ring of chunk slots: the gather may run three chunks ahead of the DMA
    hipEvent_t ev_dma_[UPLOAD_SLOTS] = {};
    // Two-launch leaf hashing of an uploaded segment (merkle.h): the head over the first 17 columns has run (state in d_scratch_)
    bool leaf_head_done_ = false;
    // decides it for a segment of `cols` columns that arrives over PCIe and launches the head once `cols_extended` >= 17 of them exist
    int maybe_leaf_head(uint32_t cols, uint32_t cols_extended, const fe* lde);
    bool pool_bound_ = false;                                 // the gather workers have been placed (prover_upload.cpp)
    void* h_stage_[UPLOAD_SLOTS] = {}; size_t stage_bytes_ = 0;   // pinned staging ring, one chunk (<= 32 MB) each
    HostPool* pool_ = nullptr;
    // elements of d_scratch_: inverse arrays and their scratch (<= 7 local LDE columns), OOD folds (>= 4n and the
    // per-level power tables of up to five points, which dominate for tiny traces)
    // order of the evaluations inside the trace / composition LDE columns this rank holds (coset-major, common.h)
    LdeOrder lde_order() const { return LdeOrder{1u, logb_ - logG_, logn_}; }
    // (beyond 64 columns also the first level of the out-of-domain fold of C columns at up to AIR_MAX_OFFSETS points, eval_bitrev in
    // prover.cpp: up to 64 columns the terms above hold it)
    uint64_t scratch_elems() const {
        const uint64_t ood = C_ <= 64 ? 0 : 2ull * C_ * AIR_MAX_OFFSETS * std::max<uint64_t>(1, n_ >> 8) + 8ull * AIR_MAX_OFFSETS * 256;
        return std::max<uint64_t>(std::max<uint64_t>(std::max<uint64_t>(Nl_ * 7, 4 * n_), 8192), ood);
    }
    // ---- round 2 (prover_round2.cpp)
    // the 2n-point paths of round 2 by shape: this rank holds the cosets c0 = rank and c0 + b/2 (always on one GPU), or one coset per rank (G = b)
    bool sub_coset_shape() const { return logb_ >= logG_ + 1; }
    bool pair_shape() const { return G_ > 1 && logb_ == logG_ && d_post_comp0_; }
    int fill_cairo_consts(CompositionConsts& K, const fe rap[3], const std::vector<BoundaryConstraint>& bcs, uint32_t n_transitions);
    // S: the periods, summed.  Strided constraints (air.strides): their classes and exemption products (plan), the device descriptor
    // with its pointers still unset (sdev), the exemption products' roots in the order sdev.kind_root0 names (sroots), the entries of
    // all classes' [b][s] tables (stab), where build_air_block put the descriptor in the upload (o_sdev), and per constraint the
    // exempted rows the composition really uses (ex_eff: ex_rows, or a strided constraint's own count).
    struct AirProgramHost {
        AirProgram prog; std::vector<AirOpDev> dops; std::vector<AirPeriodicCol> pcols; uint64_t S = 0; uint32_t max_ex = 0;
        AirStridePlan plan; AirStrideDev sdev; std::vector<fe> sroots; uint64_t stab = 0; size_t o_sdev = 0; std::vector<uint32_t> ex_eff;
        bool strided() const { return !plan.classes.empty(); }
    };
    int build_air_program(const AirStatement& st, const AirDescHost& air, size_t n_rap, AirProgramHost& out);
    int build_air_block(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, AirProgramHost& ph,
                        const std::vector<uint32_t>& order, std::initializer_list<std::pair<size_t, size_t*>> extra, AirCompTables& tabs,
                        const AirProgram*& prog_dev);
    struct Round2Air;   // what composition_core is given; the two members below it are where Cairo and a program AIR differ
    int round2_evaluate(const Round2Air& air, uint64_t count, uint32_t stride_log, const fe* binv, fe* out);
    int round2_boundary_inverses(const Round2Air& air, fe* binv, fe* inv_scratch, uint64_t count, uint32_t logM, const fe* roots_m, const fe& hp, ShardMap sm);
    int composition_core(Round2Air air, uint8_t root_out[32]);
    int composition_sub_coset(const Round2Air& air, int* flag, int* flag_pref);
    int composition_pair(const Round2Air& air, int* flag);
    int composition_whole_domain(const Round2Air& air);
    int split_2n_and_extend(const fe* post);
    CompositionConsts* d_comp_consts_ = nullptr;
    std::unique_ptr<CompositionConsts> h_comp_chk_;    // host copy of od_.comp_consts_chk (stays put until the upload has happened)
    bool check_pending_ = false;
    std::vector<uint8_t> h_air_up_;                    // host side of the upload into od_.air_buf
    std::vector<uint8_t> h_report_;                    // host copy of od_.air_report
    bool h_full_ = false;     // the composition polynomial of this proof has degree >= 2n: its halves are in od_.hfull
    fe* d_post_comp_ = nullptr;                        // shape-only post-factor table of the 2n-point inverse transform (setup)
    fe* d_post_comp0_ = nullptr;                       // the same for c0 = 0 (one coset per rank)
    std::vector<fe> bpre_points_; bool bpre_valid_ = false;   // od_.bpre holds the boundary inverses for these points (prefetch_boundary_inverses)

    sp_ctx* c_;
    ProofOptionsHost opt_{};
    uint64_t n_ = 0, N_ = 0;
    uint32_t logn_ = 0, logb_ = 0, logN_ = 0, Cm_ = 0, Ca_ = 0, C_ = 0;
    // Sharding: G = min(world, blowup) groups; the rank with role r = rank mod G holds the LDE points with
    // global index i = r (mod G) - the cosets c = c_loc * G + r - as Nl_ = N / G local points, local natural index
    // l = i div G.  Ranks beyond the blowup factor are replicas of the role they share (world_ > G_).
    uint32_t world_ = 1, wrank_ = 0;   // communicator size and rank
    uint32_t G_ = 1, rank_ = 0, logG_ = 0;   // groups, this rank's role, log2(G_)
    uint64_t Nl_ = 0;
    fe* d_local_ = nullptr;    // [Nl] 32-byte items: local leaf digests (send side of the exchange)
    fe* d_recv_ = nullptr;     // [Nl] 32-byte items: the digests of this rank's contiguous leaf range, by source rank
    fe* d_cstage_ = nullptr; uint32_t cpr_max_ = 0;       // [world][cpr_max][n] coefficient all-gather (column-sharded interpolation)
    digest32* d_roots_ = nullptr;                          // [world] subtree roots
    // Every device buffer that is allocated on first use or grown on demand (grow()); free_all() resets the struct as a whole.
    struct OnDemand {
        DevBuf<fe> gather;                       // all-gather landing zone
        DevBuf<fe> small;                        // out-of-domain values of this rank's columns and their all-gather
        DevBuf<fe> fullN;                        // [N] whole-domain scratch when FRI layer 0 is sharded (exceptional paths)
        DevBuf<int> flags_all;                   // [world] flags of the row-sharded trace check
        DevBuf<fe> deepx;                        // DEEP inverses when they outgrow the shared scratch
        DevBuf<uint64_t> flagbits;               // the 0 / 1 columns of a row-major upload as bitmaps (binary_cols_hint_)
        DevBuf<CompositionConsts> comp_consts_chk;   // the constants of an early constraint check (composition_precheck)
        DevBuf<uint8_t> air_buf; DevBuf<fe> ex_roots;   // program AIRs (composition_air): header, ops, constants and per-proof tables in one buffer; exempted rows' roots
        // auxiliary programs (commit_aux_program): ops, constants and column tables of every chunk in one buffer, and the N / D
        // workspace (denominators, batch-inversion scratch, scan block totals - or, before those, one sort group's carried values,
        // (key, row) pairs and radix histograms); kept across proofs of a shape
        DevBuf<uint8_t> auxp_buf; DevBuf<fe> auxp_ws;
        DevBuf<uint64_t> air_report;             // check_trace_air: per-constraint counters, values and boundary results, one block (AirReport)
        DevBuf<fe> stride;                       // strided constraints of a program AIR: [E] U, [E] 1 / Z, [E] scratch (E = b x the classes' periods, summed)
        DevBuf<fe> periodic;                     // periodic columns of a program AIR: [b S] tables, [S] values being transformed, [S] scratch (S = sum of the periods)
        DevBuf<uint8_t> fri_chain;               // [state 32 B][L x constants][L x zeta constants][L x roots]
        DevBuf<int> side_flags;                  // [SIDE_FLAGS]
        DevBuf<fe> bpre;                         // [3][2n] boundary inverses + [3][2n] scratch
        DevBuf<uint8_t> auxws;                   // workspace of the Cairo auxiliary trace, carved into auxws_ for auxws_pm_ public cells
        DevBuf<fe> hfull, hnat;                  // general (degree >= 2n) composition polynomial: N/2 coefficients per half; its natural-order staging
    } od_;
    // the slice of the trace rows this rank checks in round 2 (the Cairo constraint check is row-local: the trace is replicated)
    uint64_t check_row0() const { return (world_ > 1 && n_ >= 256ull * world_) ? (n_ / world_) * wrank_ : 0; }
    uint64_t check_rows() const { return (world_ > 1 && n_ >= 256ull * world_) ? (wrank_ + 1 == world_ ? n_ - (n_ / world_) * wrank_ : n_ / world_) : n_; }
    int ensure_gather(uint64_t elems) { return grow(od_.gather, elems); }
    int ensure_deep_scratch(uint64_t elems);
    // columns by role (several ranks): role r works on the cols_per_role columns from role_first_col on (the last blocks overlap
    // instead of being ragged)
    uint32_t cols_per_role(uint32_t cols) const { return (cols + G_ - 1) / G_; }
    uint32_t role_first_col(uint32_t role, uint32_t cols) const { return std::min(role * cols_per_role(cols), cols - cols_per_role(cols)); }
    int full_domain_buffer(fe** out);
    // stream_ordered: the caller consumes the result on the compute stream only (or waits for that stream itself): with a transport
    // that can enqueue on a stream the exchange takes its place between the kernels instead of costing a host round trip
    int all_gather(const void* send_dev, void* recv_dev, uint64_t bytes_per_rank, bool stream_ordered = false);
    // The same in two halves: begin() starts the exchange behind everything queued on the compute stream so far - on the
    // communication stream when the transport is stream-ordered, by blocking in the hook otherwise - and end() makes the compute
    // stream wait for it.  What is queued on the compute stream between the two runs beside the exchange.
    static constexpr int COMM_BLOCKS = 4;
    hipStream_t comm_stream_ = nullptr;
    hipEvent_t ev_comm_fork_ = nullptr, ev_comm_done_[COMM_BLOCKS] = {};
    bool comm_async() const { return c_->allgather_async != nullptr; }
    int all_gather_begin(const void* send_dev, void* recv_dev, uint64_t bytes_per_rank, int slot);
    int all_gather_end(int slot);
    void count_all_gather(uint64_t bytes_per_rank) { c_->stat_ag_calls += 1; c_->stat_ag_bytes += bytes_per_rank; c_->stat_recv_bytes += bytes_per_rank * (world_ - 1); }
    void count_all_to_all(uint64_t bytes) { c_->stat_a2a_calls += 1; c_->stat_a2a_bytes += bytes * (G_ - 1); c_->stat_recv_bytes += bytes * (G_ - 1); }
    // recv[s] = the block rank s addressed to this role: send = [G][bytes], recv = [G][bytes]
    int exchange_blocks(const void* send_dev, void* recv_dev, uint64_t bytes_per_block, bool stream_ordered = false);
    ShardMap shard_map() const { return ShardMap{logb_, logG_, rank_}; }
    fe rank_coset_offset() const { return fe_mul(h_, fe_pow_u64(host_primitive_root((int)logN_), rank_)); }   // h w_N^rank: offset of this rank's first coset
    bool has_rc_ = false;
    fe h_, hinv_, g_;                       // coset offset, its inverse, trace generator
    std::vector<void*> allocs_;             // buffers outside the arena (grown on demand, or when the arena could not be had)
    uint64_t alloc_bytes_ = 0;              // bytes of those
    // One device allocation for everything setup() sizes: a context that proves traces of different shapes re-carves it instead
    // of freeing and allocating ~25 buffers (22 GB at config #3) - hipFree / hipMalloc of that took 35 ms on some boxes of the
    // pool and 0.4 - 1.9 s on others (profiles/r03_pinned_upload.txt).  It only ever grows.
    uint8_t* arena_ = nullptr;
    uint64_t arena_cap_ = 0, arena_off_ = 0;
    bool measuring_ = false; uint64_t measured_ = 0;
    void publish_device_bytes() { c_->prover_device_bytes = arena_cap_ + alloc_bytes_; }
    fe *d_coeffs_ = nullptr, *d_lde_ = nullptr, *d_t1_ = nullptr, *d_t2_ = nullptr;
    fe* d_trace_ = nullptr;  // [C][n] the trace itself, natural order (kept for the constraint check of round 2)
    fe *d_h12s_ = nullptr, *d_h12_ = nullptr, *d_scratch_ = nullptr;  // scratch: 4N elements
    TreeBuf tree_main_, tree_aux_, tree_comp_;
    // FRI layer k: N >> k evaluations; layers below fri_rep_ are sharded (local natural order, N >> k >> logG elements and
    // a sharded tree), the others replicated on every rank
    std::vector<fe*> d_fri_evals_;
    std::vector<TreeBuf> fri_trees_;
    uint32_t fri_rep_ = 0;                  // first replicated layer (0: the whole FRI is replicated)
    bool fri_sharded(uint32_t k) const { return k < fri_rep_; }
    uint32_t fri_layer_ = 0;                // number of committed layers so far
    fe fri_offset_, fri_offset_inv_;        // h^(2^layer) and its inverse
    fe half_, binv_;                        // 1/2, 1/blowup
    std::vector<uint8_t> h_auxp_up_;                   // host side of the upload into od_.auxp_buf
    DeepConsts* d_deep_consts_ = nullptr;
    fe* d_deep_gammas_ = nullptr;                      // [AIR_MAX_OFFSETS][C], behind the DeepConsts in the same allocation
    static size_t deep_gammas_at() { return (sizeof(DeepConsts) + 255) & ~size_t(255); }
    unsigned long long* d_nonce_ = nullptr;
    PinnedBuf h_pin_;         // for readback(): 4 KB, more when a report asks for it
    PinnedBuf h_open_pin_;    // landing zone of the openings' download (kept across proofs)
    PinnedBuf h_flags_;       // HostFlags
    int ensure_pin() { return h_pin_.ensure(4096, "pinned read-back slot"); }
    int ensure_host_flags() { return h_flags_.ensure(64, "pinned flag slot"); }
    HostFlags& host_flags() { return *static_cast<HostFlags*>(h_flags_.p); }
    // Side stream: latency-bound work that does not wait for the next challenge runs beside the compute stream instead of in
    // its way - a batch inversion is one chain of ~260 dependent field products (~0.3 ms whatever the size).
    //   * boundary denominators 1 / (x - g^step) of round 2 (shape and public inputs only): during round 1;
    //   * DEEP denominators 1 / (x - z g^k), 1 / (x - z^2) of round 4 (known once z is sampled): during round 3;
    //   * the range-check half of the Cairo auxiliary trace beside its memory half.
    hipStream_t side_stream_ = nullptr;
    hipEvent_t ev_side_fork_ = nullptr, ev_side_deep_ = nullptr, ev_side_bnd_ = nullptr, ev_side_aux_ = nullptr;
    int ensure_side();
    int ensure_side_flags() { return grow(od_.side_flags, SIDE_FLAGS); }
    int* side_flag(SideFlag f) { return od_.side_flags.p + f; }
    int prefetch_deep_inverses();           // from ood(): z_ is set
    bool deep_pref_ = false;
    // the challenge-free part of the Cairo auxiliary trace (sorts) beside round 1's transforms and hashing
    const PublicInputs* presort_pub_ = nullptr; bool presorted_ = false;
    hipEvent_t ev_side_presort_ = nullptr;
    std::vector<fe> pm_addr_h_, pm_val_h_;  // get_pub_memory_addrs and the matching values (host copies behind the async uploads)
    int public_memory_lists(const PublicInputs& pub);
    int ensure_aux_workspace(uint64_t pm);
    int launch_aux_presort();               // from commit_trace(0, ..) once the main trace columns are queued
  public:
    // round 2's boundary denominators ahead of time (whole-proof entry points call it before round 1; optional)
    int prefetch_boundary_inverses(const std::vector<uint64_t>& steps);
    // optional, before commit_trace(0, ..) of a Cairo proof: sort the memory accesses and the offsets while round 1 runs
    void request_aux_presort(const PublicInputs& pub) { presort_pub_ = &pub; }
    // optional, before commit_trace(0, ..) from a row-major host table: columns [0, count) are 0 / 1 in a valid trace
    void hint_binary_columns(uint32_t count) { binary_cols_hint_ = count; }
  private:
    fe* d_memcols_ = nullptr;               // natural-order main-trace columns 19..29 kept for the auxiliary trace
    AuxWorkspace auxws_{}; uint64_t auxws_pm_ = 0;
    fe* d_post_deep_ = nullptr;             // shape-only post-factor table of round 4 (setup)
    fe z_; fe h1_z2_, h2_z2_;
    std::vector<fe> trace_ood_;
    std::vector<uint32_t> offsets_{0, 1};   // transition offsets of the AIR (frame rows); Cairo: {0, 1}
    enum class Stage { New, Setup, MainCommitted, AuxCommitted, Composed, OodDone, FriRunning, FriDone };
    Stage stage_ = Stage::New;
    // round 1 is over: both segments, or the main segment of an AIR without auxiliary columns
    bool segments_committed() const { return stage_ == Stage::AuxCommitted || (stage_ == Stage::MainCommitted && Ca_ == 0); }
    void segment_committed(int segment) { stage_ = segment == 0 ? Stage::MainCommitted : Stage::AuxCommitted; }
};

// The prover of a context with the host-side buffers of the round-level ABI: one object whichever entry point created it, so a
// caller can size and warm everything with sp_prove_setup while its trace is still being built and prove with any of them.
struct ProverHolder : public sp_deletable {
    StarkProver prover;
    Openings open;
    std::vector<uint8_t> trace_evals, comp_evals, fri_evals, fri_evals_sym;
    float round_ms[5] = {0, 0, 0, 0, 0};
    hipEvent_t round_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // round timing of the whole-proof drivers (created once, kept)
    explicit ProverHolder(sp_ctx* c) : prover(c) {}
    ~ProverHolder() override { for (auto& e : round_ev) if (e) (void)hipEventDestroy(e); }
};
ProverHolder* prover_holder(sp_ctx* c, bool create);

// Whole proof on the device: generate_cairo_proof (reference src/cairo/air.rs:1165-1171) + serialize
// (src/starks/proof/stark.rs:161-218). main_trace: row-major n x cols in the context encoding.
int cairo_prove(sp_ctx* ctx, const uint8_t* main_trace, uint64_t n, uint32_t cols, const PublicInputs& pub,
                const ProofOptionsHost& opt, std::vector<uint8_t>& proof_out, float round_ms[5],
                StarkProver::TraceSource src = StarkProver::TRACE_HOST_ROWS, int col_enc = -1, uint64_t col_stride = 0);
// Whole proof for an AIR given as a constraint program: `prove::<F, A>` (reference src/starks/prover.rs:532-766) + serialize.
// st: the statement as air_statement_from_c accepted it for n rows.  main_trace: row-major n x st.air.main_cols in the context
// encoding (host memory).  round_ms: device time of rounds 1 - 4 in [1..4], as cairo_prove.
int air_prove(sp_ctx* ctx, const AirStatement& st, const uint8_t* main_trace, uint64_t n, const ProofOptionsHost& opt, std::vector<uint8_t>& proof_out,
              float round_ms[5]);
// With st.main (a main-trace program) main_trace holds the input columns only - row-major n x st.main->input_cols, host or device memory
// by st.main->input_location - here and in air_check_trace.  air_main_trace: the table that program builds, row-major n x main_cols in
// the context encoding, to host memory; no commitment.
int air_main_trace(sp_ctx* ctx, const AirStatement& st, const uint8_t* inputs, uint64_t n, uint8_t* rows_out);
// Which constraints of a program AIR a trace breaks, and where (sp_air_check_trace): round 1 as air_prove runs it - the same ingest and
// auxiliary builders -, then StarkProver::check_trace_air; no proof.  rap_given (nullable): the RAP challenges, instead of the ones a
// proof under *opt would sample; opt may be null only with them.  One GPU (SP_E_UNSUPPORTED on a context with world > 1).
int air_check_trace(sp_ctx* ctx, const AirStatement& st, const uint8_t* main_trace, uint64_t n, const ProofOptionsHost* opt,
                    const std::vector<fe>* rap_given, std::vector<AirViolationHost>& out);

}  // namespace sp
