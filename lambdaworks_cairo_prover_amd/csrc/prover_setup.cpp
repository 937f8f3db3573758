// Lifetime, memory and transport of the prover (see prover.h): what setup() carves and what grows on demand, the first-proof
// warm-up, and the collectives between ranks.  The rounds themselves are in prover.cpp.
#include "prover_internal.h"

namespace sp {

void host_pool_delete(HostPool* p);

StarkProver::~StarkProver() {
    free_all();
    if (arena_) (void)hipFree(arena_);
    arena_ = nullptr; arena_cap_ = 0;
    c_->prover_device_bytes = 0;
    for (auto& e : ev_dma_) if (e) (void)hipEventDestroy(e);
    for (auto& u : up_ev_) for (hipEvent_t e : {u.dma0, u.dma1, u.ready, u.done}) if (e) (void)hipEventDestroy(e);
    if (up_start_) (void)hipEventDestroy(up_start_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    if (pool_) host_pool_delete(pool_);
    for (auto& p : h_stage_) { if (p) (void)hipHostFree(p); p = nullptr; }
    for (hipEvent_t e : {ev_side_fork_, ev_side_deep_, ev_side_bnd_, ev_side_aux_, ev_side_presort_}) if (e) (void)hipEventDestroy(e);
    if (side_stream_) (void)hipStreamDestroy(side_stream_);
    if (ev_comm_fork_) (void)hipEventDestroy(ev_comm_fork_);
    for (auto& e : ev_comm_done_) if (e) (void)hipEventDestroy(e);
    if (comm_stream_) (void)hipStreamDestroy(comm_stream_);
}

int StarkProver::ensure_side() {
    if (!side_stream_) SP_HIP_CHECK(hipStreamCreateWithFlags(&side_stream_, hipStreamNonBlocking));
    for (hipEvent_t* e : {&ev_side_fork_, &ev_side_deep_, &ev_side_bnd_, &ev_side_aux_, &ev_side_presort_})
        if (!*e) SP_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return SP_OK;
}

void StarkProver::free_all() {
    (void)hipSetDevice(c_->device);
    (void)hipStreamSynchronize(c_->stream);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    if (side_stream_) (void)hipStreamSynchronize(side_stream_);
    if (comm_stream_) (void)hipStreamSynchronize(comm_stream_);
    od_ = {};            // carved from the arena / allocs_ like the rest: gone with the shape
    reset_proof_flags();
    // (the page-locked buffers do not depend on the shape: they stay until the prover goes)
    for (void* p : allocs_) (void)hipFree(p);
    allocs_.clear();
    alloc_bytes_ = 0;
    arena_off_ = 0;      // the arena itself stays: the next shape is carved out of it
    publish_device_bytes();
}

int StarkProver::alloc(void** p, size_t bytes) {
    const uint64_t aligned = ((uint64_t)(bytes ? bytes : 1) + 255) & ~(uint64_t)255;
    if (measuring_) { *p = reinterpret_cast<void*>(uintptr_t(256)); measured_ += aligned; return SP_OK; }   // (sizing pass of setup_impl)
    if (arena_ && arena_off_ + aligned <= arena_cap_) {
        *p = arena_ + arena_off_;
        arena_off_ += aligned;
        return SP_OK;
    }
    *p = nullptr;
    if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        sp_set_error("hipMalloc failed (" + std::to_string(bytes) + " bytes)");
        return SP_E_ALLOC;
    }
    allocs_.push_back(*p);
    alloc_bytes_ += bytes;
    publish_device_bytes();
    return SP_OK;
}

int StarkProver::setup(uint64_t n, uint32_t main_cols, uint32_t aux_cols, bool has_rc, const ProofOptionsHost& opt) {
    const int rc = setup_impl(n, main_cols, aux_cols, has_rc, opt);
    if (rc != SP_OK) {   // a failed (re)shaping leaves nothing behind: the next setup() of the same shape starts from scratch
        free_all();
        n_ = 0; ready_ = false; stage_ = Stage::New;
    }
    return rc;
}

int StarkProver::setup_impl(uint64_t n, uint32_t main_cols, uint32_t aux_cols, bool has_rc, const ProofOptionsHost& opt) {
    offsets_ = {0, 1};
    int k = sp_log2_exact(n), lb = sp_log2_exact(opt.blowup_factor);
    if (k < 1 || lb < 1 || k + lb > 30 || (1u << lb) > CAIRO_MAX_BLOWUP) { sp_set_error("setup: trace length and blowup factor must be powers of two (blowup 2 .. 128, at most 2^30 LDE points)"); return SP_E_INVALID_ARG; }
    if (main_cols + aux_cols > (uint32_t)AIR_MAX_COLS) { sp_set_error("setup: more than 1024 trace columns (main + aux)"); return SP_E_INVALID_ARG; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    if (c_->world < 1 || (c_->world & (c_->world - 1)) || c_->rank < 0 || c_->rank >= c_->world) {
        sp_set_error("setup: world size must be a power of two");
        return SP_E_INVALID_ARG;
    }
    if (c_->world > 1 && !c_->allgather) { sp_set_error("setup: world > 1 needs sp_set_collective / sp_comm_init_rccl"); return SP_E_STATE; }
    if (ready_ && (arena_ || !allocs_.empty()) && n == n_ && main_cols == Cm_ && aux_cols == Ca_ && has_rc == has_rc_ && opt.blowup_factor == opt_.blowup_factor &&
        opt.coset_offset == opt_.coset_offset && (uint32_t)c_->world == world_ && (uint32_t)c_->rank == wrank_ && c_->opt_shard_interpolation == shard_mode_) {
        // same shape as the previous proof on this context: keep every device buffer and table
        opt_ = opt; stage_ = Stage::Setup; fri_layer_ = 0;
        reset_proof_flags();
        return SP_OK;
    }
    free_all();
    ready_ = false; stage_ = Stage::New;
    opt_ = opt; n_ = n; logn_ = (uint32_t)k; logb_ = (uint32_t)lb; logN_ = logn_ + logb_; N_ = n << lb;
    Cm_ = main_cols; Ca_ = aux_cols; C_ = main_cols + aux_cols; has_rc_ = has_rc;
    world_ = (uint32_t)c_->world; wrank_ = (uint32_t)c_->rank; shard_mode_ = c_->opt_shard_interpolation;
    // one or more LDE cosets per group; with more ranks than cosets the surplus ranks replicate a role (moving half a coset's
    // LDE over one xGMI link costs more than computing it)
    G_ = std::min<uint32_t>(world_, 1u << lb); logG_ = (uint32_t)sp_log2_exact(G_); rank_ = wrank_ & (G_ - 1);
    Nl_ = N_ >> logG_;
    // Interpolation by column with an all-gather of the coefficients, or on every rank?  A rank saves
    // (1 - 1/G) of the size-n inverse transforms (n log n / 2 butterflies per column at ~1.35e11 / s) and receives (1 - 1/G) of the
    // coefficients (32 n bytes per column over G - 1 links): sharding pays when  64 x 1.35e11 < (G - 1) x link bytes/s x log2 n.
    // (sp_model_shard_interpolation.)  On 46 GB/s per link that needs (G - 1) log2 n > 188 - no shape this prover sees - so mode 2
    // interpolates everywhere unless the fabric is faster: the rate sp_comm_measure found (sp_comm_init_rccl runs it once per
    // communicator) or the one the caller states (SP_OPT_LINK_GBS wins); an exchange that overlaps the transforms completely
    // (stream-ordered transport) is worth at most the inverse transforms it replaces, 3 - 5 ms at 2^20 rows.
    shard_interp_ = false;
    if (G_ > 1) {
        if (c_->opt_shard_interpolation == 1) shard_interp_ = true;
        else if (c_->opt_shard_interpolation == 2) shard_interp_ = sp_model_shard_interpolation(c_->link_gbs_for_model(), G_, (uint32_t)k) == 1;
        // SP_COMM_LOG: the mode and the rate it was chosen from, once per set-up shape and rank (what a first multi-GPU run is read by)
        static const bool comm_log = std::getenv("SP_COMM_LOG") != nullptr;
        if (comm_log)
            std::fprintf(stderr, "[stark252 rank %u/%u] 2^%d rows, %u groups: interpolation %s (SP_OPT_SHARD_INTERPOLATION = %d; link %.1f GB/s per direction - %s; by column pays above %.1f)\n",
                         wrank_, world_, k, G_, shard_interp_ ? "by column + coefficient all-gather" : "on every rank", c_->opt_shard_interpolation, c_->link_gbs_for_model(),
                         c_->opt_link_gbs_explicit ? "stated" : (c_->measured_link[1] > 0 ? "measured all-gather rate / 1.25" : "assumed"),
                         64.0 * 1.35e11 / ((double)(G_ - 1) * (double)k) / 1e9);
    }
    if (G_ > 1 && N_ < 2ull * G_ * G_) { sp_set_error("setup: the LDE domain is too small for this many ranks"); return SP_E_INVALID_ARG; }
    double _tp = wall_ms();
    sp_ctx* ctx = c_;
    h_ = fe_from_u64(opt.coset_offset);
    if (fe_is_zero(h_)) return SP_E_INVALID_ARG;
    hinv_ = fe_inv(h_);
    half_ = fe_inv(fe_from_u64(2)); binv_ = fe_inv(fe_from_u64(1ull << lb));
    g_ = host_primitive_root((int)logn_);
    // Every buffer whose size setup() knows, in one pass that runs twice: first to size the arena, then to carve it.
    auto allocate_all = [&]() -> int {
        SP_TRY(alloc((void**)&d_coeffs_, sizeof(fe) * n_ * C_));
        SP_TRY(alloc((void**)&d_trace_, sizeof(fe) * n_ * C_));
        SP_TRY(alloc((void**)&d_lde_, sizeof(fe) * std::max<uint64_t>(Nl_, n_) * C_));  // >= n per column: also stages the raw rows
        SP_TRY(alloc((void**)&d_t1_, sizeof(fe) * n_));
        SP_TRY(alloc((void**)&d_t2_, sizeof(fe) * n_));
        SP_TRY(alloc((void**)&d_h12s_, sizeof(fe) * n_ * 2));
        SP_TRY(alloc((void**)&d_h12_, sizeof(fe) * Nl_ * 2));
        SP_TRY(alloc((void**)&d_scratch_, sizeof(fe) * scratch_elems()));
        d_local_ = d_recv_ = d_cstage_ = nullptr; d_roots_ = nullptr;   // (several ranks only)
        if (G_ > 1) {
            SP_TRY(alloc((void**)&d_local_, sizeof(fe) * Nl_));
            SP_TRY(alloc((void**)&d_recv_, sizeof(fe) * Nl_));
            SP_TRY(alloc((void**)&d_roots_, sizeof(digest32) * world_));
            if (shard_interp_) {
                cpr_max_ = (std::max(Cm_, Ca_) + G_ - 1) / G_;
                SP_TRY(alloc((void**)&d_cstage_, sizeof(fe) * (uint64_t)world_ * cpr_max_ * n_));
            }
        }
        SP_TRY(alloc_tree(tree_main_, N_, G_ > 1));
        SP_TRY(alloc_tree(tree_aux_, N_, G_ > 1));
        SP_TRY(alloc_tree(tree_comp_, N_, G_ > 1));
        SP_TRY(alloc((void**)&d_comp_consts_, sizeof(CompositionConsts)));
        // DeepConsts, then gamma_{j,k} as [frame rows][columns]: one upload per proof
        SP_TRY(alloc((void**)&d_deep_consts_, deep_gammas_at() + sizeof(fe) * AIR_MAX_OFFSETS * C_));
        d_deep_gammas_ = reinterpret_cast<fe*>(reinterpret_cast<uint8_t*>(d_deep_consts_) + deep_gammas_at());
        SP_TRY(alloc((void**)&d_nonce_, sizeof(unsigned long long)));
        // FRI: layers of at least 2^opt_fri_shard_min_log leaves (and at least 2 G^2, so that every rank owns whole blocks of the
        // digest exchange) stay sharded; from layer fri_rep_ on every rank holds the whole layer.  The last, uncommitted fold
        // output (layer log n) is always replicated.
        fri_rep_ = 0;
        if (G_ > 1)
            while (fri_rep_ < logn_ && (N_ >> fri_rep_) >= std::max<uint64_t>(1ull << c_->opt_fri_shard_min_log, 2ull * G_ * G_)) ++fri_rep_;
        d_fri_evals_.clear(); fri_trees_.clear();
        for (uint32_t l = 0; l <= logn_; ++l) {
            fe* e = nullptr;
            const uint64_t M = N_ >> l;
            SP_TRY(alloc((void**)&e, sizeof(fe) * (fri_sharded(l) ? M >> logG_ : M)));
            d_fri_evals_.push_back(e);
            if (l < logn_) { TreeBuf t; SP_TRY(alloc_tree(t, M, fri_sharded(l))); fri_trees_.push_back(t); }
        }
        SP_TRY(alloc((void**)&d_post_comp_, sizeof(fe) * 2 * n_));
        SP_TRY(alloc((void**)&d_post_deep_, sizeof(fe) * n_));
        d_post_comp0_ = nullptr;
        if (G_ > 1 && logG_ == logb_) SP_TRY(alloc((void**)&d_post_comp0_, sizeof(fe) * 2 * n_));
        return SP_OK;
    };
    measuring_ = true; measured_ = 0;
    const int rc_measure = allocate_all();
    measuring_ = false;
    SP_TRY(rc_measure);
    {
        // room for what a Cairo proof allocates on first use (auxiliary-trace workspace, side-stream inverses): those allocations find
        // their place in the arena too instead of costing a hipMalloc each
        size_t sort_tmp = 0;
        const uint64_t lazy = (Ca_ == 18 ? aux_workspace_bytes(n_, 4096, &sort_tmp) : 0) + sizeof(fe) * 19 * n_ + (4u << 20);
        const uint64_t need = measured_ + lazy;
        if (arena_cap_ < need) {
            if (arena_) (void)hipFree(arena_);
            arena_ = nullptr; arena_cap_ = 0;
            void* a = nullptr;
            if (hipMalloc(&a, need) == hipSuccess) { arena_ = static_cast<uint8_t*>(a); arena_cap_ = need; }
            else (void)hipGetLastError();     // no single block of that size: the buffers are allocated one by one
        }
        arena_off_ = 0;
        publish_device_bytes();
    }
    SP_TRY(allocate_all());
    d_memcols_ = d_trace_ + 19 * n_;  // pc .. off_op1 columns of the main trace (input of the Cairo auxiliary trace)
    SP_TIMEPOINT("  setup: device allocations");
    // T1[q] = n^-1 h^rev(q): turns the unscaled DIF output into h-scaled coefficients c_k h^k (bit-reversed order)
    fe ninv = fe_inv(fe_from_u64(n_));
    SP_TRY(gen_power_table(c_->stream, d_t1_, n_, logn_, h_, ninv));
    // T2[q] = N^-1 h^-rev(q): composition-polynomial split
    fe Ninv = fe_inv(fe_from_u64(N_));
    SP_TRY(gen_power_table(c_->stream, d_t2_, n_, logn_, hinv_, Ninv));
    const fe* roots = nullptr;
    SP_TRY(c_->ntt->roots((int)logN_, &roots));
    // post factors of the 2n-point composition split and of the one-coset DEEP interpolation: functions of the shape and of
    // this rank's first coset only, so they are generated once per setup instead of once per proof
    {
        const fe wN = host_primitive_root((int)logN_);
        const fe u = fe_inv(fe_pow_u64(wN, rank_));  // w_N^-c0
        const fe minv = fe_inv(fe_from_u64(2 * n_));
        const fe base = fe_mul(hinv_, fe_sqr(u));
        SP_TRY(gen_power_table(c_->stream, d_post_comp_, n_, logn_, base, minv));
        SP_TRY(gen_power_table(c_->stream, d_post_comp_ + n_, n_, logn_, base, fe_mul(minv, fe_mul(hinv_, u))));
        SP_TRY(gen_power_table(c_->stream, d_post_deep_, n_, logn_, u, fe_inv(fe_from_u64(n_))));
        if (d_post_comp0_) {   // one coset per rank: the composition pair (0, b/2) is interpolated with c0 = 0 everywhere
            SP_TRY(gen_power_table(c_->stream, d_post_comp0_, n_, logn_, hinv_, minv));
            SP_TRY(gen_power_table(c_->stream, d_post_comp0_ + n_, n_, logn_, hinv_, fe_mul(minv, hinv_)));
        }
    }
    SP_TIMEPOINT("  setup: tables");
    ready_ = true;
    stage_ = Stage::Setup;
    return SP_OK;
}

// sp_prewarm, first half: everything a first proof would otherwise create on its critical path that is not device memory of the
// shape - the page-locked read-back slots (hipHostMalloc costs ~1 ms a piece), the side stream and its events, the copy stream
// and the upload timers, and for callers of the row-major entry points the page-locked ring and the parked gather threads.
int StarkProver::warm_plumbing(bool host_rows) {
    SP_HIP_CHECK(hipSetDevice(c_->device));
    SP_TRY(ensure_pin());
    SP_TRY(ensure_host_flags());
    SP_TRY(ensure_side());
    SP_TRY(ensure_upload((uint32_t)UPLOAD_MAX_GROUPS));
    if (host_rows) SP_TRY(ensure_ring_and_pool());
    return SP_OK;
}
// sp_prewarm, second half: round 1's kernel sequence at the REAL shape on whatever the arena holds (the transforms have no
// data-dependent control flow and accept any 256-bit operand; the hash kernels convert and absorb whatever they read) - the
// size-specific kernel variants take their first launch here, and the device reaches its clocks before the trace exists.
int StarkProver::warm_round1() {
    if (!ready_ || stage_ != Stage::Setup) return SP_E_STATE;
    SP_HIP_CHECK(hipSetDevice(c_->device));
    SP_HIP_CHECK(hipMemsetAsync(d_trace_, 0, sizeof(fe) * n_ * C_, c_->stream));
    // Column slice by column slice, with a look at sp_prewarm_cancel's flag between slices: a caller whose trace is ready does not wait
    // for the rest of the ramp.  The whole of it costs 15 ms at config #4's shape and 50 ms at config #3's and makes the first proof
    // 1 - 2 ms faster than a fifth of it does (tools/experiments/ab_prewarm_r1.sh; SP_PREWARM_R1_FRAC bounds it for experiments).
    static const double frac = [] { const char* e = std::getenv("SP_PREWARM_R1_FRAC"); return e ? std::min(1.0, std::max(0.0, std::atof(e))) : 1.0; }();
    auto cancelled = [this] { return c_->prewarm_cancel.load(std::memory_order_acquire) != 0; };
    bool stop = false;
    for (int seg = 0; seg < 2 && !stop; ++seg) {
        const uint32_t col0 = seg ? Cm_ : 0, cols = seg ? Ca_ : Cm_;
        if (!cols) continue;
        const uint32_t tc = std::max<uint32_t>(1, (uint32_t)(cols * frac)), slice = std::max<uint32_t>(1, cols / 8);
        for (uint32_t c0 = 0; c0 < tc && !stop; c0 += slice) {
            const uint32_t w = std::min(slice, tc - c0);
            SP_TRY(interpolate_extend(d_trace_ + (uint64_t)(col0 + c0) * n_, d_coeffs_ + (uint64_t)(col0 + c0) * n_, d_lde_ + (uint64_t)(col0 + c0) * Nl_, w));
            SP_TRY(wait_stream());
            stop = cancelled();
        }
        if (stop || tc < cols) break;
        TreeBuf& t = seg ? tree_aux_ : tree_main_;
        const MerkleHash mh = merkle_hash(false);
        if (t.top == t.sub) {
            SP_TRY(merkle_hash_leaves(c_->stream, d_lde_ + (uint64_t)col0 * Nl_, Nl_, cols, Nl_, t.sub, lde_order(), mh));
            SP_TRY(merkle_reduce(c_->stream, t.sub, Nl_, nullptr, mh));
        } else {
            SP_TRY(merkle_hash_leaves_flat(c_->stream, d_lde_ + (uint64_t)col0 * Nl_, Nl_, cols, Nl_, reinterpret_cast<digest32*>(d_local_), lde_order(), mh));
            SP_TRY(merkle_reduce(c_->stream, t.sub, t.sub_leaves, nullptr, mh));
        }
        SP_TRY(wait_stream());
        stop = cancelled();
    }
    // the composition columns' shape too: two columns, the 2n-point inverse transform
    SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(d_h12s_, (int)logn_ + 1, 1, 2 * n_, d_post_comp_));
    SP_TRY(c_->ntt->lde_coset_major(d_h12s_, d_h12_, (int)logn_, (int)logb_, 2, n_, Nl_, (int)logG_, (int)rank_));
    SP_TRY(wait_stream());
    return SP_OK;
}

int StarkProver::alloc_tree(TreeBuf& t, uint64_t leaves_total, bool sharded) {
    t.sub_leaves = sharded ? leaves_total >> logG_ : leaves_total;
    SP_TRY(alloc((void**)&t.sub, sizeof(digest32) * (2 * t.sub_leaves - 1)));
    t.top = t.sub;
    if (sharded) SP_TRY(alloc((void**)&t.top, sizeof(digest32) * (2ull * G_ - 1)));
    return SP_OK;
}

// Frees a buffer this prover outgrew (everything that could still read it has finished first).
void StarkProver::release(void* p, size_t bytes) {
    if (!p) return;
    (void)hipStreamSynchronize(c_->stream);
    if (side_stream_) (void)hipStreamSynchronize(side_stream_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    auto it = std::find(allocs_.begin(), allocs_.end(), p);
    if (it == allocs_.end()) return;     // carved out of the arena: the space comes back with the next setup()
    allocs_.erase(it);
    (void)hipFree(p);
    alloc_bytes_ -= std::min<uint64_t>(alloc_bytes_, bytes);
    publish_device_bytes();
}

// DEEP inverses beyond the shared scratch (many frame rows on a small blowup): one buffer, grown on demand, kept across proofs
int StarkProver::ensure_deep_scratch(uint64_t elems) {
    bool moved = false;
    const int rc = grow(od_.deepx, elems, &moved);
    if (moved) deep_pref_ = false;      // (the prefetched inverses went with the old block)
    return rc;
}

// [N] scratch for the paths that need the whole domain on every rank (constraint-violating traces, G = b)
int StarkProver::full_domain_buffer(fe** out) {
    if (!fri_sharded(0)) { *out = d_fri_evals_[0]; return SP_OK; }   // free until round 4
    SP_TRY(grow(od_.fullN, N_));
    *out = od_.fullN.p;
    return SP_OK;
}

// Blocking all-gather through the context hook: every rank contributes bytes_per_rank, recv = [world][bytes_per_rank]
// (the first G slots are the G distinct roles).
namespace {
// brackets one stream-ordered exchange with two events on the stream it is enqueued on (sp_comm_time_ms reads them back)
struct CommSpan {
    sp_ctx* c; hipStream_t st; bool on = false;
    CommSpan(sp_ctx* ctx, hipStream_t stream) : c(ctx), st(stream) {
        if (c->comm_ev_used + 2 > 8192) return;
        hipEvent_t e = c->comm_event();
        if (e && hipEventRecord(e, st) == hipSuccess) on = true; else if (e) --c->comm_ev_used;
    }
    ~CommSpan() {
        if (!on) return;
        hipEvent_t e = c->comm_event();
        if (!e || hipEventRecord(e, st) != hipSuccess) c->comm_ev_used -= e ? 2 : 1;      // (an unpaired begin is dropped)
    }
};
struct BlockingSpan {
    sp_ctx* c; double t0 = wall_ms();
    explicit BlockingSpan(sp_ctx* ctx) : c(ctx) {}
    ~BlockingSpan() { c->stat_comm_blocking_ms += wall_ms() - t0; }
};
}  // namespace

// a hook's non-zero return as the prover's error
static int hook_result(int rc, const char* what) {
    if (rc != 0) { sp_set_error(std::string(what) + " failed (" + std::to_string(rc) + ")"); return SP_E_HIP; }
    return SP_OK;
}

int StarkProver::all_gather(const void* send_dev, void* recv_dev, uint64_t bytes_per_rank, bool stream_ordered) {
    const bool async = stream_ordered && comm_async();
    int rc;
    if (async) { CommSpan span(c_, c_->stream); rc = c_->allgather_async(c_->allgather_user, send_dev, recv_dev, bytes_per_rank, c_->stream); }
    else { SP_HIP_CHECK(sp_stream_wait_polling(c_->stream)); BlockingSpan span(c_); rc = c_->allgather(c_->allgather_user, send_dev, recv_dev, bytes_per_rank); }
    SP_TRY(hook_result(rc, async ? "stream-ordered all-gather" : "all-gather hook"));
    count_all_gather(bytes_per_rank);
    return SP_OK;
}

int StarkProver::all_gather_begin(const void* send_dev, void* recv_dev, uint64_t bytes_per_rank, int slot) {
    if (slot < 0 || slot >= COMM_BLOCKS) return SP_E_INVALID_ARG;
    if (!comm_async()) return all_gather(send_dev, recv_dev, bytes_per_rank);
    if (!comm_stream_) {
        SP_HIP_CHECK(hipStreamCreateWithFlags(&comm_stream_, hipStreamNonBlocking));
        SP_HIP_CHECK(hipEventCreateWithFlags(&ev_comm_fork_, hipEventDisableTiming));
        for (auto& e : ev_comm_done_) SP_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    SP_HIP_CHECK(hipEventRecord(ev_comm_fork_, c_->stream));            // the send block is complete behind this point
    SP_HIP_CHECK(hipStreamWaitEvent(comm_stream_, ev_comm_fork_, 0));
    int rc;
    { CommSpan span(c_, comm_stream_); rc = c_->allgather_async(c_->allgather_user, send_dev, recv_dev, bytes_per_rank, comm_stream_); }
    SP_TRY(hook_result(rc, "stream-ordered all-gather"));
    SP_HIP_CHECK(hipEventRecord(ev_comm_done_[slot], comm_stream_));
    count_all_gather(bytes_per_rank);
    return SP_OK;
}
int StarkProver::all_gather_end(int slot) {
    if (!comm_async()) return SP_OK;
    SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, ev_comm_done_[slot], 0));
    return SP_OK;
}

// Block d of `send` goes to the rank with role d; recv[s] = what role s addressed to this rank.  One all-to-all when the
// hook exists (every rank is its own role then); otherwise an all-gather of the whole send array and a local selection.
int StarkProver::exchange_blocks(const void* send_dev, void* recv_dev, uint64_t bytes, bool stream_ordered) {
    const bool async = stream_ordered && comm_async() && c_->alltoall_async && world_ == G_;
    if (async || (c_->alltoall && world_ == G_)) {   // (also with a stream-ordered all-gather but no such all-to-all: one host round trip beats G times the bytes)
        int rc;
        if (async) { CommSpan span(c_, c_->stream); rc = c_->alltoall_async(c_->allgather_user, send_dev, recv_dev, bytes, c_->stream); }
        else { SP_HIP_CHECK(sp_stream_wait_polling(c_->stream)); BlockingSpan span(c_); rc = c_->alltoall(c_->allgather_user, send_dev, recv_dev, bytes); }
        SP_TRY(hook_result(rc, async ? "stream-ordered all-to-all" : "all-to-all hook"));
        count_all_to_all(bytes);
        return SP_OK;
    }
    const uint64_t per_rank = bytes * G_;
    SP_TRY(ensure_gather((per_rank * world_ + sizeof(fe) - 1) / sizeof(fe)));
    SP_TRY(all_gather(send_dev, od_.gather.p, per_rank, stream_ordered));
    const uint8_t* g = reinterpret_cast<const uint8_t*>(od_.gather.p);
    for (uint32_t src = 0; src < G_; ++src)   // the first G slots are the G roles
        SP_HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t*>(recv_dev) + (uint64_t)src * bytes, g + (uint64_t)src * per_rank + (uint64_t)rank_ * bytes, bytes,
                                    hipMemcpyDeviceToDevice, c_->stream));
    return SP_OK;
}

int StarkProver::ensure_aux_workspace(uint64_t pm) {
    if (od_.auxws.p && pm <= auxws_pm_) return SP_OK;
    size_t sort_tmp = 0;
    uint64_t cap = std::max<uint64_t>(pm, 1024);
    size_t bytes = aux_workspace_bytes(n_, cap, &sort_tmp);
    presorted_ = false;                  // (what a presort left is carved for fewer cells)
    SP_TRY(grow(od_.auxws, bytes));      // (a context reused with a growing public memory does not keep every workspace it outgrew)
    auxws_pm_ = cap;
    aux_workspace_carve(auxws_, od_.auxws.p, n_, cap, sort_tmp);
    return SP_OK;
}

}  // namespace sp
