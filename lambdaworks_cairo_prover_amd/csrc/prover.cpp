// Round-by-round STARK prover on the device (see prover.h). Host code only: it sequences kernels on the context
// stream, keeps every polynomial / evaluation / tree resident in HBM and moves only roots, challenges and openings.
#include "prover_internal.h"
#include <unordered_map>
#include <cstring>
#include <cmath>
#include <functional>

namespace sp {

int StarkProver::wait_stream() {
    SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
    return SP_OK;
}

int StarkProver::readback(void* dst_host, const void* src_dev, size_t bytes) {
    SP_TRY(ensure_pin());
    if (bytes > h_pin_.bytes) SP_TRY(h_pin_.ensure(bytes, "pinned read-back slot"));   // (nothing is in flight into the slot between two calls)
    SP_HIP_CHECK(hipMemcpyAsync(h_pin_.p, src_dev, bytes, hipMemcpyDeviceToHost, c_->stream));
    SP_TRY(wait_stream());
    memcpy(dst_host, h_pin_.p, bytes);
    return SP_OK;
}

// DEEP denominators of round 4 on the side stream while round 3 evaluates the polynomials at z (same arrays, same batch
// inversion as deep_fri_begin's inline path; valid-trace form only: one coset of n points).
int StarkProver::prefetch_deep_inverses() {
    deep_pref_ = false;
    if (h_full_) return SP_OK;
    const uint32_t R = (uint32_t)offsets_.size(), npts = R + 1;
    SP_TRY(ensure_side());
    SP_TRY(ensure_deep_scratch((2ull * npts + 1) * n_));
    SP_TRY(ensure_side_flags());
    fe pts[AIR_MAX_OFFSETS + 1];
    for (uint32_t k = 0; k < R; ++k) pts[k] = fe_mul(z_, fe_pow_u64(g_, offsets_[k]));
    pts[R] = fe_sqr(z_);
    const fe* roots_n = nullptr;
    SP_TRY(c_->ntt->roots((int)logn_, &roots_n));
    const fe hp = fe_mul(h_, fe_pow_u64(host_primitive_root((int)logN_), rank_));
    SP_HIP_CHECK(hipEventRecord(ev_side_fork_, c_->stream));          // (the buffer's previous readers are behind this point)
    SP_HIP_CHECK(hipStreamWaitEvent(side_stream_, ev_side_fork_, 0));
    SP_HIP_CHECK(hipMemsetAsync(side_flag(SIDE_DEEP_INV), 0, sizeof(int), side_stream_));
    SP_TRY(coset_minus_points(side_stream_, od_.deepx.p, n_, logn_, roots_n, hp, pts, npts, ShardMap{0, 0, 0}));
    SP_TRY(batch_inverse(side_stream_, od_.deepx.p, od_.deepx.p + (uint64_t)npts * n_, (uint64_t)npts * n_, side_flag(SIDE_DEEP_INV)));
    SP_HIP_CHECK(hipEventRecord(ev_side_deep_, side_stream_));
    deep_pref_ = true;
    return SP_OK;
}

// Boundary denominators of round 2 for a constraint-satisfying trace (the 2n points of this rank's coset pair), computed on
// the side stream while round 1 runs.  composition_core uses them when it takes that path with the same boundary points.
int StarkProver::prefetch_boundary_inverses(const std::vector<uint64_t>& steps_in) {
    bpre_valid_ = false;
    if (!ready_ || logb_ < logG_ + 1) return SP_OK;
    std::vector<uint64_t> steps;
    for (uint64_t s : steps_in) if (std::find(steps.begin(), steps.end(), s) == steps.end()) steps.push_back(s);
    if (steps.empty() || steps.size() > 3) return SP_OK;
    SP_HIP_CHECK(hipSetDevice(c_->device));
    SP_TRY(ensure_side());
    const uint64_t M = 2 * n_;
    SP_TRY(grow(od_.bpre, 6 * M));
    SP_TRY(ensure_side_flags());
    bpre_points_.clear();
    for (uint64_t s : steps) bpre_points_.push_back(fe_pow_u64(g_, s));
    const fe* roots_m = nullptr;
    SP_TRY(c_->ntt->roots((int)logn_ + 1, &roots_m));
    const uint32_t nd = (uint32_t)bpre_points_.size();
    SP_HIP_CHECK(hipEventRecord(ev_side_fork_, c_->stream));
    SP_HIP_CHECK(hipStreamWaitEvent(side_stream_, ev_side_fork_, 0));
    SP_HIP_CHECK(hipMemsetAsync(side_flag(SIDE_BND_INV), 0, sizeof(int), side_stream_));
    SP_TRY(coset_minus_points(side_stream_, od_.bpre.p, M, logn_ + 1, roots_m, rank_coset_offset(), bpre_points_.data(), nd, ShardMap{0, 0, 0}));
    SP_TRY(batch_inverse(side_stream_, od_.bpre.p, od_.bpre.p + 3 * M, (uint64_t)nd * M, side_flag(SIDE_BND_INV)));
    SP_HIP_CHECK(hipEventRecord(ev_side_bnd_, side_stream_));
    bpre_valid_ = true;
    return SP_OK;
}

// batch_commit (reference prover.rs:96-104) / FriLayer::new's tree (fri_commitment.rs:39) over leaves this rank holds in local
// natural order.  Several ranks: the 32-byte leaf digests are exchanged so that rank d owns the contiguous leaves
// [d N/G, (d+1) N/G) - block d of the local digest array is exactly this rank's share of that range - then every rank reduces
// its subtree, the G subtree roots are all-gathered and the top log2 G levels finished everywhere.
int StarkProver::commit_local(const fe* cols_dev, uint64_t stride, uint32_t ncols, uint64_t L, LdeOrder order, TreeBuf& tree, uint8_t root_out[32],
                              bool single_element_tree, const FriChallenge* ch) {
    const MerkleHash mh = merkle_hash(single_element_tree);
    const bool head_done = leaf_head_done_;
    leaf_head_done_ = false;
    if (tree.top == tree.sub) {   // the whole tree on this rank
        if (head_done && mh == MerkleHash::KECCAK256 && merkle_split_supported(ncols))   // the first 17 columns were absorbed while the rest uploaded
            SP_TRY(merkle_hash_leaves_tail(c_->stream, cols_dev, stride, ncols, L, reinterpret_cast<const uint64_t*>(d_scratch_), tree.sub, order));
        else
        SP_TRY(merkle_hash_leaves(c_->stream, cols_dev, stride, ncols, L, tree.sub, order, mh));
        SP_TRY(merkle_reduce(c_->stream, tree.sub, L, ch, mh));
    } else {
        if (L != tree.sub_leaves || L > Nl_) return SP_E_STATE;
        // (both exchanges are consumed on the compute stream, and the read-back of the root below waits for it: stream-ordered
        // where the transport can - two host round trips less per commitment)
        SP_TRY(merkle_hash_leaves_flat(c_->stream, cols_dev, stride, ncols, L, reinterpret_cast<digest32*>(d_local_), order, mh));
        SP_TRY(exchange_blocks(d_local_, d_recv_, (L >> logG_) * sizeof(digest32), true));
        // recv[s][j] = leaf (first + j) G + s of the global order = leaf j G + s of this rank's range
        SP_TRY(interleave_shards(c_->stream, d_recv_, tree.sub + (L - 1), L >> logG_, ShardMap{logG_, logG_, 0}));
        SP_TRY(merkle_reduce(c_->stream, tree.sub, L, nullptr, mh));
        SP_TRY(all_gather(tree.sub, d_roots_, sizeof(digest32), true));
        SP_HIP_CHECK(hipMemcpyAsync(tree.top + (G_ - 1), d_roots_, G_ * sizeof(digest32), hipMemcpyDeviceToDevice, c_->stream));
        SP_TRY(merkle_reduce(c_->stream, tree.top, G_, ch, mh));
    }
    if (ch) return SP_OK;
    return readback(root_out, tree.top, 32);
}

int StarkProver::commit_trace(int segment, const uint8_t* rows_host, uint32_t cols, uint8_t root_out[32], TraceSource src, int col_enc, uint64_t col_stride) {
    const uint32_t binary_hint = binary_cols_hint_;   // (this call only, whatever becomes of it: a later table on this prover need not be a Cairo trace)
    binary_cols_hint_ = 0;
    if (!rows_host || !root_out) return SP_E_INVALID_ARG;
    if (!((segment == 0 && stage_ == Stage::Setup && cols == Cm_) || (segment == 1 && stage_ == Stage::MainCommitted && cols == Ca_))) {
        sp_set_error("commit_trace: wrong segment order or column count");
        return SP_E_STATE;
    }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    for (double& x : c_->upload_stats) x = 0.0;
    leaf_head_done_ = false;
    // An upload that fails half-way must not return while copies from the caller's buffer are still in flight (the caller is free
    // to release it): every non-OK exit of the host paths waits for the copy and the compute stream first.
    auto drained = [this](int rc) {
        if (rc != SP_OK) {
            if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
            (void)hipStreamSynchronize(c_->stream);
            (void)hipGetLastError();
            leaf_head_done_ = false;
        }
        return rc;
    };
    if (src == TRACE_DEVICE_BUILD) {
        if (segment != 0) return SP_E_INVALID_ARG;
        return drained(commit_trace_built(*reinterpret_cast<const TraceBuildInput*>(rows_host), root_out));
    }
    if (src == TRACE_HOST_COLUMNS) {
        if (col_enc >= 0 && col_enc != SP_FE_MONT_LIMBS && col_enc != SP_FE_CANON_BE) return SP_E_INVALID_ARG;
        if (col_stride && col_stride < n_) return SP_E_INVALID_ARG;
        return drained(commit_trace_columns(segment, rows_host, cols, col_enc, col_stride ? col_stride : n_, root_out));
    }
    const bool rows_on_device = src == TRACE_DEVICE_ROWS;
    static const uint64_t pipeline_min_bytes = [] { const char* e = std::getenv("SP_UPLOAD_MIN_MB"); return (uint64_t)(e ? std::max(0, std::atoi(e)) : 64) << 20; }();
    static const bool no_pack = std::getenv("SP_UPLOAD_NO_FLAG_PACK") != nullptr;      // (A/B switch)
    const uint32_t binary_cols = (segment == 0 && !no_pack && (n_ & 63) == 0) ? std::min(binary_hint, cols) : 0u;
    if (!rows_on_device && G_ == 1 && cols >= 8 && (uint64_t)n_ * cols * 32 >= pipeline_min_bytes) {
        int rc = drained(commit_trace_pipelined(segment, rows_host, cols, root_out, 0, 0, false, binary_cols));
        if (rc == SP_RETRY_RAW_UPLOAD) rc = drained(commit_trace_pipelined(segment, rows_host, cols, root_out));   // (not a trace with 0 / 1 flags)
        return rc;
    }
    if (!rows_on_device && G_ > 1 && cols >= 2 * G_ && (uint64_t)n_ * cols * 32 >= pipeline_min_bytes) {
        int rc = drained(commit_trace_rows_sharded(segment, rows_host, cols, root_out, binary_cols));
        if (rc == SP_RETRY_RAW_UPLOAD) rc = drained(commit_trace_rows_sharded(segment, rows_host, cols, root_out, 0));
        return rc;
    }
    const uint32_t col0 = segment == 0 ? 0 : Cm_;
    // staging: the raw rows sit in this segment's (not yet written) LDE area: cols*N*32 >= cols*n*32 bytes
    uint8_t* raw = reinterpret_cast<uint8_t*>(d_lde_ + (uint64_t)col0 * std::max<uint64_t>(Nl_, n_));
    fe* trace = d_trace_ + (uint64_t)col0 * n_;
    if (rows_on_device) {
        SP_TRY(rows_to_columns(c_->stream, c_->enc, rows_host, n_, cols, trace, n_));
    } else {
        SP_HIP_CHECK(hipMemcpyAsync(raw, rows_host, (size_t)n_ * cols * 32, hipMemcpyHostToDevice, c_->stream));
        SP_TRY(rows_to_columns(c_->stream, c_->enc, raw, n_, cols, trace, n_));
    }
    if (segment == 0) SP_TRY(launch_aux_presort());
    return commit_segment_resident(segment, cols, root_out);
}

// interpolate_and_commit (reference prover.rs:126-159) from the reference's row-major host table with SEVERAL ranks.  Every rank
// holds the same table (the shim's `&TraceTable`), so no rank needs to push all of it through its own PCIe link - and on one host
// the G gathers of the whole table would go through the same memory controllers: the rank with role r gathers and uploads the
// ceil(cols / G) columns from min(r cpr, cols - cpr) on only (the upload ring of the one-GPU path, restricted to that window), and
// the natural-order columns are all-gathered over the fabric: cols n 32 bytes in total (1.1 GB at 2^20 x 34: ~3 ms on the link
// model) instead of G times that through the host (20 ms of PCIe per rank, and the host's memory bandwidth shared by all).
// Every rank needs the whole trace anyway - the auxiliary trace and the exact constraint check read it - so the all-gather carries
// trace VALUES and the interpolation follows as configured (SP_OPT_SHARD_INTERPOLATION).
int StarkProver::commit_trace_rows_sharded(int segment, const uint8_t* rows_host, uint32_t cols, uint8_t root_out[32], uint32_t binary_cols) {
    const uint32_t col0 = segment == 0 ? 0 : Cm_;
    const uint32_t cpr = cols_per_role(cols);
    fe* trace = d_trace_ + (uint64_t)col0 * n_;
    {
        // The verdict of the window upload is agreed on before the all-gather of the trace - one word per rank through the same
        // transport - so that a rank whose window breaks the 0 / 1 hint, or whose upload failed, does not leave the others waiting.
        const int rc = commit_trace_pipelined(segment, rows_host, cols, root_out, role_first_col(rank_, cols), cpr, true, binary_cols);
        SP_TRY(grow(od_.flags_all, world_));
        const int mine = rc == SP_OK ? 0 : (rc == SP_RETRY_RAW_UPLOAD ? 1 : 2);
        SP_HIP_CHECK(hipMemcpyAsync(c_->d_flag, &mine, sizeof(int), hipMemcpyHostToDevice, c_->stream));
        SP_TRY(all_gather(c_->d_flag, od_.flags_all.p, sizeof(int)));
        std::vector<int> flags(world_, 0);
        SP_HIP_CHECK(hipMemcpy(flags.data(), od_.flags_all.p, sizeof(int) * world_, hipMemcpyDeviceToHost));
        if (rc != SP_OK && rc != SP_RETRY_RAW_UPLOAD) return rc;
        int worst = 0;
        for (int f : flags) worst = std::max(worst, f);
        if (worst == 2) { sp_set_error("commit_trace: the upload of another rank failed"); return SP_E_HIP; }
        if (worst == 1) return SP_RETRY_RAW_UPLOAD;
    }
    // (the LDE area of this segment is free until the transforms below: landing zone of the all-gather)
    const uint64_t block = (uint64_t)cpr * n_;
    fe* stage = nullptr;
    if ((uint64_t)world_ * block <= std::max<uint64_t>(Nl_, n_) * cols) stage = d_lde_ + (uint64_t)col0 * std::max<uint64_t>(Nl_, n_);
    else { SP_TRY(ensure_gather((uint64_t)world_ * block)); stage = od_.gather.p; }
    SP_TRY(all_gather(trace + (uint64_t)role_first_col(rank_, cols) * n_, stage, block * sizeof(fe), true));
    for (uint32_t role = 0; role < G_; ++role) {      // (the first G slots are the G roles; the own block is in place already)
        if (role == rank_) continue;
        SP_HIP_CHECK(hipMemcpyAsync(trace + (uint64_t)role_first_col(role, cols) * n_, stage + (uint64_t)role * block, block * sizeof(fe), hipMemcpyDeviceToDevice, c_->stream));
    }
    if (segment == 0) SP_TRY(launch_aux_presort());
    SP_TRY(commit_segment_resident(segment, cols, root_out));
    return finish_upload_stats(pending_up_groups_, pending_up_bytes_, pending_up_gather_ms_, pending_up_host_ms_, 1);
}

// interpolate_and_commit (reference prover.rs:126-159) of the Cairo main segment from the RUN instead of the table: the register
// states and the memory cross PCIe (24 B per step + 32 B per cell: 70 MB where the table has 1.1 GB at 2^20 rows) and the device
// writes the table itself - build_main_trace, reference src/cairo/execution_trace.rs:57-87 (trace_kernels.hip).  With several
// ranks every rank builds the whole trace from the same 70 MB: no rank waits for a gigabyte of host table.
int StarkProver::commit_trace_built(const TraceBuildInput& in, uint8_t root_out[32]) {
    if (!in.plan || !in.image) return SP_E_INVALID_ARG;
    const TracePlan& P = *in.plan;
    TraceImage& I = *in.image;
    if (!I.base || !P.dense || P.n != n_ || P.cols != Cm_ || P.steps == 0 || P.steps > n_) { sp_set_error("commit_trace: the run does not fit the prover's shape"); return SP_E_INVALID_ARG; }
    (void)I.try_pin();          // a run built before this process had a context: page-locked from here on
    bool image_pinned = false;
    const uint8_t* image = I.current(&image_pinned);
    constexpr uint32_t REG_CHUNKS = 4;
    SP_TRY(ensure_upload(REG_CHUNKS));
    SP_TRY(ensure_host_flags());
    // staging: the image and the builder's scratch sit in this segment's (not yet written) LDE area when they fit
    const size_t need = (size_t)I.bytes + main_trace_scratch_bytes(P.steps);
    uint8_t* stage = reinterpret_cast<uint8_t*>(d_lde_);
    ScopedDevAlloc tmp(c_->stream);
    if (need > sizeof(fe) * std::max<uint64_t>(Nl_, n_) * Cm_) {
        SP_TRY(tmp.alloc(need, "commit_trace"));
        stage = static_cast<uint8_t*>(tmp.p);
    }
    // The memory (and the two hole lists behind it) first, then the register states in four chunks on the copy stream: the rows of a
    // chunk's steps are written while the next chunk crosses PCIe - what stays exposed is the memory (29 MB: 0.5 ms at 2^20 rows) and
    // one chunk of registers (6 MB) instead of the whole image (54 MB: 0.96 ms).
    const double t0 = wall_ms();
    SP_HIP_CHECK(hipEventRecord(up_start_, c_->stream));             // the staging area's previous users are behind this point
    SP_HIP_CHECK(hipStreamWaitEvent(copy_stream_, up_start_, 0));
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    const MainTraceArgs a = main_trace_args(P, I, stage, d_trace_);   // (P.n == n_ and P.cols == Cm_: checked above)
    SP_HIP_CHECK(hipEventRecord(up_ev_[0].dma0, copy_stream_));
    SP_HIP_CHECK(hipMemcpyAsync(stage + I.off_mem, image + I.off_mem, I.bytes - I.off_mem, hipMemcpyHostToDevice, copy_stream_));
    const uint64_t per = ((P.steps + REG_CHUNKS - 1) / REG_CHUNKS + 255) & ~(uint64_t)255;
    uint32_t chunks_used = 0;
    for (uint32_t k = 0; k < REG_CHUNKS; ++k) {
        const uint64_t s0 = std::min<uint64_t>(P.steps, k * per), s1 = std::min<uint64_t>(P.steps, (k + 1) * per);
        if (s0 == s1) break;
        // (one copy in flight at a time: a copy enqueued while the engine is busy may be given a second SDMA engine, and a stream
        // hopping between two ran at 27 - 37 GB/s instead of 56 - see commit_trace_columns)
        SP_HIP_CHECK(hipStreamSynchronize(copy_stream_));
        if (k) SP_HIP_CHECK(hipEventRecord(up_ev_[k].dma0, copy_stream_));
        SP_HIP_CHECK(hipMemcpyAsync(stage + I.off_regs + 24 * s0, image + I.off_regs + 24 * s0, 24 * (s1 - s0), hipMemcpyHostToDevice, copy_stream_));
        SP_HIP_CHECK(hipEventRecord(up_ev_[k].dma1, copy_stream_));
        SP_HIP_CHECK(hipEventRecord(up_ev_[k].ready, copy_stream_));
        SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, up_ev_[k].ready, 0));
        SP_TRY(cairo_main_trace_steps(c_->stream, a, stage + I.bytes, c_->d_flag, s0, s1));
        SP_HIP_CHECK(hipEventRecord(up_ev_[k].done, c_->stream));
        chunks_used = k + 1;
    }
    SP_TRY(cairo_main_trace_finish(c_->stream, a, stage + I.bytes, c_->d_flag));
    SP_HIP_CHECK(hipMemcpyAsync(&host_flags().trace_build_oob, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    const double host_ms = wall_ms() - t0;
    SP_TRY(launch_aux_presort());
    SP_TRY(commit_segment_resident(0, Cm_, root_out));        // (its read-back of the root waits for everything above)
    if (host_flags().trace_build_oob) { sp_set_error("commit_trace: a trace row reads beyond the run's memory image"); return SP_E_INVALID_ARG; }
    return finish_upload_stats(chunks_used, I.bytes, 0.0, host_ms, image_pinned ? 4 : 5);
}

// Second half of interpolate_and_commit: the segment's columns sit in natural order in d_trace_.
int StarkProver::commit_segment_resident(int segment, uint32_t cols, uint8_t root_out[32]) {
    const uint32_t col0 = segment == 0 ? 0 : Cm_;
    fe* coeffs = d_coeffs_ + (uint64_t)col0 * n_;
    // interpolate_fft (reference trace.rs:104-110): natural -> bit-reversed h-scaled coefficients (the trace stays intact)
    fe* lde = d_lde_ + (uint64_t)col0 * Nl_;
    if (G_ > 1 && shard_interp_ && d_cstage_ && cols >= G_) {
        // columns are independent (prover.rs:174-183): role s interpolates the cpr columns from min(s cpr, cols - cpr) on
        // (the last blocks overlap instead of being ragged), all-gathers bring every coefficient everywhere (§8(e) item 1).
        // With a stream-ordered transport the cpr columns go in up to four blocks: the exchange of block k runs on the
        // communication stream beside the inverse transforms of block k + 1 and the LDE of block k - 1; a blocking transport
        // keeps the one exchange (every call is a host round trip through the hook).
        const uint32_t cpr = cols_per_role(cols);
        const uint32_t K = comm_async() ? std::min<uint32_t>(cpr, (uint32_t)COMM_BLOCKS) : 1u;
        const uint32_t bc = (cpr + K - 1) / K;
        std::vector<uint8_t> extended(cols, 0);
        struct Block { uint32_t j0, w; fe* stage; };
        std::vector<Block> blocks;
        uint64_t stage_off = 0;
        for (uint32_t j0 = 0; j0 < cpr; j0 += bc) {
            const uint32_t w = std::min(bc, cpr - j0);
            blocks.push_back(Block{j0, w, d_cstage_ + stage_off});
            stage_off += (uint64_t)world_ * w * n_;
        }
        auto finish = [&](size_t k) -> int {   // block k has arrived: into the coefficient array, then evaluate_offset_fft of its columns
            const Block& b = blocks[k];
            SP_TRY(all_gather_end((int)k));
            for (uint32_t role = 0; role < G_; ++role)
                SP_HIP_CHECK(hipMemcpyAsync(coeffs + (uint64_t)(role_first_col(role, cols) + b.j0) * n_, b.stage + (uint64_t)role * b.w * n_, (uint64_t)b.w * n_ * sizeof(fe),
                                            hipMemcpyDeviceToDevice, c_->stream));
            if (K == 1) return SP_OK;          // one exchange: the whole segment is extended in one launch below
            for (uint32_t role = 0; role < G_; ++role)
                for (uint32_t j = 0; j < b.w;) {   // runs of columns not extended yet (the ranges of the last roles overlap)
                    const uint32_t c = role_first_col(role, cols) + b.j0 + j;
                    if (extended[c]) { ++j; continue; }
                    uint32_t run = 0;
                    while (j + run < b.w && !extended[c + run]) { extended[c + run] = 1; ++run; }
                    SP_TRY(c_->ntt->lde_coset_major(coeffs + (uint64_t)c * n_, lde + (uint64_t)c * Nl_, (int)logn_, (int)logb_, run, n_, Nl_, (int)logG_, (int)rank_));
                    j += run;
                }
            return SP_OK;
        };
        for (size_t k = 0; k < blocks.size(); ++k) {
            const Block& b = blocks[k];
            fe* mine = b.stage + (uint64_t)wrank_ * b.w * n_;      // in place: slot `rank` of the receive block is the send buffer
            SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(mine, (int)logn_, b.w, n_, d_t1_, d_trace_ + (uint64_t)(col0 + role_first_col(rank_, cols) + b.j0) * n_));
            SP_TRY(all_gather_begin(mine, b.stage, (uint64_t)b.w * n_ * sizeof(fe), (int)k));
            if (k > 0) SP_TRY(finish(k - 1));
        }
        SP_TRY(finish(blocks.size() - 1));
        if (K == 1) SP_TRY(c_->ntt->lde_coset_major(coeffs, lde, (int)logn_, (int)logb_, cols, n_, Nl_, (int)logG_, (int)rank_));
    } else {
        SP_TRY(interpolate_extend(d_trace_ + (uint64_t)col0 * n_, coeffs, lde, cols));
    }
    // batch_commit (reference prover.rs:96-104) straight from the column-major LDE
    SP_TRY(commit_columns(lde, Nl_, cols, segment == 0 ? tree_main_ : tree_aux_, root_out));
    segment_committed(segment);
    return SP_OK;
}

// get_pub_memory_addrs (reference cairo/air.rs:500-517) and the matching values -> pm_addr_h_, pm_val_h_
int StarkProver::public_memory_lists(const PublicInputs& pub) {
    const uint64_t pm = pub.public_memory.size();
    pm_addr_h_.clear(); pm_val_h_.clear();
    std::vector<uint64_t> addrs;
    if (const MemorySegment* out = pub.segment(1)) {
        if (out->end < out->start || out->end - out->start > pm) { sp_set_error("commit_aux_cairo: output segment larger than the public memory"); return SP_E_INVALID_ARG; }
        uint64_t output_section = out->end - out->start, program_section = pm - output_section;
        for (uint64_t i = 1; i <= program_section; ++i) addrs.push_back(i);
        for (uint64_t a = out->start; a < out->end; ++a) addrs.push_back(a);
    } else {
        for (uint64_t i = 1; i <= pm; ++i) addrs.push_back(i);
    }
    std::unordered_map<uint64_t, const fe*> by_addr;   // the reference keeps the public memory in a HashMap (cairo/air.rs:163-181)
    by_addr.reserve(pub.public_memory.size() * 2);
    for (auto& kv : pub.public_memory) by_addr.emplace(kv.first, &kv.second);   // first entry of an address wins, as the linear scan did
    for (uint64_t a : addrs) {
        auto it = by_addr.find(a);
        if (it == by_addr.end()) { sp_set_error("commit_aux_cairo: public memory address missing"); return SP_E_INVALID_ARG; }
        pm_addr_h_.push_back(fe_from_u64(a)); pm_val_h_.push_back(*it->second);
    }
    return SP_OK;
}

// The sorts of the auxiliary trace need the main trace and the public memory but no challenge: side stream, from the moment
// the natural-order main columns are queued on the compute stream (request_aux_presort + commit_trace(0, ..)).
int StarkProver::launch_aux_presort() {
    const PublicInputs* pub = presort_pub_;
    presort_pub_ = nullptr; presorted_ = false;
    if (!pub || Ca_ != 18 || Cm_ < 34) return SP_OK;
    SP_TRY(public_memory_lists(*pub));
    const uint64_t pm = pm_addr_h_.size();
    SP_TRY(ensure_aux_workspace(pm));
    SP_TRY(ensure_side());
    SP_TRY(ensure_side_flags());
    SP_HIP_CHECK(hipEventRecord(ev_side_fork_, c_->stream));          // the main trace columns are behind this point
    SP_HIP_CHECK(hipStreamWaitEvent(side_stream_, ev_side_fork_, 0));
    SP_HIP_CHECK(hipMemsetAsync(side_flag(SIDE_PRESORT_MALFORMED), 0, 2 * sizeof(int), side_stream_));   // (and SIDE_PRESORT_WIDE_KEY behind it)
    SP_TRY(cairo_aux_presort(side_stream_, auxws_, d_memcols_, n_, pm_addr_h_.data(), pm_val_h_.data(), pm, side_flag(SIDE_PRESORT_MALFORMED), side_flag(SIDE_PRESORT_WIDE_KEY)));
    // the "address beyond the key bits" flag travels to the host behind the sorts: commit_aux_cairo reads it without a round trip of its own
    SP_TRY(ensure_host_flags());
    static_assert(offsetof(HostFlags, presort_wide_key) == offsetof(HostFlags, presort_malformed) + sizeof(int), "one copy moves both presort flags");
    SP_HIP_CHECK(hipMemcpyAsync(&host_flags().presort_malformed, side_flag(SIDE_PRESORT_MALFORMED), 2 * sizeof(int), hipMemcpyDeviceToHost, side_stream_));
    SP_HIP_CHECK(hipEventRecord(ev_side_presort_, side_stream_));
    presorted_ = true;
    return SP_OK;
}

int StarkProver::commit_aux_cairo(const PublicInputs& pub, const fe rap[3], uint8_t root_out[32]) {
    if (stage_ != Stage::MainCommitted || Ca_ != 18 || Cm_ < 34) { sp_set_error("commit_aux_cairo: main segment not committed or not a Cairo layout"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    bool pre = presorted_;
    const bool presort_ran = presorted_;
    presorted_ = false;
    if (pre) {   // an address beyond the key bits the presort looked at (a trace with a discontinuous memory): sort again, all 64 bits
        SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, ev_side_presort_, 0));
        SP_HIP_CHECK(hipEventSynchronize(ev_side_presort_));   // (the sorts ended beside round 1's transforms: no wait in practice)
        if (host_flags().presort_wide_key || host_flags().presort_malformed == 2) pre = false;
    }
    else SP_TRY(public_memory_lists(pub));     // (the presort built them from the same public inputs)
    const uint64_t pm = pm_addr_h_.size();
    if (pm != pub.public_memory.size()) { sp_set_error("commit_aux_cairo: public memory changed since the presort"); return SP_E_STATE; }
    SP_TRY(ensure_aux_workspace(pm));
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    if (pre) SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, ev_side_presort_, 0));
    SP_TRY(ensure_side());
    fe* aux_out = d_trace_ + (uint64_t)Cm_ * n_;
    int flag = 0, flag_pre = 0;
    // An address beyond 2^64 (no VM writes one, but the reference proves whatever table it is given): the presort has already said so,
    // or the 64-bit sort below does - then once more with the four-limb sort.
    bool all_limbs = presort_ran && host_flags().presort_malformed == 2;
    for (int attempt = 0; attempt < 2; ++attempt) {
        SP_TRY(cairo_aux_trace_device(c_->stream, auxws_, d_memcols_, n_, pm_addr_h_.data(), pm_val_h_.data(), pm, rap, aux_out, c_->d_flag,
                                      side_stream_, ev_side_fork_, ev_side_aux_, pre, all_limbs));
        SP_HIP_CHECK(hipMemcpyAsync(&flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
        if (pre) SP_HIP_CHECK(hipMemcpyAsync(&flag_pre, side_flag(SIDE_PRESORT_MALFORMED), sizeof(int), hipMemcpyDeviceToHost, c_->stream));
        SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));  // flags
        if (!flag) flag = flag_pre;
        if (flag != 2 || all_limbs) break;
        all_limbs = true; pre = false; flag = flag_pre = 0;
        SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    }
    if (flag) { sp_set_error("commit_aux_cairo: a permutation denominator of the auxiliary trace is zero (the reference's batch inversion fails on this trace and these challenges too)"); return flag == 1 ? SP_E_ZERO_INVERSE : SP_E_INVALID_ARG; }
    return commit_segment_resident(1, Ca_, root_out);
}

// sum_q A[q] y^rev(q) for `vectors` arrays of 2^k elements and `points` points, by repeated folding
// (DESIGN.md "Out-of-domain evaluation"): one level maps M elements to M >> l.
// scratch: at least 3 * 2^k elements (two ping-pong buffers and the per-level power tables).
// after_first (nullable): host work to do once the first - long - level is queued (it runs beside that kernel).
static int eval_bitrev(sp_ctx* c, const fe* arrays, uint64_t vec_stride, uint32_t vectors, uint32_t k, const std::vector<fe>& ys,
                       fe* scratch, uint64_t scratch_elems, std::vector<fe>& out /*[vectors][points]*/,
                       const std::function<int()>* after_first = nullptr) {
    const uint32_t points = (uint32_t)ys.size();
    std::vector<fe> ycur = ys;
    const fe* in = arrays;
    uint64_t in_stride = vec_stride;
    uint32_t in_points = 1;
    uint64_t M = 1ULL << k;
    // level sizes: 2^8 terms per output while that leaves >= 2^16 outputs in flight, then 2^4 (a level with few outputs and
    // long serial sums runs one wave per SIMD for hundreds of microseconds)
    std::vector<uint32_t> ls;
    {
        uint32_t kk = k;
        const double lt0 = std::log2((double)vectors * points);
        while (kk > 0) {
            const int room = (int)(lt0 + kk) - 16;
            uint32_t l = room >= 8 ? 8u : (uint32_t)std::max(4, room);
            l = std::min(l, kk);
            // the two ping-pong buffers hold the first level's outputs: longer sums if the scratch area demands it
            while (ls.empty() && l < std::min<uint32_t>(8, kk) && 2ull * vectors * points * (M >> l) + 8ull * points * 256 > scratch_elems) ++l;
            ls.push_back(l);
            kk -= l;
        }
    }
    const uint64_t level1 = k == 0 ? 0 : (uint64_t)vectors * points * (M >> ls[0]);
    const uint64_t tab_elems = (uint64_t)ls.size() * points * 256;
    if (2 * level1 + tab_elems > scratch_elems) { sp_set_error("eval_bitrev: scratch too small"); return SP_E_ALLOC; }
    fe* bufs[2] = {scratch, scratch + level1};
    fe* yp_dev = scratch + 2 * level1;
    int which = 0;
    if (k == 0) {
        if (after_first) SP_TRY((*after_first)());
        out.resize((size_t)vectors * points);
        for (uint32_t v = 0; v < vectors; ++v) {
            fe t;
            SP_HIP_CHECK(hipMemcpy(&t, arrays + v * vec_stride, sizeof(fe), hipMemcpyDeviceToHost));
            for (uint32_t p = 0; p < points; ++p) out[v * points + p] = t;
        }
        return SP_OK;
    }
    // power tables yp[level][p][t] = y_level^rev_l(t), y_(level+1) = y_level^(2^l): the table of a level goes up right before its
    // kernel, so the host computes the next level's table (~25 us) while the device runs this one; no synchronisation between levels
    std::vector<fe> yp(tab_elems, fe_zero());
    std::vector<fe> pw(256);
    for (size_t lev = 0; lev < ls.size(); ++lev) {
        const uint32_t l = ls[lev], Tn = 1u << l;
        for (uint32_t p = 0; p < points; ++p) {
            pw[0] = fe_one();
            for (uint32_t e = 1; e < Tn; ++e) pw[e] = fe_mul(pw[e - 1], ycur[p]);
            fe* dstp = &yp[lev * points * 256 + (size_t)p * Tn];   // compacted: the kernel indexes yp[p * T + t]
            for (uint32_t t = 0; t < Tn; ++t) {  // yp[t] = y^rev_l(t)
                uint32_t r = 0;
                for (uint32_t bit = 0; bit < l; ++bit) if ((t >> bit) & 1) r |= 1u << (l - 1 - bit);
                dstp[t] = pw[r];
            }
            fe y2 = ycur[p];
            for (uint32_t s = 0; s < l; ++s) y2 = fe_sqr(y2);
            ycur[p] = y2;
        }
        SP_HIP_CHECK(hipMemcpyAsync(yp_dev + lev * points * 256, &yp[lev * points * 256], sizeof(fe) * points * Tn, hipMemcpyHostToDevice, c->stream));
        fe* outb = bufs[which];
        SP_TRY(fold_eval_level(c->stream, in, in_stride, in_points, M, l, yp_dev + lev * points * 256, points, vectors, outb));
        if (lev == 0 && after_first) SP_TRY((*after_first)());
        M >>= l;
        in = outb; in_stride = (uint64_t)points * M; in_points = points;
        which ^= 1;
    }
    SP_HIP_CHECK(sp_stream_wait_polling(c->stream));  // yp is a local vector
    out.resize((size_t)vectors * points);
    SP_HIP_CHECK(hipMemcpyAsync(out.data(), in, out.size() * sizeof(fe), hipMemcpyDeviceToHost, c->stream));
    SP_HIP_CHECK(sp_stream_wait_polling(c->stream));
    return SP_OK;
}

int StarkProver::ood(const fe& z, fe* h1_z2, fe* h2_z2, std::vector<fe>& trace_ood) {
    if (stage_ != Stage::Composed) { sp_set_error("ood: composition polynomial not committed"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    z_ = z;
    // round 4's denominators depend on z only: side stream, beside the evaluations below (queued once the first of them runs)
    const std::function<int()> prefetch = [this]() { return prefetch_deep_inverses(); };
    // stored coefficients are c_k h^k, so evaluate at y / h (reference prover.rs:301-304, frame.rs:67-83)
    const uint32_t R = (uint32_t)offsets_.size();   // frame rows: z g^ofs for every transition offset (frame.rs:67-83)
    std::vector<fe> ys;
    for (uint32_t k = 0; k < R; ++k) ys.push_back(fe_mul(fe_mul(z, fe_pow_u64(g_, offsets_[k])), hinv_));
    std::vector<fe> tr;
    if (G_ > 1 && C_ >= G_) {
        // the polynomials are independent: role s evaluates the cpr columns from min(s cpr, C - cpr) on, the R values per column
        // are all-gathered (a few KB) - 1/G of the Horner-equivalent work per rank instead of all of it on every rank
        const uint32_t cpr = cols_per_role(C_);
        std::vector<fe> mine;
        SP_TRY(eval_bitrev(c_, d_coeffs_ + (uint64_t)role_first_col(rank_, C_) * n_, n_, cpr, logn_, ys, d_scratch_, scratch_elems(), mine, &prefetch));
        const size_t blk = (size_t)cpr * R;
        const size_t blk_cap = (size_t)C_ * AIR_MAX_OFFSETS;   // >= cpr * R: one block per rank
        SP_TRY(grow(od_.small, (1 + (uint64_t)world_) * blk_cap));
        SP_HIP_CHECK(hipMemcpyAsync(od_.small.p, mine.data(), blk * sizeof(fe), hipMemcpyHostToDevice, c_->stream));
        SP_TRY(all_gather(od_.small.p, od_.small.p + blk_cap, blk * sizeof(fe)));
        std::vector<fe> all(blk * world_);
        SP_HIP_CHECK(hipMemcpy(all.data(), od_.small.p + blk_cap, all.size() * sizeof(fe), hipMemcpyDeviceToHost));
        tr.resize((size_t)C_ * R);
        for (uint32_t role = 0; role < G_; ++role)
            std::copy(all.begin() + (size_t)role * blk, all.begin() + (size_t)(role + 1) * blk, tr.begin() + (size_t)role_first_col(role, C_) * R);
    } else {
        SP_TRY(eval_bitrev(c_, d_coeffs_, n_, C_, logn_, ys, d_scratch_, scratch_elems(), tr, &prefetch));
    }
    trace_ood.resize((size_t)R * C_);
    for (uint32_t j = 0; j < C_; ++j)
        for (uint32_t k = 0; k < R; ++k) trace_ood[(size_t)k * C_ + j] = tr[(size_t)j * R + k];
    std::vector<fe> yh = {fe_mul(fe_sqr(z), hinv_)};
    std::vector<fe> hv;
    if (!h_full_) SP_TRY(eval_bitrev(c_, d_h12s_, n_, 2, logn_, yh, d_scratch_, scratch_elems(), hv));
    else SP_TRY(eval_bitrev(c_, od_.hfull.p, N_ >> 1, 2, logN_ - 1, yh, d_scratch_, scratch_elems(), hv));
    h1_z2_ = hv[0]; h2_z2_ = hv[1];
    *h1_z2 = hv[0]; *h2_z2 = hv[1];
    trace_ood_ = trace_ood;
    stage_ = Stage::OodDone;
    return SP_OK;
}

int StarkProver::deep_fri_begin(const fe& gamma, const fe& gamma_p, const std::vector<fe>& tg, uint8_t root0_out[32]) {
    if (stage_ != Stage::OodDone) { sp_set_error("deep_fri_begin: out-of-domain evaluations missing"); return SP_E_STATE; }
    const uint32_t R = (uint32_t)offsets_.size();
    if (tg.size() != (size_t)R * C_) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const fe* roots = nullptr;
    SP_TRY(c_->ntt->roots((int)logN_, &roots));
    if (R > AIR_MAX_OFFSETS) return SP_E_INVALID_ARG;
    DeepConsts K;
    std::memset(&K, 0, sizeof(K));
    K.gamma_h1 = gamma; K.gamma_h2 = gamma_p;
    K.c_h = fe_add(fe_mul(gamma, h1_z2_), fe_mul(gamma_p, h2_z2_));
    K.cols = C_; K.rows = R;
    for (uint32_t k = 0; k < AIR_MAX_OFFSETS; ++k) K.c_t[k] = fe_zero();
    std::vector<uint8_t> up(deep_gammas_at() + sizeof(fe) * R * C_);
    fe* gam = reinterpret_cast<fe*>(up.data() + deep_gammas_at());
    for (uint32_t j = 0; j < C_; ++j)
        for (uint32_t k = 0; k < R; ++k) {
            gam[(size_t)k * C_ + j] = tg[(size_t)j * R + k];  // reference prover.rs:457-476: gamma index = j * frame_len + k
            K.c_t[k] = fe_add(K.c_t[k], fe_mul(tg[(size_t)j * R + k], trace_ood_[(size_t)k * C_ + j]));
        }
    std::memcpy(up.data(), &K, sizeof(K));
    SP_HIP_CHECK(hipMemcpyAsync(d_deep_consts_, up.data(), up.size(), hipMemcpyHostToDevice, c_->stream));
    SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
    fe pts[AIR_MAX_OFFSETS + 1];                       // z g^ofs_k for every frame row, then z^2
    for (uint32_t k = 0; k < R; ++k) pts[k] = fe_mul(z_, fe_pow_u64(g_, offsets_[k]));
    pts[R] = fe_sqr(z_);
    const uint32_t npts = R + 1;
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    bool used_pref = false;
    if (!h_full_) {
        // deg p0 <= n - 2 (every term is a quotient of a polynomial of degree < n by a linear factor), so p0 is fixed by
        // its values on ONE coset of n points: evaluate the quotient form there only (coset c0 = first coset this rank
        // holds), interpolate, and extend with the same LDE as every other column - 1/b of the pointwise work and of
        // the inversions, the same field elements.  Under coset sharding every rank gets the identical polynomial from
        // its own coset, so FRI layer 0 needs no all-gather.
        const uint32_t shift = logb_ - logG_;                 // local elements per row of the LDE matrix
        const fe* roots_n = nullptr;
        SP_TRY(c_->ntt->roots((int)logn_, &roots_n));
        const fe wN = host_primitive_root((int)logN_);
        const fe hp = fe_mul(h_, fe_pow_u64(wN, rank_));      // offset of that coset: h w_N^c0
        fe* inv = d_scratch_;                                  // [npts][n]
        fe* inv_scratch = d_scratch_ + (uint64_t)npts * n_;    // [npts n]
        fe* p0n = d_scratch_ + 2ull * npts * n_;               // [n]
        if ((2ull * npts + 1) * n_ > scratch_elems()) {   // many frame rows on a small blowup: the inverses outgrow the shared scratch
            SP_TRY(ensure_deep_scratch((2ull * npts + 1) * n_));
            inv = od_.deepx.p; inv_scratch = inv + (uint64_t)npts * n_; p0n = inv + 2ull * npts * n_;
        }
        if (deep_pref_ && od_.deepx.cap >= (2ull * npts + 1) * n_) {   // computed beside round 3 (prefetch_deep_inverses)
            inv = od_.deepx.p; p0n = inv + 2ull * npts * n_;
            SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, ev_side_deep_, 0));
            used_pref = true;
        } else {
            SP_TRY(coset_minus_points(c_->stream, inv, n_, logn_, roots_n, hp, pts, npts, ShardMap{0, 0, 0}));
            SP_TRY(batch_inverse(c_->stream, inv, inv_scratch, (uint64_t)npts * n_, c_->d_flag));
        }
        if (fri_sharded(0) && logb_ == logG_) {
            // one coset per rank and a sharded layer 0: the n points of that coset in natural order ARE this rank's share of the layer
            // (local index = row of the coset), so the quotient form is written there and nothing is interpolated or extended
            SP_TRY(deep_composition(c_->stream, d_lde_, d_h12_, d_h12_ + Nl_, n_, Nl_, shift, d_deep_consts_, d_deep_gammas_, inv, d_fri_evals_[0], lde_order(), R));
        } else {
        SP_TRY(deep_composition(c_->stream, d_lde_, d_h12_, d_h12_ + Nl_, n_, Nl_, shift, d_deep_consts_, d_deep_gammas_, inv, p0n, lde_order(), R));
        // coefficients c_j h^j in bit-reversed order: inverse DFT over the coset, times n^-1 w_N^(-c0 j)
        SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(p0n, (int)logn_, 1, n_, d_post_deep_));   // n^-1 w_N^(-c0 j): setup()
        // FRI layer 0: the evaluations this rank holds (local natural order) when the layer is sharded, the whole domain otherwise
        if (fri_sharded(0)) SP_TRY(c_->ntt->lde_from_bitrev(p0n, d_fri_evals_[0], (int)logn_, (int)logb_, 1, n_, Nl_, (int)logG_, (int)rank_));
        else SP_TRY(c_->ntt->lde_from_bitrev(p0n, d_fri_evals_[0], (int)logn_, (int)logb_, 1, n_, N_));
        }
    } else {
        // deg H >= 2n (constraint-violating trace): the quotient form on every LDE point this rank holds
        fe* inv = d_scratch_;
        if (2ull * npts * Nl_ > scratch_elems()) {   // more than two frame rows: the inverses outgrow the shared scratch
            SP_TRY(ensure_deep_scratch(2ull * npts * Nl_));
            inv = od_.deepx.p;
        }
        fe* inv_scratch = inv + (uint64_t)npts * Nl_;
        SP_TRY(coset_minus_points(c_->stream, inv, Nl_, logN_, roots, h_, pts, npts, shard_map()));
        SP_TRY(batch_inverse(c_->stream, inv, inv_scratch, (uint64_t)npts * Nl_, c_->d_flag));
        fe* p0_local = (G_ == 1 || fri_sharded(0)) ? d_fri_evals_[0] : d_local_;   // local natural order
        SP_TRY(deep_composition(c_->stream, d_lde_, d_h12_, d_h12_ + Nl_, Nl_, Nl_, 0, d_deep_consts_, d_deep_gammas_, inv, p0_local, lde_order(), R));
        if (G_ > 1 && !fri_sharded(0)) {
            SP_TRY(ensure_gather((uint64_t)world_ * Nl_));
            SP_TRY(all_gather(p0_local, od_.gather.p, Nl_ * sizeof(fe), true));
            SP_TRY(interleave_shards(c_->stream, od_.gather.p, d_fri_evals_[0], n_, shard_map()));
        }
    }
    // FRI layer 0 (reference fri/mod.rs:27-33)
    fri_layer_ = 0;
    fri_offset_ = h_; fri_offset_inv_ = hinv_;
    int flag = 0, flag_pref = 0;
    SP_HIP_CHECK(hipMemcpyAsync(&flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    if (used_pref) SP_HIP_CHECK(hipMemcpyAsync(&flag_pref, side_flag(SIDE_DEEP_INV), sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    deep_pref_ = false;
    SP_TRY(commit_local(d_fri_evals_[0], 0, 1, fri_trees_[0].sub_leaves, LdeOrder{0, 0, 0}, fri_trees_[0], root0_out, true));   // synchronises
    flag |= flag_pref;
    if (flag) { sp_set_error("deep composition: z lies on the LDE coset"); return SP_E_ZERO_INVERSE; }
    fri_layer_ = 1;
    stage_ = Stage::FriRunning;
    return SP_OK;
}

int StarkProver::fri_fold_commit(const fe& zeta, uint8_t root_out[32], fe* last_value, int* is_last) {
    if (stage_ != Stage::FriRunning) { sp_set_error("fri_fold_commit: FRI not started or already finished"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const fe* roots = nullptr;
    SP_TRY(c_->ntt->roots((int)logN_, &roots));
    const uint32_t k = fri_layer_ - 1;  // layer being folded
    const uint64_t M = N_ >> k;
    const fe half = half_;                                           // (field inversions cost ~15 us on the host: none per layer)
    fe cst = fe_mul(fe_mul(zeta, half), fri_offset_inv_);
    // In evaluation form the fold is local to a rank: the partner i + M/2 of index i has the same residue mod G (§8(e) item 4)
    if (fri_sharded(k)) {
        const uint64_t Ml = M >> logG_;
        fe* next_local = fri_sharded(k + 1) ? d_fri_evals_[k + 1] : d_local_;
        SP_TRY(fri_fold(c_->stream, d_fri_evals_[k], next_local, Ml, logN_, k, roots, half, cst, logG_, rank_));
        if (!fri_sharded(k + 1)) {   // from here on the layers are small: gather this one once and continue on every rank
            SP_TRY(ensure_gather((uint64_t)world_ * (Ml >> 1)));
            SP_TRY(all_gather(next_local, od_.gather.p, (Ml >> 1) * sizeof(fe), true));
            SP_TRY(interleave_shards(c_->stream, od_.gather.p, d_fri_evals_[k + 1], (Ml >> 1), ShardMap{logG_, logG_, 0}));
        }
    } else {
        SP_TRY(fri_fold(c_->stream, d_fri_evals_[k], d_fri_evals_[k + 1], M, logN_, k, roots, half, cst));
    }
    fri_offset_ = fe_sqr(fri_offset_); fri_offset_inv_ = fe_sqr(fri_offset_inv_);
    if (k + 1 < logn_) {
        SP_TRY(commit_local(d_fri_evals_[k + 1], 0, 1, fri_trees_[k + 1].sub_leaves, LdeOrder{0, 0, 0}, fri_trees_[k + 1], root_out, true));
        fri_layer_ += 1;
        *is_last = 0;
    } else {
        // fri_last_value is coefficient 0 of the last folded polynomial (fri/mod.rs:58-67). Its degree is below the b
        // remaining evaluation points, so c_0 = (1/b) * sum of the evaluations on the coset (for a valid trace the
        // polynomial is constant and every evaluation already equals it).
        const uint32_t bb = 1u << logb_;
        std::vector<fe> ev(bb);
        SP_TRY(readback(ev.data(), d_fri_evals_[k + 1], sizeof(fe) * bb));
        fe sum = fe_zero();
        for (auto& e : ev) sum = fe_add(sum, e);
        *last_value = fe_mul(sum, binv_);
        *is_last = 1;
        stage_ = Stage::FriDone;
    }
    return SP_OK;
}

int StarkProver::fri_commit_chain(const fe& zeta0, const uint8_t state32[32], std::vector<std::array<uint8_t, 32>>& roots_out, fe* last_value) {
    if (!fri_chain_available()) { sp_set_error("fri_commit_chain: no layer committed yet, or the next layer to fold is sharded"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const fe* roots = nullptr;
    SP_TRY(c_->ntt->roots((int)logN_, &roots));
    const uint32_t L = logn_;
    SP_TRY(grow(od_.fri_chain, 32 + (size_t)L * 96));
    uint64_t* d_state = reinterpret_cast<uint64_t*>(od_.fri_chain.p);
    fe* d_cmul = reinterpret_cast<fe*>(od_.fri_chain.p + 32);
    fe* d_cst = d_cmul + L;
    uint64_t* d_roots = reinterpret_cast<uint64_t*>(d_cst + L);
    // constants half / offset_k of every layer (offset_k = h^(2^k)) and the transcript state, in one upload
    std::vector<uint8_t>& up = h_up_fri_;     // (a member: the asynchronous copy below may still read it when an error path returns)
    up.assign(32 + (size_t)L * 32, 0);
    std::memcpy(up.data(), state32, 32);
    const uint32_t k0 = fri_layer_ - 1;           // the layer to fold first (0 on one GPU; the first replicated layer otherwise)
    fe oi = fri_offset_inv_;
    for (uint32_t k = k0; k < L; ++k) { const fe c = fe_mul(half_, oi); std::memcpy(up.data() + 32 + (size_t)k * 32, &c, 32); oi = fe_sqr(oi); }
    SP_HIP_CHECK(hipMemcpyAsync(od_.fri_chain.p, up.data(), up.size(), hipMemcpyHostToDevice, c_->stream));
    const fe cst0 = fe_mul(fe_mul(zeta0, half_), fri_offset_inv_);
    for (uint32_t k = k0; k < L; ++k) {           // fold layer k into layer k + 1 and commit it
        const uint64_t M = N_ >> k;
        const fe* c_dev = k == k0 ? nullptr : d_cst + k;   // zeta_k half / offset_k: left in device memory by the launch that produced root k
        const bool sharded_k = fri_sharded(k), sharded_k1 = k + 1 < L && fri_sharded(k + 1);
        static const bool fused = std::getenv("SP_FRI_NO_FUSED_LEAVES") == nullptr;      // (A/B switch)
        const bool fuse = fused && !sharded_k && k + 1 < L && merkle_hash(true) == MerkleHash::KECCAK256;
        if (sharded_k) {
            // several ranks, stream-ordered transport: the fold is local to a rank (the partner i + M/2 has the same residue mod G)
            const uint64_t Ml = M >> logG_;
            fe* next_local = sharded_k1 ? d_fri_evals_[k + 1] : d_local_;
            SP_TRY(fri_fold(c_->stream, d_fri_evals_[k], next_local, Ml, logN_, k, roots, half_, cst0, logG_, rank_, c_dev));
            if (!sharded_k1) {   // from here on the layers are small: gathered once, continued on every rank
                SP_TRY(ensure_gather((uint64_t)world_ * (Ml >> 1)));
                SP_TRY(all_gather(next_local, od_.gather.p, (Ml >> 1) * sizeof(fe), true));
                SP_TRY(interleave_shards(c_->stream, od_.gather.p, d_fri_evals_[k + 1], (Ml >> 1), ShardMap{logG_, logG_, 0}));
            }
        } else if (fuse) {
            SP_TRY(fri_fold_hash(c_->stream, d_fri_evals_[k], d_fri_evals_[k + 1], M, logN_, k, roots, half_, cst0, c_dev,
                                 fri_trees_[k + 1].sub + (fri_trees_[k + 1].sub_leaves - 1)));
        } else {
            SP_TRY(fri_fold(c_->stream, d_fri_evals_[k], d_fri_evals_[k + 1], M, logN_, k, roots, half_, cst0, 0, 0, c_dev));
        }
        if (k + 1 < L) {
            TreeBuf& t = fri_trees_[k + 1];
            const FriChallenge ch{d_state, d_cmul + (k + 1), d_cst + (k + 1), d_roots + 4 * (size_t)(k + 1)};
            if (sharded_k1) {
                SP_TRY(commit_local(d_fri_evals_[k + 1], 0, 1, t.sub_leaves, LdeOrder{0, 0, 0}, t, nullptr, true, &ch));
            } else {
                if (!fuse) SP_TRY(merkle_hash_leaves(c_->stream, d_fri_evals_[k + 1], 0, 1, t.sub_leaves, t.sub, LdeOrder{0, 0, 0}, merkle_hash(true)));
                SP_TRY(merkle_reduce(c_->stream, t.sub, t.sub_leaves, &ch, merkle_hash(true)));
            }
        }
    }
    for (uint32_t k = k0; k < L; ++k) { fri_offset_ = fe_sqr(fri_offset_); fri_offset_inv_ = fe_sqr(fri_offset_inv_); }
    // roots of layers k0 + 1 .. L-1 and the b evaluations of the last fold (fri/mod.rs:58-67, see fri_fold_commit)
    roots_out.assign(L - 1 - k0, std::array<uint8_t, 32>{});
    if (L - 1 > k0) {
        if ((size_t)(L - 1 - k0) * 32 > 4096) return SP_E_UNSUPPORTED;
        SP_TRY(readback(roots_out.data(), d_roots + 4 * (size_t)(k0 + 1), (size_t)(L - 1 - k0) * 32));
    }
    const uint32_t bb = 1u << logb_;
    std::vector<fe> ev(bb);
    SP_TRY(readback(ev.data(), d_fri_evals_[L], sizeof(fe) * bb));
    fe sum = fe_zero();
    for (auto& e : ev) sum = fe_add(sum, e);
    *last_value = fe_mul(sum, binv_);
    fri_layer_ = L;
    stage_ = Stage::FriDone;
    return SP_OK;
}

int StarkProver::grind(const uint8_t challenge[32], uint8_t factor, uint64_t* nonce_out) {
    SP_HIP_CHECK(hipSetDevice(c_->device));
    // expected number of trials 2^factor: ranges of about that size, four queued per host round trip (a range that starts
    // beyond an already found nonce returns at once)
    const uint64_t sub = 1ULL << std::min<uint32_t>(std::max<uint32_t>(factor, 16), 22);
    const uint64_t batch = 4 * sub;
    unsigned long long init = ~0ULL;
    SP_HIP_CHECK(hipMemcpyAsync(d_nonce_, &init, sizeof(init), hipMemcpyHostToDevice, c_->stream));
    for (uint64_t start = 0;; start += batch) {
        for (uint32_t u = 0; u < 4; ++u) SP_TRY(grind_range(c_->stream, challenge, factor, start + u * sub, sub, d_nonce_));
        unsigned long long r = 0;
        SP_TRY(readback(&r, d_nonce_, sizeof(r)));
        if (r != ~0ULL) { *nonce_out = r; return SP_OK; }
        if (start > (1ULL << 40)) { sp_set_error("grind: nonce not found"); return SP_E_UNSUPPORTED; }
    }
}

// fri_query_phase + open_deep_composition_poly (reference fri/mod.rs:74-127, prover.rs:484-529).  Every queried value and
// authentication path is gathered on the device into one staging block with the same layout on every rank; with several
// ranks the blocks are all-gathered once and the copy of the rank that owns the item is kept: LDE rows and sharded FRI values
// live on the rank with role index mod G, the lower levels of a sharded tree on the rank whose contiguous leaf range holds
// the index, the top log2 G levels everywhere.
int StarkProver::open(const std::vector<uint64_t>& iotas, Openings& o, bool values_canonical_be) {
    if (stage_ != Stage::FriDone) { sp_set_error("open: FRI commit phase not finished"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const uint32_t q = (uint32_t)iotas.size();
    if (q == 0 || q > 1024) return SP_E_INVALID_ARG;
    const uint32_t L = logn_, d0 = logN_;
    o.n_queries = q; o.n_layers = L; o.n_cols = C_; o.depth0 = d0; o.values_canonical_be = values_canonical_be;
    hipStream_t st = c_->stream;
    const LdeOrder ord = lde_order();
    struct TreeJob { const TreeBuf* t; std::vector<uint64_t> idx; size_t lower_off = 0, upper_off = 0, ipos = 0, iown = 0; uint32_t dl = 0, du = 0; };
    struct ValJob { const fe* base; uint64_t stride; uint32_t ncols; bool sharded; std::vector<uint64_t> idx, local; size_t off = 0, ipos = 0; };
    std::vector<TreeJob> tj;
    std::vector<ValJob> vj;
    std::vector<uint64_t> pos(q);
    for (uint32_t s = 0; s < q; ++s) pos[s] = iotas[s] % N_;
    auto local_row = [&](uint64_t i) -> uint64_t {   // position of LDE row i inside the coset-major columns of its owner
        return ord.at(i >> logG_);
    };
    {   // trace and composition rows
        ValJob t{d_lde_, Nl_, C_, G_ > 1, pos, {}}; ValJob c{d_h12_, Nl_, 2, G_ > 1, pos, {}};
        for (uint32_t s = 0; s < q; ++s) { uint64_t l = ((pos[s] & (G_ - 1)) == rank_) ? local_row(pos[s]) : 0; t.local.push_back(l); c.local.push_back(l); }
        vj.push_back(std::move(t)); vj.push_back(std::move(c));
    }
    tj.push_back(TreeJob{&tree_main_, pos});
    if (Ca_) tj.push_back(TreeJob{&tree_aux_, pos});
    tj.push_back(TreeJob{&tree_comp_, pos});
    for (uint32_t k = 0; k < L; ++k) {   // FRI layers: index iota mod |D_k| and its symmetric index
        const uint64_t M = N_ >> k;
        std::vector<uint64_t> idx(2 * (size_t)q);
        for (uint32_t s = 0; s < q; ++s) { idx[s] = iotas[s] % M; idx[q + s] = (iotas[s] + M / 2) % M; }
        ValJob v{d_fri_evals_[k], 0, 1, fri_sharded(k), idx, {}};
        for (uint64_t i : idx) v.local.push_back(fri_sharded(k) ? (((i & (G_ - 1)) == rank_) ? (i >> logG_) : 0) : i);
        vj.push_back(std::move(v));
        tj.push_back(TreeJob{&fri_trees_[k], idx});
    }
    // staging layout (32-byte items) and the index array (uint64)
    size_t items = 0, nidx = 0;
    for (auto& v : vj) { v.off = items; items += v.idx.size() * v.ncols; v.ipos = nidx; nidx += v.idx.size(); }
    const size_t value_items = items;        // the field elements come first in the staging block, the digests behind them
    for (auto& t : tj) {
        t.dl = (uint32_t)sp_log2_exact(t.t->sub_leaves); t.du = t.t->top == t.t->sub ? 0u : logG_;
        t.lower_off = items; items += t.idx.size() * t.dl;
        t.upper_off = items; items += t.idx.size() * t.du;
        t.ipos = nidx; nidx += t.idx.size();
        t.iown = nidx; if (t.du) nidx += t.idx.size();
    }
    std::vector<uint64_t>& hidx = h_idx_open_;   // (members, like `up` below: read by asynchronous copies)
    hidx.assign(nidx, 0);
    for (auto& v : vj) std::copy(v.local.begin(), v.local.end(), hidx.begin() + v.ipos);
    for (auto& t : tj)
        for (size_t s = 0; s < t.idx.size(); ++s) {
            hidx[t.ipos + s] = t.idx[s] & (t.t->sub_leaves - 1);
            if (t.du) hidx[t.iown + s] = t.idx[s] / t.t->sub_leaves;
        }
    // one job table for every array (values, lower and upper tree parts), uploaded with the indices: one copy, one launch
    std::vector<GatherJob> jobs;
    uint32_t max_items = 0;
    auto add_job = [&](const void* base, uint64_t stride_or_leaves, size_t idx_off, size_t out_off, size_t count, uint32_t width, uint32_t kind) {
        if (count == 0 || width == 0) return;
        jobs.push_back(GatherJob{base, stride_or_leaves, (uint64_t)idx_off, (uint64_t)out_off, (uint32_t)count, width, kind, 0u});
        max_items = std::max<uint32_t>(max_items, (uint32_t)count * width);
    };
    for (auto& v : vj) add_job(v.base, v.stride, v.ipos, v.off, v.idx.size(), v.ncols, 0);
    for (auto& t : tj) {
        add_job(t.t->sub, t.t->sub_leaves, t.ipos, t.lower_off, t.idx.size(), t.dl, 1);
        if (t.du) add_job(t.t->top, G_, t.iown, t.upper_off, t.idx.size(), t.du, 1);
    }
    const size_t idx_bytes = (nidx * sizeof(uint64_t) + 255) & ~size_t(255);
    const size_t job_bytes = (jobs.size() * sizeof(GatherJob) + 255) & ~size_t(255);
    const size_t blk_bytes = items * 32;
    const size_t need = idx_bytes + job_bytes + blk_bytes * (G_ > 1 ? 1 + (size_t)world_ : 1);
    ScopedDevAlloc tmp(st);                  // many queries on a tiny domain: own staging buffer
    uint8_t* base = reinterpret_cast<uint8_t*>(d_scratch_);
    if (need > scratch_elems() * sizeof(fe)) {
        SP_TRY(tmp.alloc(need, "open"));
        base = static_cast<uint8_t*>(tmp.p);
    }
    uint64_t* d_idx = reinterpret_cast<uint64_t*>(base);
    GatherJob* d_jobs = reinterpret_cast<GatherJob*>(base + idx_bytes);
    fe* blk = reinterpret_cast<fe*>(base + idx_bytes + job_bytes);
    fe* all_dev = blk + items;
    std::vector<uint8_t>& up = h_up_open_;
    up.assign(idx_bytes + job_bytes, 0);
    std::memcpy(up.data(), hidx.data(), nidx * sizeof(uint64_t));
    std::memcpy(up.data() + idx_bytes, jobs.data(), jobs.size() * sizeof(GatherJob));
    SP_HIP_CHECK(hipMemcpyAsync(base, up.data(), up.size(), hipMemcpyHostToDevice, st));
    SP_TRY(gather_jobs(st, d_jobs, (uint32_t)jobs.size(), max_items, d_idx, blk));
    if (values_canonical_be) SP_TRY(encode_elements(st, SP_FE_CANON_BE, blk, value_items, reinterpret_cast<uint8_t*>(blk)));   // in place, element by element
    // the download lands in a page-locked buffer kept across proofs (a pageable destination is staged by the runtime: ~2 MB per proof)
    const size_t host_items = items * (G_ > 1 ? world_ : 1);
    SP_TRY(h_open_pin_.ensure(host_items * sizeof(fe), "open: page-locked download buffer", (host_items * sizeof(fe)) / 4));
    const fe* host = static_cast<const fe*>(h_open_pin_.p);
    if (G_ > 1) {
        SP_TRY(all_gather(blk, all_dev, blk_bytes, true));
        SP_HIP_CHECK(hipMemcpyAsync(h_open_pin_.p, all_dev, host_items * sizeof(fe), hipMemcpyDeviceToHost, st));
    } else {
        SP_HIP_CHECK(hipMemcpyAsync(h_open_pin_.p, blk, host_items * sizeof(fe), hipMemcpyDeviceToHost, st));
    }
    SP_HIP_CHECK(sp_stream_wait_polling(st));   // (hidx is a local)
    auto slot = [&](uint32_t owner) -> const fe* { return host + (G_ > 1 ? (size_t)owner * items : 0); };
    auto take_values = [&](const ValJob& v, size_t s, fe* dst) {
        const uint32_t owner = v.sharded ? (uint32_t)(v.idx[s] & (G_ - 1)) : rank_;
        const fe* src = slot(owner) + v.off + s * v.ncols;
        std::copy(src, src + v.ncols, dst);
    };
    auto take_path = [&](const TreeJob& t, size_t s, digest32* dst) {
        const uint32_t owner = t.du ? (uint32_t)(t.idx[s] / t.t->sub_leaves) : rank_;
        std::memcpy(dst, slot(owner) + t.lower_off + s * t.dl, (size_t)t.dl * 32);
        if (t.du) std::memcpy(dst + t.dl, slot(rank_) + t.upper_off + s * t.du, (size_t)t.du * 32);
    };
    // (every entry is written below: no zero fill of arrays an Openings object reused across proofs already has at this size;
    // the auxiliary paths of an AIR without an auxiliary segment are the exception)
    o.trace_evals.resize((size_t)q * C_); o.comp_evals.resize((size_t)q * 2);
    o.main_paths.resize((size_t)q * d0); o.comp_paths.resize((size_t)q * d0);
    if (Ca_) o.aux_paths.resize((size_t)q * d0); else o.aux_paths.assign((size_t)q * d0, digest32{});
    size_t path_total = 0;
    for (uint32_t k = 0; k < L; ++k) path_total += d0 - k;
    o.fri_evals.resize((size_t)q * L); o.fri_evals_sym.resize((size_t)q * L);
    o.fri_paths.resize((size_t)q * path_total); o.fri_paths_sym.resize((size_t)q * path_total);
    size_t ti = 0;
    const TreeJob& jm = tj[ti++];
    const TreeJob* ja = Ca_ ? &tj[ti++] : nullptr;
    const TreeJob& jc = tj[ti++];
    for (uint32_t s = 0; s < q; ++s) {
        take_values(vj[0], s, &o.trace_evals[(size_t)s * C_]);
        take_values(vj[1], s, &o.comp_evals[(size_t)s * 2]);
        take_path(jm, s, &o.main_paths[(size_t)s * d0]);
        if (ja) take_path(*ja, s, &o.aux_paths[(size_t)s * d0]);
        take_path(jc, s, &o.comp_paths[(size_t)s * d0]);
    }
    size_t path_off = 0;
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t depth = d0 - k;
        const ValJob& v = vj[2 + k];
        const TreeJob& t = tj[ti + k];
        for (uint32_t s = 0; s < q; ++s) {
            take_values(v, s, &o.fri_evals[(size_t)s * L + k]);
            take_values(v, q + s, &o.fri_evals_sym[(size_t)s * L + k]);
            take_path(t, s, &o.fri_paths[(size_t)s * path_total + path_off]);
            take_path(t, q + s, &o.fri_paths_sym[(size_t)s * path_total + path_off]);
        }
        path_off += depth;
    }
    return SP_OK;
}

}  // namespace sp
