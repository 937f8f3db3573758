// Whole-proof drivers on top of the round-level prover (see prover.h): the proof writer, rounds 2 - 4 with the host side of the
// Fiat-Shamir transcript (transcript.h), generate_cairo_proof (reference src/cairo/air.rs:1165-1171) and prove::<F, A> for program AIRs (src/starks/prover.rs:532-766).
#include "prover_internal.h"
#include "transcript.h"
#include <array>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

namespace sp {

// ============================================================================================ whole proof (host driver)
namespace {

// Writes the proof in one pass into a buffer of its final size (every length of the format is known before the first byte).
struct ProofWriter {
    std::vector<uint8_t> b;
    size_t at = 0;
    explicit ProofWriter(size_t total) : b(total) {}
    void u64(uint64_t v) { for (int i = 7; i >= 0; --i) b[at++] = (uint8_t)(v >> (8 * i)); }
    void felt(const fe& x) { fe_to_bytes_be(x, &b[at]); at += 32; }
    // an opened value: Montgomery limbs, or already the 32 wire bytes (Openings::values_canonical_be)
    void opened(const fe& x, bool canonical_be) { if (canonical_be) { std::memcpy(&b[at], &x, 32); at += 32; } else felt(x); }
    void raw(const void* p, size_t n) { std::memcpy(&b[at], p, n); at += n; }
    void path(const digest32* p, uint32_t depth) { u64(depth); raw(p, (size_t)depth * 32); }
};

typedef std::array<uint8_t, 32> Root;

// One whole proof between its entry point and the proof writer: what begin_proof and round 1 leave for rounds 2 - 4.
struct ProofRun {
    ProverHolder* H = nullptr;   // the prover kept (with its device buffers) across proofs of the same shape on this context
    Transcript tr;
    std::vector<Root> roots;     // of the trace segments, in the order of their commitment
    double _tp = 0, head_ms = 0; // SP_TIMING's previous point; SP_TAIL_TIMING: wall time from the entry to the first event
    void trace_committed(const uint8_t root[32]) {
        roots.emplace_back();
        std::memcpy(roots.back().data(), root, 32);
        tr.append(root, 32);
    }
};

}  // namespace

// StarkProof serialization (reference proof/stark.rs:161-218, fri/fri_decommit.rs:24-45, frame.rs:86-106).
// roots: the trace-segment roots (one or two); ood: frame rows x C evaluations.
static void serialize_proof(uint64_t n, const std::vector<Root>& roots, uint32_t C, const std::vector<fe>& ood,
                            const uint8_t comp_root[32], const fe& h1z, const fe& h2z, const std::vector<std::vector<uint8_t>>& fri_roots,
                            const fe& last_value, const std::vector<uint64_t>& iotas, const Openings& o, uint64_t nonce,
                            std::vector<uint8_t>& proof_out) {
    const uint32_t L = o.n_layers, d0 = o.depth0;
    const bool be = o.values_canonical_be;
    const size_t Q = iotas.size(), R = roots.size();
    size_t path_total = 0;
    for (uint32_t k = 0; k < L; ++k) path_total += d0 - k;
    // sizes of the nested records (each is preceded by its byte length)
    const size_t frame_bytes = 16 + 32 * ood.size() + 8;
    const size_t paths_bytes = (size_t)L * 8 + path_total * 32;                       // L paths: depth word + digests
    const size_t query_bytes = 8 + paths_bytes + 8 + 8 + (size_t)L * 32 + 8 + (size_t)L * 32 + 8 + paths_bytes;
    const size_t opening_bytes = (8 + (size_t)d0 * 32) + 8 + 64 + 8 + R * (8 + (size_t)d0 * 32) + 8 + (size_t)C * 32;
    const size_t total = 8 + 8 + R * 32 + 8 + frame_bytes + 32 + 8 + 64 + 8 + fri_roots.size() * 32 + 32 + 8 + Q * (8 + query_bytes) + 8 + Q * (8 + opening_bytes) + 8;
    ProofWriter w(total);
    w.u64(n);
    w.u64(R);
    for (auto& r : roots) w.raw(r.data(), 32);
    w.u64(frame_bytes);
    w.u64(ood.size()); w.u64(32);
    for (auto& e : ood) w.felt(e);
    w.u64(C);
    w.raw(comp_root, 32);
    w.u64(32); w.felt(h1z); w.felt(h2z);
    w.u64(fri_roots.size());
    for (auto& r : fri_roots) w.raw(r.data(), 32);
    w.felt(last_value);
    w.u64(Q);
    for (size_t s = 0; s < Q; ++s) {
        w.u64(query_bytes);
        w.u64(L);
        size_t po = 0;
        for (uint32_t k = 0; k < L; ++k) { w.path(&o.fri_paths_sym[s * path_total + po], d0 - k); po += d0 - k; }
        w.u64(32);
        w.u64(L);
        for (uint32_t k = 0; k < L; ++k) w.opened(o.fri_evals_sym[s * L + k], be);
        w.u64(L);
        for (uint32_t k = 0; k < L; ++k) w.opened(o.fri_evals[s * L + k], be);
        w.u64(L);
        po = 0;
        for (uint32_t k = 0; k < L; ++k) { w.path(&o.fri_paths[s * path_total + po], d0 - k); po += d0 - k; }
    }
    w.u64(Q);
    for (size_t s = 0; s < Q; ++s) {
        w.u64(opening_bytes);
        w.path(&o.comp_paths[s * d0], d0);
        w.u64(32);
        w.opened(o.comp_evals[s * 2], be); w.opened(o.comp_evals[s * 2 + 1], be);
        w.u64(R);
        w.path(&o.main_paths[s * d0], d0);
        if (R > 1) w.path(&o.aux_paths[s * d0], d0);
        w.u64(C);
        for (uint32_t j = 0; j < C; ++j) w.opened(o.trace_evals[s * C + j], be);
    }
    w.u64(nonce);
    if (w.at != total) throw std::runtime_error("serialize_proof: size bookkeeping is off");
    proof_out.swap(w.b);
}

ProverHolder* prover_holder(sp_ctx* c, bool create) {
    ProverHolder* h = dynamic_cast<ProverHolder*>(c->prover_state_deleter_holder);
    if (!h && create) {
        delete c->prover_state_deleter_holder;
        h = new ProverHolder(c);
        c->prover_state_deleter_holder = h;
    }
    return h;
}

// What every whole proof starts with: the context's prover at this shape, the round timers and the mark in front of round 1.
static int begin_proof(sp_ctx* ctx, uint64_t n, uint32_t main_cols, uint32_t aux_cols, bool has_rc, const ProofOptionsHost& opt, ProofRun& run) {
    run.H = prover_holder(ctx, true);
    if (opt.fri_number_of_queries == 0) { sp_set_error("prove: fri_number_of_queries must be at least 1 (the reference emits a proof without openings for 0; this prover does not)"); return SP_E_INVALID_ARG; }
    for (auto& e : run.H->round_ev) if (!e) SP_HIP_CHECK(hipEventCreate(&e));
    double& _tp = run._tp;
    const double t_entry = _tp = wall_ms();
    SP_TRY(run.H->prover.setup(n, main_cols, aux_cols, has_rc, opt));
    SP_TIMEPOINT("setup (alloc + tables)");
    SP_HIP_CHECK(hipEventRecord(run.H->round_ev[0], ctx->stream));
    run.head_ms = wall_ms() - t_entry;
    return SP_OK;
}

// Rounds 2 - 4 and the proof bytes, from the transcript as round 1 left it (both segment roots appended, round_ev[1] recorded).
// B, T: numbers of boundary and transition constraints; composition(b_alpha, b_beta, t_alpha, t_beta, root_out) runs round 2 of
// this AIR with the four sampled coefficient vectors.
template <class Composition>
static int finish_proof(sp_ctx* ctx, ProofRun& run, size_t B, size_t T, const ProofOptionsHost& opt, Composition&& composition,
                        std::vector<uint8_t>& proof_out, float round_ms[5]) {
    static const bool tail_timing = std::getenv("SP_TAIL_TIMING") != nullptr;
    StarkProver* P = &run.H->prover;
    hipEvent_t* ev = run.H->round_ev;
    Transcript& tr = run.tr;
    double& _tp = run._tp;
    uint8_t root[32];
    // ---- round 2 (reference prover.rs:597-635)
    std::vector<fe> b_alpha(B), b_beta(B), t_alpha(T), t_beta(T);
    for (auto& x : b_alpha) x = tr.to_field();
    for (auto& x : b_beta) x = tr.to_field();
    for (auto& x : t_alpha) x = tr.to_field();
    for (auto& x : t_beta) x = tr.to_field();
    SP_TRY(composition(b_alpha, b_beta, t_alpha, t_beta, root));
    uint8_t comp_root[32]; std::memcpy(comp_root, root, 32);
    SP_TIMEPOINT("r2 composition");
    tr.append(root, 32);
    SP_HIP_CHECK(hipEventRecord(ev[2], ctx->stream));
    // ---- round 3 (reference prover.rs:652-684)
    const uint32_t logn = (uint32_t)sp_log2_exact(P->n()), logN = logn + (uint32_t)sp_log2_exact(opt.blowup_factor);
    const fe z = sample_z_outside_domains(tr, fe_inv(fe_from_u64(opt.coset_offset)), logn, logN);
    fe h1z, h2z;
    std::vector<fe> ood;
    SP_TRY(P->ood(z, &h1z, &h2z, ood));
    SP_TIMEPOINT("r3 ood");
    tr.append_felt(h1z); tr.append_felt(h2z);
    for (auto& e : ood) tr.append_felt(e);
    SP_HIP_CHECK(hipEventRecord(ev[3], ctx->stream));
    // ---- round 4 (reference prover.rs:327-404)
    fe gamma = tr.to_field(), gamma_p = tr.to_field();
    std::vector<fe> tg((size_t)P->frame_rows() * P->cols());
    for (auto& x : tg) x = tr.to_field();
    SP_TRY(P->deep_fri_begin(gamma, gamma_p, tg, root));
    std::vector<std::vector<uint8_t>> fri_roots;
    fri_roots.emplace_back(root, root + 32);
    tr.append(root, 32);
    fe last_value;
    for (;;) {
        fe zeta = tr.to_field();
        // From the first layer this rank holds whole (layer 0 on one GPU; behind the sharded layers otherwise) the layers follow
        // each other on the device without a host round trip; the transcript catches up afterwards.
        if (P->fri_chain_available()) {
            std::vector<Root> rest;
            SP_TRY(P->fri_commit_chain(zeta, tr.buf.data(), rest, &last_value));
            for (auto& r : rest) {
                fri_roots.emplace_back(r.begin(), r.end());
                tr.append(r.data(), 32);
                (void)tr.to_field();      // zeta_k: the device sampled the same value
            }
            break;
        }
        int is_last = 0;
        SP_TRY(P->fri_fold_commit(zeta, root, &last_value, &is_last));
        if (is_last) break;
        fri_roots.emplace_back(root, root + 32);
        tr.append(root, 32);
    }
    SP_TIMEPOINT("r4 deep + fri commit");
    tr.append_felt(last_value);
    uint8_t gch[32];
    tr.challenge(gch);
    uint64_t nonce = 0;
    SP_TRY(P->grind(gch, opt.grinding_factor, &nonce));
    tr.append_u64_be(nonce);
    SP_TIMEPOINT("r4 grinding");
    std::vector<uint64_t> iotas(opt.fri_number_of_queries);
    for (auto& x : iotas) x = tr.to_usize() % P->N();
    Openings& o = run.H->open;         // (kept with the prover: its arrays are reused by the next proof)
    SP_TRY(P->open(iotas, o, true));   // opened values as wire bytes (encoded on the device)
    SP_TIMEPOINT("r4 openings");
    const double t_open = wall_ms();
    SP_HIP_CHECK(hipEventRecord(ev[4], ctx->stream));
    SP_HIP_CHECK(hipEventSynchronize(ev[4]));
    round_ms[0] = 0.f;
    for (int r = 0; r < 4; ++r) SP_HIP_CHECK(hipEventElapsedTime(&round_ms[r + 1], ev[r], ev[r + 1]));
    const double t_ser0 = wall_ms();
    serialize_proof(P->n(), run.roots, P->cols(), ood, comp_root, h1z, h2z, fri_roots, last_value, iotas, o, nonce, proof_out);
    if (tail_timing) std::fprintf(stderr, "[sp_tail] before the first event %.3f ms, events + bookkeeping after open() %.3f ms, serialize %.3f ms\n", run.head_ms,
                                  t_ser0 - t_open, wall_ms() - t_ser0);
    return SP_OK;
}

int cairo_prove(sp_ctx* ctx, const uint8_t* main_trace, uint64_t n, uint32_t cols, const PublicInputs& pub,
                const ProofOptionsHost& opt, std::vector<uint8_t>& proof_out, float round_ms[5],
                StarkProver::TraceSource src, int col_enc, uint64_t col_stride) {
    try {
        CairoAirInfo air = cairo_air_info(pub);
        if (cols != air.main_columns) { sp_set_error("cairo_prove: main trace must have 34 columns (43 with the range-check builtin)"); return SP_E_INVALID_ARG; }
        ProofRun run;
        SP_TRY(begin_proof(ctx, n, air.main_columns, air.aux_columns, air.has_rc_builtin, opt, run));
        StarkProver* P = &run.H->prover;
        double& _tp = run._tp;
        uint8_t root[32];
        // ---- round 1 (reference prover.rs:187-224)
        P->request_aux_presort(pub);                    // the sorts of the auxiliary trace: beside round 1 too
        if (pub.num_steps >= 1 && pub.num_steps <= n)   // round 2's boundary denominators need no challenge: beside round 1
            SP_TRY(P->prefetch_boundary_inverses({0, pub.num_steps - 1, n - 1}));
        P->hint_binary_columns(16);                     // the instruction flags (air.rs:29-46): one bit per cell over PCIe from a row-major host table
        SP_TRY(P->commit_trace(0, main_trace, cols, root, src, col_enc, col_stride));
        SP_TIMEPOINT("r1 commit main (H2D+iNTT+LDE+Merkle)");
        run.trace_committed(root);
        fe rap[3] = {run.tr.to_field(), run.tr.to_field(), run.tr.to_field()};
        SP_TRY(P->commit_aux_cairo(pub, rap, root));
        SP_TIMEPOINT("r1 aux trace + commit (device)");
        run.trace_committed(root);
        SP_HIP_CHECK(hipEventRecord(run.H->round_ev[1], ctx->stream));
        std::vector<BoundaryConstraint> bcs = boundary_constraints(pub, rap, n, air.has_rc_builtin);
        const uint32_t T = air.num_transition_constraints;
        SP_TRY(P->composition_precheck(rap, bcs, T));   // runs while finish_proof samples the round 2 challenges
        auto composition = [&](const std::vector<fe>& b_alpha, const std::vector<fe>& b_beta, const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta, uint8_t* root_out) {
            return P->composition(rap, bcs, b_alpha, b_beta, t_alpha, t_beta, air.transition_degrees, air.transition_exemptions, root_out);
        };
        return finish_proof(ctx, run, bcs.size(), T, opt, composition, proof_out, round_ms);
    } catch (const std::exception& e) {
        sp_set_error(std::string("cairo_prove: ") + e.what());
        return SP_E_INVALID_ARG;
    }
}

// Round 1 of a program AIR (reference prover.rs:187-224) on a prover that begin_proof has set up: the main segment, the RAP
// challenges - sampled from the transcript, or rap_given (air_check_trace with the caller's challenges) -, the auxiliary segment by
// its kind.  Leaves main || aux on the device as round 2 reads it.
static int air_round1(sp_ctx* ctx, ProofRun& run, const AirStatement& st, const uint8_t* main_trace, uint64_t n, std::vector<fe>& rap,
                      const std::vector<fe>* rap_given = nullptr) {
    const AirDescHost& air = st.air;
    StarkProver* P = &run.H->prover;
    Transcript& tr = run.tr;
    uint8_t root[32];
    // (with a main-trace program `main_trace` holds the input columns only, in host or device memory, and the device derives the rest)
    if (st.main) SP_TRY(P->commit_main_program(st, main_trace, root));
    else SP_TRY(P->commit_trace(0, main_trace, air.main_cols, root));
    run.trace_committed(root);
    rap.assign(air.n_rap, fe_zero());
    for (auto& x : rap) x = tr.to_field();
    if (rap_given) rap = *rap_given;
    if (air.aux_cols && air.aux_kind == 2) {
        // build_auxiliary_trace of the caller's AIR (traits.rs:25-29): row-major n x aux_cols from the RAP challenges
        if (!air.aux_fn) { sp_set_error("air_prove: aux_kind 2 needs aux_fn"); return SP_E_INVALID_ARG; }
        std::vector<uint8_t> rap_bytes(std::max<size_t>(1, rap.size()) * 32), aux_rows((size_t)n * air.aux_cols * 32);
        if (!rap.empty()) SP_TRY(sp_fe_from_device(ctx->enc, reinterpret_cast<const uint8_t*>(rap.data()), rap.size(), rap_bytes.data()));
        if (air.aux_fn(air.aux_user, rap_bytes.data(), (uint32_t)rap.size(), aux_rows.data()) != 0) { sp_set_error("air_prove: the auxiliary-trace callback failed"); return SP_E_INVALID_ARG; }
        SP_TRY(P->commit_trace(1, aux_rows.data(), air.aux_cols, root));
        run.trace_committed(root);
    } else if (air.aux_cols && air.aux_kind == SP_AIR_AUX_PROGRAM && st.aux) {
        // the auxiliary program on the device, from the resident main trace (every rank holds all of it: no exchange)
        SP_TRY(P->commit_aux_program(st, rap, root));
        run.trace_committed(root);
    } else if (air.aux_cols) {
        if (air.aux_kind != 1 || air.aux_cols != 1 || air.main_cols < 2 || air.n_rap < 1) {
            sp_set_error("air_prove: unknown auxiliary-trace kind (1 = fibonacci_rap permutation column, 2 = caller-supplied)");
            return SP_E_UNSUPPORTED;
        }
        // fibonacci_rap.rs:69-93: z_0 = 1, z_i = z_(i-1) (a_(i-1) + gamma) / (b_(i-1) + gamma)
        std::vector<fe> den(n), num(n);
        for (uint64_t i = 0; i < n; ++i) {
            fe a, b;
            const uint8_t* row = main_trace + (size_t)i * air.main_cols * 32;
            if (ctx->enc == SP_FE_CANON_BE) { a = fe_from_bytes_be(row); b = fe_from_bytes_be(row + 32); }
            else { uint64_t l[4]; std::memcpy(l, row, 32); a = fe_from_lw_limbs(l); std::memcpy(l, row + 32, 32); b = fe_from_lw_limbs(l); }
            num[i] = fe_add(a, rap[0]); den[i] = fe_add(b, rap[0]);
        }
        for (auto& d : den) if (fe_is_zero(d)) { sp_set_error("air_prove: zero denominator in the permutation column"); return SP_E_ZERO_INVERSE; }
        host_batch_inverse(den);
        std::vector<uint8_t> aux_rows((size_t)n * 32);
        fe zacc = fe_one();
        for (uint64_t i = 0; i < n; ++i) {
            if (i > 0) zacc = fe_mul(zacc, fe_mul(num[i - 1], den[i - 1]));
            if (ctx->enc == SP_FE_CANON_BE) fe_to_bytes_be(zacc, &aux_rows[(size_t)i * 32]);
            else { uint64_t l[4]; fe_to_lw_limbs(zacc, l); std::memcpy(&aux_rows[(size_t)i * 32], l, 32); }
        }
        SP_TRY(P->commit_trace(1, aux_rows.data(), 1, root));
        run.trace_committed(root);
    }
    return SP_OK;
}

// The main segment a statement's main-trace program builds from `inputs`, without a commitment (sp_air_main_trace): the prover at
// this shape under the smallest options, the builder of commit_main_program, the table back on the host.
int air_main_trace(sp_ctx* ctx, const AirStatement& st, const uint8_t* inputs, uint64_t n, uint8_t* rows_out) {
    try {
        if (!st.main) { sp_set_error("air_main_trace: the statement has no main program"); return SP_E_INVALID_ARG; }
        ProofRun run;
        SP_TRY(begin_proof(ctx, n, st.air.main_cols, st.air.aux_cols, false, ProofOptionsHost{2, 1, 3, 0}, run));
        return run.H->prover.main_program_table(st, inputs, rows_out);
    } catch (const std::exception& e) {
        sp_set_error(std::string("air_main_trace: ") + e.what());
        return SP_E_INVALID_ARG;
    }
}

// boundary_constraints(rap_challenges) (traits.rs:44-47): the AIR as everything behind round 1 sees it - the descriptor itself, or, with
// boundary values computed from the challenges, a copy (`resolved`) whose boundary constraints carry them as constants.
static int air_with_boundary(const AirStatement& st, const std::vector<fe>& rap, AirDescHost& resolved, const AirDescHost*& use) {
    use = &st.air;
    if (!st.bvals) return SP_OK;
    resolved = st.air;
    if (!air_resolve_boundary_into(*st.bvals, rap, resolved.boundary)) { sp_set_error("air_prove: a boundary value's denominator is zero under these challenges"); return SP_E_ZERO_INVERSE; }
    use = &resolved;
    return SP_OK;
}

// Which constraints of a program AIR the trace breaks (sp_air_check_trace; reference validate_trace, debug.rs:13-104): round 1 as
// air_prove runs it, then the report instead of rounds 2 - 4.  opt (nullable when rap is given): the options of the proof whose
// challenges are wanted; with the caller's challenges the commitments still run (under the smallest options when none are given),
// since they are how the prover takes a trace in.
int air_check_trace(sp_ctx* ctx, const AirStatement& st, const uint8_t* main_trace, uint64_t n, const ProofOptionsHost* opt,
                    const std::vector<fe>* rap_given, std::vector<AirViolationHost>& out) {
    const AirDescHost& air = st.air;
    try {
        if (!opt && !rap_given) { sp_set_error("air_check_trace: proof options are needed to sample the RAP challenges"); return SP_E_INVALID_ARG; }
        if (rap_given && rap_given->size() != air.n_rap) { sp_set_error("air_check_trace: one RAP challenge per n_rap"); return SP_E_INVALID_ARG; }
        if (ctx->world > 1) { sp_set_error("air_check_trace: a report from a sharded context (world > 1) is not supported"); return SP_E_UNSUPPORTED; }
        const ProofOptionsHost smallest{2, 1, 3, 0};
        ProofRun run;
        SP_TRY(begin_proof(ctx, n, air.main_cols, air.aux_cols, false, opt ? *opt : smallest, run));
        std::vector<fe> rap;
        SP_TRY(air_round1(ctx, run, st, main_trace, n, rap, rap_given));
        AirDescHost resolved;
        const AirDescHost* use = nullptr;
        SP_TRY(air_with_boundary(st, rap, resolved, use));
        return run.H->prover.check_trace_air(st, *use, rap, out);
    } catch (const std::exception& e) {
        sp_set_error(std::string("air_check_trace: ") + e.what());
        return SP_E_INVALID_ARG;
    }
}

// prove::<F, A> for a program AIR (reference src/starks/prover.rs:532-766): same rounds, the AIR-specific parts come from
// the descriptor - RAP challenges (n_rap field samples), auxiliary trace (by kind: the fibonacci_rap column and the caller's
// callback on the host - the example AIRs are tiny -, an auxiliary program on the device), boundary constraints, transition program.
int air_prove(sp_ctx* ctx, const AirStatement& st, const uint8_t* main_trace, uint64_t n, const ProofOptionsHost& opt, std::vector<uint8_t>& proof_out,
              float round_ms[5]) {
    const AirDescHost& air = st.air;
    try {
        ProofRun run;
        SP_TRY(begin_proof(ctx, n, air.main_cols, air.aux_cols, false, opt, run));
        StarkProver* P = &run.H->prover;
        std::vector<fe> rap;
        // ---- round 1 (reference prover.rs:187-224)
        SP_TRY(air_round1(ctx, run, st, main_trace, n, rap));
        SP_HIP_CHECK(hipEventRecord(run.H->round_ev[1], ctx->stream));
        AirDescHost resolved;
        const AirDescHost* use = nullptr;
        SP_TRY(air_with_boundary(st, rap, resolved, use));
        auto composition = [&](const std::vector<fe>& b_alpha, const std::vector<fe>& b_beta, const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta, uint8_t* root_out) {
            return P->composition_air(st, *use, rap, b_alpha, b_beta, t_alpha, t_beta, root_out);
        };
        return finish_proof(ctx, run, air.boundary.size(), air.degrees.size(), opt, composition, proof_out, round_ms);
    } catch (const std::exception& e) {
        sp_set_error(std::string("air_prove: ") + e.what());
        return SP_E_INVALID_ARG;
    }
}

}  // namespace sp
