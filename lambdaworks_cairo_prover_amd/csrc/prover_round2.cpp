// Round 2 of the prover (see prover.h): constraint composition for the Cairo AIR and for AIRs given as a constraint program, the
// exact trace check that picks the evaluation path, the H1 / H2 split, LDE and commitment.  Host code only.
#include "prover_internal.h"
#include <unordered_map>
#include <cstring>
#include <numeric>

namespace sp {

// Boundary constraints by row: the distinct steps in order of first appearance and, per constraint, which of them it sits on.
struct StepGroups { std::vector<uint64_t> steps; std::vector<uint32_t> group; };
static StepGroups group_by_step(const std::vector<BoundaryConstraint>& bcs) {
    StepGroups g;
    std::unordered_map<uint64_t, uint32_t> group_of;
    for (const BoundaryConstraint& bc : bcs) {
        const auto ins = group_of.emplace(bc.step, (uint32_t)g.steps.size());
        if (ins.second) g.steps.push_back(bc.step);
        g.group.push_back(ins.first->second);
    }
    return g;
}

// The per-coset tables of a composition with degree bound D = f n.  On the LDE domain x^n takes the b values xn = h^n w_b^c
// (reference evaluator.rs:156-171), and the degree adjustments x^(D - n (deg - 1)) and x^(D - n) are powers of it (evaluator.rs:142-154,
// :78-82; the Cairo AIR has f = 2, cairo/air.rs:855-857).  Row c of `coef` (rows `stride` elements apart): t_alpha[k] xn^(f - degrees[k] + 1)
// + t_beta[k] for the transitions, then b_alpha[j] xn^(f - 1) + b_beta[j] for the boundary constraints in the order given;
// zerofier[c] = 1 / (xn - 1).  f >= 1 and every degree in 1 .. f + 1 (the callers check); hn = h^n.
static void coset_tables(const fe& hn, uint32_t logb, uint32_t f, const std::vector<uint32_t>& degrees, const std::vector<fe>& t_alpha,
                         const std::vector<fe>& t_beta, const std::vector<fe>& b_alpha, const std::vector<fe>& b_beta, fe* coef, size_t stride, fe* zerofier) {
    const uint32_t b = 1u << logb, T = (uint32_t)degrees.size(), B = (uint32_t)b_alpha.size();
    const fe wb = host_primitive_root((int)logb);
    std::vector<fe> zf(b), pw(f + 1);   // pw[e] = xn^e
    fe xn = hn;
    for (uint32_t c = 0; c < b; ++c) {
        pw[0] = fe_one();
        for (uint32_t e = 1; e <= f; ++e) pw[e] = fe_mul(pw[e - 1], xn);
        fe* row = coef + (size_t)c * stride;
        for (uint32_t k = 0; k < T; ++k) row[k] = fe_add(fe_mul(t_alpha[k], pw[f - degrees[k] + 1]), t_beta[k]);
        for (uint32_t j = 0; j < B; ++j) row[T + j] = fe_add(fe_mul(b_alpha[j], pw[f - 1]), b_beta[j]);
        zf[c] = fe_sub(xn, fe_one());
        xn = fe_mul(xn, wb);
    }
    host_batch_inverse(zf);
    std::copy(zf.begin(), zf.end(), zerofier);
}

// What the second half of round 2 (composition_core and its three paths) is given.  The two kinds of AIR differ in the trace check
// (composition_core), round2_evaluate and round2_boundary_inverses only.  Cairo (prog == nullptr): K (per-coset coefficients,
// zerofier, boundary data) is complete, composition_core uploads it; `points` are the distinct boundary points g^step, one inverse
// array each.  A program AIR: its program, tables (tabs) and exempted rows' roots are on the device, `points` lists its distinct
// boundary points, and one inverse array 1 / Z_B(x) serves all of them.
struct StarkProver::Round2Air {
    const std::vector<fe>& points;
    const CompositionConsts* K;
    const AirProgram* prog;
    const AirCompTables* tabs;
    const fe* ex_roots;
    bool allow_sub_coset;          // the caller knows deg H < 2n for a constraint-satisfying trace
    const fe* roots = nullptr;     // of the LDE domain (composition_core sets it)
};

// The fields of the Cairo constants that the trace check and the composition both read (everything else zero).
int StarkProver::fill_cairo_consts(CompositionConsts& K, const fe rap[3], const std::vector<BoundaryConstraint>& bcs, uint32_t n_transitions) {
    std::memset(&K, 0, composition_consts_bytes(1u << logb_));   // (the per-coset tables only as far as this proof's blowup factor reaches)
    for (size_t j = 0; j < bcs.size(); ++j) {
        if (bcs[j].col >= C_) return SP_E_INVALID_ARG;
        K.bcol[j] = bcs[j].col; K.bvalue[j] = bcs[j].value; K.bstep[j] = bcs[j].step;
    }
    K.h = h_;
    K.rap[0] = rap[0]; K.rap[1] = rap[1]; K.rap[2] = rap[2];
    K.two = fe_from_u64(2);
    K.b15 = fe_from_u64(1ULL << 15); K.b16 = fe_from_u64(1ULL << 16); K.b32 = fe_from_u64(1ULL << 32); K.b48 = fe_from_u64(1ULL << 48);
    K.n_boundary = (uint32_t)bcs.size(); K.n_transitions = n_transitions; K.main_cols = Cm_; K.has_rc_builtin = has_rc_ ? 1 : 0;
    return SP_OK;
}

int StarkProver::composition_precheck(const fe rap[3], const std::vector<BoundaryConstraint>& bcs, uint32_t n_transitions) {
    check_pending_ = false;
    if (!segments_committed()) { sp_set_error("composition_precheck: trace segments not committed"); return SP_E_STATE; }
    if (n_transitions > CAIRO_MAX_TRANSITIONS || bcs.size() > CAIRO_MAX_BOUNDARY) return SP_E_INVALID_ARG;
    // the check only runs where composition_core would run it (2n-point paths)
    if (!sub_coset_shape() && !pair_shape()) return SP_OK;
    SP_HIP_CHECK(hipSetDevice(c_->device));
    SP_TRY(grow(od_.comp_consts_chk, 1));
    if (!h_comp_chk_) h_comp_chk_.reset(new CompositionConsts());
    SP_TRY(fill_cairo_consts(*h_comp_chk_, rap, bcs, n_transitions));
    SP_HIP_CHECK(hipMemcpyAsync(od_.comp_consts_chk.p, h_comp_chk_.get(), composition_consts_bytes(1u << logb_), hipMemcpyHostToDevice, c_->stream));
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    SP_TRY(cairo_trace_check(c_->stream, d_trace_, n_, od_.comp_consts_chk.p, c_->d_flag, check_row0(), check_rows()));
    check_pending_ = true;
    return SP_OK;
}

int StarkProver::composition(const fe rap[3], const std::vector<BoundaryConstraint>& bcs, const std::vector<fe>& b_alpha,
                             const std::vector<fe>& b_beta, const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta,
                             const std::vector<uint32_t>& degrees, const std::vector<uint32_t>& exemptions, uint8_t root_out[32]) {
    if (!segments_committed()) { sp_set_error("composition: trace segments not committed"); return SP_E_STATE; }
    const uint32_t T = (uint32_t)t_alpha.size(), B = (uint32_t)bcs.size();
    if (T > CAIRO_MAX_TRANSITIONS || B > CAIRO_MAX_BOUNDARY || t_beta.size() != T || b_alpha.size() != B || b_beta.size() != B ||
        degrees.size() != T || exemptions.size() != T) return SP_E_INVALID_ARG;
    SP_HIP_CHECK(hipSetDevice(c_->device));
    CompositionConsts K;
    SP_TRY(fill_cairo_consts(K, rap, bcs, T));
    // --- boundary denominators: distinct steps -> points g^step, one inverse array each
    const StepGroups g = group_by_step(bcs);
    if (g.steps.size() > 3) { sp_set_error("composition: more than 3 distinct boundary steps"); return SP_E_UNSUPPORTED; }
    std::copy(g.group.begin(), g.group.end(), K.bden);
    std::vector<fe> points;
    for (uint64_t s : g.steps) points.push_back(fe_pow_u64(g_, s));
    K.g_last = fe_pow_u64(g_, n_ - 1);
    // --- per-coset constants; the kernel knows the degrees 1 .. 3 with D = 2n, and one exempted row
    for (uint32_t k = 0; k < T; ++k)
        if (degrees[k] < 1 || degrees[k] > 3 || exemptions[k] > 1) return SP_E_UNSUPPORTED;
    coset_tables(fe_pow_u64(h_, n_), logb_, 2, degrees, t_alpha, t_beta, b_alpha, b_beta, &K.coef[0][0], COMP_MAX_TERMS, K.zerofier);
    // the kernel hard-codes which Cairo constraints are exempted / selector-gated; check the caller agrees
    PublicInputs dummy;
    if (has_rc_) dummy.memory_segments.push_back({0, 0, 0});
    const CairoAirInfo ref = cairo_air_info(dummy);
    if (ref.transition_degrees != degrees || ref.transition_exemptions != exemptions) {
        sp_set_error("composition: only the Cairo AIR constraint set is implemented on the device");
        return SP_E_UNSUPPORTED;
    }
    return composition_core(Round2Air{points, &K, nullptr, nullptr, nullptr, true}, root_out);
}

// Values nobody reads (directly or through other unread values) are not part of the program the device runs: giving such a value
// "any" slot would overwrite a live one when all AIR_MAX_LIVE are taken.  Liveness backwards from the OUT ops, then slots.
int air_assign_slots(const std::vector<AirOpHost>& ops, std::vector<AirOpDev>& dops, const char* live_error) {
    const uint32_t n_src = (uint32_t)ops.size();
    dops.clear();
    std::vector<uint8_t> live(n_src, 0);
    for (uint32_t t = n_src; t-- > 0;) {
        const AirOpHost& o = ops[t];
        if (o.op == 5) { live[t] = 1; live[o.b] = 1; }
        else if (live[t] && air_op_takes_two_values(o.op)) { live[o.a] = 1; live[o.b] = 1; }
        else if (live[t] && air_op_takes_one_value(o.op)) live[o.a] = 1;   // (an integer LIMB: b is an immediate)
    }
    std::vector<uint32_t> last_use(n_src, 0);
    for (uint32_t t = 0; t < n_src; ++t) {
        if (!live[t]) continue;
        const AirOpHost& o = ops[t];
        if (air_op_takes_two_values(o.op)) { last_use[o.a] = t; last_use[o.b] = t; }
        else if (air_op_takes_one_value(o.op)) last_use[o.a] = t;
        else if (o.op == 5) last_use[o.b] = t;
    }
    std::vector<uint16_t> slot_of(n_src, 0), free_slots;
    for (int sl = AIR_MAX_LIVE - 1; sl >= 0; --sl) free_slots.push_back((uint16_t)sl);
    std::vector<std::vector<uint32_t>> dying(n_src);    // values whose last use is op t
    for (uint32_t t = 0; t < n_src; ++t) if (live[t] && ops[t].op != 5) dying[last_use[t]].push_back(t);
    for (uint32_t t = 0; t < n_src; ++t) {
        if (!live[t]) continue;
        const AirOpHost& o = ops[t];
        AirOpDev d{};
        d.op = o.op;
        if (air_op_takes_two_values(o.op)) { d.a = slot_of[o.a]; d.b = slot_of[o.b]; }
        else if (air_op_takes_one_value(o.op)) { d.a = slot_of[o.a]; d.b = (uint16_t)o.b; }
        else if (o.op == 5) { d.a = (uint16_t)o.a; d.b = slot_of[o.b]; }
        else { d.a = (uint16_t)o.a; d.b = (uint16_t)o.b; }
        for (uint32_t v : dying[t]) free_slots.push_back(slot_of[v]);   // operands read before the result is written
        if (o.op != 5) {
            if (free_slots.empty()) { sp_set_error(live_error); return SP_E_UNSUPPORTED; }
            d.dst = free_slots.back(); free_slots.pop_back();
            slot_of[t] = d.dst;
        }
        dops.push_back(d);
    }
    return SP_OK;
}

int air_periodic_tables(hipStream_t st, NttEngine& ntt, fe* vals, fe* ws, fe* tab, uint32_t cnt, uint32_t logp, uint32_t logn, uint32_t logb, const fe& h) {
    if (logp > logn || cnt == 0) return SP_E_INVALID_ARG;
    const uint64_t p = 1ull << logp;
    const fe hq = fe_pow_u64(h, (1ull << logn) >> logp);   // x -> x^(n/p) takes the coset h <w_N> to hq <w_(p b)>
    if (p <= AIR_PERIODIC_DIRECT_MAX) {
        const fe* roots_pb = nullptr;
        SP_TRY(ntt.roots((int)(logp + logb), &roots_pb));
        return air_periodic_table_direct(st, vals, ws, tab, cnt, logp, logb, hq, roots_pb);
    }
    // as a trace column: unscaled bit-reversed inverse transform with the post factors p^-1 hq^rev(position), then the coset-major LDE
    SP_TRY(gen_power_table(st, ws, p, logp, hq, fe_inv(fe_from_u64(p))));
    SP_TRY(ntt.dif_natural_to_bitrev_inverse(vals, (int)logp, cnt, p, ws));
    return ntt.lde_coset_major(vals, tab, (int)logp, (int)logb, cnt, p, p << logb);
}

int air_stride_class_tables(hipStream_t st, NttEngine& ntt, fe* u, fe* z, uint32_t logs, uint32_t offset, uint32_t logn, uint32_t logb, const fe& h) {
    if (logs > logn || (offset >> logs)) return SP_E_INVALID_ARG;
    const uint64_t m = (1ull << logn) >> logs;   // n / s: x -> x^m takes the coset h <w_N> to h^m <w_(s b)>, row o to g^(o m)
    const fe* roots_sb = nullptr;
    SP_TRY(ntt.roots((int)(logs + logb), &roots_sb));
    return air_stride_tables(st, u, z, logs, logb, fe_pow_u64(h, m), fe_pow_u64(host_primitive_root((int)logn), offset * m), roots_sb);
}

// The device form of an AIR's constraint program, and what of the descriptor goes with it: checked against the committed trace, values
// in slots, the periodic columns' places, the exemptions as both the composition and the trace check use them.
int StarkProver::build_air_program(const AirStatement& st, const AirDescHost& air, size_t n_rap, AirProgramHost& out) {
    const uint32_t T = (uint32_t)air.degrees.size(), B = (uint32_t)air.boundary.size(), R = (uint32_t)air.offsets.size();
    if (T == 0 || T > AIR_MAX_TRANSITIONS || B > AIR_MAX_BOUNDARY || R == 0 || R > AIR_MAX_OFFSETS || air.exemptions.size() != T ||
        air.ops.size() > AIR_MAX_OPS || air.consts.size() > AIR_MAX_CONSTS || air.consts.size() + n_rap > 65535 || n_rap != air.n_rap ||
        air.main_cols != Cm_ || air.aux_cols != Ca_ || air.degree_bound_factor < 1) {
        sp_set_error("composition_air: descriptor out of range or inconsistent with the committed trace");
        return SP_E_INVALID_ARG;
    }
    const uint32_t f = air.degree_bound_factor;
    // --- validate the program (every operand refers to an earlier value, cells exist) and build the device copy: every
    //     value gets a slot of the per-point value file, released after its last use (the program is straight-line)
    AirProgram& prog = out.prog;
    std::memset(&prog, 0, sizeof(prog));
    std::vector<AirOpDev>& dops = out.dops;
    prog.n_ops = (uint32_t)air.ops.size();
    prog.n_offsets = R;
    for (uint32_t k = 0; k < R; ++k) prog.offsets[k] = air.offsets[k];
    // --- periodic columns: column k's values at pvals + off_k (off_k = the periods before it, summed), its table at ptab + off_k b
    //     (at most 64 of them, each a power of two <= n: the statement's decoder has seen to that)
    const uint32_t Kp = st.n_periodic();
    std::vector<AirPeriodicCol>& pcols = out.pcols;
    pcols.assign(Kp, AirPeriodicCol{});
    uint64_t S = 0;
    for (uint32_t k = 0; k < Kp; ++k) {
        const uint64_t p = st.periodic->cols[k].size();
        pcols[k] = AirPeriodicCol{(uint32_t)sp_log2_exact(p), 0u, S};
        S += p;
    }
    out.S = S;
    if (air_program_first_bad_op(air.ops, R, C_, air.consts.size() + n_rap, T, Kp) < air.ops.size()) { sp_set_error("composition_air: malformed constraint program"); return SP_E_INVALID_ARG; }
    SP_TRY(air_assign_slots(air.ops, dops, "composition_air: more than 64 values alive at once in the constraint program"));
    prog.n_ops = (uint32_t)dops.size();
    // --- transition exemptions (traits.rs:49-79, evaluator.rs:299-323): distinct non-zero counts; with
    //     num_transition_exemptions == 1 every exempted constraint uses the first of them
    //     (constraints of a stride class keep their own count and their own roots, below)
    if (!air_stride_plan(air, n_, out.plan)) { sp_set_error("composition_air: malformed strides of the transition constraints"); return SP_E_INVALID_ARG; }
    const AirStridePlan& plan = out.plan;
    std::vector<uint32_t> uniq;
    for (uint32_t k = 0; k < T; ++k) {
        const uint32_t e = air.exemptions[k];
        if (plan.cls[k] < 0 && e > 0 && std::find(uniq.begin(), uniq.end(), e) == uniq.end()) uniq.push_back(e);
    }
    if (uniq.size() > AIR_MAX_EXEMPT_KINDS) { sp_set_error("composition_air: too many distinct exemption counts"); return SP_E_UNSUPPORTED; }
    uint32_t max_ex = 0;
    for (size_t q = 0; q < uniq.size(); ++q) { prog.ex_count[q] = uniq[q]; max_ex = std::max(max_ex, uniq[q]); }
    if (max_ex >= n_) { sp_set_error("composition_air: exemptions exceed the trace length"); return SP_E_INVALID_ARG; }
    out.max_ex = max_ex;
    for (uint32_t k = 0; k < T; ++k) {
        const uint32_t e = air.exemptions[k], d = air.degrees[k];
        if (d < 1 || d > f + 1) { sp_set_error("composition_air: transition degree above the composition degree bound"); return SP_E_INVALID_ARG; }
        if (e && plan.cls[k] < 0) {
            size_t idx = air.num_transition_exemptions == 1 ? 0 : (size_t)(std::find(uniq.begin(), uniq.end(), e) - uniq.begin());
            prog.ex_kind[k] = 1 + (uint32_t)idx;
        }
        prog.ex_rows[k] = prog.ex_kind[k] ? prog.ex_count[prog.ex_kind[k] - 1] : 0;   // rows the composition really exempts for this constraint (what the trace check must mirror)
    }
    out.ex_eff.assign(prog.ex_rows, prog.ex_rows + T);
    // --- stride classes: the rows = o (mod s), zerofier x^(n/s) - g^(o n/s); an exemption product per (class, e) over the LAST e rows
    //     of the progression, o + s (n/s - 1 - t)
    AirStrideDev& sd = out.sdev;
    std::memset(&sd, 0, sizeof(sd));
    out.sroots.clear();
    out.stab = 0;
    if (!out.strided()) return SP_OK;
    sd.n_classes = (uint32_t)plan.classes.size(); sd.n_kinds = (uint32_t)plan.kinds.size();
    for (uint32_t q = 0; q < sd.n_classes; ++q) {
        sd.logs[q] = (uint32_t)sp_log2_exact(plan.classes[q].period); sd.off[q] = plan.classes[q].offset;
        sd.tab_off[q] = out.stab;
        out.stab += (uint64_t)plan.classes[q].period << logb_;
    }
    for (uint32_t j = 0; j < sd.n_kinds; ++j) {
        const AirStrideHost& c = plan.classes[plan.kinds[j].first];
        const uint32_t e = plan.kinds[j].second;
        sd.kind_count[j] = e; sd.kind_root0[j] = (uint32_t)out.sroots.size();
        for (uint32_t t = 0; t < e; ++t) out.sroots.push_back(fe_pow_u64(g_, c.offset + (uint64_t)c.period * (n_ / c.period - 1 - t)));
    }
    for (uint32_t k = 0; k < T; ++k) {
        if (plan.cls[k] < 0) continue;
        const AirStrideHost& c = plan.classes[plan.cls[k]];
        sd.cls[k] = (uint8_t)(1 + plan.cls[k]); sd.kind[k] = (uint8_t)(1 + plan.kind[k]);
        sd.last[k] = c.offset + (uint64_t)c.period * (n_ / c.period - 1 - air.exemptions[k]);
        out.ex_eff[k] = air.exemptions[k];
    }
    return SP_OK;
}

// The part of od_.air_buf that the composition and the trace check share, laid out and filled in h_air_up_ (every region 256-byte
// aligned): the AirProgram header with its ops / consts pointers set, the slotted ops, the constants followed by the RAP challenges,
// bvalue / bstep / bcol with constraint order[j] at position j, the periodic descriptors and values, the stride classes' descriptor
// (AirStrideDev) and exemption roots; behind them one region per entry
// of `extra` (its bytes, and where its offset goes), which the caller fills.  od_.air_buf is grown to the whole block; the caller
// uploads it in one copy.  tabs: T, B, bvalue, bstep, bcol, pcols, pvals, strides set, the rest zero.
int StarkProver::build_air_block(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, AirProgramHost& ph,
                                 const std::vector<uint32_t>& order, std::initializer_list<std::pair<size_t, size_t*>> extra,
                                 AirCompTables& tabs, const AirProgram*& prog_dev) {
    const uint32_t B = (uint32_t)air.boundary.size(), Kp = (uint32_t)ph.pcols.size();
    for (const BoundaryConstraint& bc : air.boundary)
        if (bc.col >= C_ || bc.step >= n_) { sp_set_error("composition_air: boundary constraint outside the trace"); return SP_E_INVALID_ARG; }
    UploadLayout lay;
    const size_t o_prog = lay.place(sizeof(AirProgram)), o_ops = lay.place(sizeof(AirOpDev) * ph.dops.size()),
                 o_consts = lay.place(sizeof(fe) * (air.consts.size() + rap.size())), o_bval = lay.place(sizeof(fe) * B),
                 o_bstep = lay.place(sizeof(uint64_t) * B), o_bcol = lay.place(sizeof(uint32_t) * B),
                 o_pcols = lay.place(sizeof(AirPeriodicCol) * Kp), o_pvals = lay.place(sizeof(fe) * ph.S);
    const size_t o_sdev = ph.strided() ? lay.place(sizeof(AirStrideDev)) : 0, o_sroots = ph.strided() ? lay.place(sizeof(fe) * ph.sroots.size()) : 0;
    for (const auto& x : extra) *x.second = lay.place(x.first);
    SP_TRY(grow(od_.air_buf, lay.bytes));
    std::vector<uint8_t>& up = h_air_up_;
    up.assign(lay.bytes, 0);
    auto dev_at = [&](size_t off) { return od_.air_buf.p + off; };
    ph.prog.ops = reinterpret_cast<const AirOpDev*>(dev_at(o_ops));
    ph.prog.consts = reinterpret_cast<const fe*>(dev_at(o_consts));
    std::memcpy(up.data() + o_prog, &ph.prog, sizeof(AirProgram));
    if (!ph.dops.empty()) std::memcpy(up.data() + o_ops, ph.dops.data(), sizeof(AirOpDev) * ph.dops.size());
    fill_consts_then_rap(up.data() + o_consts, air.consts, rap);
    fe* hbval = reinterpret_cast<fe*>(up.data() + o_bval);
    uint64_t* hbstep = reinterpret_cast<uint64_t*>(up.data() + o_bstep);
    uint32_t* hbcol = reinterpret_cast<uint32_t*>(up.data() + o_bcol);
    for (uint32_t jp = 0; jp < B; ++jp) {
        const BoundaryConstraint& bc = air.boundary[order[jp]];
        hbval[jp] = bc.value; hbstep[jp] = bc.step; hbcol[jp] = bc.col;
    }
    if (Kp) std::memcpy(up.data() + o_pcols, ph.pcols.data(), sizeof(AirPeriodicCol) * Kp);
    for (uint32_t k = 0; k < Kp; ++k) std::memcpy(up.data() + o_pvals + sizeof(fe) * ph.pcols[k].off, st.periodic->cols[k].data(), sizeof(fe) * st.periodic->cols[k].size());
    std::memset(&tabs, 0, sizeof(tabs));
    tabs.T = (uint32_t)air.degrees.size(); tabs.B = B;
    tabs.bvalue = reinterpret_cast<const fe*>(dev_at(o_bval));
    tabs.bstep = reinterpret_cast<const uint64_t*>(dev_at(o_bstep));
    tabs.bcol = reinterpret_cast<const uint32_t*>(dev_at(o_bcol));
    if (Kp) {
        tabs.pcols = reinterpret_cast<const AirPeriodicCol*>(dev_at(o_pcols));
        tabs.pvals = reinterpret_cast<const fe*>(dev_at(o_pvals));
    }
    if (ph.strided()) {   // the class descriptors and the exemption roots (sdev.u / zinv / beta: composition_air, in the upload at ph.o_sdev)
        ph.o_sdev = o_sdev;
        ph.sdev.roots = reinterpret_cast<const fe*>(dev_at(o_sroots));
        std::memcpy(up.data() + o_sdev, &ph.sdev, sizeof(AirStrideDev));
        if (!ph.sroots.empty()) std::memcpy(up.data() + o_sroots, ph.sroots.data(), sizeof(fe) * ph.sroots.size());
        tabs.strides = reinterpret_cast<const AirStrideDev*>(dev_at(o_sdev));
    }
    prog_dev = reinterpret_cast<const AirProgram*>(dev_at(o_prog));
    return SP_OK;
}

int StarkProver::composition_air(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, const std::vector<fe>& b_alpha,
                                 const std::vector<fe>& b_beta, const std::vector<fe>& t_alpha, const std::vector<fe>& t_beta, uint8_t root_out[32]) {
    if (!segments_committed()) { sp_set_error("composition: trace segments not committed"); return SP_E_STATE; }
    const uint32_t T = (uint32_t)air.degrees.size(), B = (uint32_t)air.boundary.size();
    if (t_alpha.size() != T || t_beta.size() != T || b_alpha.size() != B || b_beta.size() != B) {
        sp_set_error("composition_air: descriptor out of range or inconsistent with the committed trace");
        return SP_E_INVALID_ARG;
    }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    AirProgramHost ph;
    SP_TRY(build_air_program(st, air, rap.size(), ph));
    const uint32_t b = 1u << logb_, f = air.degree_bound_factor;
    const std::vector<AirPeriodicCol>& pcols = ph.pcols;
    const uint32_t Kp = (uint32_t)pcols.size(), max_ex = ph.max_ex;
    uint64_t deg_bound = 0;   // of H for a constraint-satisfying trace
    for (uint32_t k = 0; k < T; ++k) {
        // deg C_k <= d (n - 1); times x^(n (f - d + 1)); times the exemption product; over x^n - 1
        const uint32_t d = air.degrees[k];
        //   (a strided constraint: times x^(n (f - d) + n/s), over x^(n/s) - g^(o n/s) - the same f n - d + e + 1 coefficients)
        deg_bound = std::max<uint64_t>(deg_bound, (uint64_t)d * (n_ - 1) + n_ * (f - d + 1) + ph.ex_eff[k] - n_ + 1);
    }
    deg_bound = std::max<uint64_t>(deg_bound, (n_ - 1) + n_ * (f - 1));   // boundary terms
    const bool allow_sub = deg_bound <= 2 * n_;                            // deg H < 2n: 2n evaluations fix it
    if (max_ex) {
        SP_TRY(grow(od_.ex_roots, std::max<uint32_t>(max_ex, 64)));
        std::vector<fe> er(max_ex);
        for (uint32_t j = 0; j < max_ex; ++j) er[j] = fe_pow_u64(g_, n_ - 1 - j);
        SP_HIP_CHECK(hipMemcpyAsync(od_.ex_roots.p, er.data(), sizeof(fe) * max_ex, hipMemcpyHostToDevice, c_->stream));
        SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
    }
    // --- boundary constraints grouped by row (first appearance order): one factor (x - g^s) per distinct row
    const StepGroups g = group_by_step(air.boundary);
    const uint32_t nd = (uint32_t)g.steps.size();
    std::vector<uint32_t> gend(nd, 0), at(nd, 0), order(B);   // where group q ends; the constraint at grouped position j'
    for (uint32_t q : g.group) ++gend[q];
    std::partial_sum(gend.begin(), gend.end(), gend.begin());
    for (uint32_t q = 1; q < nd; ++q) at[q] = gend[q - 1];
    for (uint32_t j = 0; j < B; ++j) order[at[g.group[j]]++] = j;
    // --- the device copy: the shared block (build_air_block) and behind it this proof's tables, one upload
    const uint32_t nterm = T + B;
    size_t o_zf, o_coef, o_gpt, o_gend;
    AirCompTables tabs;
    const AirProgram* prog_dev = nullptr;
    SP_TRY(build_air_block(st, air, rap, ph, order,
                           {{sizeof(fe) * b, &o_zf}, {sizeof(fe) * b * nterm, &o_coef}, {sizeof(fe) * nd, &o_gpt}, {sizeof(uint32_t) * nd, &o_gend}}, tabs, prog_dev));
    std::vector<uint8_t>& up = h_air_up_;
    auto dev_at = [&](size_t off) { return od_.air_buf.p + off; };
    fe* hzf = reinterpret_cast<fe*>(up.data() + o_zf);
    fe* hcoef = reinterpret_cast<fe*>(up.data() + o_coef);
    fe* hgpt = reinterpret_cast<fe*>(up.data() + o_gpt);
    std::memcpy(up.data() + o_gend, gend.data(), sizeof(uint32_t) * nd);
    std::vector<fe> points(nd);
    for (uint32_t q = 0; q < nd; ++q) hgpt[q] = points[q] = fe_pow_u64(g_, g.steps[q]);
    std::vector<fe> ga(B), gb(B);                              // the boundary coefficients in grouped order
    for (uint32_t jp = 0; jp < B; ++jp) { ga[jp] = b_alpha[order[jp]]; gb[jp] = b_beta[order[jp]]; }
    coset_tables(fe_pow_u64(h_, n_), logb_, f, air.degrees, t_alpha, t_beta, ga, gb, hcoef, nterm, hzf);
    if (ph.strided()) {
        // a strided constraint's slot of coef holds alpha_k (x^n)^(f - d_k) per coset - U = x^(n/s) and beta_k join it in the kernel
        AirStrideDev* hsd = reinterpret_cast<AirStrideDev*>(up.data() + ph.o_sdev);
        SP_TRY(grow(od_.stride, 3 * ph.stab));
        hsd->u = od_.stride.p; hsd->zinv = od_.stride.p + ph.stab;
        const fe wb = host_primitive_root((int)logb_);
        fe xn = fe_pow_u64(h_, n_);
        for (uint32_t c = 0; c < b; ++c, xn = fe_mul(xn, wb))
            for (uint32_t k = 0; k < T; ++k)
                if (ph.plan.cls[k] >= 0) hcoef[(size_t)c * nterm + k] = fe_mul(t_alpha[k], fe_pow_u64(xn, f - air.degrees[k]));
        for (uint32_t k = 0; k < T; ++k) if (ph.plan.cls[k] >= 0) hsd->beta[k] = t_beta[k];
    }
    SP_HIP_CHECK(hipMemcpyAsync(od_.air_buf.p, up.data(), up.size(), hipMemcpyHostToDevice, c_->stream));
    tabs.h = h_; tabs.ndist = nd;
    tabs.zerofier = reinterpret_cast<const fe*>(dev_at(o_zf));
    tabs.coef = reinterpret_cast<const fe*>(dev_at(o_coef));
    tabs.gpoint = reinterpret_cast<const fe*>(dev_at(o_gpt));
    tabs.gend = reinterpret_cast<const uint32_t*>(dev_at(o_gend));
    if (Kp) {
        // [b S] tables, [S] working copy of the values (the transforms run in place), [S] scratch.  Every rank builds all b cosets:
        // the kernel indexes by the global LDE index.
        const uint64_t S = ph.S;
        SP_TRY(grow(od_.periodic, S * (b + 2)));
        fe* tab = od_.periodic.p;
        fe* work = tab + S * b;
        fe* ws = work + S;
        SP_HIP_CHECK(hipMemcpyAsync(work, tabs.pvals, sizeof(fe) * S, hipMemcpyDeviceToDevice, c_->stream));
        for (uint32_t k = 0; k < Kp;) {   // neighbours of one period in one batch
            uint32_t cnt = 1;
            while (k + cnt < Kp && pcols[k + cnt].logp == pcols[k].logp) ++cnt;
            SP_TRY(air_periodic_tables(c_->stream, *c_->ntt, work + pcols[k].off, ws, tab + pcols[k].off * b, cnt, pcols[k].logp, logn_, logb_, h_));
            k += cnt;
        }
        tabs.ptab = tab;
    }
    if (ph.strided()) {
        // per class [b][s] U and U - g^(o n/s), all b cosets on every rank (the kernel indexes by the global LDE index); one batch
        // inversion over all classes, its zero flag looked at before composition_core takes the flag over
        fe* u = od_.stride.p;
        fe* z = u + ph.stab;
        SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
        for (uint32_t q = 0; q < ph.sdev.n_classes; ++q) {
            SP_TRY(air_stride_class_tables(c_->stream, *c_->ntt, u + ph.sdev.tab_off[q], z + ph.sdev.tab_off[q], ph.sdev.logs[q], ph.sdev.off[q], logn_, logb_, h_));
        }
        SP_TRY(batch_inverse(c_->stream, z, z + ph.stab, ph.stab, c_->d_flag));
        int zero = 0;
        SP_HIP_CHECK(hipMemcpyAsync(&zero, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
        SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
        if (zero) { sp_set_error("composition_air: a stride class's zerofier vanishes on the LDE domain"); return SP_E_ZERO_INVERSE; }
    }
    offsets_ = air.offsets;
    return composition_core(Round2Air{points, nullptr, prog_dev, &tabs, od_.ex_roots.p, allow_sub}, root_out);
}

// validate_trace (reference debug.rs:13-104) for a program AIR, on the device: the program and the descriptor's boundary constraints
// (in the descriptor's order - the report names them by index) go up in one block, the report comes back in one.
int StarkProver::check_trace_air(const AirStatement& st, const AirDescHost& air, const std::vector<fe>& rap, std::vector<AirViolationHost>& out) {
    out.clear();
    if (!segments_committed()) { sp_set_error("check_trace_air: trace segments not committed"); return SP_E_STATE; }
    if (world_ > 1) { sp_set_error("check_trace_air: a report from a sharded context is not supported"); return SP_E_UNSUPPORTED; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    AirProgramHost ph;
    SP_TRY(build_air_program(st, air, rap.size(), ph));
    const uint32_t T = (uint32_t)air.degrees.size(), B = (uint32_t)air.boundary.size();
    std::vector<uint32_t> order(B);
    std::iota(order.begin(), order.end(), 0u);
    AirCompTables tabs;
    const AirProgram* prog_dev = nullptr;
    SP_TRY(build_air_block(st, air, rap, ph, order, {}, tabs, prog_dev));
    SP_HIP_CHECK(hipMemcpyAsync(od_.air_buf.p, h_air_up_.data(), h_air_up_.size(), hipMemcpyHostToDevice, c_->stream));
    // the report block, in 8-byte words: value [4 T] | bcell [4 B] | count [T] | first [T] | last [T] | bbad [B / 2]
    const uint64_t w_value = 0, w_bcell = w_value + 4ull * T, w_count = w_bcell + 4ull * B, w_first = w_count + T, w_last = w_first + T,
                   w_bbad = w_last + T, words = w_bbad + (B + 1) / 2;
    SP_TRY(grow(od_.air_report, words));
    uint64_t* rp = od_.air_report.p;
    SP_HIP_CHECK(hipMemsetAsync(rp, 0, words * sizeof(uint64_t), c_->stream));
    SP_HIP_CHECK(hipMemsetAsync(rp + w_first, 0xFF, (size_t)T * sizeof(uint64_t), c_->stream));
    AirReport rep;
    rep.value = reinterpret_cast<fe*>(rp + w_value);
    rep.bcell = reinterpret_cast<fe*>(rp + w_bcell);
    rep.count = reinterpret_cast<unsigned long long*>(rp + w_count);
    rep.first = reinterpret_cast<unsigned long long*>(rp + w_first);
    rep.last = reinterpret_cast<unsigned long long*>(rp + w_last);
    rep.bbad = reinterpret_cast<uint32_t*>(rp + w_bbad);
    SP_TRY(air_trace_report(c_->stream, d_trace_, n_, tabs, prog_dev, rep));
    h_report_.resize(words * sizeof(uint64_t));
    SP_TRY(readback(h_report_.data(), rp, h_report_.size()));   // (waits for the stream: the upload above is done with h_air_up_)
    const uint64_t* h = reinterpret_cast<const uint64_t*>(h_report_.data());
    auto fe_at = [&](uint64_t word) { fe x; std::memcpy(&x, h + word, sizeof(fe)); return x; };
    for (uint32_t k = 0; k < T; ++k)
        if (h[w_count + k]) out.push_back(AirViolationHost{0u, k, h[w_count + k], h[w_first + k], h[w_last + k], fe_at(w_value + 4ull * k)});
    const uint32_t* bbad = reinterpret_cast<const uint32_t*>(h + w_bbad);
    for (uint32_t j = 0; j < B; ++j)
        if (bbad[j]) out.push_back(AirViolationHost{1u, j, 1, air.boundary[j].step, air.boundary[j].step, fe_at(w_bcell + 4ull * j)});
    return SP_OK;
}

int StarkProver::round2_evaluate(const Round2Air& air, uint64_t count, uint32_t stride_log, const fe* binv, fe* out) {
    if (air.prog) return air_composition(c_->stream, d_lde_, count, Nl_, stride_log, logN_, logb_, air.roots, *air.tabs, air.prog, air.ex_roots, binv, out, logG_, rank_);
    return cairo_composition(c_->stream, d_lde_, count, Nl_, stride_log, logN_, logb_, air.roots, d_comp_consts_, binv, out, logG_, rank_);
}

// boundary inverses of `count` points x_i = hp w^i (roots of 2^logM, shard map sm): Cairo [nd][count] 1 / (x - g^s), a program
// AIR [count] 1 / Z_B(x); scratch: [3 count]
int StarkProver::round2_boundary_inverses(const Round2Air& air, fe* binv, fe* inv_scratch, uint64_t count, uint32_t logM, const fe* roots_m, const fe& hp, ShardMap sm) {
    const uint32_t nd = (uint32_t)air.points.size();
    if (!nd) return SP_OK;
    if (air.prog) {
        SP_TRY(boundary_vanishing(c_->stream, binv, count, logM, roots_m, hp, air.tabs->gpoint, nd, sm));
        return batch_inverse(c_->stream, binv, inv_scratch, count, c_->d_flag);
    }
    SP_TRY(coset_minus_points(c_->stream, binv, count, logM, roots_m, hp, air.points.data(), nd, sm));
    return batch_inverse(c_->stream, binv, inv_scratch, (uint64_t)nd * count, c_->d_flag);
}

// interpolate_offset_fft + even/odd split in one inverse transform of the 2n evaluations H(hp w_2n^i) in d_h12s_: position q < n of
// the bit-reversed output is 2n c_j hp^j for j = 2k, position n + q for j = 2k + 1 (k = rev_n(q)); the post factors leave
// a_k h^k = c_2k h^k and b_k h^k = c_(2k+1) h^k:  (2n)^-1 (h^-1 u^2)^k  and  (2n)^-1 (h^-1 u) (h^-1 u^2)^k,  u = w_N^-c0
// (tables: setup()).  Then the LDE of H1 and H2.
int StarkProver::split_2n_and_extend(const fe* post) {
    SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(d_h12s_, (int)logn_ + 1, 1, 2 * n_, post));
    h_full_ = false;
    return c_->ntt->lde_coset_major(d_h12s_, d_h12_, (int)logn_, (int)logb_, 2, n_, Nl_, (int)logG_, (int)rank_);
}

// Sub-coset path: this rank holds both cosets c0 = rank and c0 + b/2 (always on one GPU).  The 2n points are x_i = hp w_2n^i with
// hp = h w_N^c0: under coset sharding every rank works on its own pair of cosets and obtains the same polynomial, so the composition
// evaluations need no all-gather.  *flag, *flag_pref: where the zero-denominator flags land (read by the caller behind the commitment).
int StarkProver::composition_sub_coset(const Round2Air& air, int* flag, int* flag_pref) {
    const uint64_t M = 2 * n_;
    const uint32_t nd = (uint32_t)air.points.size();
    const fe* roots_m = nullptr;
    SP_TRY(c_->ntt->roots((int)logn_ + 1, &roots_m));
    const fe* binv = d_scratch_;              // [ndist][2n], scratch [3 * 2n] behind it
    bool pref = nd && !air.prog && bpre_valid_ && nd == bpre_points_.size();
    for (uint32_t j = 0; pref && j < nd; ++j) pref = fe_eq(air.points[j], bpre_points_[j]);
    if (pref) {                               // computed beside round 1 (prefetch_boundary_inverses)
        binv = od_.bpre.p;
        SP_HIP_CHECK(hipStreamWaitEvent(c_->stream, ev_side_bnd_, 0));
        SP_HIP_CHECK(hipMemcpyAsync(flag_pref, side_flag(SIDE_BND_INV), sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    } else {
        SP_TRY(round2_boundary_inverses(air, d_scratch_, d_scratch_ + 3 * M, M, logn_ + 1, roots_m, rank_coset_offset(), ShardMap{0, 0, 0}));
    }
    SP_TRY(round2_evaluate(air, M, logb_ - logG_ - 1, binv, d_h12s_));   // [2n] evaluations H(hp w_2n^i), then [H1s | H2s]
    SP_HIP_CHECK(hipMemcpyAsync(flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    return split_2n_and_extend(d_post_comp_);
}

// Pair path, one coset per rank (G = b): the 2n points of the cosets 0 and b/2 live on two ranks - every rank evaluates its own
// coset, the evaluations are all-gathered and the pair (0, b/2) is interpolated everywhere.
int StarkProver::composition_pair(const Round2Air& air, int* flag) {
    SP_TRY(round2_boundary_inverses(air, d_scratch_, d_scratch_ + 3 * Nl_, Nl_, logN_, air.roots, h_, shard_map()));
    SP_TRY(round2_evaluate(air, Nl_, 0, d_scratch_, d_local_));      // H on this rank's coset
    SP_HIP_CHECK(hipMemcpyAsync(flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    SP_TRY(ensure_gather((uint64_t)world_ * Nl_));
    SP_TRY(all_gather(d_local_, od_.gather.p, Nl_ * sizeof(fe), true));
    const uint32_t other = G_ >> 1;                                  // the rank that holds coset b/2
    if (other != 1) SP_HIP_CHECK(hipMemcpyAsync(od_.gather.p + n_, od_.gather.p + (uint64_t)other * n_, n_ * sizeof(fe), hipMemcpyDeviceToDevice, c_->stream));
    SP_TRY(interleave_shards(c_->stream, od_.gather.p, d_h12s_, n_, ShardMap{1, 1, 0}));   // H(h w_2n^i): even i from coset 0, odd i from coset b/2
    return split_2n_and_extend(d_post_comp0_);                       // post factors of c0 = 0
}

// Whole-domain path: every rank evaluates H on the cosets it holds, the evaluations are all-gathered, and the coefficients decide
// between the H1 / H2 of a trace that satisfies its constraints (h_full_ = false) and the general split.
int StarkProver::composition_whole_domain(const Round2Air& air) {
    fe* comp = nullptr;                       // [N] whole-domain composition evaluations
    SP_TRY(full_domain_buffer(&comp));
    fe* comp_local = G_ == 1 ? comp : d_local_;
    SP_TRY(round2_boundary_inverses(air, d_scratch_, d_scratch_ + 3 * Nl_, Nl_, logN_, air.roots, h_, shard_map()));
    SP_TRY(round2_evaluate(air, Nl_, 0, d_scratch_, comp_local));
    if (G_ > 1) {  // composition-polynomial reduction: all-gather the per-coset evaluations
        SP_TRY(ensure_gather((uint64_t)world_ * Nl_));
        SP_TRY(all_gather(comp_local, od_.gather.p, Nl_ * sizeof(fe), true));
        SP_TRY(interleave_shards(c_->stream, od_.gather.p, comp, n_, shard_map()));
    }
    // --- interpolate_offset_fft + even/odd split (reference evaluation_table.rs:27-33, prover.rs:250-252)
    SP_TRY(c_->ntt->dif_natural_to_bitrev_inverse(comp, (int)logN_, 1, N_, nullptr));
    int flag = 0;
    SP_HIP_CHECK(hipMemcpyAsync(&flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
    if (flag) { sp_set_error("composition: zero boundary denominator"); return SP_E_ZERO_INVERSE; }
    SP_TRY(high_coeff_check(c_->stream, comp, N_, logb_, c_->d_flag));
    SP_HIP_CHECK(hipMemcpyAsync(&flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));
    h_full_ = flag != 0;
    if (!h_full_) {
        SP_TRY(split_composition(c_->stream, comp, n_, logb_, d_t2_, hinv_, d_h12s_, d_h12s_ + n_));
        return c_->ntt->lde_coset_major(d_h12s_, d_h12_, (int)logn_, (int)logb_, 2, n_, Nl_, (int)logG_, (int)rank_);
    }
    // the trace violates its constraints: deg H >= 2n and the reference still proves it (longer H1, H2).  Every rank
    // holds all of H, evaluates H1, H2 on the whole domain and keeps the points of its own cosets.
    SP_TRY(grow(od_.hfull, N_));
    fe* t_half = d_scratch_;  // N/2 entries: N^-1 h^(-rev_{N/2}(q))
    if ((N_ >> 1) > scratch_elems()) { sp_set_error("composition: scratch too small"); return SP_E_ALLOC; }
    SP_TRY(gen_power_table(c_->stream, t_half, N_ >> 1, logN_ - 1, hinv_, fe_inv(fe_from_u64(N_))));
    SP_TRY(split_composition_full(c_->stream, comp, N_, t_half, hinv_, od_.hfull.p, od_.hfull.p + (N_ >> 1)));
    // H1, H2 of N/2 coefficients each: natural-order evaluations first, then into the coset-major order of every other column
    SP_TRY(grow(od_.hnat, 2 * N_));
    SP_TRY(c_->ntt->lde_from_bitrev(od_.hfull.p, od_.hnat.p, (int)logN_ - 1, 1, 2, N_ >> 1, N_));
    return natural_to_coset_major(c_->stream, od_.hnat.p, N_, d_h12_, Nl_, 2, lde_order(), logG_, rank_);
}

// Shared second half of round 2.  A trace that satisfies its constraints gives deg H < 2n, and then 2n evaluations fix H.  Decide
// that EXACTLY by checking the constraints on the trace itself (n rows, no divisions): clean -> evaluate the composition on the 2n
// points of the cosets 0 and b/2 only (sub-coset or pair path); otherwise (the reference still proves such traces, with longer
// H1/H2) fall back to the whole domain and the general split, so the bytes are identical for every input.
int StarkProver::composition_core(Round2Air air, uint8_t root_out[32]) {
    SP_TRY(c_->ntt->roots((int)logN_, &air.roots));
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const bool cairo = !air.prog;
    const bool prechecked = check_pending_ && cairo;   // composition_precheck queued the constraint check (and cleared the flag) already
    check_pending_ = false;
    if (cairo) SP_HIP_CHECK(hipMemcpyAsync(d_comp_consts_, air.K, composition_consts_bytes(1u << logb_), hipMemcpyHostToDevice, c_->stream));
    if (!prechecked) SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    int flag = 0, flag_pref = 0;   // of the 2n-point paths: looked at behind the commitment's read-back, which waits for the stream - no wait of their own
    bool sub_coset = air.allow_sub_coset && sub_coset_shape(), pair_path = air.allow_sub_coset && pair_shape();
    if (sub_coset || pair_path) {
        if (!cairo) SP_TRY(air_trace_check(c_->stream, d_trace_, n_, *air.tabs, air.prog, c_->d_flag));
        else if (!prechecked) SP_TRY(cairo_trace_check(c_->stream, d_trace_, n_, d_comp_consts_, c_->d_flag, check_row0(), check_rows()));
        if (cairo && world_ > 1 && n_ >= 256ull * world_) {
            // every rank checked its own n / world rows of the (replicated) trace: one flag per rank, combined everywhere
            SP_TRY(grow(od_.flags_all, world_));
            SP_TRY(all_gather(c_->d_flag, od_.flags_all.p, sizeof(int), true));
            std::vector<int> flags(world_, 0);
            SP_HIP_CHECK(hipMemcpyAsync(flags.data(), od_.flags_all.p, sizeof(int) * world_, hipMemcpyDeviceToHost, c_->stream));
            SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));  // (also: K is a stack object)
            for (int f : flags) flag |= f;
        } else {
            SP_HIP_CHECK(hipMemcpyAsync(&flag, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
            SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));  // (also: K is a stack object)
        }
        sub_coset = sub_coset && flag == 0;
        pair_path = pair_path && flag == 0;
        SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    } else {
        SP_HIP_CHECK(sp_stream_wait_polling(c_->stream));  // K is a stack object
    }
    if (sub_coset) SP_TRY(composition_sub_coset(air, &flag, &flag_pref));
    else if (pair_path) SP_TRY(composition_pair(air, &flag));
    else SP_TRY(composition_whole_domain(air));
    bpre_valid_ = false;
    c_->proof_info[0] = (sub_coset || pair_path) ? 1u : (h_full_ ? 3u : 2u);
    c_->proof_info[1] = fri_rep_; c_->proof_info[2] = G_; c_->proof_info[3] = (G_ > 1 && shard_interp_) ? 1u : 0u;
    SP_TRY(commit_columns(d_h12_, Nl_, 2, tree_comp_, root_out));
    if ((sub_coset || pair_path) && (flag | flag_pref)) { sp_set_error("composition: zero boundary denominator"); return SP_E_ZERO_INVERSE; }
    stage_ = Stage::Composed;
    return SP_OK;
}

}  // namespace sp
