// Stand-alone check of the statement decoder (csrc/air_desc.cpp) for sanitizer builds: malformed and well-formed C structs of every
// part through sp::air_statement_from_c, each with the verdict it must get, and the host model on what was accepted.  No GPU, no
// library: build and run on the CPU, from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//     tools/air_statement_check.cpp lambdaworks_cairo_prover_amd/csrc/air_desc.cpp lambdaworks_cairo_prover_amd/csrc/cairo_air_host.cpp \
//     lambdaworks_cairo_prover_amd/csrc/cairo_host.cpp -o /tmp/air_statement_check && /tmp/air_statement_check
#include "../lambdaworks_cairo_prover_amd/csrc/air_desc.h"
#include <cstdio>
#include <cstring>
#include <functional>

namespace {
int failures = 0;
struct Felt { uint8_t b[32]; };
Felt felt(uint64_t v) { Felt f{}; for (int i = 0; i < 8; ++i) f.b[31 - i] = (uint8_t)(v >> (8 * i)); return f; }

// x' = x + K on one main column, one auxiliary column (a running product of gamma - x, over gamma - x), x_0 = 3 and z_0 from the
// challenge; every part in its well-formed form, for a trace of 16 rows
struct Parts {
    sp_air_op ops[5] = {{0, 0, 1, 0, 0}, {0, 0, 0, 0, 0}, {6, 0, 0, 0, 0}, {2, 0, 1, 2, 0}, {5, 0, 0, 3, 0}};   // (LOAD next, LOAD cur, PERIODIC, ADD - never run here)
    sp_air_boundary boundary[2] = {};
    sp_air_desc d{};
    sp_air_op aux_ops[4] = {{1, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {3, 0, 0, 1, 0}, {6, 0, 7, 0, 0}};   // gamma, x, gamma - x, table read at shift 7
    sp_air_aux_column aux_cols[1] = {{SP_AIR_AUX_PRODUCT, 2, 2, 0}};
    sp_air_aux_desc aux{};
    // sorted(): x sorted by itself (16 key bits) with gamma - x carried, and a product that reads the sorted x one row ahead
    sp_air_op sort_ops[6] = {{1, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, {3, 0, 0, 1, 0}, {0, 0, 1, 1, 0}, {3, 0, 0, 3, 0}, {6, 0, 7, 0, 0}};
    sp_air_aux_column sort_cols[3] = {{SP_AIR_AUX_SORTED, 1, 1, 16}, {SP_AIR_AUX_SORTED, 2, 1, 16}, {SP_AIR_AUX_PRODUCT, 2, 4, 0}};
    sp_air_op many_ops[17] = {};                 // 17 LOADs of x, each the key of a group of its own
    sp_air_aux_column many_cols[17];
    Felt keys[8];
    sp_air_periodic_column pcols[65];
    sp_air_periodic_desc per{};
    sp_air_stride strides[2] = {{4, 1}, {1, 0}};
    sp_air_stride_desc sd{};
    Felt bconsts[1] = {felt(77)};
    sp_air_op bops[3] = {{1, 0, 1, 0, 0}, {1, 0, 0, 0, 0}, {3, 0, 0, 1, 0}};   // gamma, 77, gamma - 77
    sp_air_boundary_value bvalues[2] = {{1, 2, 2, 0}, {0, 2, SP_AIR_AUX_NO_DEN, 0}};
    sp_air_boundary_desc bv{};
    // a main program (use 'm'): x the one input; inv = INV_OR_ZERO(x), f = (1 - x inv) / 1, bit 3 of x, the running sum of f, a product of x over x
    Felt mconsts[1] = {felt(1)};
    sp_air_op mops[7] = {{0, 0, 0, 0, 0}, {0, 0, 0, 1, 0}, {4, 0, 0, 1, 0}, {1, 0, 0, 0, 0}, {3, 0, 3, 2, 0}, {0, 0, 7, 2, 0}, {0, 0, 0, 0, 0}};
    sp_air_main_column mcols[5] = {{SP_AIR_MAIN_INV_OR_ZERO, 0, SP_AIR_AUX_NO_DEN, 0}, {SP_AIR_MAIN_VALUE, 4, 3, 0}, {SP_AIR_MAIN_BIT, 0, SP_AIR_AUX_NO_DEN, 3},
                                   {SP_AIR_MAIN_SUM, 5, SP_AIR_AUX_NO_DEN, 0}, {SP_AIR_MAIN_PRODUCT, 0, 6, 0}};
    sp_air_main_desc mp{};
    // a main program with a chain group (use 'r': through the _rec policy, 'R': without it): x the one input; a group of two in blocks of
    // four rows, seeds x and K (op 6), steps x0 x1 and x0 + K; then x0 one row ahead as a VALUE
    // (ops 7 and 8, beyond n_ops until a case of the _div policy - use 'd' - asks for them: x / K, and a sum behind that quotient)
    sp_air_op rops[9] = {{0, 0, 0, 0, 0}, {6, 0, 0, 0, 0}, {0, 0, 0, 1, 0}, {0, 0, 0, 2, 0}, {4, 0, 2, 3, 0}, {2, 0, 2, 1, 0}, {0, 0, 1, 1, 0}, {7, 0, 0, 1, 0}, {2, 0, 7, 7, 0}};
    sp_air_main_column rcols[3] = {{SP_AIR_MAIN_CHAIN, 4, 0, 2}, {SP_AIR_MAIN_CHAIN, 5, 1, 2 + 256}, {SP_AIR_MAIN_VALUE, 6, SP_AIR_AUX_NO_DEN, 0}};
    sp_air_main_desc rp{};
    // a main program with a lookup multiplicity (use 'l': through the _lk policy, 'L': through the _rec policy alone): x the one input;
    // v = x + K (VALUE, op 6), m = COUNT of X = v in T = K with 16 key bits, the running sum of m one row ahead; and one of 17 COUNT columns
    // (ops 5 and 6, beyond n_ops until a case of the _multi policy - use 'j' - asks for them: the list cells of X = v and of X = x, v;
    // ops 7 .. 22 are there for a case to fill)
    sp_air_op lops[23] = {{0, 0, 0, 0, 0}, {6, 0, 0, 0, 0}, {2, 0, 0, 1, 0}, {0, 0, 0, 1, 0}, {0, 0, 1, 2, 0}, {12, 0, 3, 0xFFFF, 0}, {12, 0, 0, 5, 0}};
    sp_air_main_column lcols[3] = {{SP_AIR_MAIN_VALUE, 2, SP_AIR_AUX_NO_DEN, 0}, {SP_AIR_MAIN_COUNT, 3, 1, 16}, {SP_AIR_MAIN_SUM, 4, SP_AIR_AUX_NO_DEN, 0}};
    sp_air_main_column many_lcols[17];
    sp_air_main_desc lp{};
    Parts() {
        for (auto& c : many_lcols) c = sp_air_main_column{SP_AIR_MAIN_COUNT, 0, 1, 64};
        lp.size = sizeof(sp_air_main_desc); lp.input_cols = 1; lp.n_ops = 5; lp.ops = lops; lp.n_consts = 1; lp.consts = mconsts[0].b; lp.n_cols = 3; lp.cols = lcols;
        for (uint32_t j = 0; j < 17; ++j) many_cols[j] = sp_air_aux_column{SP_AIR_AUX_SORTED, j, j, 16};
        for (int j = 0; j < 8; ++j) keys[j] = felt(100 + j);
        for (auto& c : pcols) c = sp_air_periodic_column{8, 0, keys[0].b};
        boundary[0].col = 0; boundary[1].col = 1;
        d.main_cols = 1; d.aux_cols = 1; d.n_offsets = 2; d.offsets[1] = 1; d.n_transitions = 1; d.degrees[0] = 1; d.exemptions[0] = 1;
        d.num_transition_exemptions = 1; d.degree_bound_factor = 2; d.n_ops = 5; d.ops = ops; d.n_rap = 1; d.aux_kind = SP_AIR_AUX_PROGRAM;
        d.n_boundary = 2; d.boundary = boundary;
        aux.n_ops = 3; aux.ops = aux_ops; aux.n_cols = 1; aux.cols = aux_cols;
        per.n_cols = 1; per.cols = pcols;
        sd.n = 1; sd.strides = strides;
        bv.n_ops = 3; bv.ops = bops; bv.n_consts = 1; bv.consts = bconsts[0].b; bv.n_values = 2; bv.values = bvalues;
        mp.size = sizeof(sp_air_main_desc); mp.input_cols = 1; mp.n_ops = 7; mp.ops = mops; mp.n_consts = 1; mp.consts = mconsts[0].b; mp.n_cols = 5; mp.cols = mcols;
        rp.size = sizeof(sp_air_main_desc); rp.input_cols = 1; rp.n_ops = 7; rp.ops = rops; rp.n_consts = 1; rp.consts = mconsts[0].b; rp.n_cols = 3; rp.cols = rcols;
    }
    void with_chain() { d.main_cols = 4; }
    void many_counts(uint32_t count) { d.main_cols = 1 + count; lp.n_ops = 2; lp.n_cols = count; lp.cols = many_lcols; }
    void with_main() { d.main_cols = 6; }
    void sorted() { d.aux_cols = 3; aux.n_ops = 5; aux.ops = sort_ops; aux.n_cols = 3; aux.cols = sort_cols; }
    void many(uint32_t groups) { d.aux_cols = groups; aux.n_ops = 17; aux.ops = many_ops; aux.n_cols = groups; aux.cols = many_cols; }
};

// use: which parts go to the decoder (x p s b m r R l L, upper case P: the auxiliary program may read the periodic columns; m: the main
// program, for which the AIR gets its six main columns first; r / R the chain program with and without the _rec policy; l / L the
// lookup program under the _lk policy and under the _rec policy alone; k the chain program under the _link policy; d the chain program
// under the _div policy, i under the _int policy, j the lookup program under the _multi policy)
void run(const char* label, const char* use, bool want_ok, const std::function<void(Parts&)>& patch) {
    Parts p;
    if (std::strchr(use, 'm')) p.with_main();
    if (std::strchr(use, 'r') || std::strchr(use, 'R') || std::strchr(use, 'l') || std::strchr(use, 'L') || std::strchr(use, 'k') || std::strchr(use, 'd') || std::strchr(use, 'i') || std::strchr(use, 'j')) p.with_chain();
    patch(p);
    auto has = [&](char c) { return std::strchr(use, c) != nullptr; };
    using sp::AirMainLevel;   // the highest level a use-letter implies wins
    const AirMainLevel level = has('j') ? AirMainLevel::Multi : has('i') ? AirMainLevel::Int : has('d') ? AirMainLevel::Div : has('k') ? AirMainLevel::Link : has('l') ? AirMainLevel::Lk : has('r') || has('L') ? AirMainLevel::Rec : AirMainLevel::Main;
    sp::AirStatement st;
    const std::string refused = sp::air_statement_from_c(&p.d, has('x') ? &p.aux : nullptr, has('p') ? &p.per : nullptr, has('s') ? &p.sd : nullptr,
                                                         has('b') ? &p.bv : nullptr, has('P'), 16, st,
                                                         has('m') ? &p.mp : has('r') || has('R') || has('k') || has('d') || has('i') ? &p.rp : has('l') || has('L') || has('j') ? &p.lp : nullptr,
                                                         level);
    const bool ok = refused.empty();
    if (ok != want_ok) { ++failures; std::printf("FAIL %-44s wanted %s, got %s\n", label, want_ok ? "accepted" : "refused", ok ? "accepted" : refused.c_str()); return; }
    std::printf("ok   %-44s %s\n", label, ok ? "accepted" : refused.substr(0, 60).c_str());
    if (!ok) return;
    // the model on what was accepted: stride plan and zerofier, periodic columns as polynomials, boundary values under a challenge
    sp::AirStridePlan plan;
    bool fine = sp::air_stride_plan(st.air, 16, plan) && st.aux.has_value() == has('x') && st.periodic.has_value() == has('p') && st.bvals.has_value() == has('b') &&
                (st.aux_periodic() != nullptr) == (has('P') && has('p')) && st.main.has_value() == (has('m') || has('r') || has('l') || has('k') || has('d') || has('i') || has('j')) &&
                st.main_level == (has('j') ? AirMainLevel::Multi : has('i') ? AirMainLevel::Int : has('d') ? AirMainLevel::Div : has('k') ? AirMainLevel::Link : has('l') ? AirMainLevel::Lk : has('r') ? AirMainLevel::Rec : AirMainLevel::Main) && !st.unsupported;
    if (st.main && has('l') && !has('r') && st.main->cols.size() == 3) {   // what the prover's chunking reads of a COUNT column
        const auto& c = st.main->cols;
        fine = fine && c[1].kind == SP_AIR_MAIN_COUNT && c[1].key_bits == p.lcols[1].pad && c[1].num_op == 3 && c[1].den_op == 1 && c[1].reads == 1 && c[0].key_bits == 0 &&
               c[2].key_bits == 0 && c[2].reads == 2;
    }
    if (st.main && has('j') && !has('i') && st.main->cols.size() == 3) {   // what the prover's chunking reads of a joint COUNT column: the list's length, the key bits apart
        const auto& c = st.main->cols;
        const bool joint = (p.lcols[1].pad & 256u) != 0;
        uint32_t cells = 0;
        for (uint32_t t = joint ? p.lcols[1].num_op : 0xFFFFu; t != 0xFFFFu; t = p.lops[t].b) ++cells;
        fine = fine && c[1].kind == SP_AIR_MAIN_COUNT && c[1].key_bits == (p.lcols[1].pad & 255u) && c[1].list_len == cells && c[1].num_op == p.lcols[1].num_op &&
               c[1].den_op == 1 && c[1].reads == 1 && c[0].list_len == 0 && c[2].list_len == 0 && st.main->ops.size() == p.lp.n_ops;
    }
    if (st.main && has('d')) {   // what the prover's chunking reads behind a quotient: the ops as they came, reads through op 7
        const auto& c = st.main->cols;
        fine = fine && c.size() == 3 && st.main->ops.size() == p.rp.n_ops && c[0].kind == SP_AIR_MAIN_CHAIN && c[2].reads == 1;
        for (uint32_t t = 0; t < p.rp.n_ops; ++t) fine = fine && st.main->ops[t].op == p.rops[t].op;
    }
    if (st.main && has('k')) {   // what the prover's chunking reads of a linked group: l, j and k apart
        const auto& c = st.main->cols;
        fine = fine && c.size() == 3 && c[0].chain_log == (p.rcols[0].pad & 255u) && c[0].chain_link == (p.rcols[0].pad >> 16) && c[0].chain_pos == 0 &&
               c[1].chain_pos == 1 && c[1].chain_link == c[0].chain_link && c[2].chain_link == 0;
    }
    if (st.main && has('r')) {   // what the prover's chunking reads of a chain group
        const auto& c = st.main->cols;
        fine = fine && c.size() == 3 && c[0].chain_link == 0 && c[0].kind == SP_AIR_MAIN_CHAIN && c[0].chain_log == (p.rcols[0].pad & 255u) && c[0].chain_pos == 0 && c[1].chain_log == c[0].chain_log && c[1].chain_pos == 1 &&
               c[2].chain_log == 0 && c[2].reads == 1;
    }
    if (st.main && has('m')) {   // what the prover's chunking reads: which derived columns each column needs, and the bit
        const auto& c = st.main->cols;
        fine = fine && c.size() == 5 && c[0].reads == 0 && c[1].reads == 1 && c[2].reads == 0 && c[2].bit == p.mcols[2].pad && c[3].reads == 2 && c[4].reads == 0 &&
               st.main->input_cols == 1 && st.main->ops.size() == 7 && st.main->consts.size() == 1;
    }
    const fe x = fe_from_u64(5);
    for (const sp::AirStrideHost& c : plan.classes) { fe Z, E; sp::air_stride_eval(c.period, c.offset, 1, 16, x, Z, E); fine = fine && !fe_is_zero(Z); }
    if (st.periodic)
        for (const auto& col : st.periodic->cols) {   // P(g^i) = values[i mod period]
            const fe at = sp::air_periodic_eval(sp::air_periodic_interpolate(col), 16, fe_pow_u64(sp::air_root_of_unity(4), 11));
            fine = fine && fe_eq(fe_reduce_once(at), fe_reduce_once(col[11 % col.size()]));
        }
    if (st.bvals) {
        std::vector<sp::BoundaryConstraint> bcs = st.air.boundary;
        fine = fine && sp::air_resolve_boundary_into(*st.bvals, {fe_from_u64(80)}, bcs) && fe_eq(fe_reduce_once(bcs[1].value), fe_one()) &&
               fe_eq(fe_reduce_once(bcs[0].value), fe_from_u64(3)) && !sp::air_resolve_boundary_into(*st.bvals, {fe_from_u64(77)}, bcs);
    }
    if (!fine) { ++failures; std::printf("FAIL %-44s the host model disagrees\n", label); }
}
}  // namespace

int main() {
    const auto none = [](Parts&) {};
    // ---- well-formed, one of each kind
    run("plain", "", true, [](Parts& p) { p.ops[2] = sp_air_op{1, 0, 0, 0, 0}; });
    run("auxiliary program", "x", true, none);
    run("periodic columns", "p", true, none);
    run("periodic columns beside an auxiliary program", "xp", true, none);
    run("64 periodic columns", "p", true, [](Parts& p) { p.per.n_cols = 64; });
    run("strides", "ps", true, none);
    run("boundary values", "xb", true, none);
    run("auxiliary program reading a table (_pub)", "xpP", true, [](Parts& p) { p.aux.n_ops = 4; });
    run("everything", "xpsbP", true, [](Parts& p) { p.aux.n_ops = 4; });
    run("sorted columns and a product that reads one", "x", true, [](Parts& p) { p.sorted(); });
    run("sorted: pad 0 is 64 bits", "x", true, [](Parts& p) { p.sorted(); p.sort_cols[0].pad = p.sort_cols[1].pad = 0; });
    run("sorted: 64 key bits", "x", true, [](Parts& p) { p.sorted(); p.sort_cols[0].pad = 64; p.sort_cols[1].pad = 0; });
    run("sorted: a carried value reads a table (_pub)", "xpP", true, [](Parts& p) { p.sorted(); p.aux.n_ops = 6; p.sort_cols[1].num_op = 5; });
    run("sorted: 16 groups", "x", true, [](Parts& p) { p.many(16); });
    run("pad is ignored for products and sums", "x", true, [](Parts& p) { p.aux_cols[0].pad = 65; });
    // ---- malformed sorted columns
    run("sorted: kind 3", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].kind = 3; });
    run("sorted: no key op", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].den_op = SP_AIR_AUX_NO_DEN; });
    run("sorted: key op beyond the program", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].den_op = 5; });
    run("sorted: pad 65", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[0].pad = p.sort_cols[1].pad = 65; });
    run("sorted: a group that disagrees on the key bits", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].pad = 8; });
    run("sorted: LOAD of a product column", "x", false, [](Parts& p) { p.sorted(); p.sort_ops[3].b = 3; });
    run("sorted: LOAD beyond main + aux", "x", false, [](Parts& p) { p.sorted(); p.sort_ops[3].b = 4; });
    run("sorted: a key that reads a sorted column", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].den_op = 4; });
    run("sorted: a value that reads a sorted column", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[1].num_op = 4; });
    run("sorted: 17 groups", "x", false, [](Parts& p) { p.many(17); });
    run("LOAD of an auxiliary column without sorted columns", "x", false, [](Parts& p) { p.sorted(); p.sort_cols[0].kind = p.sort_cols[1].kind = SP_AIR_AUX_SUM; });
    // ---- malformed: the table of tests/test_air_statement.py
    run("n_offsets = 9", "xp", false, [](Parts& p) { p.d.n_offsets = 9; });
    run("a count without its array", "", false, [](Parts& p) { p.d.ops = nullptr; });
    run("period no power of two", "p", false, [](Parts& p) { p.pcols[0].period = 6; });
    run("period longer than the trace", "p", false, [](Parts& p) { p.pcols[0].period = 32; });
    run("period 2^31", "p", false, [](Parts& p) { p.pcols[0].period = 1u << 31; });
    run("65 periodic columns", "p", false, [](Parts& p) { p.per.n_cols = 65; });
    run("null values", "p", false, [](Parts& p) { p.pcols[0].values = nullptr; });
    run("strides: not one per transition", "ps", false, [](Parts& p) { p.sd.n = 2; });
    run("strides: offset >= period", "ps", false, [](Parts& p) { p.strides[0].offset = 4; });
    run("strides: null", "ps", false, [](Parts& p) { p.sd.strides = nullptr; });
    run("aux: op 6 outside _pub", "xp", false, [](Parts& p) { p.aux.n_ops = 4; });
    run("aux: op 6 beyond the columns", "xpP", false, [](Parts& p) { p.aux.n_ops = 4; p.aux_ops[3].b = 1; });
    run("aux: n_cols != aux_cols", "x", false, [](Parts& p) { p.aux.n_cols = 2; });
    run("aux: aux_kind is not a program", "x", false, [](Parts& p) { p.d.aux_kind = 1; });
    run("aux: no ops", "x", false, [](Parts& p) { p.aux.n_ops = 0; });
    run("aux: 65536 ops", "x", false, [](Parts& p) { p.aux.n_ops = 65536; });
    run("aux: operand is a later op", "x", false, [](Parts& p) { p.aux_ops[2].b = 3; });
    run("aux: column names an op beyond the program", "x", false, [](Parts& p) { p.aux_cols[0].den_op = 3; });
    run("bvals: null ops", "xb", false, [](Parts& p) { p.bv.ops = nullptr; });
    run("bvals: null consts", "xb", false, [](Parts& p) { p.bv.consts = nullptr; });
    run("bvals: null values", "xb", false, [](Parts& p) { p.bv.values = nullptr; });
    run("bvals: no ops", "xb", false, [](Parts& p) { p.bv.n_ops = 0; });
    run("bvals: 2^32 - 1 ops", "xb", false, [](Parts& p) { p.bv.n_ops = 0xFFFFFFFFu; });
    run("bvals: LOAD", "xb", false, [](Parts& p) { p.bops[0].op = 0; });
    run("bvals: OUT", "xb", false, [](Parts& p) { p.bops[2].op = 5; });
    run("bvals: PERIODIC", "xb", false, [](Parts& p) { p.bops[0].op = 6; });
    run("bvals: op 7", "xb", false, [](Parts& p) { p.bops[2].op = 7; });
    run("bvals: operand is itself", "xb", false, [](Parts& p) { p.bops[2].a = 2; });
    run("bvals: operand is later", "xb", false, [](Parts& p) { p.bops[2].b = 3; });
    run("bvals: constant beyond consts + rap", "xb", false, [](Parts& p) { p.bops[1].a = 2; });
    run("bvals: num_op beyond the program", "xb", false, [](Parts& p) { p.bvalues[0].num_op = 3; });
    run("bvals: den_op beyond the program", "xb", false, [](Parts& p) { p.bvalues[0].den_op = 3; });
    run("bvals: boundary >= n_boundary", "xb", false, [](Parts& p) { p.bvalues[0].boundary = 2; });
    run("bvals: a boundary named twice", "xb", false, [](Parts& p) { p.bvalues[1].boundary = 1; });
    // ---- main programs
    run("main program", "m", true, none);
    run("main program beside everything", "xpsbPm", true, [](Parts& p) { p.aux.n_ops = 4; });
    run("main program: inputs on the device", "m", true, [](Parts& p) { p.mp.input_location = 1; });
    run("main program: bit 251", "m", true, [](Parts& p) { p.mcols[2].pad = 251; });
    run("main: size", "m", false, [](Parts& p) { p.mp.size -= 4; });
    run("main: null ops", "m", false, [](Parts& p) { p.mp.ops = nullptr; });
    run("main: null consts", "m", false, [](Parts& p) { p.mp.consts = nullptr; });
    run("main: null cols", "m", false, [](Parts& p) { p.mp.cols = nullptr; });
    run("main: no input column", "m", false, [](Parts& p) { p.mp.input_cols = 0; p.mp.n_cols = 6; });
    run("main: columns do not add up", "m", false, [](Parts& p) { p.mp.n_cols = 4; });
    run("main: input_cols 2^32 - 1", "m", false, [](Parts& p) { p.mp.input_cols = 0xFFFFFFFFu; p.mp.n_cols = 7; });
    run("main: input_location 2", "m", false, [](Parts& p) { p.mp.input_location = 2; });
    run("main: no ops", "m", false, [](Parts& p) { p.mp.n_ops = 0; });
    run("main: 2^32 - 1 ops", "m", false, [](Parts& p) { p.mp.n_ops = 0xFFFFFFFFu; });
    run("main: 4097 constants", "m", false, [](Parts& p) { p.mp.n_consts = 4097; });
    run("main: unknown kind", "m", false, [](Parts& p) { p.mcols[1].kind = 5; });
    run("main: bit 252", "m", false, [](Parts& p) { p.mcols[2].pad = 252; });
    run("main: a denominator on INV_OR_ZERO", "m", false, [](Parts& p) { p.mcols[0].den_op = 3; });
    run("main: a denominator on BIT", "m", false, [](Parts& p) { p.mcols[2].den_op = 3; });
    run("main: OUT", "m", false, [](Parts& p) { p.mops[4].op = 5; });
    run("main: PERIODIC", "m", false, [](Parts& p) { p.mops[1].op = 6; });
    run("main: op 7", "m", false, [](Parts& p) { p.mops[4].op = 7; });
    run("main: operand is itself", "m", false, [](Parts& p) { p.mops[2].a = 2; });
    run("main: operand is later", "m", false, [](Parts& p) { p.mops[2].b = 6; });
    run("main: shift 8", "m", false, [](Parts& p) { p.mops[5].a = 8; });
    run("main: LOAD beyond the main columns", "m", false, [](Parts& p) { p.mops[5].b = 6; });
    run("main: constant beyond consts", "m", false, [](Parts& p) { p.mops[3].a = 1; });
    run("main: a column loads itself", "m", false, [](Parts& p) { p.mops[0].b = 1; });
    run("main: a column loads a later one", "m", false, [](Parts& p) { p.mops[1].b = 4; });
    run("main: num_op beyond the program", "m", false, [](Parts& p) { p.mcols[3].num_op = 7; });
    run("main: den_op beyond the program", "m", false, [](Parts& p) { p.mcols[1].den_op = 7; });
    run("main: aux_kind 1", "m", false, [](Parts& p) { p.d.aux_kind = 1; });
    run("main: aux_kind 2", "m", false, [](Parts& p) { p.d.aux_kind = 2; });
    // ---- chain groups and op 6 in a main program (the _rec policy)
    run("chain group and op 6", "pr", true, none);
    run("chain group beside everything", "xpsbPr", true, [](Parts& p) { p.aux.n_ops = 4; });
    run("chain: the whole trace one block", "pr", true, [](Parts& p) { p.rcols[0].pad = 4; p.rcols[1].pad = 4 + 256; });
    run("chain: without the policy bit", "pR", false, none);
    run("chain: op 6 without the policy bit", "pR", false, [](Parts& p) { p.rcols[0].kind = p.rcols[1].kind = SP_AIR_MAIN_VALUE; p.rcols[0].pad = p.rcols[1].pad = 0; p.rops[2].b = p.rops[3].b = p.rops[6].b = 0; });
    run("chain: op 6 without periodic columns", "r", false, none);
    run("chain: periodic column 1 of 1", "pr", false, [](Parts& p) { p.rops[1].b = 1; });
    run("chain: op 6 at shift 8", "pr", false, [](Parts& p) { p.rops[1].a = 8; });
    run("chain: j = 1 opens", "pr", false, [](Parts& p) { p.rcols[0].pad = 2 + 256; });
    run("chain: j skips", "pr", false, [](Parts& p) { p.rcols[1].pad = 2 + 512; });
    run("chain: j = 2^24 - 1", "pr", false, [](Parts& p) { p.rcols[1].pad = 0xFFFFFF02u; });
    run("chain: l = 0", "pr", false, [](Parts& p) { p.rcols[0].pad = 0; p.rcols[1].pad = 256; });
    run("chain: blocks longer than the trace", "pr", false, [](Parts& p) { p.rcols[0].pad = 5; p.rcols[1].pad = 5 + 256; });
    run("chain: l = 255", "pr", false, [](Parts& p) { p.rcols[0].pad = 255; p.rcols[1].pad = 255 + 256; });
    run("chain: members differ in l", "pr", false, [](Parts& p) { p.rcols[1].pad = 3 + 256; });
    run("chain: a step reads its group at shift 1", "pr", false, [](Parts& p) { p.rops[2].a = 1; });
    run("chain: a seed reads its group", "pr", false, [](Parts& p) { p.rcols[1].den_op = 2; });
    run("chain: a step reads a later column", "pr", false, [](Parts& p) { p.rops[3].b = 3; });
    run("chain: no seed", "pr", false, [](Parts& p) { p.rcols[0].den_op = SP_AIR_AUX_NO_DEN; });
    run("chain: step beyond the program", "pr", false, [](Parts& p) { p.rcols[1].num_op = 7; });
    run("chain: seed beyond the program", "pr", false, [](Parts& p) { p.rcols[1].den_op = 7; });
    run("chain: kind 6", "pr", false, [](Parts& p) { p.rcols[2].kind = 6; });
    run("chain: aux_kind 2", "pr", false, [](Parts& p) { p.d.aux_kind = 2; });
    // ---- lookup multiplicities in a main program (the _lk policy)
    run("count column", "pl", true, none);
    run("count beside everything", "xpsbPl", true, [](Parts& p) { p.aux.n_ops = 4; });
    run("count: 1 key bit", "pl", true, [](Parts& p) { p.lcols[1].pad = 1; });
    run("count: 64 key bits", "pl", true, [](Parts& p) { p.lcols[1].pad = 64; });
    run("count: 16 columns", "pl", true, [](Parts& p) { p.many_counts(16); });
    run("count: a chain program under the _lk policy", "prl", true, none);
    run("count: under the _rec policy alone", "pL", false, none);
    run("count: no table", "pl", false, [](Parts& p) { p.lcols[1].den_op = SP_AIR_AUX_NO_DEN; });
    run("count: 0 key bits", "pl", false, [](Parts& p) { p.lcols[1].pad = 0; });
    run("count: 65 key bits", "pl", false, [](Parts& p) { p.lcols[1].pad = 65; });
    run("count: 2^32 - 1 key bits", "pl", false, [](Parts& p) { p.lcols[1].pad = 0xFFFFFFFFu; });
    run("count: X reads a later column", "pl", false, [](Parts& p) { p.lops[3].b = 3; });
    run("count: T reads the column itself", "pl", false, [](Parts& p) { p.lcols[1].den_op = 4; });
    run("count: X beyond the program", "pl", false, [](Parts& p) { p.lcols[1].num_op = 5; });
    run("count: T beyond the program", "pl", false, [](Parts& p) { p.lcols[1].den_op = 5; });
    run("count: 17 columns", "pl", false, [](Parts& p) { p.many_counts(17); });
    run("count: kind 7", "pl", false, [](Parts& p) { p.lcols[2].kind = 7; });
    run("count: op 6 without periodic columns", "l", false, none);
    run("count: aux_kind 2", "pl", false, [](Parts& p) { p.d.aux_kind = 2; });
    // ---- linked chain groups (the _link policy): l = 2 throughout, k in bits 16 and up of pad
    const auto linked = [](uint32_t k, uint32_t k1) { return [k, k1](Parts& p) { p.rcols[0].pad = 2 + (k << 16); p.rcols[1].pad = 2 + 256 + (k1 << 16); }; };
    const auto carried = [](uint32_t k) { return [k](Parts& p) { p.rcols[0].pad = 2 + (k << 16); p.rcols[1].pad = 2 + 256 + (k << 16); p.rcols[1].den_op = 2; }; };
    run("link: a chain program with k = 0", "pk", true, none);
    run("link: a lookup program", "pl", true, none);
    run("link: runs of two blocks", "pk", true, linked(1, 1));
    run("link: the whole trace one run", "pk", true, linked(2, 2));
    run("link: a seed reads the carry", "pk", true, carried(1));
    run("link: beside everything", "xpsbPk", true, [&](Parts& p) { p.aux.n_ops = 4; carried(2)(p); });
    run("link: a run longer than the trace", "pk", false, linked(3, 3));
    run("link: k = 63", "pk", false, linked(63, 63));
    run("link: k = 65535", "pk", false, linked(65535, 65535));
    run("link: members differ in k", "pk", false, linked(2, 1));
    run("link: k on the second column alone", "pk", false, linked(0, 1));
    run("link: a seed reads its group, k = 0", "pk", false, carried(0));
    run("link: a seed reads its group at shift 1", "pk", false, [&](Parts& p) { carried(1)(p); p.rcols[1].den_op = 6; });
    run("link: j = 1 opens", "pk", false, [](Parts& p) { p.rcols[0].pad = 2 + 256 + (1u << 16); });
    run("link: l = 0", "pk", false, [](Parts& p) { p.rcols[0].pad = 1u << 16; p.rcols[1].pad = 256 + (1u << 16); });
    run("link: k through the _rec policy", "pr", false, linked(1, 1));
    run("link: k through the _lk policy", "prl", false, linked(1, 1));
    run("link: op 6 without periodic columns", "k", false, none);
    // ---- quotients behind chain seeds and steps (the _div policy): op 7 over earlier ops, and nowhere else
    const auto step_divides = [](Parts& p) { p.rops[4].op = 7; };                                   // x0' = x0 / x1
    const auto with_quotient = [](Parts& p) { p.rp.n_ops = 9; };                                    // ops 7 (x / K) and 8 (behind it) join
    const auto third_is = [](uint32_t kind, uint32_t num_op, uint32_t den_op, uint32_t pad) {
        return [=](Parts& p) { p.rp.n_ops = 9; p.rcols[2] = sp_air_main_column{kind, num_op, den_op, pad}; };
    };
    run("div: a chain program without op 7", "pd", true, none);
    run("div: a chain program under the _lk letters too", "prld", true, none);
    run("div: DIV in a step", "pd", true, step_divides);
    run("div: DIV in a seed", "pd", true, [&](Parts& p) { with_quotient(p); p.rcols[0].den_op = 7; });
    run("div: a quotient of a quotient", "pd", true, [&](Parts& p) { step_divides(p); p.rops[5] = sp_air_op{7, 0, 4, 1, 0}; });
    run("div: one quotient behind two next values", "pd", true, [&](Parts& p) { step_divides(p); p.rops[5] = sp_air_op{2, 0, 4, 1, 0}; });
    run("div: a DIV that nothing reaches", "pd", true, with_quotient);
    run("div: a step behind a quotient", "pd", true, [&](Parts& p) { with_quotient(p); p.rcols[1].num_op = 8; });
    run("div: DIV in a linked seed beside a carry", "pd", true, [&](Parts& p) { carried(1)(p); with_quotient(p); p.rcols[0].den_op = 7; });
    run("div: beside everything", "xpsbPd", true, [&](Parts& p) { p.aux.n_ops = 4; step_divides(p); });
    run("div: a VALUE that is a quotient", "pd", false, third_is(SP_AIR_MAIN_VALUE, 7, SP_AIR_AUX_NO_DEN, 0));
    run("div: a VALUE behind a quotient", "pd", false, third_is(SP_AIR_MAIN_VALUE, 8, SP_AIR_AUX_NO_DEN, 0));
    run("div: a VALUE whose D is a quotient", "pd", false, third_is(SP_AIR_MAIN_VALUE, 0, 7, 0));
    run("div: an INV_OR_ZERO behind a quotient", "pd", false, third_is(SP_AIR_MAIN_INV_OR_ZERO, 8, SP_AIR_AUX_NO_DEN, 0));
    run("div: a BIT behind a quotient", "pd", false, third_is(SP_AIR_MAIN_BIT, 8, SP_AIR_AUX_NO_DEN, 3));
    run("div: a SUM behind a quotient", "pd", false, third_is(SP_AIR_MAIN_SUM, 8, SP_AIR_AUX_NO_DEN, 0));
    run("div: a PRODUCT whose D is a quotient", "pd", false, third_is(SP_AIR_MAIN_PRODUCT, 0, 8, 0));
    run("div: a COUNT whose X is behind a quotient", "pd", false, third_is(SP_AIR_MAIN_COUNT, 8, 0, 16));
    run("div: a COUNT whose T is behind a quotient", "pd", false, third_is(SP_AIR_MAIN_COUNT, 0, 8, 16));
    run("div: operand is itself", "pd", false, [](Parts& p) { p.rops[4] = sp_air_op{7, 0, 4, 3, 0}; });
    run("div: operand is later", "pd", false, [](Parts& p) { p.rops[4] = sp_air_op{7, 0, 2, 5, 0}; });
    run("div: operand beyond the program", "pd", false, [](Parts& p) { p.rops[4] = sp_air_op{7, 0, 2, 9, 0}; });
    run("div: op 8", "pd", false, [](Parts& p) { p.rops[4].op = 8; });
    run("div: OUT", "pd", false, [](Parts& p) { p.rops[4].op = 5; });
    run("div: op 6 without periodic columns", "d", false, none);
    run("div: DIV in a step through the _link policy", "pk", false, step_divides);
    run("div: DIV in a step through the _lk policy", "prl", false, step_divides);
    run("div: DIV in a step through the _rec policy", "pr", false, step_divides);
    run("div: DIV in a step without any policy", "pR", false, step_divides);
    run("div: a DIV that nothing reaches through the _link policy", "pk", false, with_quotient);
    run("div: a DIV that nothing reaches through the _rec policy", "pr", false, with_quotient);
    // ---- integer ops behind chain seeds and steps (the _int policy, use 'i'): ops 8 .. 11 over earlier ops, and nowhere else
    const auto step_is = [](sp_air_op o) { return [=](Parts& p) { p.rops[4] = o; }; };
    const auto third_behind_int = [](uint32_t kind, uint32_t num_op, uint32_t den_op, uint32_t pad) {   // op 7 becomes x OR K, op 8 stays behind it
        return [=](Parts& p) { p.rp.n_ops = 9; p.rops[7] = sp_air_op{10, 0, 0, 1, 0}; p.rcols[2] = sp_air_main_column{kind, num_op, den_op, pad}; };
    };
    run("int: a chain program without the ops", "pi", true, none);
    run("int: LIMB in a step", "pi", true, step_is(sp_air_op{8, 0, 2, 8 + 256 * 16, 0}));
    run("int: the widest LIMB", "pi", true, step_is(sp_air_op{8, 0, 2, 0 + 256 * 252, 0}));
    run("int: the top bit", "pi", true, step_is(sp_air_op{8, 0, 2, 251 + 256, 0}));
    run("int: AND, OR and XOR in a step", "pi", true, [](Parts& p) { p.rops[4] = sp_air_op{9, 0, 2, 3, 0}; p.rops[5] = sp_air_op{11, 0, 4, 1, 0}; });
    run("int: XOR in a seed", "pi", true, [](Parts& p) { p.rp.n_ops = 9; p.rops[7] = sp_air_op{11, 0, 0, 1, 0}; p.rcols[0].den_op = 7; });
    run("int: beside op 7", "pi", true, [](Parts& p) { p.rops[4].op = 7; p.rops[5] = sp_air_op{8, 0, 4, 31 + 256 * 40, 0}; });
    run("int: an integer op that nothing reaches", "pi", true, [](Parts& p) { p.rp.n_ops = 9; p.rops[7] = sp_air_op{10, 0, 0, 1, 0}; });
    run("int: LIMB with width 0", "pi", false, step_is(sp_air_op{8, 0, 2, 8, 0}));
    run("int: LIMB with lo + width = 253", "pi", false, step_is(sp_air_op{8, 0, 2, 200 + 256 * 53, 0}));
    run("int: LIMB whose operand is later", "pi", false, step_is(sp_air_op{8, 0, 5, 256, 0}));
    run("int: LIMB whose operand is itself", "pi", false, step_is(sp_air_op{8, 0, 4, 256, 0}));
    run("int: AND whose operand is itself", "pi", false, step_is(sp_air_op{9, 0, 2, 4, 0}));
    run("int: XOR whose operand is beyond the program", "pi", false, step_is(sp_air_op{11, 0, 2, 9, 0}));
    run("int: op 12", "pi", false, step_is(sp_air_op{12, 0, 2, 3, 0}));
    run("int: a VALUE that is an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_VALUE, 7, SP_AIR_AUX_NO_DEN, 0));
    run("int: a VALUE behind an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_VALUE, 8, SP_AIR_AUX_NO_DEN, 0));
    run("int: a BIT behind an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_BIT, 8, SP_AIR_AUX_NO_DEN, 3));
    run("int: a COUNT whose T is behind an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_COUNT, 0, 8, 16));
    run("int: a FETCH whose V is an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_FETCH, 0, 0, 16 + 256 * 7));
    run("int: a LIMB column behind an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_LIMB, 8, SP_AIR_AUX_NO_DEN, 256 * 8));
    run("int: a WORD column whose D is behind an integer op", "pi", false, third_behind_int(SP_AIR_MAIN_WORD, 0, 8, 2 + 256 * 8));
    run("int: a LIMB column over the input beside the group", "pi", true, [](Parts& p) { p.rcols[2] = sp_air_main_column{SP_AIR_MAIN_LIMB, 0, SP_AIR_AUX_NO_DEN, 256 * 8}; });
    run("int: LIMB in a step through the _div policy", "pd", false, step_is(sp_air_op{8, 0, 2, 8 + 256 * 16, 0}));
    run("int: XOR in a step through the _rec policy", "pr", false, step_is(sp_air_op{11, 0, 2, 3, 0}));
    run("int: op 6 without periodic columns", "i", false, none);
    run("aux: op 8 through the _int policy", "xpi", false, [](Parts& p) { p.aux_ops[2].op = 8; });
    // ---- one COUNT column over a list of looked-up values (the _multi policy, use 'j'): bit 8 of the pad, op 12 cells behind num_op
    const auto joint = [](uint32_t n_ops, uint32_t num_op, uint32_t den_op, uint32_t pad) {
        return [=](Parts& p) { p.lp.n_ops = n_ops; p.lcols[1] = sp_air_main_column{SP_AIR_MAIN_COUNT, num_op, den_op, pad}; };
    };
    const auto joint_and = [&](const std::function<void(Parts&)>& more) { return [=](Parts& p) { joint(7, 6, 1, 16 + 256)(p); more(p); }; };
    run("multi: a lookup program without a list", "pj", true, none);
    run("multi: cells that no column names", "pj", true, [](Parts& p) { p.lp.n_ops = 7; });
    run("multi: a list of two", "pj", true, joint(7, 6, 1, 16 + 256));
    run("multi: a list of one", "pj", true, joint(6, 5, 1, 64 + 256));
    run("multi: one key bit", "pj", true, joint(7, 6, 1, 1 + 256));
    run("multi: a list of sixteen", "pj", true, [&](Parts& p) { for (uint16_t t = 7; t < 21; ++t) p.lops[t] = sp_air_op{12, 0, 0, (uint16_t)(t - 1), 0}; joint(21, 20, 1, 16 + 256)(p); });
    run("multi: a list of seventeen", "pj", false, [&](Parts& p) { for (uint16_t t = 7; t < 22; ++t) p.lops[t] = sp_air_op{12, 0, 0, (uint16_t)(t - 1), 0}; joint(22, 21, 1, 16 + 256)(p); });
    run("multi: a pad with bit 9", "pj", false, joint(7, 6, 1, 16 + 256 + 512));
    run("multi: a pad with bit 31", "pj", false, joint(7, 6, 1, 16 + 256 + (1u << 31)));
    run("multi: bit 8 and a num_op that is no cell", "pj", false, joint(7, 3, 1, 16 + 256));
    run("multi: a cell behind a column without bit 8", "pj", false, joint(7, 6, 1, 16));
    run("multi: key_bits 0", "pj", false, joint(7, 6, 1, 256));
    run("multi: key_bits 65", "pj", false, joint(7, 6, 1, 65 + 256));
    run("multi: no table", "pj", false, joint(7, 6, SP_AIR_AUX_NO_DEN, 16 + 256));
    run("multi: a cell as the table", "pj", false, joint(7, 6, 5, 16 + 256));
    run("multi: a num_op beyond the program", "pj", false, joint(7, 7, 1, 16 + 256));
    run("multi: a cell whose a is itself", "pj", false, joint_and([](Parts& p) { p.lops[5].a = 5; }));
    run("multi: a cell whose a is later", "pj", false, joint_and([](Parts& p) { p.lops[5].a = 6; }));
    run("multi: a cell whose a is a cell", "pj", false, joint_and([](Parts& p) { p.lops[6].a = 5; }));
    run("multi: a cell whose b is a value", "pj", false, joint_and([](Parts& p) { p.lops[6].b = 3; }));
    run("multi: a cell whose b is itself", "pj", false, joint_and([](Parts& p) { p.lops[6].b = 6; }));
    run("multi: a cell whose b is beyond the program", "pj", false, joint_and([](Parts& p) { p.lops[5].b = 0xFFFE; }));
    run("multi: an ADD of a cell", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 8; p.lops[7] = sp_air_op{2, 0, 6, 0, 0}; }));
    run("multi: a MUL by a cell", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 8; p.lops[7] = sp_air_op{4, 0, 0, 5, 0}; }));
    run("multi: an OUT of a cell", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 8; p.lops[7] = sp_air_op{5, 0, 0, 6, 0}; }));
    run("multi: a VALUE that is a cell", "pj", false, joint_and([](Parts& p) { p.lcols[0].num_op = 5; }));
    run("multi: a SUM over a cell", "pj", false, joint_and([](Parts& p) { p.lcols[2].den_op = 6; }));
    run("multi: an X that reads its own column", "pj", false, joint_and([](Parts& p) { p.lops[5].a = 4; }));
    run("multi: an X behind a quotient", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 9; p.lops[7] = sp_air_op{7, 0, 0, 1, 0}; p.lops[8] = sp_air_op{12, 0, 7, 6, 0}; p.lcols[1].num_op = 8; }));
    run("multi: an X behind an integer op", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 9; p.lops[7] = sp_air_op{8, 0, 0, 256 * 8, 0}; p.lops[8] = sp_air_op{12, 0, 7, 0xFFFF, 0}; p.lcols[1].num_op = 8; }));
    run("multi: op 13", "pj", false, joint_and([](Parts& p) { p.lp.n_ops = 8; p.lops[7] = sp_air_op{13, 0, 0, 1, 0}; }));
    run("multi: a seventeenth COUNT column, joint", "pj", false, [](Parts& p) { p.many_counts(17); p.lp.n_ops = 7; p.many_lcols[16] = sp_air_main_column{SP_AIR_MAIN_COUNT, 6, 1, 64 + 256}; });
    run("multi: sixteen COUNT columns, one joint", "pj", true, [](Parts& p) { p.many_counts(16); p.lp.n_ops = 7; p.many_lcols[15] = sp_air_main_column{SP_AIR_MAIN_COUNT, 6, 1, 64 + 256}; });
    run("multi: a cell through the _lk policy", "pl", false, joint(7, 6, 1, 16 + 256));
    run("multi: bit 8 through the _lk policy", "pl", false, joint(5, 3, 1, 16 + 256));
    run("multi: cells that no column names through the _lk policy", "pl", false, [](Parts& p) { p.lp.n_ops = 7; });
    run("multi: the chain program through the _multi policy", "pij", true, [](Parts& p) { (void)p; });
    run("aux: op 12 through the _multi policy", "xpj", false, [](Parts& p) { p.aux_ops[2].op = 12; });
    run("aux: op 7", "x", false, [](Parts& p) { p.aux_ops[2].op = 7; });
    run("aux: op 7 through the _div policy", "xpd", false, [](Parts& p) { p.aux_ops[2].op = 7; });
    run("no main column", "", false, [](Parts& p) { p.d.main_cols = 0; p.ops[2] = sp_air_op{1, 0, 0, 0, 0}; });
    run("1025 columns", "", false, [](Parts& p) { p.d.main_cols = 1024; p.ops[2] = sp_air_op{1, 0, 0, 0, 0}; });
    std::printf("%s\n", failures ? "FAILED" : "all verdicts as expected");
    return failures ? 1 : 0;
}
