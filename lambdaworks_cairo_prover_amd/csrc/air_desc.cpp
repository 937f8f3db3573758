// The statement of a program AIR on the host (air_desc.h): its one decoder and validator, and the model of its parts that the
// prover, the trace check, the verifier and the test seams share - program rules, stride plans and zerofiers, boundary values from
// the challenges, periodic columns as polynomials.
#include "air_desc.h"
#include "common.h"
#include <algorithm>
#include <stdexcept>

namespace sp {

fe air_root_of_unity(int order) {   // the field's 2^192-th root, squared down
    fe w = fe_from_bytes_be((const uint8_t*)"\x00\x52\x82\xdb\x87\x52\x9c\xfa\x3f\x04\x64\x51\x9c\x8b\x0f\xa5\xad\x18\x71\x48\xe1\x1a\x61\x61\x60\x70\x02\x4f\x42\xf8\xef\x94");
    for (int i = order; i < 192; ++i) w = fe_sqr(w);
    return w;
}

size_t air_program_first_bad_op(const std::vector<AirOpHost>& ops, uint32_t load_a_end, uint32_t load_b_end, size_t n_values, uint32_t n_out,
                                uint32_t n_periodic, bool div, bool ints, bool lists) {
    auto value = [&](uint32_t i, size_t t) { return i < t && ops[i].op != 5 && ops[i].op != AIR_OP_ALSO; };   // an earlier op that produces a value
    for (size_t t = 0; t < ops.size(); ++t) {
        const AirOpHost& o = ops[t];
        bool ok;
        switch (o.op) {
            case 0: ok = o.a < load_a_end && o.b < load_b_end; break;
            case 1: ok = o.a < n_values; break;
            case 2: case 3: case 4: ok = value(o.a, t) && value(o.b, t); break;
            case 5: ok = o.a < n_out && value(o.b, t); break;
            case 6: ok = o.a < load_a_end && o.b < n_periodic; break;
            case 7: ok = div && value(o.a, t) && value(o.b, t); break;
            case 8: ok = ints && value(o.a, t) && (o.b >> 8) >= 1 && (o.b & 255u) + (o.b >> 8) <= AIR_MAIN_LIMB_MAX_END; break;
            case 9: case 10: case 11: ok = ints && value(o.a, t) && value(o.b, t); break;
            case 12: ok = lists && value(o.a, t) && (o.b == AIR_LIST_END || (o.b < t && ops[o.b].op == AIR_OP_ALSO)); break;
            default: ok = false;
        }
        if (!ok) return t;
    }
    return ops.size();
}

// ---- the decoder: one function per part, each with one caller (air_boundary_from_c: sp_air_boundary_resolve too)
namespace {
template <class Op> void ops_from_c(const Op* ops, uint32_t n, std::vector<AirOpHost>& out) {
    out.reserve(n);
    for (uint32_t i = 0; i < n; ++i) out.push_back(AirOpHost{ops[i].op, ops[i].a, ops[i].b});
}
void consts_from_c(const uint8_t* consts, uint32_t n, std::vector<fe>& out) {
    out.reserve(n);
    for (uint32_t i = 0; i < n; ++i) out.push_back(fe_from_bytes_be(consts + 32 * (size_t)i));
}

// sp_air_desc -> AirDescHost; false for counts out of range or a count without its array
bool air_desc_from_c(const sp_air_desc* d, AirDescHost& a) {
    if (d->n_offsets == 0 || d->n_offsets > 8 || d->n_transitions == 0 || d->n_transitions > 64 || (d->n_ops && !d->ops) ||
        (d->n_consts && !d->consts) || (d->n_boundary && !d->boundary)) return false;
    a.main_cols = d->main_cols; a.aux_cols = d->aux_cols;
    a.offsets.assign(d->offsets, d->offsets + d->n_offsets);
    a.degrees.assign(d->degrees, d->degrees + d->n_transitions);
    a.exemptions.assign(d->exemptions, d->exemptions + d->n_transitions);
    a.num_transition_exemptions = d->num_transition_exemptions;
    a.degree_bound_factor = d->degree_bound_factor;
    ops_from_c(d->ops, d->n_ops, a.ops);
    consts_from_c(d->consts, d->n_consts, a.consts);
    a.n_rap = d->n_rap; a.aux_kind = d->aux_kind; a.aux_fn = d->aux_fn; a.aux_user = d->aux_user;
    for (uint32_t i = 0; i < d->n_boundary; ++i)
        a.boundary.push_back(BoundaryConstraint{d->boundary[i].col, d->boundary[i].step, fe_from_bytes_be(d->boundary[i].value)});
    return true;
}

// sp_air_periodic_desc -> AirPeriodicHost for a trace of n rows; false for more than 64 columns, a count without its array, null
// values, a period that is no power of two or exceeds n
bool air_periodic_from_c(const sp_air_periodic_desc* d, uint64_t n, AirPeriodicHost& out) {
    if (d->n_cols > AIR_MAX_PERIODIC || (d->n_cols && !d->cols)) return false;
    for (uint32_t k = 0; k < d->n_cols; ++k) {   // every column first: nothing is allocated for a descriptor that is refused
        const sp_air_periodic_column& c = d->cols[k];
        if (c.period == 0 || (c.period & (c.period - 1)) || c.period > n || !c.values) return false;
    }
    for (uint32_t k = 0; k < d->n_cols; ++k) {
        out.cols.emplace_back();
        consts_from_c(d->cols[k].values, d->cols[k].period, out.cols.back());
    }
    return true;
}

// sp_air_stride_desc -> air.strides for a trace of n rows (a power of two), checked by air_stride_plan: prover, trace check and
// verifier all read a descriptor's strides through here
bool air_strides_from_c(const sp_air_stride_desc* d, uint64_t n, AirDescHost& air) {
    if (d->n != air.exemptions.size() || !d->strides || sp_log2_exact(n) < 0) return false;
    for (uint32_t k = 0; k < d->n; ++k) air.strides.push_back(AirStrideHost{d->strides[k].period, d->strides[k].offset});
    AirStridePlan plan;
    return air_stride_plan(air, n, plan);
}

// sp_air_aux_desc -> AirAuxHost, as far as the C view goes: its AIR wants one, counts have their arrays and stay within the bounds
bool aux_from_c(const AirDescHost& air, const sp_air_aux_desc* x, AirAuxHost& aux) {
    if (air.aux_kind != SP_AIR_AUX_PROGRAM || air.aux_cols == 0 || x->n_cols != air.aux_cols || (x->n_ops && !x->ops) || (x->n_consts && !x->consts) ||
        !x->cols || x->n_ops > AIR_LIMIT_OPS || x->n_consts > AIR_LIMIT_CONSTS) return false;
    ops_from_c(x->ops, x->n_ops, aux.ops);
    consts_from_c(x->consts, x->n_consts, aux.consts);
    for (uint32_t k = 0; k < x->n_cols; ++k) aux.cols.push_back(AirAuxColumnHost{x->cols[k].kind, x->cols[k].num_op, x->cols[k].den_op,
                                                                                 x->cols[k].kind == SP_AIR_AUX_SORTED ? (x->cols[k].pad ? x->cols[k].pad : 64u) : 0u});   // (pad 0: 64 bits; kinds 0 and 1 ignore it)
    return true;
}

// The auxiliary program against its AIR: operands refer to earlier ops, LOADs to main columns - or to SORTED auxiliary columns - at
// shifts 0 .. 7, CONSTs to the constants or the n_rap challenges, PERIODICs to one of n_periodic columns (0: none), every column's ops
// exist; a sorted column has a key op and 1 .. 64 key bits, its group agrees on them, there are at most SP_AIR_AUX_MAX_SORT_GROUPS
// groups, and nothing behind its key or its value reads a sorted column.  "" or what is wrong.
std::string validate_aux_program(const AirAuxHost& aux, uint32_t main_cols, uint32_t n_rap, uint32_t n_periodic) {
    const size_t n_ops = aux.ops.size();
    if (n_ops == 0) return "auxiliary program: no ops";
    if (aux.consts.size() + n_rap > 65535) return "auxiliary program: constants and RAP challenges exceed the 16-bit operand range";
    bool any_sorted = false;
    for (const AirAuxColumnHost& c : aux.cols) any_sorted |= c.kind == SP_AIR_AUX_SORTED;
    // (a program without sorted columns is held to the main columns, as it always was)
    const uint32_t load_b_end = main_cols + (any_sorted ? (uint32_t)aux.cols.size() : 0u);
    const size_t bad = air_program_first_bad_op(aux.ops, AIR_LIMIT_AUX_SHIFT + 1, load_b_end, aux.consts.size() + n_rap, 0, n_periodic);   // (no OUT: the columns name their ops)
    if (bad < n_ops)
        return "auxiliary program: malformed op " + std::to_string(bad) + " (LOAD needs a shift of 0 .. 7 and a main column, CONST a constant or a RAP "
               "challenge, ADD / SUB / MUL earlier ops; there is no OUT, and PERIODIC only through sp_air_prove_pub: a shift of 0 .. 7 and a periodic column)";
    for (size_t k = 0; k < aux.cols.size(); ++k) {
        const AirAuxColumnHost& c = aux.cols[k];
        if (c.kind > SP_AIR_AUX_SORTED || c.num_op >= n_ops || (c.den_op != SP_AIR_AUX_NO_DEN && c.den_op >= n_ops))
            return "auxiliary program: column " + std::to_string(k) + " has an unknown kind or names an op beyond the program";
    }
    if (!any_sorted) return "";
    // reads[t]: the value of op t depends on a sorted column
    std::vector<uint8_t> reads(n_ops, 0);
    for (size_t t = 0; t < n_ops; ++t) {
        const AirOpHost& o = aux.ops[t];
        if (o.op == 0 && o.b >= main_cols) {   // a LOAD of an auxiliary column
            if (aux.cols[o.b - main_cols].kind != SP_AIR_AUX_SORTED)
                return "auxiliary program: op " + std::to_string(t) + " loads auxiliary column " + std::to_string(o.b - main_cols) + ", which is not a sorted column";
            reads[t] = 1;
        } else if (o.op >= 2 && o.op <= 4) reads[t] = reads[o.a] | reads[o.b];
    }
    std::vector<std::pair<uint32_t, uint32_t>> groups;   // (key op, key bits)
    for (size_t k = 0; k < aux.cols.size(); ++k) {
        const AirAuxColumnHost& c = aux.cols[k];
        if (c.kind != SP_AIR_AUX_SORTED) continue;
        const std::string who = "auxiliary program: sorted column " + std::to_string(k);
        if (c.den_op == SP_AIR_AUX_NO_DEN) return who + " names no key op (den_op)";
        if (c.key_bits == 0 || c.key_bits > 64) return who + " has " + std::to_string(c.key_bits) + " key bits (pad: 1 .. 64, or 0 for 64)";
        if (reads[c.num_op] || reads[c.den_op]) return who + " reads a sorted column through its key or its value";
        size_t g = 0;
        while (g < groups.size() && groups[g].first != c.den_op) ++g;
        if (g == groups.size()) {
            if (g == SP_AIR_AUX_MAX_SORT_GROUPS) return who + " opens more than " + std::to_string(SP_AIR_AUX_MAX_SORT_GROUPS) + " sort groups";
            groups.emplace_back(c.den_op, c.key_bits);
        } else if (groups[g].second != c.key_bits) return who + " disagrees with its group (key op " + std::to_string(c.den_op) + ") on the key bits";
    }
    return "";
}

// sp_air_main_desc -> AirMainHost against its AIR: "" or what is wrong.  Every count and pointer first; then the ops (0 .. 4 over
// earlier ops, LOADs of main columns at shifts 0 .. 7), the columns' kinds, and - following the operands - which derived columns
// the ops behind each column load: only earlier ones.  rec (the _rec entry points): op 6 over the statement's n_periodic periodic
// columns and SP_AIR_MAIN_CHAIN columns too - groups with j = 0, 1, .. and one l, seeds that read nothing of their group, steps that
// read it at shift 0 only; without rec kind 5 is an unknown kind and op 6 a malformed op.  lk (the _lk entry points, with rec):
// SP_AIR_MAIN_COUNT columns too - a table, key_bits in 1 .. 64, at most 16 of them; without lk kind 6 is an unknown kind.  link (the
// _link entry points, with lk): a CHAIN column's pad is l + 256 j + 65536 k, runs of 2^k blocks; with k >= 1 a seed may load its own
// group at shift 0; without link j = pad >> 8, so a pad with bits at or above 16 is a j out of sequence.  div (the _div entry points,
// with link): op 7 DIV over earlier ops, behind the seeds and steps of CHAIN columns only; a column of any other kind that depends on
// one is refused, and without div op 7 is a malformed op.  fetch (the _fetch entry points, with div): SP_AIR_MAIN_FETCH columns too - a
// table key, pad = key_bits (1 .. 64) + 256 v_op below 2^24, X, T and V over earlier columns and behind no op 7, at most 64 of them;
// without fetch kind 7 is an unknown kind.  word (the _word entry points, with fetch): SP_AIR_MAIN_LIMB columns too - no denominator,
// pad = lo + 256 width below 2^16, 1 <= width, lo + width <= 252 - and SP_AIR_MAIN_WORD columns - a second operand, pad = fn + 256 bits
// below 2^16, fn 0 .. 2, bits 1 .. 251 -, both over earlier columns and behind no op 7; without word kinds 8 and 9 are unknown kinds.
// ints (the _int entry points, with word): ops 8 LIMB and 9 .. 11 AND / OR / XOR over earlier ops, behind the seeds and steps of CHAIN
// columns only, as op 7; a column of any other kind that depends on one is refused, and without ints they are malformed ops.
// lists (the _multi entry points, with ints): a COUNT column whose pad carries bit 8 (pad = key_bits + 256) counts a list of 1 .. 16
// looked-up values, the op 12 cells from its num_op on, all over earlier columns and behind no op 7 .. 11; a cell is nothing else of
// any column and no operand, and without lists op 12 is a malformed op and such a pad a key_bits out of range.
std::string main_from_c(const AirDescHost& air, const sp_air_main_desc* m, uint64_t n, uint32_t n_periodic, AirMainLevel level, AirMainHost& out) {
    const bool rec = air_main_allows_chains(level), lk = air_main_allows_counts(level), link = air_main_allows_runs(level);
    const bool div = air_main_allows_quotients(level), fetch = air_main_allows_fetches(level), word = air_main_allows_words(level);
    const bool ints = air_main_allows_int_ops(level), lists = air_main_allows_lists(level);
    if (m->size != sizeof(sp_air_main_desc)) return "main program: sp_air_main_desc.size is not sizeof(sp_air_main_desc)";
    if (!m->ops || !m->consts || !m->cols) return "main program: null ops, consts or cols";
    if (m->input_cols == 0 || m->n_cols == 0 || (uint64_t)m->input_cols + m->n_cols != air.main_cols)
        return "main program: input_cols (>= 1) + n_cols (>= 1) must be air->main_cols";
    if (m->input_location > 1) return "main program: input_location is 0 (host memory) or 1 (device memory)";
    if (m->n_ops == 0 || m->n_ops > AIR_LIMIT_OPS || m->n_consts > AIR_LIMIT_CONSTS) return "main program: 1 .. 65535 ops and at most 4096 constants";
    std::vector<AirOpHost> ops;
    ops_from_c(m->ops, m->n_ops, ops);
    const size_t n_ops = ops.size();
    if (rec)
        for (size_t t = 0; t < n_ops; ++t)
            if (ops[t].op == 6 && ops[t].b >= n_periodic)
                return "main program: op " + std::to_string(t) + " reads periodic column " + std::to_string(ops[t].b) + ", and the statement has " +
                       std::to_string(n_periodic) + " (ext->periodic)";
    // (no OUT target; a periodic column only through the _rec entry points: elsewhere ops 0 .. 4 are all that is left)
    const size_t bad = air_program_first_bad_op(ops, AIR_LIMIT_AUX_SHIFT + 1, air.main_cols, m->n_consts, 0, rec ? n_periodic : 0u, div, ints, lists);
    if (bad < n_ops && lists) {   // (what is wrong with a list cell, or with an op that takes one for a value, by name)
        const AirOpHost& o = ops[bad];
        const std::string who = "main program: op " + std::to_string(bad);
        const auto cell = [&](uint32_t i) { return i < bad && ops[i].op == AIR_OP_ALSO; };
        if (o.op == AIR_OP_ALSO && (o.a >= bad || ops[o.a].op == 5 || ops[o.a].op == AIR_OP_ALSO))
            return who + " is a list cell (op 12) whose a = " + std::to_string(o.a) + " is no earlier value op (a cell names one looked-up value, and no cell)";
        if (o.op == AIR_OP_ALSO)
            return who + " is a list cell (op 12) whose b = " + std::to_string(o.b) + " is neither 0xFFFF nor an earlier cell (b names the rest of the list)";
        if ((air_op_takes_two_values(o.op) && (cell(o.a) || cell(o.b))) || (air_op_takes_one_value(o.op) && cell(o.a)) || (o.op == 5 && cell(o.b)))
            return who + " takes a list cell (op 12) for an operand, and a cell has no value";
    }
    if (bad < n_ops && ints && air_op_is_integer(ops[bad].op)) {   // (what is wrong with an integer op, by name)
        const AirOpHost& o = ops[bad];
        const std::string who = "main program: op " + std::to_string(bad);
        const auto earlier = [&](uint32_t i) { return i < bad && ops[i].op != 5; };
        if (!earlier(o.a) || (o.op != 8 && !earlier(o.b)))
            return who + " is an integer op (op " + std::to_string(o.op) + ") whose operands are not earlier values (LIMB: a; AND / OR / XOR: a and b)";
        if ((o.b >> 8) == 0) return who + " is a LIMB op with width = 0 (b = lo + 256 width, 1 <= width, lo + width <= 252)";
        return who + " is a LIMB op with lo + width = " + std::to_string((o.b & 255u) + (o.b >> 8)) + " (b = lo + 256 width, 1 <= width, lo + width <= 252)";
    }
    if (bad < n_ops && ints)
        return "main program: malformed op " + std::to_string(bad) + " (LOAD needs a shift of 0 .. 7 and a main column, CONST a constant, ADD / SUB / MUL / DIV / "
               "AND / OR / XOR earlier ops, LIMB an earlier op and lo + 256 width, op 6 a shift of 0 .. 7 and a periodic column; there is no OUT and no RAP challenge)";
    if (bad < n_ops && div)
        return "main program: malformed op " + std::to_string(bad) + " (LOAD needs a shift of 0 .. 7 and a main column, CONST a constant, ADD / SUB / MUL / DIV "
               "earlier ops, op 6 a shift of 0 .. 7 and a periodic column; there is no OUT and no RAP challenge)";
    if (bad < n_ops)
        return "main program: malformed op " + std::to_string(bad) + " (LOAD needs a shift of 0 .. 7 and a main column, CONST a constant, ADD / SUB / MUL earlier "
               "ops; there is no OUT and no RAP challenge, and op 6 - a shift of 0 .. 7 and a periodic column - only through the _rec entry points)";
    // reads[t]: one more than the highest derived column the value of op t depends on (0: inputs only); shifted[t]: the same over the
    // LOADs at a shift other than 0 alone (what a chain's step may not do to its own group); chain_only[t]: the value of op t depends on
    // a chain-only op - CHAIN_QUOT: a quotient (an op 7 is op t or stands behind it), CHAIN_INT: an integer op 8 .. 11 -, which only the
    // seed and the step of a CHAIN column may
    constexpr uint8_t CHAIN_QUOT = 1, CHAIN_INT = 2;
    std::vector<uint32_t> reads(n_ops, 0), shifted(n_ops, 0);
    std::vector<uint8_t> chain_only(n_ops, 0);
    std::vector<uint32_t> list_len(n_ops, 0);   // of an op 12: the cells of its list, itself included (capped one above the limit)
    const auto chain_only_refused = [](const std::string& who, uint8_t marks) {
        if (marks & CHAIN_QUOT)
            return who + " depends on a quotient (op 7), which only the seed or the step of a CHAIN column may: a row-local quotient is a VALUE column's N / D";
        return who + " depends on an integer op (ops 8 .. 11), which only the seed or the step of a CHAIN column may: a row-local limb or word is a LIMB or WORD column";
    };
    for (size_t t = 0; t < n_ops; ++t) {
        const AirOpHost& o = ops[t];
        if (o.op == 0 && o.b >= m->input_cols) { reads[t] = o.b - m->input_cols + 1; shifted[t] = o.a ? reads[t] : 0u; }
        else if (air_op_takes_two_values(o.op)) {
            reads[t] = std::max(reads[o.a], reads[o.b]); shifted[t] = std::max(shifted[o.a], shifted[o.b]);
            chain_only[t] = (o.op == 7 ? CHAIN_QUOT : air_op_is_integer(o.op) ? CHAIN_INT : 0) | chain_only[o.a] | chain_only[o.b];
        } else if (air_op_takes_one_value(o.op)) {   // (b is lo + 256 width, no value)
            reads[t] = reads[o.a]; shifted[t] = shifted[o.a];
            chain_only[t] = CHAIN_INT | chain_only[o.a];
        } else if (o.op == AIR_OP_ALSO) {   // a cell stands for its whole list: what any X of it reads, and how many there are
            const bool more = o.b != AIR_LIST_END;
            reads[t] = std::max(reads[o.a], more ? reads[o.b] : 0u); shifted[t] = std::max(shifted[o.a], more ? shifted[o.b] : 0u);
            chain_only[t] = chain_only[o.a] | (more ? chain_only[o.b] : 0);
            list_len[t] = std::min<uint32_t>(1u + (more ? list_len[o.b] : 0u), AIR_MAIN_COUNT_MAX_LIST + 1);
        }
    }
    // (a cell is the num_op of a joint COUNT column and nothing else of any column)
    const auto is_cell = [&](uint32_t t) { return t < n_ops && ops[t].op == AIR_OP_ALSO; };
    const auto cell_refused = [](const std::string& who) {
        return who + " names a list cell (op 12), which only the num_op of a COUNT column with bit 8 of its pad may (a cell has no value)";
    };
    std::vector<AirMainColumnHost> cols;
    cols.reserve(m->n_cols);
    uint32_t g0 = 0, g_end = 0;   // the chain group that column k belongs to is [g0, g_end), when k < g_end
    uint32_t n_count = 0, n_fetch = 0;
    for (uint32_t k = 0; k < m->n_cols; ++k) {
        const sp_air_main_column& c = m->cols[k];
        const std::string who = "main program: derived column " + std::to_string(k);
        const bool den = c.den_op != SP_AIR_AUX_NO_DEN;
        if (c.kind > (word ? SP_AIR_MAIN_WORD : fetch ? SP_AIR_MAIN_FETCH : lk ? SP_AIR_MAIN_COUNT : rec ? SP_AIR_MAIN_CHAIN : SP_AIR_MAIN_PRODUCT))
            return who + " has an unknown kind";
        const bool joint = lists && c.kind == SP_AIR_MAIN_COUNT && (c.pad & AIR_MAIN_COUNT_LIST_BIT);
        if (lists && ((den && is_cell(c.den_op)) || (!joint && is_cell(c.num_op)) ||
                      (c.kind == SP_AIR_MAIN_FETCH && is_cell((c.pad >> 8) & 65535u))))
            return cell_refused(who);
        if (c.kind == SP_AIR_MAIN_LIMB || c.kind == SP_AIR_MAIN_WORD) {   // (row-local, as a BIT column: the rules of a VALUE column's operands)
            const bool limb = c.kind == SP_AIR_MAIN_LIMB;
            const uint32_t low = c.pad & 255u, high = (c.pad >> 8) & 255u;   // LIMB: lo, width; WORD: fn, bits
            if (c.pad >> 16)
                return who + (limb ? " is a LIMB column whose pad has a bit at or above 16 (pad = lo + 256 width)" : " is a WORD column whose pad has a bit at or above 16 (pad = fn + 256 bits)");
            if (limb && den) return who + " is a LIMB column and takes no denominator";
            if (!limb && !den) return who + " is a WORD column without a second operand (den_op names it)";
            if (limb && high == 0) return who + " is a LIMB column with width = 0 (1 <= width, lo + width <= 252)";
            if (limb && low + high > AIR_MAIN_LIMB_MAX_END)
                return who + " is a LIMB column with lo + width = " + std::to_string(low + high) + " (1 <= width, lo + width <= 252)";
            if (!limb && low >= AIR_MAIN_WORD_FUNCTIONS) return who + " is a WORD column with fn = " + std::to_string(low) + " (0 AND, 1 OR, 2 XOR)";
            if (!limb && (high == 0 || high > AIR_MAIN_WORD_MAX_BITS)) return who + " is a WORD column with bits = " + std::to_string(high) + " (1 .. 251)";
            if (c.num_op >= n_ops || (den && c.den_op >= n_ops)) return who + " names an op beyond the program";
            if (const uint8_t marks = chain_only[c.num_op] | (den ? chain_only[c.den_op] : 0)) return chain_only_refused(who, marks);
            const uint32_t r = std::max(reads[c.num_op], den ? reads[c.den_op] : 0u);
            if (r > k) return who + " reads derived column " + std::to_string(r - 1) + ", which is not an earlier one";
            cols.push_back(AirMainColumnHost{c.kind, c.num_op, c.den_op, low, r, 0u, 0u, 0u, 0u, 0u, high});
            continue;
        }
        if (c.kind == SP_AIR_MAIN_FETCH) {
            const uint32_t key_bits = c.pad & 255u, v_op = (c.pad >> 8) & 65535u;
            if (c.pad >> 24) return who + " is a FETCH column whose pad has a bit at or above 24 (pad = key_bits + 256 v_op)";
            if (!den) return who + " is a FETCH column without a table key (den_op names the table key)";
            if (key_bits == 0 || key_bits > AIR_MAIN_FETCH_MAX_KEY_BITS) return who + " is a FETCH column with key_bits = " + std::to_string(key_bits) + " (1 .. 64)";
            if (c.num_op >= n_ops || c.den_op >= n_ops) return who + " names an op beyond the program";
            if (v_op >= n_ops || ops[v_op].op == 5) return who + " is a FETCH column with v_op = " + std::to_string(v_op) + ", which is beyond the program or an OUT";
            if (const uint8_t marks = chain_only[c.num_op] | chain_only[c.den_op] | chain_only[v_op]) return chain_only_refused(who, marks);
            const uint32_t r = std::max(std::max(reads[c.num_op], reads[c.den_op]), reads[v_op]);
            if (r > k) return who + " reads derived column " + std::to_string(r - 1) + ", which is not an earlier one";
            if (++n_fetch > AIR_MAIN_FETCH_MAX_COLS) return who + " is the program's FETCH column number " + std::to_string(n_fetch) + " (at most 64)";
            cols.push_back(AirMainColumnHost{c.kind, c.num_op, c.den_op, 0u, r, 0u, 0u, key_bits, 0u, v_op});
            continue;
        }
        if (c.kind == SP_AIR_MAIN_COUNT) {
            if (!den) return who + " is a COUNT column without a table (den_op names the table value)";
            if (lists && (c.pad >> 9)) return who + " is a COUNT column whose pad has a bit above 8 (pad = key_bits, and + 256 when num_op names a list of looked-up values)";
            const uint32_t key_bits = joint ? c.pad & 255u : c.pad;
            if (key_bits == 0 || key_bits > AIR_MAIN_COUNT_MAX_KEY_BITS) return who + " is a COUNT column with key_bits = " + std::to_string(key_bits) + " (1 .. 64)";
            if (c.num_op >= n_ops || c.den_op >= n_ops) return who + " names an op beyond the program";
            if (joint && !is_cell(c.num_op))
                return who + " is a COUNT column with bit 8 of its pad whose num_op = " + std::to_string(c.num_op) + " is no list cell (op 12 names the looked-up values)";
            if (joint && list_len[c.num_op] > AIR_MAIN_COUNT_MAX_LIST) return who + " is a COUNT column with a list of more than 16 looked-up values";
            if (const uint8_t marks = chain_only[c.num_op] | chain_only[c.den_op]) return chain_only_refused(who, marks);
            const uint32_t r = std::max(reads[c.num_op], reads[c.den_op]);
            if (r > k) return who + " reads derived column " + std::to_string(r - 1) + ", which is not an earlier one";
            if (++n_count > AIR_MAIN_COUNT_MAX_COLS) return who + " is the program's COUNT column number " + std::to_string(n_count) + " (at most 16)";
            cols.push_back(AirMainColumnHost{c.kind, c.num_op, c.den_op, 0u, r, 0u, 0u, key_bits});
            cols.back().list_len = joint ? list_len[c.num_op] : 0u;
            continue;
        }
        if (c.kind == SP_AIR_MAIN_CHAIN) {
            const auto pos = [link](uint32_t pad) { return link ? (pad >> 8) & 255u : pad >> 8; };
            const uint32_t l = c.pad & 255u, j = pos(c.pad), kr = link ? c.pad >> 16 : 0u;   // kr: the k of a run of 2^k blocks
            if (k >= g_end) {   // it must open a group: the run of CHAIN columns with j = 1, 2, .. behind it
                if (j != 0) return who + " is a CHAIN column with j = " + std::to_string(j) + " out of sequence (no group is open: j = 0 opens one)";
                g0 = k; g_end = k + 1;
                while (g_end < m->n_cols && m->cols[g_end].kind == SP_AIR_MAIN_CHAIN && pos(m->cols[g_end].pad) != 0) {
                    const uint32_t jj = pos(m->cols[g_end].pad);
                    const std::string member = "main program: derived column " + std::to_string(g_end);
                    if (jj != g_end - g0) return member + " is a CHAIN column with j = " + std::to_string(jj) + " out of sequence (the next of its group is " + std::to_string(g_end - g0) + ")";
                    if (jj >= AIR_MAIN_CHAIN_MAX_WIDTH) return member + " makes its chain group longer than 16 columns";
                    ++g_end;
                }
            }
            if (l == 0 || l >= 64 || (1ull << l) > n) return who + " is a CHAIN column with l = " + std::to_string(l) + " (block length 2^l: 1 <= l and 2^l <= n)";
            if (l != (m->cols[g0].pad & 255u)) return who + " differs from its chain group in l (" + std::to_string(l) + " against " + std::to_string(m->cols[g0].pad & 255u) + ")";
            if (kr > AIR_MAIN_LINK_MAX_LOG) return who + " is a CHAIN column with k = " + std::to_string(kr) + " (runs of 2^k blocks: k <= " + std::to_string(AIR_MAIN_LINK_MAX_LOG) + ")";
            if (kr && (l + kr >= 64 || (1ull << (l + kr)) > n))
                return who + " is a CHAIN column with l + k = " + std::to_string(l + kr) + " (a run is 2^(l + k) rows: 2^(l + k) <= n)";
            if (link && kr != (m->cols[g0].pad >> 16)) return who + " differs from its chain group in k (" + std::to_string(kr) + " against " + std::to_string(m->cols[g0].pad >> 16) + ")";
            if (!den) return who + " is a CHAIN column without a seed (den_op names the seed op)";
            if (c.num_op >= n_ops || c.den_op >= n_ops) return who + " names an op beyond the program";
            const uint32_t r = std::max(reads[c.num_op], reads[c.den_op]);
            if (r > g_end) return who + " reads derived column " + std::to_string(r - 1) + ", which is not an earlier one";
            if (kr == 0 && reads[c.den_op] > g0) return who + " has a seed that loads derived column " + std::to_string(reads[c.den_op] - 1) + " of its own chain group";
            if (shifted[c.den_op] > g0)   // (k >= 1: a load of the group at shift 0 is the carry)
                return who + " has a seed that loads derived column " + std::to_string(shifted[c.den_op] - 1) + " of its own chain group at a shift other than 0";
            if (shifted[c.num_op] > g0)
                return who + " has a step that loads derived column " + std::to_string(shifted[c.num_op] - 1) + " of its own chain group at a shift other than 0";
            cols.push_back(AirMainColumnHost{c.kind, c.num_op, c.den_op, 0u, r, l, j, 0u, kr});
            continue;
        }
        if (c.num_op >= n_ops || (den && c.den_op >= n_ops)) return who + " names an op beyond the program";
        if (const uint8_t marks = chain_only[c.num_op] | (den ? chain_only[c.den_op] : 0)) return chain_only_refused(who, marks);
        if (den && (c.kind == SP_AIR_MAIN_INV_OR_ZERO || c.kind == SP_AIR_MAIN_BIT)) return who + " is an INV_OR_ZERO or a BIT and takes no denominator";
        if (c.kind == SP_AIR_MAIN_BIT && c.pad > 251) return who + " names bit " + std::to_string(c.pad) + " (0 .. 251)";
        const uint32_t r = std::max(reads[c.num_op], den ? reads[c.den_op] : 0u);
        if (r > k) return who + " reads derived column " + std::to_string(r - 1) + ", which is not an earlier one";
        cols.push_back(AirMainColumnHost{c.kind, c.num_op, c.den_op, c.kind == SP_AIR_MAIN_BIT ? c.pad : 0u, r});
    }
    out.input_cols = m->input_cols; out.input_location = m->input_location;
    out.ops.swap(ops);
    consts_from_c(m->consts, m->n_consts, out.consts);
    out.cols.swap(cols);
    return "";
}
}  // namespace

const char* const AIR_BOUNDARY_VALUES_MALFORMED = "malformed boundary values (ops 1 - 4 over earlier ops, each boundary < n_boundary and named once, num_op / den_op "
                                                  "inside the program, the bounds of sp_air_limits)";
bool air_boundary_from_c(const sp_air_boundary_desc* d, uint32_t n_boundary, uint32_t n_rap, AirBoundaryHost& out) {
    if (!d->ops || !d->consts || !d->values || d->n_ops == 0 || d->n_ops > AIR_LIMIT_OPS || d->n_consts > AIR_LIMIT_CONSTS ||
        (uint64_t)d->n_consts + n_rap > 65535 || d->n_values > AIR_LIMIT_BOUNDARY) return false;   // (all counts first: nothing is allocated for a descriptor that is refused)
    std::vector<AirOpHost> ops;
    ops_from_c(d->ops, d->n_ops, ops);
    // (no cell to LOAD, no OUT target, no periodic column: ops 1 - 4 are all that is left)
    if (air_program_first_bad_op(ops, 0, 0, (size_t)d->n_consts + n_rap, 0, 0) < ops.size()) return false;
    std::vector<uint32_t> named;
    for (uint32_t j = 0; j < d->n_values; ++j) {
        const sp_air_boundary_value& e = d->values[j];
        if (e.boundary >= n_boundary || e.num_op >= d->n_ops || (e.den_op != SP_AIR_AUX_NO_DEN && e.den_op >= d->n_ops)) return false;
        named.push_back(e.boundary);
    }
    std::sort(named.begin(), named.end());
    if (std::adjacent_find(named.begin(), named.end()) != named.end()) return false;
    out.ops.swap(ops);
    consts_from_c(d->consts, d->n_consts, out.consts);
    for (uint32_t j = 0; j < d->n_values; ++j) out.values.push_back(AirBoundaryValueHost{d->values[j].boundary, d->values[j].num_op, d->values[j].den_op});
    return true;
}

std::string air_statement_from_c(const sp_air_desc* d, const sp_air_aux_desc* aux, const sp_air_periodic_desc* periodic, const sp_air_stride_desc* strides,
                                 const sp_air_boundary_desc* bvals, bool aux_reads_periodic, uint64_t n, AirStatement& st, const sp_air_main_desc* main,
                                 AirMainLevel main_level) {
    AirDescHost& air = st.air;
    st.aux_reads_periodic = aux_reads_periodic;
    st.main_level = main_level;
    if (!air_desc_from_c(d, air)) return "malformed AIR descriptor (1 .. 8 frame rows, 1 .. 64 transition constraints, every count with its array)";
    if (periodic && !air_periodic_from_c(periodic, n, st.periodic.emplace()))
        return "malformed periodic columns (at most 64, each a power-of-two number of values, at most the trace length)";
    if (strides && !air_strides_from_c(strides, n, air))
        return "malformed strides (one per transition, a power-of-two period <= the trace length, offset < period, exemptions < n / period and degree <= "
               "degree_bound_factor for a period > 1, at most 4 classes and 4 exemption products)";
    if (aux && !aux_from_c(air, aux, st.aux.emplace()))
        return "malformed auxiliary program (needs aux_kind SP_AIR_AUX_PROGRAM and aux->n_cols == air->aux_cols >= 1, every count with its array, at most "
               "65535 ops and 4096 constants)";
    if (bvals && !air_boundary_from_c(bvals, d->n_boundary, d->n_rap, st.bvals.emplace())) return AIR_BOUNDARY_VALUES_MALFORMED;
    if (air.main_cols == 0 || (uint64_t)air.main_cols + air.aux_cols > AIR_LIMIT_COLS) return "column count out of range (1 .. 1024 columns, main + aux)";
    if (air.boundary.size() > AIR_LIMIT_BOUNDARY) return "more than 4096 boundary constraints";
    if (air.consts.size() > AIR_LIMIT_CONSTS) return "more than 4096 constants";
    if (air.consts.size() + air.n_rap > 65535) return "constants and RAP challenges exceed the 16-bit operand range";
    if (air.ops.size() > AIR_LIMIT_OPS) return "more than 65535 ops";
    if (main) {
        // (only the _rec, _lk, _link and _div entry points let a main program hold chain columns and read the periodic columns, only
        // _lk, _link and _div COUNT columns, only _link and _div runs of blocks, only _div quotients behind chain seeds and steps; the
        // _fetch entry points all of that and FETCH columns, the _word entry points LIMB and WORD columns on top, the _int entry points
        // ops 8 .. 11 behind chain seeds and steps on top of that)
        const std::string refused = main_from_c(air, main, n, st.n_periodic(), st.main_level, st.main.emplace());
        if (!refused.empty()) return refused;
    }
    // (only the _pub entry points let an auxiliary program read the periodic columns: 0 of them from everywhere else)
    if (st.aux) {
        const std::string refused = validate_aux_program(*st.aux, air.main_cols, air.n_rap, st.aux_periodic() ? st.n_periodic() : 0u);
        if (!refused.empty()) return refused;
    }
    if (st.main && air.aux_kind != 0 && air.aux_kind != SP_AIR_AUX_PROGRAM) {
        st.unsupported = true;
        return "a main program needs aux_kind 0 or SP_AIR_AUX_PROGRAM (kinds 1 and 2 build the auxiliary segment from a host table of the main segment)";
    }
    return "";
}

bool air_resolve_boundary(const AirBoundaryHost& bvals, const std::vector<fe>& rap, std::vector<fe>& values) {
    const size_t nc = bvals.consts.size();
    std::vector<fe> v(bvals.ops.size());
    for (size_t t = 0; t < bvals.ops.size(); ++t) {
        const AirOpHost& o = bvals.ops[t];
        switch (o.op) {
            case 1: v[t] = o.a < nc ? bvals.consts[o.a] : rap[o.a - nc]; break;
            case 2: v[t] = fe_add(v[o.a], v[o.b]); break;
            case 3: v[t] = fe_sub(v[o.a], v[o.b]); break;
            default: v[t] = fe_mul(v[o.a], v[o.b]); break;
        }
    }
    std::vector<fe> dens;
    for (const AirBoundaryValueHost& e : bvals.values)
        if (e.den_op != SP_AIR_AUX_NO_DEN) {
            if (fe_is_zero(v[e.den_op])) return false;
            dens.push_back(v[e.den_op]);
        }
    if (!dens.empty()) host_batch_inverse(dens);
    values.clear();
    size_t d = 0;
    for (const AirBoundaryValueHost& e : bvals.values)
        values.push_back(e.den_op != SP_AIR_AUX_NO_DEN ? fe_mul(v[e.num_op], dens[d++]) : v[e.num_op]);
    return true;
}

bool air_resolve_boundary_into(const AirBoundaryHost& bvals, const std::vector<fe>& rap, std::vector<BoundaryConstraint>& boundary) {
    std::vector<fe> values;
    if (!air_resolve_boundary(bvals, rap, values)) return false;
    for (size_t j = 0; j < values.size(); ++j) boundary[bvals.values[j].boundary].value = values[j];
    return true;
}

// q from its values on <w_p>: an in-place radix-2 inverse transform (bit-reversal, then butterflies with w_p^-1), times 1/p
std::vector<fe> air_periodic_interpolate(const std::vector<fe>& values) {
    const size_t p = values.size();
    const int lp = sp_log2_exact(p);
    if (lp < 0) throw std::runtime_error("malformed: periodic column period");
    std::vector<fe> a(p);
    for (size_t i = 0; i < p; ++i) {
        size_t r = 0;
        for (int bit = 0; bit < lp; ++bit) r |= ((i >> bit) & 1) << (lp - 1 - bit);
        a[r] = values[i];
    }
    const fe winv = lp ? fe_inv(air_root_of_unity(lp)) : fe_one();
    for (int s = 1; s <= lp; ++s) {
        const size_t m = size_t(1) << s, half = m >> 1;
        const fe wm = fe_pow_u64(winv, p / m);
        std::vector<fe> tw(half);
        tw[0] = fe_one();
        for (size_t j = 1; j < half; ++j) tw[j] = fe_mul(tw[j - 1], wm);
        for (size_t k = 0; k < p; k += m)
            for (size_t j = 0; j < half; ++j) {
                const fe t = fe_mul(tw[j], a[k + j + half]), u = a[k + j];
                a[k + j] = fe_add(u, t);
                a[k + j + half] = fe_sub(u, t);
            }
    }
    const fe pinv = fe_inv(fe_from_u64(p));
    for (auto& x : a) x = fe_mul(x, pinv);
    return a;
}

fe air_periodic_eval(const std::vector<fe>& coeffs, uint64_t n, const fe& point) {
    const fe y = fe_pow_u64(point, n / coeffs.size());
    fe acc = fe_zero();
    for (size_t m = coeffs.size(); m-- > 0;) acc = fe_add(fe_mul(acc, y), coeffs[m]);
    return acc;
}

bool air_stride_plan(const AirDescHost& air, uint64_t n, AirStridePlan& out) {
    const size_t T = air.exemptions.size();
    out = AirStridePlan{};
    out.cls.assign(T, -1); out.kind.assign(T, -1);
    if (air.strides.empty()) return true;
    if (air.strides.size() != T) return false;
    for (size_t k = 0; k < T; ++k) {
        const uint32_t s = air.strides[k].period, o = air.strides[k].offset, e = air.exemptions[k];
        if (s == 0 || (s & (s - 1)) || s > n || o >= s) return false;
        if (s == 1) continue;
        // C_k / Z_k has degree d n - n/s: the adjustment x^(n (f - d) + n/s) exists for d <= f only (a (1, 0) constraint may have d = f + 1)
        if (e >= n / s || k >= air.degrees.size() || air.degrees[k] > air.degree_bound_factor) return false;
        size_t q = 0;
        while (q < out.classes.size() && (out.classes[q].period != s || out.classes[q].offset != o)) ++q;
        if (q == out.classes.size()) {
            if (q == AIR_MAX_STRIDE_CLASSES) return false;
            out.classes.push_back(air.strides[k]);
        }
        out.cls[k] = (int)q;
        if (!e) continue;
        const std::pair<uint32_t, uint32_t> want((uint32_t)q, e);
        size_t j = 0;
        while (j < out.kinds.size() && out.kinds[j] != want) ++j;
        if (j == out.kinds.size()) {
            if (j == AIR_MAX_STRIDE_EXEMPT_KINDS) return false;
            out.kinds.push_back(want);
        }
        out.kind[k] = (int)j;
    }
    return true;
}

void air_stride_eval(uint32_t s, uint32_t o, uint32_t e, uint64_t n, const fe& x, fe& Z, fe& E) {
    const uint64_t m = n / s;                       // rows of the progression
    const fe g = air_root_of_unity(sp_log2_exact(n));
    Z = fe_sub(fe_pow_u64(x, m), fe_pow_u64(g, (uint64_t)o * m));
    E = fe_one();
    const fe gs_inv = fe_inv(fe_pow_u64(g, s));
    fe root = fe_pow_u64(g, o + (uint64_t)s * (m - 1));   // the last row of the progression, then s rows down at a time
    for (uint32_t t = 0; t < e; ++t) {
        E = fe_mul(E, fe_sub(x, root));
        root = fe_mul(root, gs_inv);
    }
}

}  // namespace sp
