// The column builders of a program AIR (see prover.h): the auxiliary segment from the statement's auxiliary program and the main
// segment from its main-trace program, each as one upload block, one workspace and a sequence of launches on the context stream.
// Host code only.
#include "prover_internal.h"
#include "sort_kernels.h"
#include <array>
#include <cstddef>
#include <cstring>

namespace sp {

// Chunks of columns bound the workspace: a chunk holds at most max(1, AUXP_CHUNK_ELEMS / n) columns, so its denominators take
// at most max(2^22, n) elements (128 MB up to 2^22 rows, 32 bytes a row beyond) and the batch inversion as much scratch again,
// whatever the number of auxiliary columns.  The numerators are written straight into the trace columns they become.
// Sorted columns (SP_AIR_AUX_SORTED) come first, one sort group at a time in the same workspace: the carried values of a group go
// through it at most a chunk's worth of columns per pass, beside the (key, row) pairs and the radix sort's histograms (24 bytes a row).
// A chunk of products and sums is a run of such columns: a sorted column ends it.
static constexpr uint64_t AUXP_CHUNK_ELEMS = 1ull << 22;

// The program `src` with an OUT behind every op whose value is wanted - outs[t]: the codes op t is stored under - (a value then lives
// only until it is stored), slots by air_assign_slots (which drops what these OUTs do not need).  reads_periodic: an op 6 is among
// what air_assign_slots kept, a table read that feeds one of these OUTs; divides: an op 7 is among them, a quotient that does; integers:
// an op 8 .. 11 is, an integer function that does.
static int program_with_outs(const std::vector<AirOpHost>& src, const std::vector<std::vector<uint32_t>>& outs, const char* live_error,
                             std::vector<AirOpDev>& dev, bool& reads_periodic, bool& divides, bool& integers) {
    std::vector<AirOpHost> ext;
    std::vector<uint32_t> at(src.size());
    for (size_t t = 0; t < src.size(); ++t) {
        AirOpHost o = src[t];
        // (a list cell of a joint COUNT column: a leaf that holds a list, no value - never uploaded.  Its at[t] stays 0 and must never be
        // read: the decoder lets no value op and no OUT name a cell, so nothing below remaps an operand through it)
        if (o.op == AIR_OP_ALSO) continue;
        if (air_op_takes_two_values(o.op)) { o.a = at[o.a]; o.b = at[o.b]; }   // (LOAD, CONST and PERIODIC name cells, not values)
        else if (air_op_takes_one_value(o.op)) o.a = at[o.a];                  // (an integer LIMB: b is lo + 256 width)
        at[t] = (uint32_t)ext.size();
        ext.push_back(o);
        for (uint32_t code : outs[t]) ext.push_back(AirOpHost{5, code, at[t]});
    }
    SP_TRY(air_assign_slots(ext, dev, live_error));
    reads_periodic = divides = integers = false;
    for (const AirOpDev& o : dev) { reads_periodic |= o.op == 6; divides |= o.op == 7; integers |= air_op_is_integer(o.op); }
    return SP_OK;
}

// The periodic columns an op 6 of a column program reads, in the program's own upload block (round 2's block comes too late), as
// round 2's block holds them: AirPeriodicCol[] and the raw values, column k at pvals + off_k.  Placed last, and only when some
// program reads op 6 (src = null otherwise: nothing is placed and the device pointers are null).
struct PeriodicUpload {
    const AirPeriodicHost* src = nullptr;
    std::vector<AirPeriodicCol> cols;
    size_t o_cols = 0, o_vals = 0;
    void place(UploadLayout& lay, const AirPeriodicHost* periodic) {
        src = periodic;
        if (!src) return;
        uint64_t S = 0;
        for (const std::vector<fe>& c : src->cols) {
            cols.push_back(AirPeriodicCol{(uint32_t)sp_log2_exact(c.size()), 0u, S});
            S += c.size();
        }
        o_cols = lay.place(sizeof(AirPeriodicCol) * cols.size());
        o_vals = lay.place(sizeof(fe) * S);
    }
    void fill(uint8_t* up) const {
        if (!src) return;
        std::memcpy(up + o_cols, cols.data(), sizeof(AirPeriodicCol) * cols.size());
        for (size_t k = 0; k < cols.size(); ++k) std::memcpy(up + o_vals + sizeof(fe) * cols[k].off, src->cols[k].data(), sizeof(fe) * src->cols[k].size());
    }
    const AirPeriodicCol* cols_dev(const uint8_t* block) const { return src ? reinterpret_cast<const AirPeriodicCol*>(block + o_cols) : nullptr; }
    const fe* vals_dev(const uint8_t* block) const { return src ? reinterpret_cast<const fe*>(block + o_vals) : nullptr; }
};

// What k radix sorts of n (key, row) pairs take, carved from `base`: k arrays of keys, k of rows, the sort's histograms.
struct SortScratch {
    static constexpr uint32_t MAX = 4;
    uint64_t* keys[MAX];
    uint32_t* rows[MAX];
    void* radix;
    static uint64_t keys_el(uint64_t n) { return (n + 3) / 4; }   // (in units of 32 bytes, as the workspace is counted)
    static uint64_t rows_el(uint64_t n) { return (n + 7) / 8; }
    static uint64_t elems(uint64_t n, uint32_t k) { return k * keys_el(n) + k * rows_el(n) + (radix_sort_workspace_bytes(n) + sizeof(fe) - 1) / sizeof(fe); }
    SortScratch(fe* base, uint64_t n, uint32_t k) {
        for (uint32_t j = 0; j < k; ++j) {
            keys[j] = reinterpret_cast<uint64_t*>(base + j * keys_el(n));
            rows[j] = reinterpret_cast<uint32_t*>(base + k * keys_el(n) + j * rows_el(n));
        }
        radix = base + k * keys_el(n) + k * rows_el(n);
    }
};

// The group of this key, appended if new: columns that share an operand share one pass over it (BIT and LIMB columns their N, WORD
// columns N, D and bits, sorted columns their key).  A linear search: a chunk has few groups.
template <class Group, class Key>
static Group& group_of(std::vector<Group>& groups, const Key& key) {
    for (Group& g : groups)
        if (g.key == key) return g;
    groups.emplace_back();
    groups.back().key = key;
    return groups.back();
}

int StarkProver::commit_aux_program(const AirStatement& st, const std::vector<fe>& rap, uint8_t root_out[32]) {
    const AirAuxHost& aux = *st.aux;
    const uint32_t K = (uint32_t)aux.cols.size();
    if (stage_ != Stage::MainCommitted || K == 0 || K != Ca_) { sp_set_error("commit_aux_program: main segment not committed or auxiliary column count differs"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(K, AUXP_CHUNK_ELEMS / n_));
    const uint64_t nb = air_aux_scan_blocks(n_);
    const uint32_t n_src = (uint32_t)aux.ops.size();
    bool any_periodic = false;
    auto program = [&](const std::vector<std::vector<uint32_t>>& outs, std::vector<AirOpDev>& dev, bool& reads_periodic) -> int {
        bool divides = false, integers = false;   // (never: validate_aux_program knows no op 7 .. 11)
        SP_TRY(program_with_outs(aux.ops, outs, "aux program: more than 64 values alive at once", dev, reads_periodic, divides, integers));
        any_periodic |= reads_periodic;
        return SP_OK;
    };
    // --- per sort group: its key columns (rebuilt from the sorted keys) and its carried columns in passes of at most `chunk`; the
    //     first pass also stores the key (OUT AIR_AUX_DEN_TAG)
    struct SortPass { bool periodic; std::vector<AirOpDev> ops; std::vector<uint32_t> col_of; size_t o_ops, o_col; };
    struct SortGroup { uint32_t key = 0, key_bits = 0; std::vector<uint32_t> key_cols, carried; std::vector<SortPass> passes; size_t o_keycol = 0; };   // key: its op
    std::vector<SortGroup> groups;
    for (uint32_t k = 0; k < K; ++k) {
        const AirAuxColumnHost& c = aux.cols[k];
        if (c.kind != SP_AIR_AUX_SORTED) continue;
        SortGroup& g = group_of(groups, c.den_op);
        if (g.key_cols.empty() && g.carried.empty()) g.key_bits = c.key_bits;   // (the group's first column)
        (c.num_op == c.den_op ? g.key_cols : g.carried).push_back(k);
    }
    uint32_t max_carried = 0;
    for (SortGroup& g : groups) {
        for (size_t j0 = 0; j0 == 0 || j0 < g.carried.size(); j0 += chunk) {
            SortPass ps{};
            std::vector<std::vector<uint32_t>> outs(n_src);
            for (size_t j = j0; j < std::min<size_t>(g.carried.size(), j0 + chunk); ++j) {
                outs[aux.cols[g.carried[j]].num_op].push_back((uint32_t)ps.col_of.size());
                ps.col_of.push_back(g.carried[j]);
            }
            if (j0 == 0) outs[g.key].push_back(AIR_AUX_DEN_TAG);
            SP_TRY(program(outs, ps.ops, ps.periodic));
            max_carried = std::max(max_carried, (uint32_t)ps.col_of.size());
            g.passes.push_back(std::move(ps));
        }
    }
    if (!groups.empty() && n_ >= (1ull << 32)) { sp_set_error("commit_aux_program: sorted columns need a trace of fewer than 2^32 rows"); return SP_E_INVALID_ARG; }
    // --- per chunk of products and sums: its N and D
    struct Chunk { uint32_t k0, kc, n_den; bool periodic; std::vector<AirOpDev> ops; std::vector<uint32_t> kinds, col_of; size_t o_ops, o_kinds, o_col; };
    std::vector<Chunk> chunks;
    uint32_t max_den = 0;
    for (uint32_t k0 = 0; k0 < K;) {
        if (aux.cols[k0].kind == SP_AIR_AUX_SORTED) { ++k0; continue; }
        Chunk ch{};
        ch.k0 = k0;
        std::vector<std::vector<uint32_t>> outs(n_src);
        for (; ch.kc < chunk && k0 + ch.kc < K && aux.cols[k0 + ch.kc].kind != SP_AIR_AUX_SORTED; ++ch.kc) {
            const AirAuxColumnHost& c = aux.cols[k0 + ch.kc];
            ch.kinds.push_back(c.kind);
            outs[c.num_op].push_back(ch.kc);
            if (c.den_op != SP_AIR_AUX_NO_DEN) { outs[c.den_op].push_back(AIR_AUX_DEN_TAG + ch.n_den); ch.col_of.push_back(ch.kc); ++ch.n_den; }
        }
        SP_TRY(program(outs, ch.ops, ch.periodic));
        max_den = std::max(max_den, ch.n_den);
        k0 += ch.kc;
        chunks.push_back(std::move(ch));
    }
    // --- one upload: constants (then the RAP challenges), per sort pass its ops and value -> column table, per chunk its ops, column
    //     kinds and denominator -> column table, the periodic columns a program reads
    UploadLayout lay;
    const size_t o_consts = lay.place(sizeof(fe) * std::max<size_t>(1, aux.consts.size() + rap.size()));
    for (SortGroup& g : groups) {
        g.o_keycol = lay.place(sizeof(uint32_t) * std::max<size_t>(1, g.key_cols.size()));
        for (SortPass& ps : g.passes) {
            ps.o_ops = lay.place(sizeof(AirOpDev) * ps.ops.size());
            ps.o_col = lay.place(sizeof(uint32_t) * std::max<size_t>(1, ps.col_of.size()));
        }
    }
    for (Chunk& ch : chunks) {
        ch.o_ops = lay.place(sizeof(AirOpDev) * ch.ops.size());
        ch.o_kinds = lay.place(sizeof(uint32_t) * ch.kc);
        ch.o_col = lay.place(sizeof(uint32_t) * std::max<uint32_t>(1, ch.n_den));
    }
    PeriodicUpload per;
    per.place(lay, any_periodic ? st.aux_periodic() : nullptr);
    const size_t bytes = lay.bytes;
    SP_TRY(grow(od_.auxp_buf, bytes));
    std::vector<uint8_t>& up = h_auxp_up_;
    up.assign(bytes, 0);
    fill_consts_then_rap(up.data() + o_consts, aux.consts, rap);
    for (const SortGroup& g : groups) {
        if (!g.key_cols.empty()) std::memcpy(up.data() + g.o_keycol, g.key_cols.data(), sizeof(uint32_t) * g.key_cols.size());
        for (const SortPass& ps : g.passes) {
            std::memcpy(up.data() + ps.o_ops, ps.ops.data(), sizeof(AirOpDev) * ps.ops.size());
            if (!ps.col_of.empty()) std::memcpy(up.data() + ps.o_col, ps.col_of.data(), sizeof(uint32_t) * ps.col_of.size());
        }
    }
    for (const Chunk& ch : chunks) {
        std::memcpy(up.data() + ch.o_ops, ch.ops.data(), sizeof(AirOpDev) * ch.ops.size());
        std::memcpy(up.data() + ch.o_kinds, ch.kinds.data(), sizeof(uint32_t) * ch.kc);
        if (ch.n_den) std::memcpy(up.data() + ch.o_col, ch.col_of.data(), sizeof(uint32_t) * ch.n_den);
    }
    per.fill(up.data());
    SP_HIP_CHECK(hipMemcpyAsync(od_.auxp_buf.p, up.data(), bytes, hipMemcpyHostToDevice, c_->stream));
    // --- workspace, whichever of the two uses is larger (the sorts are over before the first chunk starts):
    //     chunks: [max_den][n] denominators, as much batch-inversion scratch, [chunk][nb] scan block totals
    //     sorts:  [max_carried][n] carried values, 2 x [n] keys, 2 x [n] rows, the radix sort's histograms (all in units of 32 bytes)
    const uint64_t ws_sort = groups.empty() ? 0 : (uint64_t)max_carried * n_ + SortScratch::elems(n_, 2);
    const uint64_t ws = std::max(2 * (uint64_t)max_den * n_ + (uint64_t)chunk * nb, ws_sort);
    SP_TRY(grow(od_.auxp_ws, ws));
    const fe* consts_dev = reinterpret_cast<const fe*>(od_.auxp_buf.p + o_consts);
    const AirPeriodicCol* pcols_dev = per.cols_dev(od_.auxp_buf.p);
    const fe* pvals_dev = per.vals_dev(od_.auxp_buf.p);
    fe* aux_cols = d_trace_ + (uint64_t)Cm_ * n_;
    SP_TRY(ensure_host_flags());
    host_flags().auxp_bad_key = 0;
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    if (!groups.empty()) {
        fe* vals = od_.auxp_ws.p;
        const SortScratch s(vals + (uint64_t)max_carried * n_, n_, 2);
        for (const SortGroup& g : groups)
            for (size_t p = 0; p < g.passes.size(); ++p) {
                const SortPass& ps = g.passes[p];
                SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, reinterpret_cast<const AirOpDev*>(od_.auxp_buf.p + ps.o_ops), (uint32_t)ps.ops.size(), consts_dev, vals,
                                          p == 0 ? s.keys[0] : nullptr, p == 0 ? s.rows[0] : nullptr, g.key_bits, c_->d_flag, ps.periodic ? pcols_dev : nullptr,
                                          ps.periodic ? pvals_dev : nullptr));
                if (p == 0) {   // ceil(key_bits / 8) passes; the sorted pairs end up in keys[1] / rows[1]
                    SP_TRY(radix_sort_pairs_u64(c_->stream, s.keys[0], s.keys[1], s.rows[0], s.rows[1], n_, g.key_bits, s.radix));
                    SP_TRY(air_aux_key_columns(c_->stream, s.keys[1], n_, aux_cols, reinterpret_cast<const uint32_t*>(od_.auxp_buf.p + g.o_keycol), (uint32_t)g.key_cols.size()));
                }
                SP_TRY(air_aux_gather(c_->stream, vals, s.rows[1], n_, aux_cols, reinterpret_cast<const uint32_t*>(od_.auxp_buf.p + ps.o_col), (uint32_t)ps.col_of.size()));
            }
        // the key-range flag rides to the host from here: a zero denominator behind it overwrites the word on the device
        SP_HIP_CHECK(hipMemcpyAsync(&host_flags().auxp_bad_key, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    }
    fe* den = od_.auxp_ws.p;
    fe* scratch = den + (uint64_t)max_den * n_;
    fe* block_tot = scratch + (uint64_t)max_den * n_;
    for (const Chunk& ch : chunks) {
        fe* cols = aux_cols + (uint64_t)ch.k0 * n_;
        const uint32_t* kinds = reinterpret_cast<const uint32_t*>(od_.auxp_buf.p + ch.o_kinds);
        SP_TRY(air_aux_terms(c_->stream, d_trace_, n_, reinterpret_cast<const AirOpDev*>(od_.auxp_buf.p + ch.o_ops), (uint32_t)ch.ops.size(), consts_dev, cols, den,
                             ch.periodic ? pcols_dev : nullptr, ch.periodic ? pvals_dev : nullptr));
        if (ch.n_den) {
            SP_TRY(batch_inverse(c_->stream, den, scratch, (uint64_t)ch.n_den * n_, c_->d_flag));
            SP_TRY(air_aux_apply_den(c_->stream, cols, den, reinterpret_cast<const uint32_t*>(od_.auxp_buf.p + ch.o_col), ch.n_den, n_));
        }
        SP_TRY(air_aux_scan(c_->stream, cols, n_, ch.kc, kinds, block_tot));
    }
    // the zero-denominator flag rides behind the columns; the read-back of the root below waits for it (and for the key-range flag)
    SP_HIP_CHECK(hipMemcpyAsync(&host_flags().auxp_zero_den, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    SP_TRY(commit_segment_resident(1, K, root_out));
    if (host_flags().auxp_bad_key == AIR_AUX_FLAG_KEY_RANGE) {
        sp_set_error("commit_aux_program: a sort key is out of range on some row (the key of a sorted column must be below 2^key_bits as a canonical integer)");
        return SP_E_INVALID_ARG;
    }
    if (host_flags().auxp_zero_den) { sp_set_error("commit_aux_program: an auxiliary column's denominator is zero on some row"); return SP_E_ZERO_INVERSE; }
    return SP_OK;
}

// ---- the main-trace program -----------------------------------------------------------------------------------------------------
// Chunks as above (at most max(1, AUXP_CHUNK_ELEMS / n) columns), and a chunk also ends before a column that reads a derived column
// of the chunk itself: LOADs wrap around the trace, so a column must be complete - its scan included - before anything reads it, and
// the stream orders one chunk behind the other.  od_.auxp_buf / od_.auxp_ws: the auxiliary program runs later on the same stream.
// A chunk places the programs and word tables its kind fills in the upload block, and no others.
struct MainChunk {
    // RowLocal: one pass of the interpreter (air_aux_terms), then what each column kind needs on top.  Workspace slots, n elements
    //   each: first the ones the batch inversion takes (the D of VALUE / SUM / PRODUCT columns, the guarded N of INV_OR_ZERO columns),
    //   then one per group of BIT columns that share their N, one per group of LIMB columns that share their N, and two (N, then D) per
    //   group of WORD columns that share N, D and bits.
    // Chain: a chain group (SP_AIR_MAIN_CHAIN), a chunk of its own that ends the chunk before it: the seeds' program and the steps',
    //   each with an OUT per group column, and one launch of air_main_chain - a lane per block, or per run of 2^log_k blocks of a
    //   linked group; nothing of the group is read before that launch is over, which the stream's order guarantees.  No workspace.
    //   A group whose programs hold an op 7 (divides) hands the launch the zero-denominator flag the batch inversions share, one
    //   whose programs hold an op 8 .. 11 (integers) the range flag the WORD columns share.
    // Count: a COUNT column (SP_AIR_MAIN_COUNT), a chunk of its own too: X's program and T's, each with the one OUT of a key pass; two
    //   launches of air_aux_sort_terms (keys out of Montgomery form, the row beside each), two radix sorts - the table's carries its
    //   rows - and one launch of air_main_count, which writes every cell of the column.  Its arrays (4 x [n] keys, 4 x [n] rows, the
    //   radix histograms) lie at the start of the workspace: the chunk before it is over, the chunk behind it starts after the count.
    // Fetch: a run of at most AIR_MAIN_FETCH_MAX_GROUP consecutive FETCH columns (SP_AIR_MAIN_FETCH) with one X, one T and one key_bits,
    //   none of which reads a derived column of the run; a chunk of its own that ends the chunk before it.  X's program and T's, each
    //   with the one OUT of a key pass, and V's with an OUT per group column: two launches of air_aux_sort_terms - X's pairs stay in row
    //   order -, one of air_aux_terms into kc workspace slots, one radix sort of the table's pairs and one launch of air_main_fetch,
    //   which writes every cell of the group.  Its arrays (3 x [n] keys, 3 x [n] rows, the radix histograms) lie at the start of the
    //   workspace, the kc slots behind them.
    // CountMany: a joint COUNT column (bit 8 of its pad: one multiplicity column for the L looked-up values of a list), a chunk of
    //   its own as a COUNT column is.  T's program with the one OUT of a key pass and the L looked-up values' with an OUT each: one
    //   launch of air_aux_sort_terms and one radix sort - the table's, the only sort -, one launch of air_main_list_keys and
    //   air_main_count_many, which searches the sorted table from every looked-up key, adds into n 64-bit counters (zeroed on the
    //   stream on every run) and writes every cell of the column.  Its arrays (2 x [n] keys, 2 x [n] rows, the radix histograms, then
    //   L x [n] keys and [n] counters) lie at the start of the workspace.
    enum class Kind { RowLocal, Chain, Count, Fetch, CountMany };
    static constexpr int N_PROG = 3;
    static constexpr int TERMS = 0, STEP = 0, SEED = 1, KEY_X = 0, KEY_T = 1, TABLE_V = 2;   // which of prog[] a kind's programs are
    Kind kind = Kind::RowLocal;
    uint32_t k0 = 0, kc = 0;                 // derived columns [k0, k0 + kc)
    std::vector<AirOpDev> prog[N_PROG];      // in upload order: RowLocal TERMS (and none); Chain STEP, SEED; Count KEY_X, KEY_T; Fetch those and TABLE_V
    size_t o_prog[N_PROG] = {0, 0, 0};
    bool periodic = false;                   // one of the chunk's programs reads a periodic column
    // RowLocal
    uint32_t n_inv = 0, n_slots = 0;                              // n_inv: slots the batch inversion takes; n_slots: those and the BIT, LIMB and WORD groups'
    // KINDS: 0 product / 1 sum per column (read for scanned columns only); DEN_COL: air_aux_apply_den's table; GUARD: air_main_zero_guard's;
    // BIT_G / BIT_E, LIMB_G / LIMB_E and WORD_G / WORD_E: the group and entry tables of air_main_bits, air_main_limbs and air_main_words
    enum Tab { KINDS, DEN_COL, GUARD, BIT_G, BIT_E, LIMB_G, LIMB_E, WORD_G, WORD_E, N_TAB };
    std::vector<uint32_t> tab[N_TAB];
    size_t o_tab[N_TAB] = {};
    std::vector<std::pair<uint32_t, uint32_t>> scans;            // runs of SUM / PRODUCT columns: (first, count)
    // Chain
    uint32_t log_s = 0, log_k = 0;           // blocks of 2^log_s rows; log_k >= 1: runs of 2^log_k blocks
    bool divides = false;                    // the slotted seed or step program holds an op 7: the launch takes the zero flag
    bool integers = false;                   // it holds an op 8 .. 11: the launch takes the range flag
    // Count, Fetch, CountMany
    uint32_t key_bits = 0;
    // CountMany
    uint32_t n_lists = 0;                    // L, the looked-up values of the list
};

struct MainPlan {
    std::vector<MainChunk> chunks;
    uint32_t chunk = 0, max_slots = 0, max_inv = 0;
    bool any_count = false, any_fetch = false, any_word = false, any_int = false;   // (any_count: COUNT columns of either form)
    bool any_plain_count = false;            // a COUNT column of the old form: its four pair sets
    bool any_verdict() const { return any_count || any_fetch || any_word || any_int; }   // the three verdict words behind the workspace are in use
    uint32_t max_fetch = 0;                  // the widest FETCH group
    uint32_t max_lists = 0;                  // the longest list of a joint COUNT column (0: none)
    size_t o_consts = 0, bytes = 0;          // the upload block: the constants, per chunk its programs and tables, the periodic columns
    PeriodicUpload per;
    uint64_t ws_elems = 0;                   // the workspace; the three verdict words lie behind it
};

// Planning: the chunks and their programs, the upload block's layout and the workspace's size.  No HIP call.
static int plan_main_program(const AirStatement& st, uint64_t n, MainPlan& P) {
    const AirMainHost& mp = *st.main;
    const uint32_t K = (uint32_t)mp.cols.size(), n_src = (uint32_t)mp.ops.size();
    P.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(K, AUXP_CHUNK_ELEMS / n));
    bool any_periodic = false;
    // (a chunk's programs share one flag)
    auto program = [&](const std::vector<std::vector<uint32_t>>& outs, MainChunk& ch, int which) -> int {
        bool reads_periodic = false, divides = false, integers = false;
        SP_TRY(program_with_outs(mp.ops, outs, "main program: more than 64 values alive at once", ch.prog[which], reads_periodic, divides, integers));
        ch.periodic |= reads_periodic;
        any_periodic |= reads_periodic;
        // (only the chain kernel's DIV instantiations know op 7, and only the statement's level lets it in)
        if (divides && (ch.kind != MainChunk::Kind::Chain || !air_main_allows_quotients(st.main_level))) {
            sp_set_error("commit_main_program: op 7 outside a chain group's programs (the decoder should have refused it)");
            return SP_E_INVALID_ARG;
        }
        ch.divides |= divides;
        // (nor does anything else know ops 8 .. 11: the chain kernel's INT instantiations alone)
        if (integers && (ch.kind != MainChunk::Kind::Chain || !air_main_allows_int_ops(st.main_level))) {
            sp_set_error("commit_main_program: an integer op (8 .. 11) outside a chain group's programs (the decoder should have refused it)");
            return SP_E_INVALID_ARG;
        }
        ch.integers |= integers;
        P.any_int |= integers;
        return SP_OK;
    };
    for (uint32_t k0 = 0; k0 < K;) {
        MainChunk ch;
        ch.k0 = k0;
        std::vector<std::vector<uint32_t>> outs(n_src);
        if (mp.cols[k0].kind == SP_AIR_MAIN_CHAIN) {   // the whole group (the decoder saw to j = 0, 1, .. and one l)
            std::vector<std::vector<uint32_t>> seeds(n_src);
            ch.kind = MainChunk::Kind::Chain;
            ch.log_s = mp.cols[k0].chain_log;
            ch.log_k = mp.cols[k0].chain_link;
            do {
                const AirMainColumnHost& c = mp.cols[k0 + ch.kc];
                seeds[c.den_op].push_back(ch.kc);
                outs[c.num_op].push_back(ch.kc);
                ++ch.kc;
            } while (k0 + ch.kc < K && mp.cols[k0 + ch.kc].kind == SP_AIR_MAIN_CHAIN && mp.cols[k0 + ch.kc].chain_pos != 0);
            if (ch.kc > AIR_MAIN_CHAIN_WIDTH || ch.log_s + ch.log_k >= 64 || n >> (ch.log_s + ch.log_k) == 0) { sp_set_error("commit_main_program: a chain group the decoder should have refused"); return SP_E_INVALID_ARG; }
            SP_TRY(program(seeds, ch, MainChunk::SEED));
            SP_TRY(program(outs, ch, MainChunk::STEP));
        } else if (mp.cols[k0].kind == SP_AIR_MAIN_COUNT && mp.cols[k0].list_len) {
            const AirMainColumnHost& c = mp.cols[k0];
            std::vector<std::vector<uint32_t>> table(n_src);
            bool fine = air_main_allows_lists(st.main_level) && c.key_bits >= 1 && c.key_bits <= 64 && c.den_op < n_src && c.list_len <= AIR_MAIN_COUNT_MAX_LIST;
            uint32_t cell = c.num_op;
            for (uint32_t k = 0; fine && k < c.list_len; ++k) {   // X_k is the a of the k-th cell; the last cell's b ends the list
                fine = cell < n_src && mp.ops[cell].op == AIR_OP_ALSO && mp.ops[cell].a < n_src;
                if (!fine) break;
                outs[mp.ops[cell].a].push_back(AIR_AUX_DEN_TAG + k);
                cell = mp.ops[cell].b;
            }
            if (!fine || cell != AIR_LIST_END) { sp_set_error("commit_main_program: a joint COUNT column the decoder should have refused"); return SP_E_INVALID_ARG; }
            table[c.den_op].push_back(AIR_AUX_DEN_TAG);
            ch.kind = MainChunk::Kind::CountMany;
            ch.kc = 1;
            ch.key_bits = c.key_bits;
            ch.n_lists = c.list_len;
            SP_TRY(program(outs, ch, MainChunk::KEY_X));
            SP_TRY(program(table, ch, MainChunk::KEY_T));
            P.any_count = true;
            P.max_lists = std::max(P.max_lists, ch.n_lists);
        } else if (mp.cols[k0].kind == SP_AIR_MAIN_COUNT) {
            const AirMainColumnHost& c = mp.cols[k0];
            std::vector<std::vector<uint32_t>> table(n_src);
            if (c.key_bits == 0 || c.key_bits > 64 || c.den_op >= n_src) { sp_set_error("commit_main_program: a COUNT column the decoder should have refused"); return SP_E_INVALID_ARG; }
            outs[c.num_op].push_back(AIR_AUX_DEN_TAG);
            table[c.den_op].push_back(AIR_AUX_DEN_TAG);
            ch.kind = MainChunk::Kind::Count;
            ch.kc = 1;
            ch.key_bits = c.key_bits;
            SP_TRY(program(outs, ch, MainChunk::KEY_X));
            SP_TRY(program(table, ch, MainChunk::KEY_T));
            P.any_count = P.any_plain_count = true;
        } else if (mp.cols[k0].kind == SP_AIR_MAIN_FETCH) {
            const AirMainColumnHost& c = mp.cols[k0];
            std::vector<std::vector<uint32_t>> table(n_src), values(n_src);
            if (c.key_bits == 0 || c.key_bits > 64 || c.num_op >= n_src || c.den_op >= n_src) { sp_set_error("commit_main_program: a FETCH column the decoder should have refused"); return SP_E_INVALID_ARG; }
            outs[c.num_op].push_back(AIR_AUX_DEN_TAG);
            table[c.den_op].push_back(AIR_AUX_DEN_TAG);
            ch.kind = MainChunk::Kind::Fetch;
            ch.key_bits = c.key_bits;
            for (; ch.kc < AIR_MAIN_FETCH_MAX_GROUP && k0 + ch.kc < K; ++ch.kc) {
                const AirMainColumnHost& g = mp.cols[k0 + ch.kc];
                if (g.kind != SP_AIR_MAIN_FETCH || g.num_op != c.num_op || g.den_op != c.den_op || g.key_bits != c.key_bits || g.reads > k0) break;
                if (g.value_op >= n_src) { sp_set_error("commit_main_program: a FETCH column the decoder should have refused"); return SP_E_INVALID_ARG; }
                values[g.value_op].push_back(ch.kc);
            }
            if (ch.kc == 0) { sp_set_error("commit_main_program: a FETCH column that reads itself (the decoder should have refused it)"); return SP_E_INVALID_ARG; }
            SP_TRY(program(outs, ch, MainChunk::KEY_X));
            SP_TRY(program(table, ch, MainChunk::KEY_T));
            SP_TRY(program(values, ch, MainChunk::TABLE_V));
            P.any_fetch = true;
            P.max_fetch = std::max(P.max_fetch, ch.kc);
        } else {
            struct LimbGroup { uint32_t key = 0; std::vector<uint32_t> entries; };                  // key: N's op
            struct WordGroup { std::array<uint32_t, 3> key{}; std::vector<uint32_t> entries; };     // key: N's op, D's op, bits
            std::vector<LimbGroup> bits, limbs;
            std::vector<WordGroup> words;
            for (; ch.kc < P.chunk && k0 + ch.kc < K && mp.cols[k0 + ch.kc].reads <= k0 && mp.cols[k0 + ch.kc].kind != SP_AIR_MAIN_CHAIN &&
                   mp.cols[k0 + ch.kc].kind != SP_AIR_MAIN_COUNT && mp.cols[k0 + ch.kc].kind != SP_AIR_MAIN_FETCH; ++ch.kc) {
                const AirMainColumnHost& c = mp.cols[k0 + ch.kc];
                const bool scanned = c.kind == SP_AIR_MAIN_SUM || c.kind == SP_AIR_MAIN_PRODUCT;
                ch.tab[MainChunk::KINDS].push_back(c.kind == SP_AIR_MAIN_SUM ? 1u : 0u);
                if (scanned) {
                    if (!ch.scans.empty() && ch.scans.back().first + ch.scans.back().second == ch.kc) ++ch.scans.back().second;
                    else ch.scans.emplace_back(ch.kc, 1u);
                }
                if (c.kind == SP_AIR_MAIN_BIT) {    // (col, bit) beside the others of its N
                    std::vector<uint32_t>& e = group_of(bits, c.num_op).entries;
                    e.insert(e.end(), {ch.kc, c.bit});
                    continue;
                }
                if (c.kind == SP_AIR_MAIN_LIMB) {   // (col, lo, width) beside the others of its N
                    if (c.width == 0 || c.bit + c.width > AIR_MAIN_LIMB_MAX_END) { sp_set_error("commit_main_program: a LIMB column the decoder should have refused"); return SP_E_INVALID_ARG; }
                    std::vector<uint32_t>& e = group_of(limbs, c.num_op).entries;
                    e.insert(e.end(), {ch.kc, c.bit, c.width});
                    continue;
                }
                if (c.kind == SP_AIR_MAIN_WORD) {   // (col, fn) beside the others of its N, D and bits
                    if (c.width == 0 || c.width > AIR_MAIN_WORD_MAX_BITS || c.bit >= AIR_MAIN_WORD_FUNCTIONS || c.den_op >= n_src) {
                        sp_set_error("commit_main_program: a WORD column the decoder should have refused");
                        return SP_E_INVALID_ARG;
                    }
                    std::vector<uint32_t>& e = group_of(words, std::array<uint32_t, 3>{c.num_op, c.den_op, c.width}).entries;
                    e.insert(e.end(), {ch.kc, c.bit});
                    continue;
                }
                if (c.kind == SP_AIR_MAIN_INV_OR_ZERO) {
                    outs[c.num_op].push_back(AIR_AUX_DEN_TAG + ch.n_inv);
                    ch.tab[MainChunk::GUARD].insert(ch.tab[MainChunk::GUARD].end(), {ch.n_inv, ch.kc});
                    ch.tab[MainChunk::DEN_COL].push_back(ch.kc);
                    ++ch.n_inv;
                    continue;
                }
                outs[c.num_op].push_back(ch.kc);
                if (c.den_op != SP_AIR_AUX_NO_DEN) { outs[c.den_op].push_back(AIR_AUX_DEN_TAG + ch.n_inv); ch.tab[MainChunk::DEN_COL].push_back(ch.kc); ++ch.n_inv; }
            }
            ch.n_slots = ch.n_inv;
            // a group's slot, and its entries - 2 words each for a BIT group, 3 for a LIMB group - behind those of the groups before it
            auto place_groups = [&](const std::vector<LimbGroup>& groups, MainChunk::Tab g_tab, MainChunk::Tab e_tab, uint32_t words_each) {
                std::vector<uint32_t> &gtab = ch.tab[g_tab], &etab = ch.tab[e_tab];
                for (const LimbGroup& g : groups) {
                    outs[g.key].push_back(AIR_AUX_DEN_TAG + ch.n_slots);
                    gtab.insert(gtab.end(), {ch.n_slots++, (uint32_t)etab.size() / words_each, (uint32_t)g.entries.size() / words_each});
                    etab.insert(etab.end(), g.entries.begin(), g.entries.end());
                }
            };
            place_groups(bits, MainChunk::BIT_G, MainChunk::BIT_E, 2);
            place_groups(limbs, MainChunk::LIMB_G, MainChunk::LIMB_E, 3);
            for (const WordGroup& g : words) {   // N's slot, D's behind it
                std::vector<uint32_t> &gtab = ch.tab[MainChunk::WORD_G], &etab = ch.tab[MainChunk::WORD_E];
                outs[g.key[0]].push_back(AIR_AUX_DEN_TAG + ch.n_slots);
                outs[g.key[1]].push_back(AIR_AUX_DEN_TAG + ch.n_slots + 1);
                gtab.insert(gtab.end(), {ch.n_slots, (uint32_t)etab.size() / 2, (uint32_t)g.entries.size() / 2, g.key[2]});
                ch.n_slots += 2;
                etab.insert(etab.end(), g.entries.begin(), g.entries.end());
                P.any_word = true;
            }
            SP_TRY(program(outs, ch, MainChunk::TERMS));
            P.max_slots = std::max(P.max_slots, ch.n_slots);
            P.max_inv = std::max(P.max_inv, ch.n_inv);
        }
        k0 += ch.kc;
        P.chunks.push_back(std::move(ch));
    }
    // --- one upload: the constants, per chunk its programs and tables, the periodic columns an op 6 reads (st.periodic)
    UploadLayout lay;
    P.o_consts = lay.place(sizeof(fe) * std::max<size_t>(1, mp.consts.size()));
    for (MainChunk& ch : P.chunks) {
        for (int w = 0; w < MainChunk::N_PROG; ++w)
            if (!ch.prog[w].empty()) ch.o_prog[w] = lay.place(sizeof(AirOpDev) * ch.prog[w].size());
        for (int w = 0; w < MainChunk::N_TAB; ++w)
            if (!ch.tab[w].empty()) ch.o_tab[w] = lay.place(sizeof(uint32_t) * ch.tab[w].size());
    }
    const AirPeriodicHost* periodic = air_main_allows_chains(st.main_level) && st.periodic ? &*st.periodic : nullptr;
    if (any_periodic && !periodic) { sp_set_error("commit_main_program: op 6 without periodic columns (the decoder should have refused it)"); return SP_E_INVALID_ARG; }
    P.per.place(lay, any_periodic ? periodic : nullptr);
    P.bytes = lay.bytes;
    // --- workspace, the largest of what a row-local chunk, a COUNT column and a FETCH group take:
    //     chunks:  [max_slots][n] slots, [max_inv][n] batch-inversion scratch, [chunk][nb] scan block totals
    //     counts:  4 x [n] keys, 4 x [n] rows, the radix sort's histograms (all in units of 32 bytes)
    //     fetches: 3 x [n] keys, 3 x [n] rows, the radix sort's histograms, [max_fetch][n] table values
    if ((P.any_count || P.any_fetch) && n >= (1ull << 32)) { sp_set_error("commit_main_program: COUNT and FETCH columns need a trace of fewer than 2^32 rows"); return SP_E_INVALID_ARG; }
    //     joint counts: 2 x [n] keys, 2 x [n] rows, the radix sort's histograms, [max_lists][n] looked-up keys, [n] counters
    P.ws_elems = std::max(((uint64_t)P.max_slots + P.max_inv) * n + (uint64_t)P.chunk * air_aux_scan_blocks(n), P.any_plain_count ? SortScratch::elems(n, 4) : 0);
    if (P.max_lists) P.ws_elems = std::max(P.ws_elems, SortScratch::elems(n, 2) + ((uint64_t)P.max_lists + 1) * SortScratch::keys_el(n));
    if (P.any_fetch) P.ws_elems = std::max(P.ws_elems, SortScratch::elems(n, 3) + (uint64_t)P.max_fetch * n);
    return SP_OK;
}

// Launching: the ingest, the upload and the chunks one behind the other.  The three verdict words lie inside the one element behind
// ws_elems, in the order of HostFlags' auxp_bad_key, auxp_missing_key and auxp_bad_word, which one copy fills: the key-range flag of
// the COUNT and FETCH columns, which no batch inversion before or behind overwrites there; the missing-key flag of the FETCH columns,
// which neither a key pass nor a batch inversion does; the range flag of the WORD columns, which air_main_words writes, and a chain
// group with integer ops with a value of its own (AIR_MAIN_FLAG_INT_RANGE).
int StarkProver::build_main_program(const AirStatement& st, const uint8_t* inputs) {
    const AirMainHost& mp = *st.main;
    const uint32_t I = mp.input_cols, K = (uint32_t)mp.cols.size();
    if (!inputs) return SP_E_INVALID_ARG;
    if (stage_ != Stage::Setup || I + K != Cm_) { sp_set_error("commit_main_program: wrong segment order, or input and derived columns are not the main segment"); return SP_E_STATE; }
    SP_HIP_CHECK(hipSetDevice(c_->device));
    binary_cols_hint_ = 0;
    for (double& x : c_->upload_stats) x = 0.0;
    leaf_head_done_ = false;
    MainPlan P;
    SP_TRY(plan_main_program(st, n_, P));
    SP_TRY(grow(od_.auxp_buf, P.bytes));
    std::vector<uint8_t>& up = h_auxp_up_;
    up.assign(P.bytes, 0);
    fill_consts_then_rap(up.data() + P.o_consts, mp.consts, {});
    for (const MainChunk& ch : P.chunks) {
        for (int w = 0; w < MainChunk::N_PROG; ++w)
            if (!ch.prog[w].empty()) std::memcpy(up.data() + ch.o_prog[w], ch.prog[w].data(), sizeof(AirOpDev) * ch.prog[w].size());
        for (int w = 0; w < MainChunk::N_TAB; ++w)
            if (!ch.tab[w].empty()) std::memcpy(up.data() + ch.o_tab[w], ch.tab[w].data(), sizeof(uint32_t) * ch.tab[w].size());
    }
    P.per.fill(up.data());
    SP_TRY(grow(od_.auxp_ws, P.ws_elems + 1));
    SP_TRY(ensure_host_flags());
    static_assert(offsetof(HostFlags, auxp_missing_key) == offsetof(HostFlags, auxp_bad_key) + sizeof(int) &&
                  offsetof(HostFlags, auxp_bad_word) == offsetof(HostFlags, auxp_bad_key) + 2 * sizeof(int), "the verdict words are copied as one block");
    host_flags().auxp_bad_key = host_flags().auxp_missing_key = host_flags().auxp_bad_word = 0;
    // --- ingest: the plain staged copy (the inputs are a small part of the table; their raw rows sit in the segment's LDE area,
    //     which is written only by the transforms behind the last chunk), then rows -> columns [0, I)
    if (mp.input_location == 1) {
        SP_TRY(rows_to_columns(c_->stream, c_->enc, inputs, n_, I, d_trace_, n_));
    } else {
        uint8_t* raw = reinterpret_cast<uint8_t*>(d_lde_);
        SP_HIP_CHECK(hipMemcpyAsync(raw, inputs, (size_t)n_ * I * 32, hipMemcpyHostToDevice, c_->stream));
        SP_TRY(rows_to_columns(c_->stream, c_->enc, raw, n_, I, d_trace_, n_));
    }
    SP_HIP_CHECK(hipMemcpyAsync(od_.auxp_buf.p, up.data(), P.bytes, hipMemcpyHostToDevice, c_->stream));
    SP_HIP_CHECK(hipMemsetAsync(c_->d_flag, 0, sizeof(int), c_->stream));
    const fe* consts_dev = reinterpret_cast<const fe*>(od_.auxp_buf.p + P.o_consts);
    fe* ws = od_.auxp_ws.p;
    int* key_flag = reinterpret_cast<int*>(ws + P.ws_elems);
    int* miss_flag = key_flag + 1;
    int* word_flag = key_flag + 2;
    if (P.any_verdict()) SP_HIP_CHECK(hipMemsetAsync(key_flag, 0, 3 * sizeof(int), c_->stream));
    const SortScratch s(ws, n_, 4);   // a COUNT column: X's pairs in keys / rows [0] and [1], T's in [2] and [3]
    const SortScratch f(ws, n_, 3);   // a FETCH group: T's pairs in keys / rows [0] and [1], X's in [2]; the table values behind
    fe* fetch_vals = ws + SortScratch::elems(n_, 3);
    const SortScratch j(ws, n_, 2);   // a joint COUNT column: T's pairs in keys / rows [0] and [1]; the looked-up keys and the counters behind
    uint64_t* list_keys = reinterpret_cast<uint64_t*>(ws + SortScratch::elems(n_, 2));
    uint64_t* list_counters = list_keys + (uint64_t)P.max_lists * 4 * SortScratch::keys_el(n_);
    fe* scratch = ws + (uint64_t)P.max_slots * n_;
    fe* block_tot = scratch + (uint64_t)P.max_inv * n_;
    auto tab = [&](const MainChunk& ch, MainChunk::Tab w) { return ch.tab[w].empty() ? nullptr : reinterpret_cast<const uint32_t*>(od_.auxp_buf.p + ch.o_tab[w]); };
    auto count = [](const MainChunk& ch, MainChunk::Tab w, uint32_t words_each) { return (uint32_t)ch.tab[w].size() / words_each; };
    for (const MainChunk& ch : P.chunks) {
        fe* cols = d_trace_ + (uint64_t)(I + ch.k0) * n_;
        const AirOpDev* prog[MainChunk::N_PROG];   // (a program the chunk's kind does not have: no ops, and not read)
        uint32_t n_prog[MainChunk::N_PROG];
        for (int w = 0; w < MainChunk::N_PROG; ++w) { prog[w] = reinterpret_cast<const AirOpDev*>(od_.auxp_buf.p + ch.o_prog[w]); n_prog[w] = (uint32_t)ch.prog[w].size(); }
        const AirPeriodicCol* pc = ch.periodic ? P.per.cols_dev(od_.auxp_buf.p) : nullptr;
        const fe* pv = ch.periodic ? P.per.vals_dev(od_.auxp_buf.p) : nullptr;
        switch (ch.kind) {
        case MainChunk::Kind::Chain:
            SP_TRY(air_main_chain(c_->stream, d_trace_, n_, ch.log_s, ch.log_k, I + ch.k0, ch.kc, prog[MainChunk::SEED], n_prog[MainChunk::SEED], prog[MainChunk::STEP],
                                  n_prog[MainChunk::STEP], consts_dev, pc, pv, ch.divides ? c_->d_flag : nullptr, ch.integers ? word_flag : nullptr));
            break;
        case MainChunk::Kind::Count:   // key passes, sorts (the sorted pairs end up in keys / rows [1] and [3]), the join
            SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, prog[MainChunk::KEY_X], n_prog[MainChunk::KEY_X], consts_dev, nullptr, s.keys[0], s.rows[0], ch.key_bits, key_flag, pc, pv));
            SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, prog[MainChunk::KEY_T], n_prog[MainChunk::KEY_T], consts_dev, nullptr, s.keys[2], s.rows[2], ch.key_bits, key_flag, pc, pv));
            SP_TRY(radix_sort_pairs_u64(c_->stream, s.keys[0], s.keys[1], s.rows[0], s.rows[1], n_, ch.key_bits, s.radix));
            SP_TRY(radix_sort_pairs_u64(c_->stream, s.keys[2], s.keys[3], s.rows[2], s.rows[3], n_, ch.key_bits, s.radix));
            SP_TRY(air_main_count(c_->stream, s.keys[1], s.keys[3], s.rows[3], n_, cols));
            break;
        case MainChunk::Kind::CountMany:   // the table's key pass and sort (into keys / rows [1]), the looked-up keys, search and add, store
            SP_HIP_CHECK(hipMemsetAsync(list_counters, 0, sizeof(uint64_t) * n_, c_->stream));
            SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, prog[MainChunk::KEY_T], n_prog[MainChunk::KEY_T], consts_dev, nullptr, j.keys[0], j.rows[0], ch.key_bits, key_flag, pc, pv));
            SP_TRY(radix_sort_pairs_u64(c_->stream, j.keys[0], j.keys[1], j.rows[0], j.rows[1], n_, ch.key_bits, j.radix));
            SP_TRY(air_main_list_keys(c_->stream, d_trace_, n_, prog[MainChunk::KEY_X], n_prog[MainChunk::KEY_X], consts_dev, list_keys, ch.n_lists, ch.key_bits, key_flag, pc, pv));
            SP_TRY(air_main_count_many(c_->stream, list_keys, ch.n_lists, j.keys[1], j.rows[1], n_, list_counters, cols));
            break;
        case MainChunk::Kind::Fetch:   // key passes (X's pairs stay in row order), V's terms, the table's sort (into keys / rows [1]), the join
            SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, prog[MainChunk::KEY_T], n_prog[MainChunk::KEY_T], consts_dev, nullptr, f.keys[0], f.rows[0], ch.key_bits, key_flag, pc, pv));
            SP_TRY(air_aux_sort_terms(c_->stream, d_trace_, n_, prog[MainChunk::KEY_X], n_prog[MainChunk::KEY_X], consts_dev, nullptr, f.keys[2], f.rows[2], ch.key_bits, key_flag, pc, pv));
            SP_TRY(air_aux_terms(c_->stream, d_trace_, n_, prog[MainChunk::TABLE_V], n_prog[MainChunk::TABLE_V], consts_dev, fetch_vals, nullptr, pc, pv));
            SP_TRY(radix_sort_pairs_u64(c_->stream, f.keys[0], f.keys[1], f.rows[0], f.rows[1], n_, ch.key_bits, f.radix));
            SP_TRY(air_main_fetch(c_->stream, f.keys[2], f.keys[1], f.rows[1], fetch_vals, n_, cols, ch.kc, miss_flag));
            break;
        case MainChunk::Kind::RowLocal:
            // OUT a < AIR_AUX_DEN_TAG stores N of chunk column a, OUT AIR_AUX_DEN_TAG + s stores into workspace slot s
            SP_TRY(air_aux_terms(c_->stream, d_trace_, n_, prog[MainChunk::TERMS], n_prog[MainChunk::TERMS], consts_dev, cols, ws, pc, pv));
            SP_TRY(air_main_zero_guard(c_->stream, ws, cols, tab(ch, MainChunk::GUARD), count(ch, MainChunk::GUARD, 2), n_));
            if (ch.n_inv) {
                SP_TRY(batch_inverse(c_->stream, ws, scratch, (uint64_t)ch.n_inv * n_, c_->d_flag));
                SP_TRY(air_aux_apply_den(c_->stream, cols, ws, tab(ch, MainChunk::DEN_COL), ch.n_inv, n_));
            }
            SP_TRY(air_main_bits(c_->stream, ws, cols, tab(ch, MainChunk::BIT_G), tab(ch, MainChunk::BIT_E), count(ch, MainChunk::BIT_G, 3), n_));
            SP_TRY(air_main_limbs(c_->stream, ws, cols, tab(ch, MainChunk::LIMB_G), tab(ch, MainChunk::LIMB_E), count(ch, MainChunk::LIMB_G, 3), n_));
            SP_TRY(air_main_words(c_->stream, ws, cols, tab(ch, MainChunk::WORD_G), tab(ch, MainChunk::WORD_E), count(ch, MainChunk::WORD_G, 4), n_, word_flag));
            for (const auto& run : ch.scans)
                SP_TRY(air_aux_scan(c_->stream, cols + (uint64_t)run.first * n_, n_, run.second, tab(ch, MainChunk::KINDS) + run.first, block_tot));
            break;
        }
    }
    // the zero-denominator flag rides behind the columns; whoever reads the root (or the table) back waits for it
    SP_HIP_CHECK(hipMemcpyAsync(&host_flags().auxp_zero_den, c_->d_flag, sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    if (P.any_verdict()) SP_HIP_CHECK(hipMemcpyAsync(&host_flags().auxp_bad_key, key_flag, 3 * sizeof(int), hipMemcpyDeviceToHost, c_->stream));
    return SP_OK;
}

// What the flags say once the stream has drained: the key range first (as commit_aux_program), then a missing key, then a word operand
// or an integer op's out of range (one word: whichever stored last), then a zero denominator.
static int main_program_verdict(const HostFlags& f) {
    if (f.auxp_bad_key == AIR_AUX_FLAG_KEY_RANGE) {
        sp_set_error("commit_main_program: a lookup key is out of range on some row (X and T of a COUNT column must be below 2^key_bits as canonical integers)");
        return SP_E_INVALID_ARG;
    }
    if (f.auxp_missing_key == AIR_MAIN_FLAG_MISSING_KEY) {
        sp_set_error("commit_main_program: a fetched key is in no table row (every X of a FETCH column must equal the T of some row)");
        return SP_E_INVALID_ARG;
    }
    if (f.auxp_bad_word == AIR_MAIN_FLAG_WORD_RANGE) {
        sp_set_error("commit_main_program: a word operand is out of range on some row (both operands of a WORD column must be below 2^bits as canonical integers)");
        return SP_E_INVALID_ARG;
    }
    if (f.auxp_bad_word == AIR_MAIN_FLAG_INT_RANGE) {
        sp_set_error("commit_main_program: an integer op's operand is out of range on some row (both operands of an AND, OR or XOR op must be below 2^251 as canonical integers)");
        return SP_E_INVALID_ARG;
    }
    if (f.auxp_zero_den) { sp_set_error("commit_main_program: a derived main column's denominator is zero on some row"); return SP_E_ZERO_INVERSE; }
    return SP_OK;
}

int StarkProver::commit_main_program(const AirStatement& st, const uint8_t* inputs, uint8_t root_out[32]) {
    if (!root_out) return SP_E_INVALID_ARG;
    const double t0 = wall_ms();
    int rc = build_main_program(st, inputs);
    const double host_ms = wall_ms() - t0;
    if (rc == SP_OK) rc = launch_aux_presort();
    if (rc == SP_OK) rc = commit_segment_resident(0, Cm_, root_out);
    if (rc != SP_OK) {   // (nothing returns while a copy from the caller's inputs may still be in flight)
        (void)hipStreamSynchronize(c_->stream);
        (void)hipGetLastError();
        return rc;
    }
    SP_TRY(main_program_verdict(host_flags()));
    return finish_upload_stats(0, st.main->input_location == 1 ? 0 : (uint64_t)n_ * st.main->input_cols * 32, 0.0, host_ms, 0);
}

int StarkProver::main_program_table(const AirStatement& st, const uint8_t* inputs, uint8_t* rows_out) {
    if (!rows_out) return SP_E_INVALID_ARG;
    int rc = build_main_program(st, inputs);
    // the columns in the context encoding, through the (unused) LDE area, then transposed on the host
    uint8_t* enc_dev = reinterpret_cast<uint8_t*>(d_lde_);
    std::vector<uint8_t> by_col;
    if (rc == SP_OK) rc = encode_elements(c_->stream, c_->enc, d_trace_, (uint64_t)Cm_ * n_, enc_dev);
    if (rc == SP_OK) { by_col.resize((size_t)Cm_ * n_ * 32); rc = readback(by_col.data(), enc_dev, by_col.size()); }
    if (rc != SP_OK) {
        (void)hipStreamSynchronize(c_->stream);
        (void)hipGetLastError();
        return rc;
    }
    SP_TRY(main_program_verdict(host_flags()));
    for (uint32_t c = 0; c < Cm_; ++c)
        for (uint64_t i = 0; i < n_; ++i) std::memcpy(rows_out + ((size_t)i * Cm_ + c) * 32, by_col.data() + ((size_t)c * n_ + i) * 32, 32);
    return SP_OK;
}

}  // namespace sp
