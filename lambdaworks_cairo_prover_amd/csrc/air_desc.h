// Host forms of the C views of include/stark252_hip.h that the prover and the verifier share: proof options, and the statement of a
// program AIR - sp_air_desc with its optional parts sp_air_aux_desc, sp_air_periodic_desc, sp_air_stride_desc and sp_air_boundary_desc -
// as one AirStatement, its one decoder and validator, and the host model of its parts.  Host only (no device headers); air_desc.cpp.
#pragma once
#include "cairo_air_host.h"
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace sp {

struct ProofOptionsHost { uint8_t blowup_factor; uint64_t fri_number_of_queries; uint64_t coset_offset; uint8_t grinding_factor; };
inline ProofOptionsHost proof_options_from_c(const sp_proof_options* o) {
    return ProofOptionsHost{o->blowup_factor, o->fri_number_of_queries, o->coset_offset, o->grinding_factor};
}

// Host form of sp_air_stride: constraint k is enforced on the rows i = offset (mod period), period a power of two.
struct AirStrideHost { uint32_t period = 1, offset = 0; };
// Constraints with one (period, offset), period > 1, share a zerofier: a stride class.  An exemption product belongs to a (class, e > 0).
constexpr uint32_t AIR_MAX_STRIDE_CLASSES = 4, AIR_MAX_STRIDE_EXEMPT_KINDS = 4;

// Host form of sp_air_desc.
struct AirOpHost { uint8_t op; uint32_t a, b; };   // as the caller wrote it: operands are indices of earlier ops
struct AirDescHost {
    uint32_t main_cols = 0, aux_cols = 0;
    std::vector<uint32_t> offsets, degrees, exemptions;
    uint32_t num_transition_exemptions = 1, degree_bound_factor = 1;
    std::vector<AirOpHost> ops;
    std::vector<fe> consts;
    uint32_t n_rap = 0, aux_kind = 0;
    sp_aux_trace_fn aux_fn = nullptr; void* aux_user = nullptr;   // aux_kind 2: build_auxiliary_trace supplied by the caller
    std::vector<BoundaryConstraint> boundary;
    std::vector<AirStrideHost> strides;   // per transition constraint (sp_air_stride_desc); empty: every constraint on every row
};
// The bounds of a statement (sp_air_limits reports them; prover.h holds them against the kernels' AIR_MAX_*), and the row shifts an
// auxiliary program's LOAD and PERIODIC may name.
constexpr uint32_t AIR_LIMIT_COLS = 1024, AIR_LIMIT_BOUNDARY = 4096, AIR_LIMIT_CONSTS = 4096, AIR_LIMIT_OPS = 65535, AIR_LIMIT_AUX_SHIFT = 7;

// Host form of sp_air_aux_desc: the auxiliary program of an AIR with aux_kind SP_AIR_AUX_PROGRAM.
struct AirAuxColumnHost { uint32_t kind, num_op, den_op, key_bits = 0; };   // key_bits: 1 .. 64 for a SORTED column (den_op is its group's key), else 0
struct AirAuxHost {
    std::vector<AirOpHost> ops;
    std::vector<fe> consts;
    std::vector<AirAuxColumnHost> cols;
};

// Host form of sp_air_main_desc: the program that derives main columns input_cols .. main_cols - 1 from the caller's input columns.
// reads: derived columns [0, reads) are what the ops behind this column load (0: inputs only); the decoder holds reads <= its index
// (for a CHAIN column: <= the end of its group for the step, <= the group's first column for the seed).  chain_log / chain_pos: the
// l and j of a CHAIN column's pad (block length 2^l, position in its group), 0 for the other kinds.
// key_bits: the pad of a COUNT column (its X is num_op, its T den_op), 0 for the other kinds.
// chain_link: the k of a CHAIN column's pad through the _link entry points - runs of 2^k blocks, a seed inside a run reads the last
// state of the block before it (0: every block on its own, and always 0 through every other entry point).
// value_op: the v_op of a FETCH column's pad (its X is num_op, its T den_op, its key_bits the low byte of the pad), 0 for the other kinds.
// width: the width of a LIMB column (its lo is `bit`) or the bits of a WORD column (its fn is `bit`), 0 for the other kinds.
// list_len: the L of a joint COUNT column, whose num_op names the first of L op 12 cells (X_0 the a of that cell, X_1 that of its b, ..),
// 0 for a COUNT column of the old form and for the other kinds.
constexpr uint32_t AIR_MAIN_CHAIN_MAX_WIDTH = 16;
constexpr uint32_t AIR_MAIN_LINK_MAX_LOG = 62;   // (l >= 1 and l + k <= log2 n <= 63)
constexpr uint32_t AIR_MAIN_COUNT_MAX_KEY_BITS = 64, AIR_MAIN_COUNT_MAX_COLS = 16;
constexpr uint32_t AIR_MAIN_FETCH_MAX_KEY_BITS = 64, AIR_MAIN_FETCH_MAX_GROUP = 16, AIR_MAIN_FETCH_MAX_COLS = 64;
constexpr uint32_t AIR_MAIN_LIMB_MAX_END = 252, AIR_MAIN_WORD_MAX_BITS = 251, AIR_MAIN_WORD_FUNCTIONS = 3;   // (lo + width <= 252; 2^251 < p)
// A joint COUNT column (main_level Multi): bit 8 of its pad, and its num_op names a list of op 12 cells, one per looked-up value
constexpr uint32_t AIR_MAIN_COUNT_LIST_BIT = 256, AIR_MAIN_COUNT_MAX_LIST = 16, AIR_OP_ALSO = 12, AIR_LIST_END = 0xFFFF;
constexpr uint32_t AIR_MAIN_INT_OPS = 4;   // ops 8 .. 11; the LIMB op shares AIR_MAIN_LIMB_MAX_END, AND / OR / XOR take operands below 2^AIR_MAIN_WORD_MAX_BITS
struct AirMainColumnHost { uint32_t kind, num_op, den_op, bit, reads, chain_log = 0, chain_pos = 0, key_bits = 0, chain_link = 0, value_op = 0, width = 0, list_len = 0; };
struct AirMainHost {
    uint32_t input_cols = 0, input_location = 0;   // 0: the inputs are host memory, 1: device memory
    std::vector<AirOpHost> ops;
    std::vector<fe> consts;
    std::vector<AirMainColumnHost> cols;
};

// Host form of sp_air_periodic_desc: column k repeats cols[k] (a power-of-two number of values, at most the trace length).
constexpr uint32_t AIR_MAX_PERIODIC = 64;
struct AirPeriodicHost { std::vector<std::vector<fe>> cols; };
// P(point) of one periodic column on a trace of n rows: q interpolated from the values (a size-period inverse transform),
// evaluated at point^(n / period).  What the verifier uses for P_k(z g^offset) and what sp_air_periodic_eval returns.
std::vector<fe> air_periodic_interpolate(const std::vector<fe>& values);
fe air_periodic_eval(const std::vector<fe>& coeffs, uint64_t n, const fe& point);

// The strides of an AIR sorted into classes and exemption products, for a trace of n rows.  cls[k]: -1 for a (1, 0) constraint, else
// its class; kind[k]: -1 without exempted rows (or for a (1, 0) constraint), else its entry of `kinds` = (class, e).
struct AirStridePlan {
    std::vector<AirStrideHost> classes;
    std::vector<std::pair<uint32_t, uint32_t>> kinds;
    std::vector<int> cls, kind;
};
// false for strides that break a rule of sp_air_stride_desc: not one per transition, a period that is zero, no power of two or above
// n, offset >= period, exemptions[k] >= n / period or degrees[k] > degree_bound_factor for a period > 1 (the quotient by the smaller
// zerofier has degree d n - n/s, which fits under f n for d <= f only), more classes or exemption products than the limits.  Reads
// air.strides / exemptions / degrees / degree_bound_factor only; empty strides give a plan without classes.
bool air_stride_plan(const AirDescHost& air, uint64_t n, AirStridePlan& out);
// Z(x) = x^(n/s) - g^(o n/s) and E(x) = prod_{t<e} (x - g^(o + s (n/s - 1 - t))) of a stride (s, o) with e exempted rows on a trace of
// n rows (all already checked: s | n, o < s, e <= n/s).  What the verifier's step 2 uses and sp_air_stride_eval returns.
void air_stride_eval(uint32_t s, uint32_t o, uint32_t e, uint64_t n, const fe& x, fe& Z, fe& E);

// Host form of sp_air_boundary_desc: boundary values that are N / D of a program over constants and the RAP challenges (ops 1 - 4).
struct AirBoundaryValueHost { uint32_t boundary, num_op, den_op; };
struct AirBoundaryHost {
    std::vector<AirOpHost> ops;
    std::vector<fe> consts;
    std::vector<AirBoundaryValueHost> values;
};
// sp_air_boundary_desc -> AirBoundaryHost for an AIR with n_boundary boundary constraints and n_rap challenges; false - before anything
// is allocated or copied - for null members, counts beyond sp_air_limits, an op other than 1 - 4, an operand that is no earlier op,
// boundary >= n_boundary, a boundary named twice, num_op / den_op beyond the program.  Called by air_statement_from_c, and by
// sp_air_boundary_resolve with an unbounded n_boundary.
bool air_boundary_from_c(const sp_air_boundary_desc* d, uint32_t n_boundary, uint32_t n_rap, AirBoundaryHost& out);
extern const char* const AIR_BOUNDARY_VALUES_MALFORMED;   // what both callers say on false
// The one resolver: values[j] = N_j / D_j under these challenges (one batch inversion).  false when a D is zero.  Prover, trace check,
// verifier and sp_air_boundary_resolve all go through it.
bool air_resolve_boundary(const AirBoundaryHost& bvals, const std::vector<fe>& rap, std::vector<fe>& values);
// air.boundary with the resolved values put in: what everything behind round 1's challenges sees as constants.
bool air_resolve_boundary_into(const AirBoundaryHost& bvals, const std::vector<fe>& rap, std::vector<BoundaryConstraint>& boundary);

// The rules of a straight-line program (op 0 LOAD, 1 CONST, 2 ADD, 3 SUB, 4 MUL, 5 OUT, 6 PERIODIC): a LOAD has a < load_a_end and
// b < load_b_end, a CONST names one of n_values constants or RAP challenges, ADD / SUB / MUL take two earlier ops that are not
// OUTs, an OUT one of n_out targets and such an op (n_out 0: no OUT at all), a PERIODIC a < load_a_end and one of n_periodic
// periodic columns (0: the program cannot read any).  Returns the index of the first op that breaks them, ops.size() when none
// does.  div (a main-trace program through the _div entry points, and nothing else): op 7 DIV takes two earlier ops that are not OUTs
// too; without it op 7 is the unknown op it always was.  ints (a main-trace program through the _int entry points, and nothing else):
// op 8 LIMB takes one such op and the immediate b = lo + 256 width with 1 <= width and lo + width <= 252, ops 9 .. 11 AND / OR / XOR two
// such ops; without it they are the unknown ops they always were.  lists (a main-trace program through the _multi entry points, and
// nothing else): op 12 ALSO is a list cell - a an earlier value, b an earlier op 12 or 0xFFFF -, which has no value: no value op takes
// one for an operand; without it op 12 is the unknown op it always was.
size_t air_program_first_bad_op(const std::vector<AirOpHost>& ops, uint32_t load_a_end, uint32_t load_b_end, size_t n_values, uint32_t n_out,
                                uint32_t n_periodic, bool div = false, bool ints = false, bool lists = false);
// ADD, SUB, MUL, DIV and the integer AND, OR and XOR: the ops whose a and b name earlier values (what the slot assignment and the
// operand walks follow).  Op 8, the integer LIMB, has one: its a names an earlier value, its b is the immediate lo + 256 width, which
// nothing remaps and nothing takes for a slot.
inline bool air_op_takes_two_values(uint8_t op) { return (op >= 2 && op <= 4) || op == 7 || (op >= 9 && op <= 11); }
inline bool air_op_takes_one_value(uint8_t op) { return op == 8; }
// ops 8 .. 11: functions of a value's canonical integer, behind a chain group's seeds and steps only (main_level Int)
inline bool air_op_is_integer(uint8_t op) { return op >= 8 && op <= 11; }
// the primitive root of unity of order 2^order (lambdaworks get_primitive_root_of_unity)
fe air_root_of_unity(int order);

// What a main-trace program may hold, one ordered level - each brings the ones before it with it:
//   Main   VALUE, INV_OR_ZERO, BIT, SUM and PRODUCT columns over ops 0 .. 4
//   Rec    (the _rec entry points) CHAIN columns too, and op 6 reads the periodic columns
//   Lk     (the _lk entry points) COUNT columns too, lookup multiplicities
//   Link   (the _link entry points) a chain group's blocks may form runs seeded from the block before
//   Div    (the _div entry points) op 7 DIV behind the seeds and steps of CHAIN columns: quotients inside a recurrence
//   Fetch  (the _fetch entry points) FETCH columns too, looked-up values
//   Word   (the _word entry points) LIMB and WORD columns too, limbs and bitwise functions of canonical integers
//   Int    (the _int entry points) ops 8 .. 11 behind the seeds and steps of CHAIN columns: integer functions inside a recurrence
//   Multi  (the _multi entry points) joint COUNT columns too: one multiplicity column for a list of looked-up values (op 12)
enum class AirMainLevel : uint8_t { Main, Rec, Lk, Link, Div, Fetch, Word, Int, Multi };
inline bool air_main_allows_chains(AirMainLevel l) { return l >= AirMainLevel::Rec; }   // (and op 6)
inline bool air_main_allows_counts(AirMainLevel l) { return l >= AirMainLevel::Lk; }
inline bool air_main_allows_runs(AirMainLevel l) { return l >= AirMainLevel::Link; }
inline bool air_main_allows_quotients(AirMainLevel l) { return l >= AirMainLevel::Div; }
inline bool air_main_allows_fetches(AirMainLevel l) { return l >= AirMainLevel::Fetch; }
inline bool air_main_allows_words(AirMainLevel l) { return l >= AirMainLevel::Word; }
inline bool air_main_allows_int_ops(AirMainLevel l) { return l >= AirMainLevel::Int; }
inline bool air_main_allows_lists(AirMainLevel l) { return l >= AirMainLevel::Multi; }

// Everything a prover, a trace check or a verifier is told about a program AIR: the descriptor (its strides inside) and its optional
// parts, each present or not.  aux_reads_periodic: whether the auxiliary program may read the periodic columns with op 6 (the _pub
// entry points; everywhere else such an op is malformed).
struct AirStatement {
    AirDescHost air;
    std::optional<AirAuxHost> aux;            // the auxiliary program of an AIR with aux_kind SP_AIR_AUX_PROGRAM
    std::optional<AirPeriodicHost> periodic;  // the periodic columns the constraint program reads with op 6
    std::optional<AirBoundaryHost> bvals;     // boundary values computed from the RAP challenges (air_resolve_boundary_into after round 1)
    std::optional<AirMainHost> main;          // the main-trace program: the caller hands over its input columns only (sp_air_prove_main)
    bool aux_reads_periodic = false;
    AirMainLevel main_level = AirMainLevel::Main;   // what the main program may hold: the entry point's suffix decides
    bool unsupported = false;                 // set with a refusal that is SP_E_UNSUPPORTED, not SP_E_INVALID_ARG (a main program beside aux_kind 1 or 2)
    // the periodic columns the auxiliary program may read: null when it may read none
    const AirPeriodicHost* aux_periodic() const { return aux_reads_periodic && periodic ? &*periodic : nullptr; }
    uint32_t n_periodic() const { return periodic ? (uint32_t)periodic->cols.size() : 0u; }
};
// The one decoder and validator of a statement for a trace of n rows: d and whichever of aux, periodic, strides (what sp_air_ext
// carries) and bvals are non-null.  Returns "" and fills `out`, or the cause of the refusal (the entry point puts its own name in
// front).  Every count and pointer of a part is judged before anything is allocated or copied for it.  The rules: those of
// sp_air_desc's counts; <= 64 periodic columns, each a power-of-two number of values <= n; strides as air_stride_plan wants them;
// an auxiliary program that fits its AIR (aux_kind, one column per auxiliary column, ops over earlier ops, LOADs of main columns - or
// of SORTED auxiliary columns, but not from the ops behind a sorted column - at shifts 0 .. 7, op 6 only with aux_reads_periodic, at
// most SP_AIR_AUX_MAX_SORT_GROUPS sort groups, each with one key_bits in 1 .. 64); boundary values as air_boundary_from_c wants them; the bounds of sp_air_limits.
// main (nullable, the prover and the trace check only): a main-trace program whose columns add up to air.main_cols, ops 0 .. 4 over
// earlier ops, LOADs at shifts 0 .. 7 of inputs or - from the ops behind derived column j - of derived columns k < j, the kinds' own
// rules (sp_air_main_desc); beside it aux_kind is 0 or SP_AIR_AUX_PROGRAM, else the refusal comes with out.unsupported set.
// main_level Rec (the _rec entry points only): the main program may also hold SP_AIR_MAIN_CHAIN columns - groups of 1 .. 16 with j = 0, 1, ..
// and one block length 2^l in 2 .. n, a seed that reads nothing of its group, a step that reads its group at shift 0 only - and read
// the periodic columns with op 6; without it kind 5 is an unknown kind and op 6 a malformed op, as ever.
// main_level Lk (the _lk entry points only; it brings Rec with it): the main program may also hold SP_AIR_MAIN_COUNT columns - at most
// 16, each with a table (den_op), key_bits (pad) in 1 .. 64, X and T over earlier columns; without it kind 6 is an unknown kind.
// main_level Link (the _link entry points only; it brings Lk with it): a CHAIN column's pad also carries k = pad >> 16 - runs of 2^k
// blocks, l + k <= log2 n, one k per group - and with k >= 1 a seed may load its own group at shift 0 (the carry); without it the
// bits at and above 16 belong to j, as ever.
// main_level Div (the _div entry points only; it brings Link with it): op 7 DIV a b = value(a) / value(b) over earlier ops, behind the
// seed or step op of a CHAIN column only - a VALUE, INV_OR_ZERO, BIT, SUM, PRODUCT or COUNT column whose N, D, X or T depends on an
// op 7 is refused (a row-local quotient is a VALUE column's N / D, which keeps the batched inversion); without it op 7 is a malformed
// op, as ever.  A zero under a DIV is a matter of the rows, not of the statement: SP_E_ZERO_INVERSE from the call that meets it.
// main_level Fetch (the _fetch entry points only; it brings Div with it): the main program may also hold SP_AIR_MAIN_FETCH columns - at
// most 64, each with a table key (den_op), pad = key_bits (1 .. 64) + 256 v_op below 2^24, X, T and V over earlier columns and behind
// no op 7; without it kind 7 is an unknown kind, as ever.  A key in no table row is a matter of the rows: SP_E_INVALID_ARG from the call.
// main_level Word (the _word entry points only; it brings Fetch with it): the main program may also hold SP_AIR_MAIN_LIMB columns - no
// denominator, pad = lo + 256 width below 2^16, 1 <= width, lo + width <= 252 - and SP_AIR_MAIN_WORD columns - a second operand
// (den_op), pad = fn + 256 bits below 2^16, fn 0 .. 2, bits 1 .. 251 -, their operands over earlier columns and behind no op 7;
// without it kinds 8 and 9 are unknown kinds.  A WORD operand at or above 2^bits is a matter of the rows: SP_E_INVALID_ARG from the call.
// main_level Int (the _int entry points only; it brings Word with it): ops 8 LIMB a, lo + 256 width and 9 .. 11 AND / OR / XOR a b over
// earlier ops, behind the seed or step op of a CHAIN column only, as op 7 - a column of any other kind whose operand depends on one is
// refused (a row-local limb or word is a LIMB or WORD column); without it they are malformed ops, as ever.  An AND / OR / XOR operand
// at or above 2^251 is a matter of the rows: SP_E_INVALID_ARG from the call.
// main_level Multi (the _multi entry points only; it brings Int with it): a COUNT column's pad may carry bit 8 (pad = key_bits + 256),
// and its num_op then names a list of 1 .. 16 cells of op 12 ALSO - a: an earlier value, one looked-up value; b: an earlier cell, the
// rest of the list, or 0xFFFF -; the column counts all of them against its one table.  A cell has no value: it is no operand, no OUT,
// no den_op and stands behind no other column.  Without it op 12 is a malformed op and such a pad a key_bits out of range, as ever.
// The constraint program itself is checked where it is turned into what runs it (build_air_program, air_verify_host).
// An sp_air_ext is taken apart by the entry point that receives it; this is the one thing it checks first: null, or what is wrong.
inline const char* air_ext_refusal(const sp_air_ext* ext) { return ext && ext->size != sizeof(sp_air_ext) ? "sp_air_ext.size is not sizeof(sp_air_ext)" : nullptr; }
std::string air_statement_from_c(const sp_air_desc* d, const sp_air_aux_desc* aux, const sp_air_periodic_desc* periodic, const sp_air_stride_desc* strides,
                                 const sp_air_boundary_desc* bvals, bool aux_reads_periodic, uint64_t n, AirStatement& out,
                                 const sp_air_main_desc* main = nullptr, AirMainLevel main_level = AirMainLevel::Main);
// `verify::<F, A>` for a program AIR (verifier.cpp): 1 accept, 0 reject; throws std::runtime_error on a malformed proof or constraint
// program.  st.aux is the prover's business and is not looked at.
int air_verify_host(const uint8_t* proof_bytes, size_t len, const AirStatement& st, const ProofOptionsHost& opt);
// The trace length a proof states (its first eight bytes): what a verifier holds a statement's periods and strides against before it
// parses the rest.  Throws std::runtime_error for a shorter proof.  verifier.cpp
uint64_t proof_trace_length(const uint8_t* proof_bytes, size_t len);

}  // namespace sp
