// Derived main-trace columns of a program AIR on the device (include/stark252_hip.h sp_air_main_desc): per-row terms from a
// straight-line program over the main columns that exist already, then what each kind needs on top - a zero guard in front of the
// chunk's one batch inversion (INV_OR_ZERO), the bits of a value (BIT), its limbs (LIMB), two values' AND, OR or XOR (WORD).  VALUE, SUM and PRODUCT columns go on through
// air_aux_apply_den and air_aux_scan (air_aux_kernels.h).  One lane per row, 256-lane blocks, every store coalesced into a column.
// CHAIN columns (block recurrences) are the exception: one lane per block of rows, which walks its block (air_main_chain).
#pragma once
#include "air_aux_kernels.h"

namespace sp {

// The per-row terms of a chunk come from air_aux_terms (air_aux_kernels.h), which documents what a main chunk's OUT codes mean.
// One chain group: columns [first_col, first_col + w) of trace, w <= AIR_MAIN_CHAIN_WIDTH, in blocks of 2^log_s rows.
// log_k = 0 (2^log_s <= n): one lane per block B < n >> log_s, 64-lane work-groups: the seed program once on row B s - OUT j stores
// column j's seed -, then for t = 0 .. s - 2 the step program on row i = B s + t - a LOAD of a group column is the lane's state (the
// decoder allows shift 0 only), every other LOAD row (i + shift) mod n of trace, OUT j the next value of column j - after which the
// state becomes the next values and goes to row i + 1.  Neither program reads the group's columns from memory: what the kernel reads
// and what it writes are apart.
// log_k >= 1, a linked group (runs of 2^log_k blocks, 2^(log_s + log_k) <= n): one lane per run R < n >> (log_s + log_k).  The lane's
// state starts as zero; for each block of its run it runs the seed program on the block's first row - a LOAD of a group column is the
// lane's state, the last row of the block before (the carry; zero on the run's first block), every other LOAD and op 6 as in the step
// program - assigns the w seeds together, and then walks the block as above.  The two cases are instantiations of one kernel body.
// zero_flag: null for a group whose programs hold no op 7 - it launches the instantiation it always launched.  Non-null (a word of
// device memory, zeroed by the caller): the programs may hold op 7 DIV a b = v[a] / v[b], one fe_inv per lane and op; a lane that meets
// a zero denominator stores 1 there (a plain store; every such lane stores the same word) and goes on with a quotient of zero, so all
// its stores stay where they belong and the caller refuses the table once the stream has drained.
// range_flag: null for a group whose programs hold no op 8 .. 11 - it launches the instantiation it always launched.  Non-null (the
// WORD columns' verdict word, zeroed by the caller): the programs may hold op 8 LIMB a, lo + 256 width = (int(v[a]) >> lo) mod 2^width
// and ops 9 .. 11 AND / OR / XOR a b over the canonical integers of v[a] and v[b] (air_words.h); a lane whose AND / OR / XOR operand is
// at or above 2^251 stores AIR_MAIN_FLAG_INT_RANGE there (a plain store; every such lane stores the same word) and goes on with the
// result masked to 251 bits, so every cell is written once and holds a canonical integer.
constexpr uint32_t AIR_MAIN_CHAIN_WIDTH = 16;
constexpr int AIR_MAIN_FLAG_INT_RANGE = 2;   // (beside AIR_MAIN_FLAG_WORD_RANGE, in the same word; air_words.h AIR_INT_OP_FLAG_RANGE)
int air_main_chain(hipStream_t st, fe* trace, uint64_t n, uint32_t log_s, uint32_t log_k, uint32_t first_col, uint32_t w, const AirOpDev* seed_ops,
                   uint32_t n_seed, const AirOpDev* step_ops, uint32_t n_step, const fe* consts, const AirPeriodicCol* pcols = nullptr,
                   const fe* pvals = nullptr, int* zero_flag = nullptr, int* range_flag = nullptr);
// One COUNT column (a lookup multiplicity): kx the n looked-up keys in ascending order, kt the n table keys in ascending order - sorted
// stably, rows[p] the row that table key p came from - all from air_aux_sort_terms and radix_sort_pairs_u64.  One lane per p: on the
// head of a run of equal table keys (p == 0 or kt[p] != kt[p - 1]) z = upper_bound(kx, kt[p]) - lower_bound(kx, kt[p]), elsewhere
// z = 0; col[rows[p]] = z as a field element.  rows is a permutation of 0 .. n - 1: every cell of col is written once.  n < 2^32.
int air_main_count(hipStream_t st, const uint64_t* kx, const uint64_t* kt, const uint32_t* rows, uint64_t n, fe* col);
// A joint COUNT column (one multiplicity column for the L = n_keys looked-up values of a list), in two calls.
// air_main_list_keys: the key pass of the looked-up values - one launch of the interpreter whose OUT AIR_AUX_DEN_TAG + k, k < n_keys,
// stores key k of row i at keys[k * n + i], out of Montgomery form; a canonical integer at or above 2^key_bits stores
// AIR_AUX_FLAG_KEY_RANGE to *flag, the word air_aux_sort_terms uses.  keys holds n_keys * n words.
int air_main_list_keys(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, uint64_t* keys, uint32_t n_keys,
                       uint32_t key_bits, int* flag, const AirPeriodicCol* pcols = nullptr, const fe* pvals = nullptr);
// air_main_count_many: kx the n_lists * n looked-up keys in any order, kt the n table keys in ascending order - sorted stably, rows[p]
// the row that table key p came from -, counters n words that the caller has zeroed on the same stream.  First one lane per looked-up
// key: p = lower_bound(kt, key) over [0, n), and where kt[p] == key one is added to counters[p], the head of the key's run of equal
// table keys - lanes of a wave that hit one head add their sum in one atomic.  Then one lane per p: col[rows[p]] = counters[p] on the
// head of a run, zero behind it, as a field element: every cell of col is written once.  1 <= n_lists <= 16, n < 2^32.
int air_main_count_many(hipStream_t st, const uint64_t* kx, uint32_t n_lists, const uint64_t* kt, const uint32_t* rows, uint64_t n, uint64_t* counters, fe* col);
// A group of w FETCH columns (looked-up values) that share their keys: kx the n looked-up keys in ROW order, kt the n table keys in
// ascending order - sorted stably, rows[p] the row that table key p came from -, vals[j * n + r] the table value of group column j on
// row r.  One lane per row i: p = lower_bound(kt, kx[i]) over [0, n) - the head of the run of equal table keys, its lowest row -, found
// = p < n and kt[p] == kx[i], and cols[j * n + i] = vals[j * n + (found ? rows[p] : 0)] for j < w.  A lane that does not find its key
// stores AIR_MAIN_FLAG_MISSING_KEY to *miss_flag (a plain store; every such lane stores the same word) and writes V of row 0, so all
// its stores stay where they belong and every cell is written once.  1 <= w, n < 2^32.
constexpr int AIR_MAIN_FLAG_MISSING_KEY = 1;
int air_main_fetch(hipStream_t st, const uint64_t* kx, const uint64_t* kt, const uint32_t* rows, const fe* vals, uint64_t n, fe* cols, uint32_t w,
                   int* miss_flag);
// INV_OR_ZERO, before the batch inversion: for k < n_inv, with (slot, col) = tab[2 k], tab[2 k + 1]: where ws[slot * n + i] is zero it
// becomes one and cols[col * n + i] = 0, elsewhere cols[col * n + i] = 1.  The inversion then meets no zero of these, and
// air_aux_apply_den leaves 0 or 1 / N in the column.
int air_main_zero_guard(hipStream_t st, fe* ws, fe* cols, const uint32_t* tab, uint32_t n_inv, uint64_t n);
// BIT: group g < n_groups is gtab[3 g .. 3 g + 2] = (slot, first, count): the value ws[slot * n + i] leaves Montgomery form once, and for
// e in [first, first + count), with (col, bit) = etab[2 e], etab[2 e + 1] (bit <= 251): cols[col * n + i] = that bit of its canonical
// integer, as the field element 0 or 1.
int air_main_bits(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n);
// LIMB: group g < n_groups is gtab[3 g .. 3 g + 2] = (slot, first, count): the value ws[slot * n + i] leaves Montgomery form once, and for
// e in [first, first + count), with (col, lo, width) = etab[3 e .. 3 e + 2] (1 <= width, lo + width <= 252): cols[col * n + i] =
// (that canonical integer >> lo) mod 2^width as a field element (air_words.h air_int_limb).
int air_main_limbs(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n);
// WORD: group g < n_groups is gtab[4 g .. 4 g + 3] = (slot, first, count, bits), 1 <= bits <= 251: a = ws[slot * n + i] and b =
// ws[(slot + 1) * n + i] leave Montgomery form once, and for e in [first, first + count), with (col, fn) = etab[2 e], etab[2 e + 1]:
// cols[col * n + i] = (a AND / OR / XOR b) mod 2^bits for fn = 0 / 1 / 2 (air_int_word).  A lane whose a or b is at or above 2^bits
// stores AIR_MAIN_FLAG_WORD_RANGE to *range_flag (a plain store; every such lane stores the same word) and writes its cells all the
// same: every cell is written once.
constexpr int AIR_MAIN_FLAG_WORD_RANGE = 1;
int air_main_words(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n, int* range_flag);

}  // namespace sp
