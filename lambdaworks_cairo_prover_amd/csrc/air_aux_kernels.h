// Auxiliary (RAP) columns of a program AIR on the device (include/stark252_hip.h sp_air_aux_desc): per-row numerators and
// denominators from a straight-line program over the main trace, then one exclusive scan per column (grand product or running
// sum); sorted columns by a key pass, the radix sort of sort_kernels.h and a gather.  The Cairo counterpart is aux_kernels.h; these kernels leave it alone.
#pragma once
#include "common.h"
#include "stark_kernels.h"

namespace sp {

// An aux program on the device is an AirOpDev list (slots assigned by air_assign_slots) whose OUT ops (op 5) write a result:
// OUT a < AIR_AUX_DEN_TAG stores the value as N of chunk column a at num[a * n + i]; OUT a = AIR_AUX_DEN_TAG + d stores it as
// denominator d at den[d * n + i].  LOAD a = row shift (0 .. 7), b = main column: row (i + a) mod n of the natural-order trace.
constexpr uint16_t AIR_AUX_DEN_TAG = 0x8000;
constexpr uint32_t AIR_AUX_MAX_SHIFT = 7;

// One thread per row: evaluates the program once and writes every N and D it names (column-major, coalesced across rows).
// trace: [main_cols][n] natural order; consts: the aux constants followed by the RAP challenges.
// pcols / pvals (both null for a program without op 6, which then launches the instantiation that reads neither): the periodic columns an op 6
// reads, a = row shift, b = column k: pvals[off_k + ((i + a) mod period_k)] - the raw values, as the exact trace check reads them.
// A row-local chunk of the main program (build_main_program) runs through the same call: trace then holds the inputs and the derived
// columns of earlier chunks, num is the chunk's first column and den the workspace - OUT AIR_AUX_DEN_TAG + s stores into slot s at
// den[s * n + i]: a denominator, the N of an INV_OR_ZERO column or the N of a BIT group.
int air_aux_terms(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, fe* num, fe* den,
                  const AirPeriodicCol* pcols = nullptr, const fe* pvals = nullptr);
// Sorted columns (SP_AIR_AUX_SORTED), one sort group at a time.  Key pass, one thread per row: the group's program, OUT a <
// AIR_AUX_DEN_TAG storing carried value a at vals[a * n + i], OUT AIR_AUX_DEN_TAG the key - taken out of Montgomery form, its low 64
// bits to keys[i] with idx[i] = i (what radix_sort_pairs_u64 sorts); a key with a bit at or above key_bits sets *flag to
// AIR_AUX_FLAG_KEY_RANGE (batch_inverse sets the same word to 1 for a zero denominator).  keys / idx may be null for a program
// without the key's OUT (further carried values of a group whose key is sorted already).  n < 2^32.
constexpr int AIR_AUX_FLAG_KEY_RANGE = 2;
int air_aux_sort_terms(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, fe* vals, uint64_t* keys,
                       uint32_t* idx, uint32_t key_bits, int* flag, const AirPeriodicCol* pcols = nullptr, const fe* pvals = nullptr);
// aux[col_of[k] * n + i] = vals[k * n + idx[i]]  for k < n_cols, i < n  (idx: a permutation of 0 .. n - 1)
int air_aux_gather(hipStream_t st, const fe* vals, const uint32_t* idx, uint64_t n, fe* aux, const uint32_t* col_of, uint32_t n_cols);
// aux[col_of[k] * n + i] = keys[i] as a field element: the key column of a group from its sorted keys
int air_aux_key_columns(hipStream_t st, const uint64_t* keys, uint64_t n, fe* aux, const uint32_t* col_of, uint32_t n_cols);
// num[col_of[d] * n + i] *= dinv[d * n + i]  for d < n_den, i < n
int air_aux_apply_den(hipStream_t st, fe* num, const fe* dinv, const uint32_t* col_of, uint32_t n_den, uint64_t n);
// In-place EXCLUSIVE scan of K columns of n elements (column k at data + k * n), shifted by one row: out[0] = identity,
// out[i] = x[0] op .. op x[i-1].  kinds[k] = 0: product (identity 1), 1: sum (identity 0).  One launch per phase for all
// columns: block totals, scan of the totals, apply.  block_tot: K * air_aux_scan_blocks(n) elements.
uint64_t air_aux_scan_blocks(uint64_t n);
int air_aux_scan(hipStream_t st, fe* data, uint64_t n, uint32_t K, const uint32_t* kinds, fe* block_tot);

}  // namespace sp
