// Derived main-trace columns of a program AIR on gfx950 (see air_main_kernels.h).
#include "air_main_kernels.h"
#include "air_interp.h"
#include "air_words.h"
#include <type_traits>

namespace sp {

// The per-row terms of a chunk are the auxiliary programs' kernel, air_aux_terms (air_aux_kernels.h): the same program shape, the
// same two destinations of an OUT.

// ---- chain groups: one lane per block of s rows, or per run of 2^log_k blocks ---------------------------------------------------
// The serial dimension is the block, s - 1 dependent steps; the n / s blocks are the parallel one.  Work-groups of one wave: the
// waves are few (n / (64 s)) and spread over the CUs this way instead of stacking four to a CU.  The state lives in a per-lane array
// beside the interpreter's values; `next` holds the step's OUTs until the program is through, since an OUT of column j may come before
// a later LOAD of the state of column j.  A lane's stores are 32 s bytes from its neighbour's and stay direct: the kernel is bound by
// its s - 1 dependent steps of several field products each, not by the n w 32 bytes it writes, and a lane fills the other quarters of
// each 128-byte line within its next three steps.
// LINKED (runs of 2^log_k blocks): the blocks of a run are serial too - a seed reads the last state of the block before -, so the lane
// walks the whole run, 2^(log_s + log_k) rows, and the n >> (log_s + log_k) runs are the parallel dimension.  The state starts as zero,
// the carry of a run's first block; after a block's last advance() it holds that block's last row, which is what the next seed
// program's LOADs of the group read (from_state, not from_trace).  An instantiation of its own, not a run-time flag: a group without
// runs (log_k = 0, which the unlinked instantiations do not read) launches the code it always launched.
// DIV (a group whose seed or step program holds an op 7): the interpreter knows DIV, one fe_inv per lane and op - a step is then
// dominated by its inversions, tens of microseconds each against well under one for a polynomial op -, and zero_flag is the word a
// lane that meets a zero denominator stores 1 to.  An instantiation of its own too: zero_flag is not read without it, and a group
// without an op 7 launches the code it always launched, whatever entry point its program came through.
// INT (a group whose seed or step program holds an op 8 .. 11): the interpreter knows the integer LIMB, AND, OR and XOR (air_interp.h) -
// each takes its operands out of Montgomery form and its result back, two to three field products beside a handful of scalar-masked
// limb operations, so a round of an ARX cipher costs what as many MULs would -, and range_flag is the word a lane whose AND / OR / XOR
// operand is at or above 2^251 stores AIR_MAIN_FLAG_INT_RANGE to.  An instantiation of its own as well, for the same reason:
// range_flag is not read without it.  The ops add no per-lane array: operands and results pass through the interpreter's value file.
template <bool PER, bool LINKED, bool DIV, bool INT>
__global__ void __launch_bounds__(64) air_main_chain_kernel(fe* __restrict__ group, const fe* __restrict__ trace, uint64_t n, uint32_t log_s, uint32_t first_col,
                                                            uint32_t w, const AirOpDev* __restrict__ seed_ops, uint32_t n_seed,
                                                            const AirOpDev* __restrict__ step_ops, uint32_t n_step, const fe* __restrict__ consts,
                                                            const AirPeriodicCol* __restrict__ pcols, const fe* __restrict__ pvals, uint32_t log_k,
                                                            int* __restrict__ zero_flag, int* __restrict__ range_flag) {
    const uint32_t log_run = LINKED ? log_s + log_k : log_s;
    const uint64_t L = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (L >= (n >> log_run)) return;   // (with fewer than 64 blocks or runs the only wave is partly empty)
    fe state[AIR_MAIN_CHAIN_WIDTH], next[AIR_MAIN_CHAIN_WIDTH];
    if constexpr (LINKED)
        for (uint32_t j = 0; j < AIR_MAIN_CHAIN_WIDTH; ++j) state[j] = fe_zero();
    uint64_t i = L << log_run;
    const AirRowPeriodic periodic{pcols, pvals, i};
    auto from_trace = [&](uint32_t shift, uint32_t col) { return fe_ld(trace + (uint64_t)col * n + ((i + shift) & (n - 1))); };
    auto from_state = [&](uint32_t shift, uint32_t col) {   // (col - first_col wraps to a large value for a column before the group)
        return col - first_col < w ? state[col - first_col] : from_trace(shift, col);
    };
    auto to_next = [&](uint32_t j, const fe& val) { next[j] = val; };
    auto advance = [&]() {
        for (uint32_t j = 0; j < w; ++j) {
            state[j] = next[j];
            fe_st(group + (uint64_t)j * n + i, next[j]);
        }
    };
    // (always inlined: a linked group calls it with one load functor for seeds and steps, and an out-of-line copy would take its
    // arguments and the captured arrays through the call's stack)
    auto run = [&](const AirOpDev* ops, uint32_t n_ops, auto load) __attribute__((always_inline)) {
        if constexpr (PER) air_run_program<true, DIV, INT>(ops, n_ops, consts, load, periodic, to_next, zero_flag, range_flag);
        else air_run_program<false, DIV, INT>(ops, n_ops, consts, load, AirNoPeriodic{}, to_next, zero_flag, range_flag);
    };
    auto block = [&](auto seed_load) {   // the seeds on the block's first row, then its s - 1 steps; leaves i on the block's last row
        run(seed_ops, n_seed, seed_load);
        advance();
        const uint64_t last = i + (1ull << log_s) - 1;
        while (i < last) {
            run(step_ops, n_step, from_state);
            ++i;
            advance();
        }
    };
    if constexpr (LINKED) {
        // a seed's LOAD of the group is the carry, the state the block before left (zero in front of a run)
        for (const uint64_t run_end = i + (1ull << log_run); i < run_end; ++i) block(from_state);
    } else {
        block(from_trace);
    }
}

// log_k = 0: an unlinked group, one lane per block; log_k >= 1: runs of 2^log_k blocks, one lane per run.  zero_flag non-null: the
// programs hold an op 7; range_flag non-null: they hold an op 8 .. 11.
int air_main_chain(hipStream_t st, fe* trace, uint64_t n, uint32_t log_s, uint32_t log_k, uint32_t first_col, uint32_t w, const AirOpDev* seed_ops,
                   uint32_t n_seed, const AirOpDev* step_ops, uint32_t n_step, const fe* consts, const AirPeriodicCol* pcols, const fe* pvals,
                   int* zero_flag, int* range_flag) {
    if (n == 0 || (n & (n - 1)) || log_s == 0 || log_s + log_k >= 64 || (1ull << (log_s + log_k)) > n || w == 0 || w > AIR_MAIN_CHAIN_WIDTH ||
        (pcols == nullptr) != (pvals == nullptr))
        return SP_E_INVALID_ARG;
    const uint64_t lanes = n >> (log_s + log_k);
    const dim3 grid((unsigned)((lanes + 63) / 64));
    fe* group = trace + (uint64_t)first_col * n;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, group, trace, n, log_s, first_col, w, seed_ops, n_seed, step_ops, n_step, consts, pcols, pvals, log_k,
                           zero_flag, range_flag);
    };
    auto pick = [&](auto div, auto ints) {   // (the two switches as types: one ladder over PER and LINKED for the four pairs)
        constexpr bool DIV = decltype(div)::value, INT = decltype(ints)::value;
        if (log_k == 0) pcols ? launch(air_main_chain_kernel<true, false, DIV, INT>) : launch(air_main_chain_kernel<false, false, DIV, INT>);
        else pcols ? launch(air_main_chain_kernel<true, true, DIV, INT>) : launch(air_main_chain_kernel<false, true, DIV, INT>);
    };
    if (range_flag) zero_flag ? pick(std::true_type{}, std::true_type{}) : pick(std::false_type{}, std::true_type{});
    else zero_flag ? pick(std::true_type{}, std::false_type{}) : pick(std::false_type{}, std::false_type{});
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- lookup multiplicities: the join of the sorted looked-up keys against the sorted table keys ---------------------------------
// One lane per sorted table position p.  The head of a run of equal table keys - the stable sort put the run's lowest row there -
// counts its key in the sorted looked-up keys with two binary searches, interleaved in one loop: each step of either is a dependent
// load of 8 bytes out of an array that the sort has just left in the L2, and the two chains overlap.  The lanes of a run behind its
// head store zero; a table of period L keeps n / L - 1 of every n / L lanes out of the loop, which costs nothing but their idle issue
// slots.  Every lane stores one cell, 32 bytes - a sector of its own - at the row the sort carried along: rows is a permutation of
// 0 .. n - 1 (the sort permutes what the key pass wrote, whatever the keys), so every cell is written exactly once and nothing needs
// a memset.  lo and hi stay in [0, n] and mid in [0, n) whatever the arrays hold - keys that were out of range leave kx ordered by
// its low bits only, the searches then end somewhere inside the array and the call is an error already.
__global__ void __launch_bounds__(256) air_main_count_kernel(const uint64_t* __restrict__ kx, const uint64_t* __restrict__ kt, const uint32_t* __restrict__ rows,
                                                             uint64_t n, fe* __restrict__ col) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint64_t key = kt[p];
    const uint32_t row = rows[p];
    uint64_t z = 0;
    if (p == 0 || kt[p - 1] != key) {
        uint64_t lo0 = 0, hi0 = n, lo1 = 0, hi1 = n;   // lower bound: first kx >= key; upper bound: first kx > key
        while (lo0 < hi0 || lo1 < hi1) {
            const uint64_t m0 = lo0 < hi0 ? lo0 + ((hi0 - lo0) >> 1) : 0, m1 = lo1 < hi1 ? lo1 + ((hi1 - lo1) >> 1) : 0;
            const uint64_t a = kx[m0], b = kx[m1];
            if (lo0 < hi0) { if (a < key) lo0 = m0 + 1; else hi0 = m0; }
            if (lo1 < hi1) { if (b <= key) lo1 = m1 + 1; else hi1 = m1; }
        }
        z = lo1 >= lo0 ? lo1 - lo0 : 0;
    }
    if (row < n) fe_st(col + row, fe_from_u64(z));
}

int air_main_count(hipStream_t st, const uint64_t* kx, const uint64_t* kt, const uint32_t* rows, uint64_t n, fe* col) {
    if (n == 0 || n >= (1ull << 32) || !kx || !kt || !rows || !col) return SP_E_INVALID_ARG;
    hipLaunchKernelGGL(air_main_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kx, kt, rows, n, col);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- joint lookup multiplicities: several looked-up values under one column, counted into the sorted table ------------------------
// The looked-up keys are not sorted: the table is, once, and every looked-up key searches it.
// Key pass of the L looked-up values of a joint COUNT column: the key pass of a sorted column (air_aux_sort_terms_kernel) with L OUTs
// and no rows - OUT AIR_AUX_DEN_TAG + k stores key k of row i at keys[k * n + i], out of Montgomery form, its range held against
// key_bits into the same flag word.  An OUT code outside [AIR_AUX_DEN_TAG, AIR_AUX_DEN_TAG + n_keys) stores nothing: the stores stay
// inside keys whatever the program holds.
template <bool PER>
__global__ void __launch_bounds__(256) air_main_list_keys_kernel(const fe* __restrict__ trace, uint64_t n, const AirOpDev* __restrict__ ops, uint32_t n_ops,
                                                                 const fe* __restrict__ consts, uint64_t* __restrict__ keys, uint32_t n_keys, uint32_t key_bits,
                                                                 int* __restrict__ flag, const AirPeriodicCol* __restrict__ pcols, const fe* __restrict__ pvals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    auto load = [&](uint32_t shift, uint32_t col) { return fe_ld(trace + (uint64_t)col * n + ((i + shift) & (n - 1))); };   // n is a power of two
    auto out = [&](uint32_t a, const fe& val) {
        const uint32_t k = a - AIR_AUX_DEN_TAG;
        if (a < AIR_AUX_DEN_TAG || k >= n_keys) return;
        const fe raw = fe_from_mont(val);
        const uint64_t key = (uint64_t)raw.v[0] | ((uint64_t)raw.v[1] << 32);
        const uint32_t high = raw.v[2] | raw.v[3] | raw.v[4] | raw.v[5] | raw.v[6] | raw.v[7];
        if (high || (key_bits < 64 && (key >> key_bits))) atomicExch(flag, AIR_AUX_FLAG_KEY_RANGE);
        keys[(uint64_t)k * n + i] = key;
    };
    if constexpr (PER) air_run_program<true>(ops, n_ops, consts, load, AirRowPeriodic{pcols, pvals, i}, out);
    else air_run_program<false>(ops, n_ops, consts, load, AirNoPeriodic{}, out);
}

int air_main_list_keys(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, uint64_t* keys, uint32_t n_keys,
                       uint32_t key_bits, int* flag, const AirPeriodicCol* pcols, const fe* pvals) {
    if (n == 0 || (n & (n - 1)) || n >= (1ull << 32) || n_keys == 0 || key_bits == 0 || key_bits > 64 || !keys || !flag || (pcols == nullptr) != (pvals == nullptr))
        return SP_E_INVALID_ARG;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace, n, ops, n_ops, consts, keys, n_keys, key_bits, flag, pcols, pvals);
    };
    pcols ? launch(air_main_list_keys_kernel<true>) : launch(air_main_list_keys_kernel<false>);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// One lane per looked-up key: q = k n + i < total = L n, so the lanes of a wave hold neighbouring rows of one X_k.  The search is the
// one of air_main_fetch_kernel - the lower bound of the key in kt, the head of its run of equal table keys; lo, hi and every probe stay
// in [0, n) whatever the arrays hold, and kt[n] is never read.  A key that is found adds 1 to the 64-bit counter of its head (L n may
// pass 2^32), a key in no table row adds nothing.  Padding rows all look up one value, so without more every lane of every wave would
// queue on one address: the lanes of a wave that hit the same head combine first.  Each turn of the loop takes the head of the first
// lane still waiting (a wave-uniform value out of v_readlane), votes which lanes wait for the same head, and lets that first lane add
// the number of votes in one atomic; a wave on one address is through in one turn and one atomic, a wave on 64 different heads in 64
// turns of a few scalar instructions each - less than its 64 searches' dependent loads.  Integer adds commute: the counters do not
// depend on the order of arrival.  No lane leaves before the loop: a lane beyond `total` or without a match just never waits.
__global__ void __launch_bounds__(256) air_main_count_many_kernel(const uint64_t* __restrict__ kx, uint64_t total, const uint64_t* __restrict__ kt, uint64_t n,
                                                                  unsigned long long* __restrict__ counters) {
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t head = 0;
    bool waiting = false;
    if (q < total) {
        const uint64_t key = kx[q];
        uint64_t lo = 0, hi = n;   // lower bound: first kt >= key
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (kt[mid] < key) lo = mid + 1; else hi = mid;
        }
        const uint64_t p = lo < n ? lo : n - 1;
        waiting = lo < n && kt[p] == key;
        head = (uint32_t)p;   // (p < n < 2^32)
    }
    const uint32_t lane = threadIdx.x & 63u;
    for (;;) {
        const unsigned long long todo = __ballot(waiting);
        if (todo == 0) break;
        const uint32_t first = (uint32_t)__ffsll(todo) - 1u;
        const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)head, (int)first);
        const bool same = waiting && head == at;
        const unsigned long long votes = __ballot(same);
        if (lane == first && at < n) atomicAdd(counters + at, (unsigned long long)__popcll(votes));
        waiting = waiting && !same;
    }
}

// One lane per sorted table position p: the counter on the head of a run of equal table keys - the stable sort put the run's lowest row
// there -, zero behind it, to the row the sort carried along.  rows is a permutation of 0 .. n - 1, so every cell of the column is
// written exactly once, as in air_main_count_kernel.
__global__ void __launch_bounds__(256) air_main_count_store_kernel(const unsigned long long* __restrict__ counters, const uint64_t* __restrict__ kt,
                                                                   const uint32_t* __restrict__ rows, uint64_t n, fe* __restrict__ col) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t row = rows[p];
    const uint64_t z = (p == 0 || kt[p - 1] != kt[p]) ? counters[p] : 0;
    if (row < n) fe_st(col + row, fe_from_u64(z));
}

int air_main_count_many(hipStream_t st, const uint64_t* kx, uint32_t n_lists, const uint64_t* kt, const uint32_t* rows, uint64_t n, uint64_t* counters, fe* col) {
    if (n == 0 || n >= (1ull << 32) || n_lists == 0 || n_lists > 16 || !kx || !kt || !rows || !counters || !col) return SP_E_INVALID_ARG;
    const uint64_t total = (uint64_t)n_lists * n;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
    hipLaunchKernelGGL(air_main_count_many_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, kx, total, kt, n, cnt);
    hipLaunchKernelGGL(air_main_count_store_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cnt, kt, rows, n, col);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- looked-up values: the join of the looked-up keys, in row order, against the sorted table keys -----------------------------
// One lane per row i, so the w stores of a lane are coalesced with its neighbours' into the group's columns.  The search is one
// chain of dependent 8-byte loads out of kt, which the sort has just left in the L2 (log2 n + 1 of them); neighbouring rows look up
// unrelated keys, so nothing of it can be shared or staged.  The lower bound of a key is the head of its run of equal table keys, and
// the stable sort put the run's lowest row there.  Each of the w gathers is a 32-byte read - a sector of its own wherever it lands, as
// in air_aux_gather - and they are independent of one another.  lo, hi and every probe stay in [0, n) whatever the arrays hold: keys
// that were out of range leave kt ordered by its low bits only, the search then ends somewhere inside the array and the call is an
// error already; kt[n] is never read, and a row that the arrays do not bound (rows is a permutation of 0 .. n - 1) reads row 0.
// No LDS, no scratch: the lane's state is a key, two bounds and one value in flight.
__global__ void __launch_bounds__(256) air_main_fetch_kernel(const uint64_t* __restrict__ kx, const uint64_t* __restrict__ kt, const uint32_t* __restrict__ rows,
                                                             const fe* __restrict__ vals, uint64_t n, fe* __restrict__ cols, uint32_t w,
                                                             int* __restrict__ miss_flag) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = kx[i];
    uint64_t lo = 0, hi = n;   // lower bound: first kt >= key
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (kt[mid] < key) lo = mid + 1; else hi = mid;
    }
    const uint64_t p = lo < n ? lo : n - 1;
    const bool found = lo < n && kt[p] == key;
    uint64_t src = found ? rows[p] : 0;
    if (src >= n) src = 0;
    if (!found) *miss_flag = AIR_MAIN_FLAG_MISSING_KEY;
    for (uint32_t j = 0; j < w; ++j) fe_st(cols + (uint64_t)j * n + i, fe_ld(vals + (uint64_t)j * n + src));
}

int air_main_fetch(hipStream_t st, const uint64_t* kx, const uint64_t* kt, const uint32_t* rows, const fe* vals, uint64_t n, fe* cols, uint32_t w,
                   int* miss_flag) {
    if (n == 0 || n >= (1ull << 32) || w == 0 || !kx || !kt || !rows || !vals || !cols || !miss_flag) return SP_E_INVALID_ARG;
    hipLaunchKernelGGL(air_main_fetch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kx, kt, rows, vals, n, cols, w, miss_flag);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// Both stores happen on every row, with values chosen by mask: no lane takes a path of its own.
__global__ void __launch_bounds__(256) air_main_zero_guard_kernel(fe* __restrict__ ws, fe* __restrict__ cols, const uint32_t* __restrict__ tab, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = tab[2 * blockIdx.y], col = tab[2 * blockIdx.y + 1];
    fe* p = ws + (uint64_t)slot * n + i;
    const fe v = fe_ld(p), one = fe_one();
    const uint32_t zero = fe_is_zero(v) ? 0xffffffffu : 0u;
    fe guarded, mark;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        guarded.v[l] = (one.v[l] & zero) | (v.v[l] & ~zero);
        mark.v[l] = one.v[l] & ~zero;
    }
    fe_st(p, guarded);
    fe_st(cols + (uint64_t)col * n + i, mark);
}

int air_main_zero_guard(hipStream_t st, fe* ws, fe* cols, const uint32_t* tab, uint32_t n_inv, uint64_t n) {
    if (n_inv == 0) return SP_OK;
    hipLaunchKernelGGL(air_main_zero_guard_kernel, dim3((unsigned)((n + 255) / 256), n_inv), dim3(256), 0, st, ws, cols, tab, n);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// The bit position is the same for every lane (it comes from the table): the limb is picked by a chain of uniform selects, not by
// indexing the value's registers.
__global__ void __launch_bounds__(256) air_main_bits_kernel(const fe* __restrict__ ws, fe* __restrict__ cols, const uint32_t* __restrict__ gtab,
                                                            const uint32_t* __restrict__ etab, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = gtab[3 * blockIdx.y], first = gtab[3 * blockIdx.y + 1], count = gtab[3 * blockIdx.y + 2];
    const fe raw = fe_from_mont(fe_ld(ws + (uint64_t)slot * n + i));
    const fe one = fe_one();
    for (uint32_t e = first; e < first + count; ++e) {
        const uint32_t col = etab[2 * e], bit = etab[2 * e + 1];
        uint32_t limb = 0;
#pragma unroll
        for (uint32_t l = 0; l < 8; ++l) limb = (bit >> 5) == l ? raw.v[l] : limb;
        const uint32_t set = 0u - ((limb >> (bit & 31)) & 1u);
        fe out;
#pragma unroll
        for (int l = 0; l < 8; ++l) out.v[l] = one.v[l] & set;
        fe_st(cols + (uint64_t)col * n + i, out);
    }
}

int air_main_bits(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n) {
    if (n_groups == 0) return SP_OK;
    hipLaunchKernelGGL(air_main_bits_kernel, dim3((unsigned)((n + 255) / 256), n_groups), dim3(256), 0, st, ws, cols, gtab, etab, n);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- limbs and bitwise words: row-local functions of a value's canonical integer -------------------------------------------------
// The shape of the bits kernel: one lane per row, blockIdx.y the group, the group's value out of Montgomery form once, then one
// column per entry.  lo and width come from the table and are the same for every lane, so air_int_limb's selects, shift amount and
// masks are scalars.  Each entry pays one fe_to_mont (a field product) and one 32-byte store, coalesced with the neighbours' into the
// column.  No LDS, no scratch.
__global__ void __launch_bounds__(256) air_main_limbs_kernel(const fe* __restrict__ ws, fe* __restrict__ cols, const uint32_t* __restrict__ gtab,
                                                             const uint32_t* __restrict__ etab, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = gtab[3 * blockIdx.y], first = gtab[3 * blockIdx.y + 1], count = gtab[3 * blockIdx.y + 2];
    const fe raw = fe_from_mont(fe_ld(ws + (uint64_t)slot * n + i));
    for (uint32_t e = first; e < first + count; ++e) {
        const uint32_t col = etab[3 * e], lo = etab[3 * e + 1], width = etab[3 * e + 2];
        fe_st(cols + (uint64_t)col * n + i, fe_to_mont(air_int_limb(raw, lo, width)));
    }
}

int air_main_limbs(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n) {
    if (n_groups == 0) return SP_OK;
    hipLaunchKernelGGL(air_main_limbs_kernel, dim3((unsigned)((n + 255) / 256), n_groups), dim3(256), 0, st, ws, cols, gtab, etab, n);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// Two values out of Montgomery form per row and group.  The range test is a compare and a plain store of the flag value - every lane
// that stores stores the same word, and no lane leaves early -; air_int_word masks its result to `bits`, so every cell is written once
// and holds a canonical integer whatever the operands were.
__global__ void __launch_bounds__(256) air_main_words_kernel(const fe* __restrict__ ws, fe* __restrict__ cols, const uint32_t* __restrict__ gtab,
                                                             const uint32_t* __restrict__ etab, uint64_t n, int* __restrict__ range_flag) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = gtab[4 * blockIdx.y], first = gtab[4 * blockIdx.y + 1], count = gtab[4 * blockIdx.y + 2], bits = gtab[4 * blockIdx.y + 3];
    const fe a = fe_from_mont(fe_ld(ws + (uint64_t)slot * n + i));
    const fe b = fe_from_mont(fe_ld(ws + (uint64_t)(slot + 1) * n + i));
    if (air_int_exceeds(a, bits) || air_int_exceeds(b, bits)) *range_flag = AIR_MAIN_FLAG_WORD_RANGE;
    for (uint32_t e = first; e < first + count; ++e) {
        const uint32_t col = etab[2 * e], fn = etab[2 * e + 1];
        fe_st(cols + (uint64_t)col * n + i, fe_to_mont(air_int_word(a, b, fn, bits)));
    }
}

int air_main_words(hipStream_t st, const fe* ws, fe* cols, const uint32_t* gtab, const uint32_t* etab, uint32_t n_groups, uint64_t n, int* range_flag) {
    if (n_groups == 0) return SP_OK;
    if (!range_flag) return SP_E_INVALID_ARG;
    hipLaunchKernelGGL(air_main_words_kernel, dim3((unsigned)((n + 255) / 256), n_groups), dim3(256), 0, st, ws, cols, gtab, etab, n, range_flag);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

}  // namespace sp
