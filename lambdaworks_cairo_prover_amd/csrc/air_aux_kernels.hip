// Auxiliary columns of a program AIR on gfx950 (see air_aux_kernels.h).
#include "air_aux_kernels.h"
#include "air_interp.h"

namespace sp {

// ---- per-row terms ------------------------------------------------------------------------------------------
// The program runs in the shared interpreter (air_interp.h): LOAD takes the row shift itself, and an OUT stores into the num / den
// column it names.  A program without op 6 runs the PER = false instantiation, which has no test for op 6 in it and does not read
// pcols / pvals; one with table reads gets the columns' descriptors and raw values through AirRowPeriodic.
template <bool PER, class Out>
__device__ __forceinline__ void air_aux_run_row(const fe* __restrict__ trace, uint64_t n, uint64_t i, const AirOpDev* __restrict__ ops, uint32_t n_ops,
                                                const fe* __restrict__ consts, const AirPeriodicCol* __restrict__ pcols, const fe* __restrict__ pvals, Out out) {
    auto load = [&](uint32_t shift, uint32_t col) { return fe_ld(trace + (uint64_t)col * n + ((i + shift) & (n - 1))); };   // n is a power of two
    if constexpr (PER) air_run_program<true>(ops, n_ops, consts, load, AirRowPeriodic{pcols, pvals, i}, out);
    else air_run_program<false>(ops, n_ops, consts, load, AirNoPeriodic{}, out);
}

template <bool PER>
__global__ void __launch_bounds__(256) air_aux_terms_kernel(const fe* __restrict__ trace, uint64_t n, const AirOpDev* __restrict__ ops, uint32_t n_ops,
                                                            const fe* __restrict__ consts, fe* __restrict__ num, fe* __restrict__ den,
                                                            const AirPeriodicCol* __restrict__ pcols, const fe* __restrict__ pvals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    air_aux_run_row<PER>(trace, n, i, ops, n_ops, consts, pcols, pvals, [&](uint32_t a, const fe& val) {
        fe* dst = a < AIR_AUX_DEN_TAG ? num + (uint64_t)a * n : den + (uint64_t)(a - AIR_AUX_DEN_TAG) * n;
        fe_st(dst + i, val);
    });
}

int air_aux_terms(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, fe* num, fe* den,
                  const AirPeriodicCol* pcols, const fe* pvals) {
    if (n == 0 || (n & (n - 1)) || (pcols == nullptr) != (pvals == nullptr)) return SP_E_INVALID_ARG;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace, n, ops, n_ops, consts, num, den, pcols, pvals); };
    pcols ? launch(air_aux_terms_kernel<true>) : launch(air_aux_terms_kernel<false>);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- sorted columns -------------------------------------------------------------------------------------------------
// Key pass: the same program shape, OUT a < AIR_AUX_DEN_TAG storing carried value a at vals[a * n + i] and OUT AIR_AUX_DEN_TAG the
// group's key: out of Montgomery form, its low 64 bits and the row become the pair the radix sort takes; anything above key_bits
// raises the flag (the sort then orders the low bits, all in bounds, and the host refuses the proof).
template <bool PER>
__global__ void __launch_bounds__(256) air_aux_sort_terms_kernel(const fe* __restrict__ trace, uint64_t n, const AirOpDev* __restrict__ ops, uint32_t n_ops,
                                                                 const fe* __restrict__ consts, fe* __restrict__ vals, uint64_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ idx, uint32_t key_bits, int* __restrict__ flag,
                                                                 const AirPeriodicCol* __restrict__ pcols, const fe* __restrict__ pvals) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    air_aux_run_row<PER>(trace, n, i, ops, n_ops, consts, pcols, pvals, [&](uint32_t a, const fe& val) {
        if (a < AIR_AUX_DEN_TAG) { fe_st(vals + (uint64_t)a * n + i, val); return; }
        const fe raw = fe_from_mont(val);
        const uint64_t key = (uint64_t)raw.v[0] | ((uint64_t)raw.v[1] << 32);
        const uint32_t high = raw.v[2] | raw.v[3] | raw.v[4] | raw.v[5] | raw.v[6] | raw.v[7];
        if (high || (key_bits < 64 && (key >> key_bits))) atomicExch(flag, AIR_AUX_FLAG_KEY_RANGE);
        keys[i] = key;
        idx[i] = (uint32_t)i;
    });
}

int air_aux_sort_terms(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, fe* vals, uint64_t* keys,
                       uint32_t* idx, uint32_t key_bits, int* flag, const AirPeriodicCol* pcols, const fe* pvals) {
    if (n == 0 || (n & (n - 1)) || n >= (1ull << 32) || key_bits == 0 || key_bits > 64 || (pcols == nullptr) != (pvals == nullptr)) return SP_E_INVALID_ARG;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace, n, ops, n_ops, consts, vals, keys, idx, key_bits, flag, pcols, pvals);
    };
    pcols ? launch(air_aux_sort_terms_kernel<true>) : launch(air_aux_sort_terms_kernel<false>);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// Gather: one lane per output element, a block's 256 outputs of one column contiguous.  The 32-byte read at vals[idx[i]] is a whole
// sector of its own wherever it lands (nothing of a neighbour's is fetched in vain, and nothing can be coalesced: the order is the
// data's); the writes are the coalesced side.  idx[i] < n: the sort permutes the rows the key pass wrote.
__global__ void __launch_bounds__(256) air_aux_gather_kernel(const fe* __restrict__ vals, const uint32_t* __restrict__ idx, uint64_t n, fe* __restrict__ aux,
                                                             const uint32_t* __restrict__ col_of) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = blockIdx.y;
    fe_st(aux + (uint64_t)col_of[k] * n + i, fe_ld(vals + (uint64_t)k * n + idx[i]));
}
int air_aux_gather(hipStream_t st, const fe* vals, const uint32_t* idx, uint64_t n, fe* aux, const uint32_t* col_of, uint32_t n_cols) {
    if (n_cols == 0) return SP_OK;
    hipLaunchKernelGGL(air_aux_gather_kernel, dim3((unsigned)((n + 255) / 256), n_cols), dim3(256), 0, st, vals, idx, n, aux, col_of);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// The key column is the sorted keys back in Montgomery form: no gather.
__global__ void __launch_bounds__(256) air_aux_key_columns_kernel(const uint64_t* __restrict__ keys, uint64_t n, fe* __restrict__ aux, const uint32_t* __restrict__ col_of) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    fe_st(aux + (uint64_t)col_of[blockIdx.y] * n + i, fe_from_u64(keys[i]));
}
int air_aux_key_columns(hipStream_t st, const uint64_t* keys, uint64_t n, fe* aux, const uint32_t* col_of, uint32_t n_cols) {
    if (n_cols == 0) return SP_OK;
    hipLaunchKernelGGL(air_aux_key_columns_kernel, dim3((unsigned)((n + 255) / 256), n_cols), dim3(256), 0, st, keys, n, aux, col_of);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

__global__ void __launch_bounds__(256) air_aux_apply_den_kernel(fe* __restrict__ num, const fe* __restrict__ dinv, const uint32_t* __restrict__ col_of, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t d = blockIdx.y;
    fe* p = num + (uint64_t)col_of[d] * n + i;
    fe_st(p, fe_mul(fe_ld(p), fe_ld(dinv + (uint64_t)d * n + i)));
}

int air_aux_apply_den(hipStream_t st, fe* num, const fe* dinv, const uint32_t* col_of, uint32_t n_den, uint64_t n) {
    if (n_den == 0) return SP_OK;
    hipLaunchKernelGGL(air_aux_apply_den_kernel, dim3((unsigned)((n + 255) / 256), n_den), dim3(256), 0, st, num, dinv, col_of, n);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

// ---- multi-column exclusive scan --------------------------------------------------------------------------------
// Same three-phase shape as prefix_product (aux_kernels.hip), with a column index in grid.y and the operation chosen by the
// column's kind (uniform over a block).
constexpr int AS_PER_THREAD = 8;
constexpr int AS_BLOCK = 256 * AS_PER_THREAD;   // 2048 elements per block

__device__ __forceinline__ fe as_op(uint32_t kind, const fe& a, const fe& b) { return kind ? fe_add(a, b) : fe_mul(a, b); }
__device__ __forceinline__ fe as_id(uint32_t kind) { return kind ? fe_zero() : fe_one(); }

// inclusive scan of the 256 per-thread partials of a block through LDS; returns this thread's EXCLUSIVE prefix
__device__ __forceinline__ fe as_block_exclusive(uint32_t kind, fe mine, fe* sh, fe* block_total) {
    const uint32_t t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        fe other = sh[t >= off ? t - off : 0];
        __syncthreads();
        if (t >= off) sh[t] = as_op(kind, other, sh[t]);
        __syncthreads();
    }
    fe excl = t == 0 ? as_id(kind) : sh[t - 1];
    if (block_total) *block_total = sh[255];
    return excl;
}

__global__ void __launch_bounds__(256) as_block_totals_kernel(const fe* __restrict__ data, uint64_t n, const uint32_t* __restrict__ kinds, fe* __restrict__ block_tot) {
    __shared__ fe sh[256];
    const uint32_t k = blockIdx.y, kind = kinds[k];
    const fe* col = data + (uint64_t)k * n;
    const uint64_t base = (uint64_t)blockIdx.x * AS_BLOCK + (uint64_t)threadIdx.x * AS_PER_THREAD;
    fe acc = as_id(kind);
    for (int j = 0; j < AS_PER_THREAD; ++j)
        if (base + j < n) acc = as_op(kind, acc, fe_ld(col + base + j));
    fe tot;
    (void)as_block_exclusive(kind, acc, sh, &tot);
    if (threadIdx.x == 0) fe_st(block_tot + (uint64_t)k * gridDim.x + blockIdx.x, tot);
}

// one block per column: the `count` block totals of column blockIdx.x -> their exclusive prefixes, in place
__global__ void __launch_bounds__(256) as_scan_totals_kernel(fe* __restrict__ block_tot, uint64_t count, const uint32_t* __restrict__ kinds) {
    __shared__ fe sh[256];
    const uint32_t kind = kinds[blockIdx.x];
    fe* tot = block_tot + (uint64_t)blockIdx.x * count;
    const uint64_t per = (count + 255) / 256, base = (uint64_t)threadIdx.x * per;
    fe acc = as_id(kind);
    for (uint64_t j = 0; j < per; ++j)
        if (base + j < count) acc = as_op(kind, acc, fe_ld(tot + base + j));
    fe run = as_block_exclusive(kind, acc, sh, nullptr);
    for (uint64_t j = 0; j < per; ++j)
        if (base + j < count) {
            const fe cur = fe_ld(tot + base + j);
            fe_st(tot + base + j, run);
            run = as_op(kind, run, cur);
        }
}

__global__ void __launch_bounds__(256) as_apply_kernel(fe* __restrict__ data, uint64_t n, const uint32_t* __restrict__ kinds, const fe* __restrict__ block_prefix) {
    __shared__ fe sh[256];
    const uint32_t k = blockIdx.y, kind = kinds[k];
    fe* col = data + (uint64_t)k * n;
    const uint64_t base = (uint64_t)blockIdx.x * AS_BLOCK + (uint64_t)threadIdx.x * AS_PER_THREAD;
    fe vals[AS_PER_THREAD];
    fe acc = as_id(kind);
#pragma unroll
    for (int j = 0; j < AS_PER_THREAD; ++j) {
        vals[j] = (base + j < n) ? fe_ld(col + base + j) : as_id(kind);
        acc = as_op(kind, acc, vals[j]);
    }
    fe run = as_op(kind, fe_ld(block_prefix + (uint64_t)k * gridDim.x + blockIdx.x), as_block_exclusive(kind, acc, sh, nullptr));
#pragma unroll
    for (int j = 0; j < AS_PER_THREAD; ++j) {
        if (base + j < n) fe_st(col + base + j, run);   // exclusive: row i gets the elements before it
        run = as_op(kind, run, vals[j]);
    }
}

uint64_t air_aux_scan_blocks(uint64_t n) { return (n + AS_BLOCK - 1) / AS_BLOCK; }

int air_aux_scan(hipStream_t st, fe* data, uint64_t n, uint32_t K, const uint32_t* kinds, fe* block_tot) {
    if (n == 0 || K == 0) return SP_OK;
    const uint64_t blocks = air_aux_scan_blocks(n);
    hipLaunchKernelGGL(as_block_totals_kernel, dim3((unsigned)blocks, K), dim3(256), 0, st, data, n, kinds, block_tot);
    hipLaunchKernelGGL(as_scan_totals_kernel, dim3(K), dim3(256), 0, st, block_tot, blocks, kinds);
    hipLaunchKernelGGL(as_apply_kernel, dim3((unsigned)blocks, K), dim3(256), 0, st, data, n, kinds, block_tot);
    SP_HIP_CHECK(hipGetLastError());
    return SP_OK;
}

}  // namespace sp
