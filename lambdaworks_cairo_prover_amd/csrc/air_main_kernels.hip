// Derived main-trace columns of a program AIR on gfx950 (see air_main_kernels.h).
#include "air_main_kernels.h"
#include "air_interp.h"

namespace sp {

// The third user of the shared interpreter's periodic-free body (beside the composition and air_aux_terms_kernel): LOAD takes the row
// shift itself, an OUT stores into the chunk column or the workspace slot it names.
__global__ void __launch_bounds__(256) air_main_terms_kernel(const fe* __restrict__ trace, uint64_t n, const AirOpDev* __restrict__ ops, uint32_t n_ops,
                                                             const fe* __restrict__ consts, fe* __restrict__ cols, fe* __restrict__ ws) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    air_run_program<false>(
        ops, n_ops, consts,
        [&](uint32_t shift, uint32_t col) { return fe_ld(trace + (uint64_t)col * n + ((i + shift) & (n - 1))); },   // n is a power of two
        AirNoPeriodic{},
        [&](uint32_t a, const fe& val) {
            fe* dst = a < AIR_AUX_DEN_TAG ? cols + (uint64_t)a * n : ws + (uint64_t)(a - AIR_AUX_DEN_TAG) * n;
            fe_st(dst + i, val);
        });
}

int air_main_terms(hipStream_t st, const fe* trace, uint64_t n, const AirOpDev* ops, uint32_t n_ops, const fe* consts, fe* cols, fe* ws) {
    if (n == 0 || (n & (n - 1))) return SP_E_INVALID_ARG;
    hipLaunchKernelGGL(air_main_terms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, trace, n, ops, n_ops, consts, cols, ws);
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

}  // namespace sp
