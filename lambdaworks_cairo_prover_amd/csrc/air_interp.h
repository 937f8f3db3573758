// The device interpreter of a straight-line AIR program (AirOpDev with slots, as air_assign_slots produces it): one lane runs the
// whole program with its values in a per-thread array (scratch); every lane of a launch reads the same op and the same constant.
// What differs between the consumers - the composition on LDE points, the exact row evaluation of the trace check and the report, the
// auxiliary columns' terms - comes in as three functors, inlined with the loop:
//   load(a, b)      -> fe   op 0: a = frame row (or, for an auxiliary program, the row shift itself), b = column
//   periodic(a, b)  -> fe   op 6: a = frame row, b = periodic column; called only when PER
//   out(a, value)           op 5: a = constraint (or the num / den column of an auxiliary program)
// PER = false leaves no test for op 6 in the generated code: a program without periodic columns runs the code it always ran.
#pragma once
#include "stark_kernels.h"
#include "air_words.h"

namespace sp {

struct AirNoPeriodic { __device__ fe operator()(uint32_t, uint32_t) const { return fe_zero(); } };

// op 6 of a row program (the auxiliary terms, the sort keys, the main terms and chains): a = row shift, b = periodic column, read
// relative to the lane's row i - held by reference, since a chain's lane moves it.  A period is a power of two <= n, so (i + shift)
// mod period is a mask and stays inside the column's own values.
struct AirRowPeriodic {
    const AirPeriodicCol* __restrict__ pcols;
    const fe* __restrict__ pvals;
    const uint64_t& i;
    __device__ fe operator()(uint32_t shift, uint32_t col) const {
        const AirPeriodicCol pc = pcols[col];
        return fe_ld(pvals + pc.off + ((i + shift) & ((1ull << pc.logp) - 1ull)));
    }
};

// op 7 of a chain group's seed and step programs (DIV): num / den by one safegcd inversion of the lane's own.  fe_inv runs the same
// instructions whatever the value, so the lanes of a wave stay together; it maps zero to zero.  Out of line: about 12 000 instructions,
// one copy per code object instead of one per program loop that can meet an op 7.  A zero denominator is a compare of the canonical
// value and a plain store of 1 to the flag word.
__device__ __noinline__ inline fe air_quotient(fe num, fe den, int* __restrict__ zero_flag) {   // (by value: in registers, not through scratch)
    if (fe_is_zero(den)) *zero_flag = 1;
    return fe_mul(num, fe_inv(den));
}

// ops 8 .. 11 of a chain group's seed and step programs: functions of the canonical integer (air_words.h), so a value leaves
// Montgomery form, is worked on and goes back - a field product each way.  The op's immediates are the same for every lane, so the
// shift amounts and masks stay scalar; the operands arrive by value, out of the value file, and nothing here indexes a register.
// LIMB: b = lo + 256 width.
__device__ __forceinline__ fe air_int_op_limb(const fe& a, uint32_t b) { return fe_to_mont(air_int_limb(fe_from_mont(a), b & 255u, b >> 8)); }
// AND / OR / XOR (fn = op - 9) of two operands below 2^251.  An operand beyond that is a compare and a plain store of the flag value -
// every lane that stores stores the same word, and no lane leaves early -; the result is masked to 251 bits, a canonical integer
// whatever the operands were.
__device__ __forceinline__ fe air_int_op_word(const fe& a, const fe& b, uint32_t fn, int* __restrict__ range_flag) {
    const fe x = fe_from_mont(a), y = fe_from_mont(b);
    if (air_int_exceeds(x, AIR_INT_OP_BITS) || air_int_exceeds(y, AIR_INT_OP_BITS)) *range_flag = AIR_INT_OP_FLAG_RANGE;
    return fe_to_mont(air_int_word(x, y, fn, AIR_INT_OP_BITS));
}

// DIV = false leaves no test for op 7 either: every consumer but the chain kernel's DIV instantiations compiles the code it compiled
// before, and zero_flag is not looked at.  INT = false does the same for ops 8 .. 11 and range_flag: only the chain kernel's INT
// instantiations know them.
template <bool PER, bool DIV = false, bool INT = false, class Load, class Periodic, class Out>
__device__ __forceinline__ void air_run_program(const AirOpDev* __restrict__ ops, uint32_t n_ops, const fe* __restrict__ consts, Load load,
                                                Periodic periodic, Out out, int* __restrict__ zero_flag = nullptr, int* __restrict__ range_flag = nullptr) {
    fe v[AIR_MAX_LIVE];
    for (uint32_t t = 0; t < n_ops; ++t) {
        const AirOpDev o = ops[t];
        fe r = fe_zero();
        if constexpr (PER) {
            if (o.op == 6) {
                v[o.dst] = periodic(o.a, o.b);
                continue;
            }
        }
        switch (o.op) {
            case 0: r = load(o.a, o.b); break;
            case 1: r = fe_ld(consts + o.a); break;
            case 2: r = fe_add(v[o.a], v[o.b]); break;
            case 3: r = fe_sub(v[o.a], v[o.b]); break;
            case 4: r = fe_mul(v[o.a], v[o.b]); break;
            default:
                if constexpr (DIV) {
                    if (o.op == 7) { r = air_quotient(v[o.a], v[o.b], zero_flag); break; }
                }
                if constexpr (INT) {
                    if (o.op == 8) { r = air_int_op_limb(v[o.a], o.b); break; }
                    if (o.op >= 9) { r = air_int_op_word(v[o.a], v[o.b], o.op - 9u, range_flag); break; }
                }
                out(o.a, v[o.b]);
                continue;
        }
        v[o.dst] = r;
    }
}

}  // namespace sp
