// The two integer functions of a main-trace program (include/stark252_hip.h SP_AIR_MAIN_LIMB, SP_AIR_MAIN_WORD) over the canonical
// integer of a field element: eight little-endian 32-bit limbs, out of Montgomery form (fe_from_mont).  They are what the shared
// interpreter (air_interp.h, field ops only) cannot express.  Here, and not in a kernel, so that an integer op of a chain group's step
// - a SHA-, Blake- or Keccak-style round - can call them too (air_interp.h, ops 8 .. 11).  lo, width, bits and fn are the same for every lane: every shift
// amount and mask below is a scalar, and no value's registers are indexed with a run-time index.
#pragma once
#include "fp.h"

namespace sp {

constexpr uint32_t AIR_WORD_AND = 0, AIR_WORD_OR = 1, AIR_WORD_XOR = 2;
// The integer ops of a chain step (ops 9 .. 11, fn = op - 9): operands below 2^251 < p, and the value a lane that meets a larger one
// stores to the WORD columns' verdict word.
constexpr uint32_t AIR_INT_OP_BITS = 251;
constexpr int AIR_INT_OP_FLAG_RANGE = 2;

// Limb l of the mask 2^bits - 1 (bits <= 256).
SP_HD uint32_t air_low_mask_limb(uint32_t bits, uint32_t l) {
    return bits >= 32 * l + 32 ? 0xffffffffu : bits <= 32 * l ? 0u : (1u << (bits - 32 * l)) - 1u;
}

// (raw >> lo) mod 2^width, lo <= 255.  The shift by whole limbs is three stages of uniform selects (by 4, 2 and 1 limbs), the shift by
// bits a funnel shift of two neighbouring limbs, the mask a scalar per limb.
SP_HD fe air_int_limb(const fe& raw, uint32_t lo, uint32_t width) {
    uint32_t t[9];
#pragma unroll
    for (int l = 0; l < 8; ++l) t[l] = raw.v[l];
    t[8] = 0u;
    const uint32_t limbs = lo >> 5, sh = lo & 31u;
#pragma unroll
    for (int step = 4; step >= 1; step >>= 1) {
        const bool take = (limbs & (uint32_t)step) != 0;
#pragma unroll
        for (int l = 0; l < 8; ++l) t[l] = take ? (l + step < 8 ? t[l + step] : 0u) : t[l];
    }
    fe out;
#pragma unroll
    for (int l = 0; l < 8; ++l)
        out.v[l] = (uint32_t)((((uint64_t)t[l + 1] << 32) | t[l]) >> sh) & air_low_mask_limb(width, (uint32_t)l);
    return out;
}

// Whether raw >= 2^bits.
SP_HD bool air_int_exceeds(const fe& raw, uint32_t bits) {
    uint32_t high = 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) high |= raw.v[l] & ~air_low_mask_limb(bits, (uint32_t)l);
    return high != 0;
}

// (a AND / OR / XOR b) mod 2^bits: the mask changes nothing for operands below 2^bits, and keeps the result below 2^251 < p - a
// canonical integer - whatever the operands hold.  fn: AIR_WORD_AND, AIR_WORD_OR, AIR_WORD_XOR.
SP_HD fe air_int_word(const fe& a, const fe& b, uint32_t fn, uint32_t bits) {
    fe out;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const uint32_t x = a.v[l], y = b.v[l];
        out.v[l] = (fn == AIR_WORD_AND ? x & y : fn == AIR_WORD_OR ? x | y : x ^ y) & air_low_mask_limb(bits, (uint32_t)l);
    }
    return out;
}

}  // namespace sp
