// The Fiat-Shamir transcript on the host, for the whole-proof drivers and the verifier: DefaultTranscript of lambdaworks-crypto
// @ a17b951 and the sampling rules of reference src/starks/transcript.rs:13-79.
#pragma once
#include "fp.h"
#include "keccak.h"
#include <vector>

namespace sp {

struct Transcript {
    std::vector<uint8_t> buf;   // after a challenge: the 32 bytes of state (what fri_commit_chain continues from on the device)
    void append(const uint8_t* d, size_t n) { buf.insert(buf.end(), d, d + n); }
    void append_felt(const fe& x) { uint8_t b[32]; fe_to_bytes_be(x, b); append(b, 32); }
    void append_u64_be(uint64_t v) { uint8_t b[8]; for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (56 - 8 * i)); append(b, 8); }   // the nonce
    void challenge(uint8_t out[32]) {
        uint8_t d[32];
        sp_keccak256_host(buf.data(), buf.size(), d);
        for (int i = 0; i < 32; ++i) out[i] = d[31 - i];
        buf.assign(out, out + 32);
    }
    fe to_field() {
        uint8_t r[32];
        challenge(r);
        r[0] &= 0x07;  // 251 random bits (transcript.rs:24-43)
        return fe_from_bytes_be(r);
    }
    uint64_t to_usize() {
        uint8_t r[32];
        challenge(r);
        uint64_t v = 0;
        for (int i = 0; i < 8; ++i) v = (v << 8) | r[i];
        return v;
    }
};

// z outside the trace domain (2^logn points) and the LDE coset (2^logN points, offset 1 / hinv): transcript.rs:53-69
inline fe sample_z_outside_domains(Transcript& t, const fe& hinv, uint32_t logn, uint32_t logN) {
    for (;;) {
        const fe z = t.to_field();
        fe a = fe_mul(z, hinv), b = z;
        for (uint32_t i = 0; i < logN; ++i) a = fe_sqr(a);
        for (uint32_t i = 0; i < logn; ++i) b = fe_sqr(b);
        if (!fe_eq(a, fe_one()) && !fe_eq(b, fe_one())) return z;
    }
}

}  // namespace sp
