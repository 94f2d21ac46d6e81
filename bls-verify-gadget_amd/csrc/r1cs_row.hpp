// Row arithmetic of the device R1CS evaluator (k_r1cs.hip): the entry code, the 14-limb accumulator, the term of one entry and the row's
// Montgomery reduction. Host and device: the kernel's row_dot walks entries through row_term and ends with redc14; the test harness
// (tests/hostsim) compiles the same functions for the host and compares them with big integers.
#pragma once
#include "fp.hpp"

namespace blsw {
namespace r1cs {

// an entry's code: the top two bits are its class, the low 30 its payload (POS / NEG: the value v, GEN: the table index)
constexpr uint32_t CLS_POS = 0u, CLS_NEG = 1u, CLS_GEN = 2u;
constexpr uint32_t PAYLOAD_BITS = 30, PAYLOAD = (1u << PAYLOAD_BITS) - 1;

#if defined(__HIPCC__)
typedef uint2 blsw_u2;
#else
struct blsw_u2 {
    uint32_t x, y;
};
#endif

struct Acc {
    uint32_t l[14];
};

BLSW_HD void acc_add(Acc& x, const Fp& v) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) x.l[i] = addc32(x.l[i], v.l[i], c);
    x.l[12] = addc32(x.l[12], 0, c);
    x.l[13] += c;
}
// x += v * z, v < 2^30
BLSW_HD void acc_add_small(Acc& x, const Fp& z, uint32_t v) {
    uint32_t hi = 0, c = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint64_t t = (uint64_t)z.l[i] * v + hi;
        hi = (uint32_t)(t >> 32);
        x.l[i] = addc32(x.l[i], (uint32_t)t, c);
    }
    x.l[12] = addc32(x.l[12], hi, c);
    x.l[13] += c;
}
// p - z (z <= p: a representative of -z below 2^381; 0 gives p, which the reduction absorbs)
BLSW_HD Fp neg_raw(const Fp& z) {
    constexpr uint32_t P[12] = BLSW_P_LIMBS;
    Fp r;
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = subb32(P[i], z.l[i], b);
    return r;
}
// Montgomery reduction of the 448-bit sum: X 2^-384 mod p. X < 2^443 (a row of < 2^32 terms below 2^411), so every partial value
// (X + M p) / 2^(32 i) stays below 2^448 and the result below p + 2^59 < 2p.
BLSW_HD_NOINLINE Fp redc14(Acc x) {
    constexpr uint32_t P[12] = BLSW_P_LIMBS;
    uint32_t* t = x.l;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const uint32_t m = t[0] * BLSW_INV32;
        uint64_t s = (uint64_t)m * P[0] + t[0];  // low word 0
#pragma unroll
        for (int j = 1; j < 12; j++) {
            s = (uint64_t)m * P[j] + t[j] + (s >> 32);
            t[j - 1] = (uint32_t)s;
        }
        s = (uint64_t)t[12] + (s >> 32);
        t[11] = (uint32_t)s;
        s = (uint64_t)t[13] + (s >> 32);
        t[12] = (uint32_t)s;
        t[13] = (uint32_t)(s >> 32);
    }
    Fp r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = t[i];
    return fp_cond_sub_p(r, t[12]);
}
// x += (the coefficient `code` stands for) * z: the class dispatch of one entry. table: the Montgomery coefficients of class GEN
BLSW_HD void row_term(Acc& x, const Fp& z, uint32_t code, const Fp* table) {
    const uint32_t cls = code >> PAYLOAD_BITS, v = code & PAYLOAD;
    if (cls == CLS_GEN) {
        acc_add(x, fp_mul(z, table[v]));
    } else {
        const Fp s = cls == CLS_NEG ? neg_raw(z) : z;
        if (v == 1)
            acc_add(x, s);
        else
            acc_add_small(x, s, v);
    }
}

}  // namespace r1cs
}  // namespace blsw
