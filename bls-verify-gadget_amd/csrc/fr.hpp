// BLS12-381 scalar field Fr (the integers mod r, r the order of G1 and G2): 8 x 32-bit limbs, Montgomery form (R = 2^256), one element per
// lane, always fully reduced — fp.hpp's idiom on the smaller modulus. The scalars of blsw_combine_points_batch and the interpolation
// coefficients of blsw_lagrange_batch (vcombine.hpp, k_combine.hip). Compiles for the host as well (tests/combine).
// The constants come from tools/gen_fr_constants.py.
#pragma once
#include "fp.hpp"
#include "fr_constants.hpp"

namespace blsw {

struct Fr {
    uint32_t l[8];
};

BLSW_HD Fr fr_zero() {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = 0;
    return r;
}
BLSW_HD Fr fr_one() {
    constexpr uint32_t R1[8] = BLSW_FR_R1_WORDS;
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = R1[i];
    return r;
}
BLSW_HD bool fr_is_zero(const Fr& a) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.l[i];
    return o == 0;
}
BLSW_HD bool fr_eq(const Fr& a, const Fr& b) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.l[i] ^ b.l[i];
    return o == 0;
}
// r = a - r if a >= r else a   (a < 2 r, given with its 9th carry word)
BLSW_HD Fr fr_cond_sub_r(const Fr& a, uint32_t top) {
    constexpr uint32_t M[8] = BLSW_FR_MOD_WORDS;
    Fr d;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d.l[i] = subb32(a.l[i], M[i], borrow);
    const bool ge = (top != 0) || (borrow == 0);
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = ge ? d.l[i] : a.l[i];
    return r;
}
BLSW_HD Fr fr_add(const Fr& a, const Fr& b) {
    Fr s;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s.l[i] = addc32(a.l[i], b.l[i], c);
    return fr_cond_sub_r(s, c);
}
BLSW_HD Fr fr_sub(const Fr& a, const Fr& b) {
    constexpr uint32_t M[8] = BLSW_FR_MOD_WORDS;
    Fr d;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d.l[i] = subb32(a.l[i], b.l[i], borrow);
    const uint32_t mask = 0u - borrow;
    uint32_t c = 0;
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = addc32(d.l[i], M[i] & mask, c);
    return r;
}
BLSW_HD Fr fr_neg(const Fr& a) { return fr_sub(fr_zero(), a); }
// Montgomery product a b R^-1 mod r, CIOS over 32-bit limbs (fp_mul_v's rows on 8 limbs: 64 + 64 multiply-adds). r < 2^255, so the running
// value stays below 2 r < 2^256 and the 9th word is 0 after every row.
BLSW_HD Fr fr_mul(const Fr& a, const Fr& b) {
    constexpr uint32_t M[8] = BLSW_FR_MOD_WORDS;
    uint32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t bi = b.l[i];
        uint64_t x[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = (uint64_t)a.l[j] * bi + t[j];
        uint32_t c = 0;
        t[0] = (uint32_t)x[0];
#pragma unroll
        for (int j = 1; j < 8; j++) t[j] = addc32((uint32_t)x[j], (uint32_t)(x[j - 1] >> 32), c);
        t[8] = addc32(t[8], (uint32_t)(x[7] >> 32), c);
        const uint32_t m = t[0] * BLSW_FR_INV32;
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = (uint64_t)m * M[j] + t[j];
        c = 0;
#pragma unroll
        for (int j = 1; j < 8; j++) t[j - 1] = addc32((uint32_t)x[j], (uint32_t)(x[j - 1] >> 32), c);
        t[7] = addc32(t[8], (uint32_t)(x[7] >> 32), c);
        t[8] = c;  // 0: t < 2 r < 2^256
    }
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = t[i];
    return fr_cond_sub_r(r, 0);
}
BLSW_HD Fr fr_sqr(const Fr& a) { return fr_mul(a, a); }
// a^(r - 2) (Fermat): the inverse of a, and 0 for a = 0. One loop, one copy of the square and of the product.
BLSW_HD Fr fr_inv(const Fr& a) {
    constexpr uint32_t E[8] = BLSW_FR_EXP_INV_WORDS;
    Fr r = fr_one();
#pragma unroll 1
    for (int i = 254; i >= 0; i--) {
        r = fr_sqr(r);
        if ((E[i >> 5] >> (i & 31)) & 1) r = fr_mul(r, a);
    }
    return r;
}
// canonical little-endian words (< r) <-> Montgomery form
BLSW_HD Fr fr_from_words(const uint32_t* w) {
    constexpr uint32_t R2[8] = BLSW_FR_R2_WORDS;
    Fr c, r2;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c.l[i] = w[i];
        r2.l[i] = R2[i];
    }
    return fr_mul(c, r2);
}
BLSW_HD void fr_to_words(const Fr& a, uint32_t* w) {
    Fr one = fr_zero();
    one.l[0] = 1;
    const Fr c = fr_mul(a, one);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = c.l[i];
}
// 32 little-endian bytes -> 8 canonical words; false for a value >= r (the range check of sk_from_le32; ZERO IS A LEGAL SCALAR here)
BLSW_HD bool fr_words_from_le32(const uint8_t* in, uint32_t* w) {
    constexpr uint32_t M[8] = BLSW_FR_MOD_WORDS;
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)in[4 * i] | ((uint32_t)in[4 * i + 1] << 8) | ((uint32_t)in[4 * i + 2] << 16) | ((uint32_t)in[4 * i + 3] << 24);
    uint32_t borrow = 0;
    for (int i = 0; i < 8; i++) (void)subb32(w[i], M[i], borrow);
    return borrow != 0;
}
BLSW_HD void fr_words_to_le32(const uint32_t* w, uint8_t* out) {
    for (int i = 0; i < 8; i++) {
        out[4 * i] = (uint8_t)w[i];
        out[4 * i + 1] = (uint8_t)(w[i] >> 8);
        out[4 * i + 2] = (uint8_t)(w[i] >> 16);
        out[4 * i + 3] = (uint8_t)(w[i] >> 24);
    }
}

}  // namespace blsw
