// Weighted point sums sum_j s_j P_j in G1 and G2 for caller-chosen full-size PUBLIC scalars, and Lagrange coefficients at 0 over Fr
// (blsw_combine_points_batch, blsw_lagrange_batch, blsw_recover_points_batch): what threshold recovery of a signature or of a group key is.
// Stages (k_combine.hip; tests/combine runs them on the host, lanes one after the other):
//   decode    k_decode_points of the aggregate path, unchanged: one lane per term, affine coordinates and a decode status
//   lagrange  (recover only) one lane per (list, j): lambda_j = prod_{m != j} id_m * (prod_{m != j} (id_m - id_j))^-1, one fr_inv per lane; a lane
//             that sees a bad id or a zero difference writes a zero row (a coefficient of valid ids is never 0). Then one lane per list: the
//             list's status, and zero rows throughout a failing list
//   scale     one lane per term: s P as a Jacobian point into the workspace. G2 through v_g2_mul_gls (vsign.hpp), G1 through v1_mul_glv below.
//             A zero scalar, an identity point, a term beyond the count and every term of a failing list give the identity (z = 0)
//   sum       one lane per list: the used terms added with the four-branch additions, one affine conversion, the compressed bytes; zeros for
//             a failing list, the infinity encoding for a sum that is the identity (blsw_aggregate_points_batch's rule)
// G1: phi(x, y) = (beta x, y) acts on G1 as multiplication by -x^2 (decode.hpp: g1_in_subgroup) and r = x^4 - x^2 + 1, so for k < r
//     k = k0 + k1 x^2,  k0 = k mod x^2,  k1 = k div x^2,  both < 2^128,     k P = k0 P + k1 (-phi(P)),   -phi(P) = (beta x, -y):
// one joint ladder of 128 doublings and ~96 mixed additions from the affine table {P, -phi(P), P - phi(P)} instead of 255 doublings and ~127
// additions.
// The ladders branch on the scalar's bits, as the signer's do: these entries are for public scalars.
#pragma once
#include "fr.hpp"
#include "vsign.hpp"

namespace blsw {

enum : int32_t { CB_BAD_COUNT = 6, CB_BAD_ID = 7 };  // BLSW_ST_BAD_INDEX, BLSW_ST_BAD_ID

// k (8 little-endian words, k < r) -> k0 = k mod x^2, k1 = k div x^2 as two 64-bit halves each, by restoring division (as v_digits_x)
BLSW_HD void v1_split_x2(const uint32_t* k, uint64_t k0[2], uint64_t k1[2]) {
    const uint64_t n[4] = {k[0] | ((uint64_t)k[1] << 32), k[2] | ((uint64_t)k[3] << 32), k[4] | ((uint64_t)k[5] << 32), k[6] | ((uint64_t)k[7] << 32)};
    uint64_t q[4] = {0, 0, 0, 0}, lo = 0, hi = 0;
#pragma unroll 1
    for (int i = 255; i >= 0; i--) {
        const uint64_t top = hi >> 63;
        hi = (hi << 1) | (lo >> 63);
        lo = (lo << 1) | ((n[i >> 6] >> (i & 63)) & 1);
        if (top || hi > BLSW_X2_HI || (hi == BLSW_X2_HI && lo >= BLSW_X2_LO)) {
            const uint64_t b = lo < BLSW_X2_LO;
            lo -= BLSW_X2_LO;
            hi -= BLSW_X2_HI + b;
            q[i >> 6] |= 1ull << (i & 63);
        }
    }
    k0[0] = lo;
    k0[1] = hi;
    k1[0] = q[0];  // k < r < x^4: the quotient has 128 bits
    k1[1] = q[1];
}
// [k] (px, py) for an affine point of G1 (in the subgroup, not the identity), k < r as 8 words. The additions carry the four branches: the
// accumulator starts as the identity, and at k = r it meets -(P + Q) at the last step (tests/test_combine.py derives where it can meet an entry).
BLSW_HD Jac1v v1_mul_glv(const Fp& px, const Fp& py, const uint32_t* k) {
    Jac1v acc = {fp_one(), fp_one(), fp_zero()};
#ifdef BLSW_COMBINE_PLAIN_G1
    // A/B build only (tools/combine_rate.py, leg d): the plain 255-step double-and-add
#pragma unroll 1
    for (int i = 254; i >= 0; i--) {
        acc = v1_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = v1_add_mixed(acc, px, py);
    }
#else
    uint64_t k0[2], k1[2];
    v1_split_x2(k, k0, k1);
    const Fp qx = fp_mul(px, K_G1_BETA()), qy = fp_neg(py);  // Q = -phi(P) = [x^2] P = (beta x, -y)
    // P + Q as an AFFINE point, by the chord (P != +-Q: x^2 != +-1 mod r and P has order r). The inversion is ~27 products, and it leaves ONE
    // addition body for every table entry: with P + Q Jacobian the lanes of a wavefront that hold digit (1, 1) walk the general addition while the
    // others wait, then wait themselves through the mixed one — measured, that ladder was 1.05x the plain one, not 1.5x (profiles/combine_rate.txt)
    const Fp lam = fp_mul(fp_sub(qy, py), fp_inv(fp_sub(qx, px)));
    const Fp bx = fp_sub(fp_sub(fp_sqr(lam), px), qx), by = fp_sub(fp_mul(lam, fp_sub(px, bx)), py);
#pragma unroll 1
    for (int i = 127; i >= 0; i--) {
        acc = v1_dbl(acc);
        const uint32_t idx = (uint32_t)((k0[i >> 6] >> (i & 63)) & 1) | (uint32_t)(((k1[i >> 6] >> (i & 63)) & 1) << 1);
        if (idx) acc = v1_add_mixed(acc, idx == 1 ? px : idx == 2 ? qx : bx, idx == 1 ? py : idx == 2 ? qy : by);
    }
#endif
    return acc;
}

BLSW_HD bool cb_words_zero(const uint32_t* w) { return (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0; }
// terms list i uses: counts == NULL means all k; a count beyond k stays as it is (CB_BAD_COUNT)
BLSW_HD uint32_t cb_count(const uint32_t* counts, uint64_t i, uint32_t k) { return counts ? counts[i] : k; }
// decode status of a scalar: 32 little-endian bytes, zero included, below r
BLSW_HD int32_t cb_scalar(const uint8_t* le32, uint32_t* w) { return fr_words_from_le32(le32, w) ? DEC_OK : DEC_BAD_ENCODING; }
// The list's status (include/blsw.h: blsw_combine_points_batch). pst, scalars: the list's own rows; lag: the status k_lagrange_status left for
// the list (recover) or DEC_OK. A well-formed identity point and a zero scalar are valid terms.
BLSW_HD int32_t cb_list_status(uint32_t count, uint32_t k, int32_t lag, const int32_t* pst, const uint8_t* scalars) {
    if (count > k) return CB_BAD_COUNT;
    if (count == 0) return DEC_IDENTITY;
    if (lag != DEC_OK) return lag;
#pragma unroll 1
    for (uint32_t j = 0; j < count; j++) {
        if (pst[j] != DEC_OK && pst[j] != DEC_IDENTITY) return pst[j];
        uint32_t w[8];
        if (cb_scalar(scalars + 32 * (uint64_t)j, w) != DEC_OK) return DEC_BAD_ENCODING;
    }
    return DEC_OK;
}
// scale: `live` = the term is used, its list is DEC_OK and its point is not the identity
BLSW_HD Jac1v cb_scale_g1(const Fp& px, const Fp& py, const uint32_t* w, bool live) {
    if (!live || cb_words_zero(w)) return {fp_one(), fp_one(), fp_zero()};
    return v1_mul_glv(px, py, w);
}
template <class PARK>
BLSW_HD Jac2 cb_scale_g2(const PARK& park, const Fp2& qx, const Fp2& qy, const uint32_t* w, bool live) {
    if (!live || cb_words_zero(w)) return {fp2_one(), fp2_one(), fp2_zero()};
    return v_g2_mul_gls(park, Jac2{qx, qy, fp2_one()}, w);
}
// sum of m Jacobian points, ld(j) -> point (vg_sum's loop): equal summands take the doubling branch, opposite ones give the identity
template <class LD>
BLSW_HD Jac1v cb_sum_g1(uint32_t m, const LD& ld) {
    Jac1v acc = {fp_one(), fp_one(), fp_zero()};
#pragma unroll 1
    for (uint32_t j = 0; j < m; j++) acc = v1_add(acc, ld(j));
    return acc;
}
template <class LD>
BLSW_HD Jac2 cb_sum_g2(uint32_t m, const LD& ld) {
    Jac2 acc = {fp2_one(), fp2_one(), fp2_zero()};
#pragma unroll 1
    for (uint32_t j = 0; j < m; j++) acc = v_add(acc, ld(j));
    return acc;
}
// the sum as compressed bytes: one inversion (the inverse of 0 is 0), the infinity encoding for the identity
BLSW_HD void cb_encode_g1(const Jac1v& s, uint8_t* out) {
    const bool inf = fp_is_zero(s.z);
    const Fp zi = fp_inv(s.z), zi2 = fp_sqr(zi);
    g1_encode(fp_mul(s.x, zi2), fp_mul(s.y, fp_mul(zi2, zi)), inf, out);
}
BLSW_HD void cb_encode_g2(const Jac2& s, uint8_t* out) {
    const bool inf = fp2_is_zero(s.z);
    const Fp2 zi = fp2_inv_inl(s.z), zi2 = v_sqr(zi);
    g2_encode(fp2_mul_inl(s.x, zi2), fp2_mul_inl(s.y, fp2_mul_inl(zi2, zi)), inf, out);
}

// lagrange, lane (list, j): ids = the list's [k][32] rows. Writes lambda_j (32 little-endian bytes), or zeros when j is beyond the count, the
// count beyond k, a used id is >= r or zero, or id_j equals another used id (the zero difference is how a duplicate shows).
BLSW_HD void cb_lagrange_lane(const uint8_t* ids, uint32_t count, uint32_t k, uint32_t j, uint8_t* out) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = count <= k && j < count;
    Fr idj = fr_zero(), num = fr_one(), den = fr_one();
    if (ok) {
        ok = fr_words_from_le32(ids + 32 * (uint64_t)j, w) && !cb_words_zero(w);
        idj = fr_from_words(w);
    }
#pragma unroll 1
    for (uint32_t m = 0; ok && m < count; m++) {
        if (m == j) continue;
        ok = fr_words_from_le32(ids + 32 * (uint64_t)m, w) && !cb_words_zero(w);
        const Fr im = fr_from_words(w);
        num = fr_mul(num, im);
        den = fr_mul(den, fr_sub(im, idj));
    }
    ok = ok && !fr_is_zero(den);
    if (ok)
        fr_to_words(fr_mul(num, fr_inv(den)), w);
    else
        for (int i = 0; i < 8; i++) w[i] = 0;
    fr_words_to_le32(w, out);
}
// lagrange, lane (list): the status after the lanes above ran — CB_BAD_COUNT, DEC_IDENTITY (no id), DEC_BAD_ENCODING for a used id >= r, else
// CB_BAD_ID for a used id that is zero or equal to another (its lane left a zero row), else DEC_OK. A failing list gets zero rows throughout.
BLSW_HD int32_t cb_lagrange_status(const uint8_t* ids, uint32_t count, uint32_t k, uint8_t* coeff) {
    int32_t st = count > k ? (int32_t)CB_BAD_COUNT : count == 0 ? (int32_t)DEC_IDENTITY : (int32_t)DEC_OK;
    if (st == DEC_OK) {
        bool bad_id = false;
#pragma unroll 1
        for (uint32_t j = 0; j < count; j++) {
            uint32_t w[8];
            if (!fr_words_from_le32(ids + 32 * (uint64_t)j, w)) {
                st = DEC_BAD_ENCODING;
                break;
            }
            uint32_t any = 0;
            for (int b = 0; b < 32; b++) any |= coeff[32 * (uint64_t)j + b];
            bad_id = bad_id || cb_words_zero(w) || any == 0;
        }
        if (st == DEC_OK && bad_id) st = CB_BAD_ID;
    }
    if (st != DEC_OK && count <= k)  // beyond k every lane of the list wrote zeros already
        for (uint64_t b = 0; b < 32 * (uint64_t)count; b++) coeff[b] = 0;
    return st;
}

}  // namespace blsw
