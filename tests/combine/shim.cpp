// TEST HARNESS ONLY (never linked into libblsw.so): compiles fr.hpp and vcombine.hpp of bls-verify-gadget_amd/csrc for the HOST with g++ and runs
// the stages of blsw_combine_points_batch, blsw_lagrange_batch and blsw_recover_points_batch (k_combine.hip), lanes one after the other, so that
// the kernels' logic is checked against Python integers and the affine group law without a GPU (pytest -m "not gpu").
#include <cstring>
#include <vector>
#include "../../bls-verify-gadget_amd/csrc/vcombine.hpp"

using namespace blsw;

namespace {
struct ParkHost {  // ParkRows on the host: the term's 16 parked points
    Jac2* p;
    void st(int slot, const Jac2& v) const { p[slot] = v; }
    Jac2 ld(int slot) const { return p[slot]; }
};
struct Stages {  // CombineArgs on the host
    uint32_t group, k;
    uint64_t n;
    const uint32_t* counts;
    const uint8_t* scalars;
    const int32_t* lag;
    int32_t* term_status;
    uint8_t* out;
    int32_t* status;
};
// k_decode_points, k_combine_status, k_combine_scale_g1 / _g2, k_combine_sum
void combine_stages(const Stages& a, const uint8_t* in) {
    const uint64_t m = a.n * a.k;
    std::vector<Fp> xy(m * (a.group == 1 ? 2 : 4));
    std::vector<int32_t> pst(m);
    for (uint64_t t = 0; t < m; t++) {
        if (a.group == 1) {
            pst[t] = g1_decode(in + t * 48, xy[2 * t], xy[2 * t + 1]);
        } else {
            Fp2 x, y;
            pst[t] = g2_decode(in + t * 96, x, y);
            xy[4 * t] = x.c0, xy[4 * t + 1] = x.c1, xy[4 * t + 2] = y.c0, xy[4 * t + 3] = y.c1;
        }
    }
    for (uint64_t i = 0; i < a.n; i++)
        a.status[i] = cb_list_status(cb_count(a.counts, i, a.k), a.k, a.lag ? a.lag[i] : (int32_t)DEC_OK, pst.data() + i * a.k, a.scalars + 32 * i * a.k);
    std::vector<Jac1v> s1(a.group == 1 ? m : 0);
    std::vector<Jac2> s2(a.group == 2 ? 16 * m : 0);
    for (uint64_t t = 0; t < m; t++) {
        const uint64_t i = t / a.k;
        const uint32_t j = (uint32_t)(t % a.k);
        uint32_t w[8];
        const int32_t ss = cb_scalar(a.scalars + 32 * t, w);
        if (a.term_status) a.term_status[2 * t] = pst[t], a.term_status[2 * t + 1] = ss;
        const bool live = a.status[i] == DEC_OK && j < cb_count(a.counts, i, a.k) && pst[t] == DEC_OK;
        if (a.group == 1) {
            s1[t] = cb_scale_g1(xy[2 * t], xy[2 * t + 1], w, live);
        } else {
            const ParkHost park = {s2.data() + 16 * t};
            park.st(0, cb_scale_g2(park, Fp2{xy[4 * t], xy[4 * t + 1]}, Fp2{xy[4 * t + 2], xy[4 * t + 3]}, w, live));
        }
    }
    for (uint64_t i = 0; i < a.n; i++) {
        const uint32_t bytes = a.group == 1 ? 48u : 96u;
        uint8_t* o = a.out + i * bytes;
        if (a.status[i] != DEC_OK) {
            memset(o, 0, bytes);
            continue;
        }
        const uint64_t first = i * a.k;
        const uint32_t count = cb_count(a.counts, i, a.k);
        if (a.group == 1)
            cb_encode_g1(cb_sum_g1(count, [&](uint32_t j) { return s1[first + j]; }), o);
        else
            cb_encode_g2(cb_sum_g2(count, [&](uint32_t j) { return s2[16 * (first + j)]; }), o);
    }
}
// k_lagrange, k_lagrange_status
void lagrange_stages(const uint8_t* ids, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* coeff, int32_t* status) {
    for (uint64_t t = 0; t < n * k; t++) {
        const uint64_t i = t / k;
        cb_lagrange_lane(ids + 32 * i * k, cb_count(counts, i, k), k, (uint32_t)(t % k), coeff + 32 * t);
    }
    for (uint64_t i = 0; i < n; i++) status[i] = cb_lagrange_status(ids + 32 * i * k, cb_count(counts, i, k), k, coeff + 32 * i * k);
}
}  // namespace

extern "C" {
// Fr, canonical words in and out through the Montgomery form: 0 add, 1 sub, 2 mul, 3 sqr, 4 inv, 5 the conversion there and back, 6 neg
int cb_fr_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const Fr x = fr_from_words(a), y = fr_from_words(b);
    Fr r;
    switch (op) {
        case 0: r = fr_add(x, y); break;
        case 1: r = fr_sub(x, y); break;
        case 2: r = fr_mul(x, y); break;
        case 3: r = fr_sqr(x); break;
        case 4: r = fr_inv(x); break;
        case 5: r = x; break;
        case 6: r = fr_neg(x); break;
        default: return -1;
    }
    fr_to_words(r, out);
    return 0;
}
// the byte decode: 1 and the words for a value below r, 0 otherwise; the bytes written back from the words
int cb_fr_decode(const uint8_t* in32, uint32_t* w, uint8_t* back32) {
    const bool ok = fr_words_from_le32(in32, w);
    fr_words_to_le32(w, back32);
    return ok ? 1 : 0;
}
// the Montgomery constants as the device holds them: R mod r, R^2 mod r, -r^-1 mod 2^32
void cb_fr_constants(uint32_t* r1, uint32_t* r2, uint32_t* inv32) {
    constexpr uint32_t R1[8] = BLSW_FR_R1_WORDS, R2[8] = BLSW_FR_R2_WORDS;
    memcpy(r1, R1, 32);
    memcpy(r2, R2, 32);
    *inv32 = BLSW_FR_INV32;
}
void cb_split(const uint32_t* k, uint64_t* out4) { v1_split_x2(k, out4, out4 + 2); }
// [k] P through the endomorphism ladder: p48 compressed, k 8 words below r -> out48 compressed; returns the point's decode status
int cb_g1_mul(const uint8_t* p48, const uint32_t* k, uint8_t* out48) {
    Fp x, y;
    const int st = g1_decode(p48, x, y);
    if (st == DEC_OK) cb_encode_g1(v1_mul_glv(x, y, k), out48);
    return st;
}
int cb_combine(uint32_t group, const uint8_t* in, const uint8_t* scalars, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* out, int32_t* status, int32_t* term_status) {
    if ((group != 1 && group != 2) || n == 0 || k == 0) return -1;
    combine_stages({group, k, n, counts, scalars, nullptr, term_status, out, status}, in);
    return 0;
}
int cb_lagrange(const uint8_t* ids, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* coeff, int32_t* status) {
    if (n == 0 || k == 0) return -1;
    lagrange_stages(ids, counts, k, n, coeff, status);
    return 0;
}
int cb_recover(uint32_t group, const uint8_t* in, const uint8_t* ids, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* out, int32_t* status) {
    if ((group != 1 && group != 2) || n == 0 || k == 0) return -1;
    std::vector<uint8_t> coeff(n * k * 32);
    std::vector<int32_t> lag(n);
    lagrange_stages(ids, counts, k, n, coeff.data(), lag.data());
    combine_stages({group, k, n, counts, coeff.data(), lag.data(), nullptr, out, status}, in);
    return 0;
}
}
