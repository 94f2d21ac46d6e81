// Bucket-method multi-scalar multiplication sum_j s_j P_j for LONG lists of PUBLIC scalars in G1 and G2 (blsw_msm_points_batch, include/blsw.h):
// the same sum, statuses and bytes as blsw_combine_points_batch (vcombine.hpp), whose per-term ladder and one-lane sum are built for many short
// lists. With c = window_bits, W = ceil(255 / c) windows and B = 2^c buckets per window (bucket 0 is never filled), M = n k terms.
// Stages (k_msm.hip; tests/msm runs the same functions on the host, lanes one after the other, the scatter order a parameter):
//   1 decode    k_decode_points and cb_list_status, unchanged. Terms of a failing list, terms beyond the count, identity points and zero scalars
//               contribute nothing (msm_term_live)
//   2 digits    one lane per term: digit w of the scalar = its bits [w c, w c + c) (the top window is narrower when c does not divide 255: a
//               scalar below r has 255 bits); a count into hist[list][w][digit] for every non-zero digit
//   3 scan      per (list, window): exclusive prefix of the counts, in place, and a copy as the scatter's cursor. 64 lanes share one row: each
//               sums its slice (msm_scan_sum), the lanes' sums are prefixed, each writes its slice (msm_scan_write)
//   4 scatter   one lane per term: its index into sorted[w][list's first term + cursor++]. The order INSIDE a bucket is whatever the cursor gave, so
//               every addition behind this stage is the four-branch form: equal summands double, opposite ones give the identity, and the sum is
//               the same group element — hence the same compressed bytes — in every order
//   5 buckets   one lane per (list, window, bucket): mixed additions of the bucket's affine points into a Jacobian sum
//   6 reduce    sum_b b B_b per window. One lane per segment of BLSW_MSM_SEGMENT buckets [lo, hi) walks hi - 1 .. lo with the running-sum pair
//               (T += B_b; A += T), which leaves A = sum (b - lo + 1) B_b, and adds (lo - 1) T by a double-and-add of at most c steps
//               (msm_segment); then one lane per (list, window) adds its segments (msm_window)
//   7 final     one lane per list: Horner over the windows from the top, c doublings each (msm_final), one inversion, cb_encode_g1 / _g2
// Judgement calls (DESIGN §8 has the figures; profiles/msm_rate.txt the measurement):
//   * no endomorphism split in G1. v1_split_x2 would give 2 k points with 128-bit scalars, half the windows and half the reductions. The bucket
//     stage's work — one mixed addition per (term, window) — stays the same (2 k terms x W / 2 windows), so only stages 6 and 7 would halve, at the
//     price of a 256-step restoring division per term and a second point per term in the workspace. Left out: see DESIGN §8 for the stage times
//   * unsigned digits. Signed digits would halve B (and with it stage 6) but need a carry pass over the windows before the histogram, a
//     conditional negation in the bucket lane, and a window more for the last carry. Left out for the same reason
//   * default c (msm_default_window): among the widths with a wide top window, by the operation count; a caller may pass any 1 .. 16
//   * one long bucket: when every scalar is equal one bucket per window holds all k terms and its lane adds them one after the other. It is
//     correct (the doubling branch serves a repeated point) and it is NOT split; include/blsw.h states the cost
// The registry form (blsw_registry_msm_batch) runs the same stages over a blsw_registry_t's records: its status rule and its claim on positions
// are further down.
// The digits and the bucket indices depend on the scalars: PUBLIC scalars only, as the ladders of vcombine.hpp.
#pragma once
#include "vcombine.hpp"
#include "registry.hpp"

namespace blsw {

#ifndef BLSW_MSM_SEGMENT
#define BLSW_MSM_SEGMENT 32  // buckets per lane of the window reduction: a lane makes 2 x 32 additions + <= c double-and-add steps, a window lane B / 32 more
#endif
#define BLSW_MSM_MAX_WINDOW 16
#define BLSW_MSM_MAX_K (1u << 24)
#define BLSW_MSM_SCAN_LANES 64  // lanes that share one histogram row in the scan
static_assert(BLSW_MSM_SEGMENT >= 1, "a segment holds a bucket");

BLSW_HD uint32_t msm_windows(uint32_t c) { return (255 + c - 1) / c; }
BLSW_HD uint32_t msm_buckets(uint32_t c) { return 1u << c; }
BLSW_HD uint32_t msm_segments(uint32_t c) { return (msm_buckets(c) + BLSW_MSM_SEGMENT - 1) / BLSW_MSM_SEGMENT; }
// The library's choice of c for lists of k terms. A window of few bits is one long bucket per digit: the TOP window holds 255 - c (W - 1) bits,
// and at 2 or 3 bits (c = 7, 9, 11, 12, 14) 4 .. 8 lanes add k / 4 .. k / 8 terms each, one after the other — measured at k = 65 536 in G1:
// c = 11 349 ms, 12 234 ms, 14 254 ms against 13 (8 top bits) 48 ms, 15 (none narrower) 60 ms, 10 (5) 90 ms (profiles/msm_rate.txt). So the
// choice is among the widths whose top window is wide — 5 (5 bits), 8 (7), 13 (8), 15 (15) — and moves up where the operation count says the
// buckets stay filled: k W bucket additions over W B lanes, then a tail of 2 SEGMENT + c + B / SEGMENT additions and W c doublings.
BLSW_HD uint32_t msm_default_window(uint32_t k) { return k < (1u << 9) ? 5 : k < (1u << 15) ? 8 : k < (1u << 19) ? 13 : 15; }
// digit `win` of a scalar below r (8 little-endian words): bits [win c, win c + c); bits from 256 on are zero
BLSW_HD uint32_t msm_digit(const uint32_t* w, uint32_t win, uint32_t c) {
    const uint32_t bit = win * c, word = bit >> 5, sh = bit & 31;
    if (word >= 8) return 0;
    uint32_t v = w[word] >> sh;
    if (sh + c > 32 && word + 1 < 8) v |= w[word + 1] << (32 - sh);  // c <= 16, so sh >= 17 here
    return v & ((1u << c) - 1);
}
// a term adds something: its list is OK, it lies below the count, its point decoded to a finite point and its scalar is not zero
BLSW_HD bool msm_term_live(int32_t list_status, uint32_t j, uint32_t count, int32_t point_status, const uint32_t* w) {
    return list_status == DEC_OK && j < count && point_status == DEC_OK && !cb_words_zero(w);
}
// scan: the slice [lo, hi) of one histogram row. msm_scan_sum -> the slice's total; msm_scan_write, given the total of the slices in front,
// replaces the counts by their exclusive prefix and copies it to the cursor row
BLSW_HD void msm_scan_slice(uint32_t B, uint32_t lane, uint32_t* lo, uint32_t* hi) {
    const uint32_t per = (B + BLSW_MSM_SCAN_LANES - 1) / BLSW_MSM_SCAN_LANES;
    *lo = lane * per < B ? lane * per : B;
    *hi = *lo + per < B ? *lo + per : B;
}
BLSW_HD uint32_t msm_scan_sum(const uint32_t* row, uint32_t lo, uint32_t hi) {
    uint32_t s = 0;
    for (uint32_t b = lo; b < hi; b++) s += row[b];
    return s;
}
BLSW_HD void msm_scan_write(uint32_t* row, uint32_t* cursor, uint32_t lo, uint32_t hi, uint32_t before) {
    for (uint32_t b = lo; b < hi; b++) {
        const uint32_t cnt = row[b];
        row[b] = before;
        cursor[b] = before;
        before += cnt;
    }
}

// The two groups behind one interface: J a Jacobian point, A an affine one; every addition is the four-branch form of vcurve.hpp
struct MsmAff1 {
    Fp x, y;
};
struct MsmAff2 {
    Fp2 x, y;
};
struct MsmG1 {
    typedef Jac1v J;
    typedef MsmAff1 A;
    static constexpr uint32_t ROWS = 3, AFF_ROWS = 2, BYTES = 48;
    static BLSW_HD J zero() { return {fp_one(), fp_one(), fp_zero()}; }
    static BLSW_HD bool is_zero(const J& p) { return fp_is_zero(p.z); }
    static BLSW_HD J add(const J& p, const J& q) { return v1_add(p, q); }
    static BLSW_HD J add_mixed(const J& p, const A& q) { return v1_add_mixed(p, q.x, q.y); }
    static BLSW_HD J dbl(const J& p) { return v1_dbl(p); }
    static BLSW_HD void encode(const J& p, uint8_t* out) { cb_encode_g1(p, out); }
};
struct MsmG2 {
    typedef Jac2 J;
    typedef MsmAff2 A;
    static constexpr uint32_t ROWS = 6, AFF_ROWS = 4, BYTES = 96;
    static BLSW_HD J zero() { return {fp2_one(), fp2_one(), fp2_zero()}; }
    static BLSW_HD bool is_zero(const J& p) { return fp2_is_zero(p.z); }
    static BLSW_HD J add(const J& p, const J& q) { return v_add(p, q); }
    static BLSW_HD J add_mixed(const J& p, const A& q) { return v_add_mixed(p, q.x, q.y); }
    static BLSW_HD J dbl(const J& p) { return v_dbl(p); }
    static BLSW_HD void encode(const J& p, uint8_t* out) { cb_encode_g2(p, out); }
};

// Registry form (blsw_registry_msm_batch): list i is indices[lo .. hi) of a CSR list over a blsw_registry_t, position p carries scalars[p]; the
// points are the registry's decoded records, G1 only. The list's status, one lane per list: bad offsets (registry_list_ok) before anything of the
// list is read; the empty list; then the earliest bad position — an index >= size (its record is never read), a key that is neither OK nor the
// identity, a scalar >= r, in this order within a position. key_status(index) -> the record's status.
// CSR lists that are valid one by one may still share positions (offsets 0, 5, 3, 8: the bad list between lets lists 0 and 2 overlap), and the sorted
// rows have one slot per position. So every OK list counts a claim on each of its positions; a list that meets a claim count other than 1 is
// summed by its own lane with the per-term ladder instead (cb_scale_g1) — right, slow, and only ever met behind a bad list.
template <class KS>
BLSW_HD int32_t msm_registry_status(const uint32_t* indices, const uint8_t* scalars, uint64_t lo, uint64_t hi, uint64_t n_indices, uint32_t size, const KS& key_status) {
    if (!registry_list_ok(lo, hi, n_indices)) return DEC_BAD_INDEX;
    if (lo == hi) return DEC_IDENTITY;
#pragma unroll 1
    for (uint64_t p = lo; p < hi; p++) {
        const uint32_t idx = indices[p];
        if (idx >= size) return DEC_BAD_INDEX;
        const int32_t st = key_status(idx);
        if (st != DEC_OK && st != DEC_IDENTITY) return st;
        uint32_t w[8];
        if (cb_scalar(scalars + 32 * p, w) != DEC_OK) return DEC_BAD_ENCODING;
    }
    return DEC_OK;
}

// 5 buckets: sorted[first .. last) name the bucket's terms, pt(t) -> the affine point of term t
template <class G, class PT>
BLSW_HD typename G::J msm_bucket(const uint32_t* sorted, uint32_t first, uint32_t last, const PT& pt) {
    typename G::J acc = G::zero();
#pragma unroll 1
    for (uint32_t p = first; p < last; p++) acc = G::add_mixed(acc, pt(sorted[p]));
    return acc;
}
// [m] T for m < 2^16, most significant bit first; doubling the identity leaves z = 0
template <class G>
BLSW_HD typename G::J msm_mul_small(const typename G::J& t, uint32_t m) {
    typename G::J acc = G::zero();
    if (G::is_zero(t)) return acc;  // an empty segment, the usual one when the buckets outnumber the terms
#pragma unroll 1
    for (int i = 15; i >= 0; i--) {
        if (m >> (i + 1)) acc = G::dbl(acc);  // nothing to double above the top bit
        if ((m >> i) & 1) acc = G::add(acc, t);
    }
    return acc;
}
// 6 reduce, lane of segment s: sum_{b in [lo, hi)} b B_b with lo = max(1, s SEGMENT), hi = min(B, (s + 1) SEGMENT); bucket(b) -> B_b
template <class G, class LD>
BLSW_HD typename G::J msm_segment(uint32_t s, uint32_t c, const LD& bucket) {
    const uint32_t B = msm_buckets(c);
    const uint32_t lo = s * BLSW_MSM_SEGMENT ? s * BLSW_MSM_SEGMENT : 1;
    const uint32_t hi = (s + 1) * BLSW_MSM_SEGMENT < B ? (s + 1) * BLSW_MSM_SEGMENT : B;
    typename G::J run = G::zero(), acc = G::zero();
#pragma unroll 1
    for (uint32_t b = hi; b > lo; b--) {
        run = G::add(run, bucket(b - 1));
        acc = G::add(acc, run);
    }
    if (lo > 1) acc = G::add(acc, msm_mul_small<G>(run, lo - 1));
    return acc;
}
// 6 reduce, lane of one (list, window): the window's sum from its segments
template <class G, class LD>
BLSW_HD typename G::J msm_window(uint32_t c, const LD& segment) {
    typename G::J acc = G::zero();
    const uint32_t S = msm_segments(c);
#pragma unroll 1
    for (uint32_t s = 0; s < S; s++) acc = G::add(acc, segment(s));
    return acc;
}
// 7 final: sum_w 2^(w c) S_w, from the top window down
template <class G, class LD>
BLSW_HD typename G::J msm_final(uint32_t c, const LD& window) {
    typename G::J acc = G::zero();
#pragma unroll 1
    for (uint32_t w = msm_windows(c); w-- > 0;) {
#pragma unroll 1
        for (uint32_t i = 0; i < c; i++) acc = G::dbl(acc);
        acc = G::add(acc, window(w));
    }
    return acc;
}

}  // namespace blsw
