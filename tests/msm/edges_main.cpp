// TEST PROGRAM (stand-alone, built with -fsanitize=address,undefined and 4 buckets per segment; run on the CPU only): the host stages of vmsm.hpp over
// the index-arithmetic edges of the histogram, the scan, the scatter and the segments. Every array — points, scalars, counts, outputs and, in
// shim.cpp, every stage's workspace part — is a heap block of exactly its stated length, so an index past an end is an error the sanitizer reports.
// Each case runs at every window width with the scatter's lanes forward and reversed; the bytes must be equal and equal to the per-term ladder's
// (cb_scale_g1, cb_sum_g1 of vcombine.hpp).
//   edges_main      prints one line per case and window, exits 0 iff everything is as expected
#include <cstdio>
#include <memory>
#include "shim.cpp"

static void unhex(const char* h, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
        unsigned v = 0;
        std::sscanf(h + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}
typedef std::vector<uint8_t> Bytes;
static Bytes le32_pow2(unsigned bit, bool minus_one = false) {  // 2^bit, or 2^bit - 1
    Bytes b(32, 0);
    if (!minus_one) {
        if (bit < 256) b[bit / 8] = (uint8_t)(1u << (bit % 8));
        return b;
    }
    for (unsigned i = 0; i < bit && i < 256; i++) b[i / 8] |= (uint8_t)(1u << (i % 8));
    return b;
}
struct Term {
    int point;  // 0: g, 1: -g, 2: the identity
    Bytes scalar;
};
struct Case {
    const char* name;
    std::vector<std::vector<Term>> lists;  // padded to the longest with zero bytes
    std::vector<uint32_t> counts;
    std::vector<int32_t> status;
};

int main() {
    uint8_t pts[3][48] = {};
    unhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb", pts[0], 48);
    std::memcpy(pts[1], pts[0], 48);
    pts[1][0] ^= 0x20;
    pts[2][0] = 0xC0;
    Bytes r_minus_1(32);
    unhex("00000000fffffffffe5bfeff02a4bd5305d8a10908d83933487d9d2953a7ed73", r_minus_1.data(), 32);
    int failures = 0;
    const uint32_t widths[] = {1, 2, 3, 5, 7, 8, 13, 16};
    for (uint32_t c : widths) {
        const uint32_t W = msm_windows(c), top = c * (W - 1);
        const Bytes zero(32, 0), one = le32_pow2(0), full = le32_pow2(c, true), next = le32_pow2(c), mid = le32_pow2(c * (W / 2)), last_window = le32_pow2(top),
                    seg_first = le32_pow2(2), seg_last = le32_pow2(2, true), bad = le32_pow2(255, true);  // 4 and 3: with 4 buckets per segment, the first of segment 1 and the last of segment 0
        const std::vector<Case> cases = {
            {"one term per edge scalar", {{{0, zero}, {0, one}, {0, full}, {0, next}, {0, mid}, {0, last_window}, {0, r_minus_1}, {0, seg_first}, {0, seg_last}}}, {9}, {DEC_OK}},
            {"all scalars equal, a point twice and its negative", {{{0, full}, {0, full}, {1, full}, {0, full}, {2, full}}}, {5}, {DEC_OK}},
            {"a total that is the identity", {{{0, r_minus_1}, {0, one}}}, {2}, {DEC_OK}},
            {"ragged counts 0, 1, k, k + 1", {{{0, full}, {0, one}, {0, next}}, {{0, r_minus_1}, {0, bad}, {0, bad}}, {{1, next}, {0, full}, {1, r_minus_1}}, {{0, one}, {0, one}, {0, one}}},
             {0, 1, 3, 4}, {DEC_IDENTITY, DEC_OK, DEC_OK, CB_BAD_COUNT}},
            {"a scalar of 2^255 - 1 in the last list", {{{0, one}, {0, full}}, {{0, one}, {0, bad}}}, {2, 2}, {DEC_OK, DEC_BAD_ENCODING}},
        };
        for (const Case& cs : cases) {
            if (c > 8 && &cs != &cases[0]) continue;  // the wide windows (65 536 buckets a window) once: their index arithmetic is the first case's
            const uint64_t n = cs.lists.size();
            uint32_t k = 0;
            for (const auto& l : cs.lists) k = l.size() > k ? (uint32_t)l.size() : k;
            const uint64_t m = n * k;
            std::unique_ptr<uint8_t[]> in(new uint8_t[m * 48]()), sc(new uint8_t[m * 32]()), out_f(new uint8_t[n * 48]), out_r(new uint8_t[n * 48]), want(new uint8_t[n * 48]());
            std::unique_ptr<uint32_t[]> counts(new uint32_t[n]);
            std::unique_ptr<int32_t[]> st_f(new int32_t[n]), st_r(new int32_t[n]);
            std::unique_ptr<uint64_t[]> reversed(new uint64_t[m]);
            for (uint64_t t = 0; t < m; t++) reversed[t] = m - 1 - t;
            for (uint64_t i = 0; i < n; i++) {
                counts[i] = cs.counts[i];
                for (size_t j = 0; j < cs.lists[i].size(); j++) {
                    std::memcpy(&in[(i * k + j) * 48], pts[cs.lists[i][j].point], 48);
                    std::memcpy(&sc[(i * k + j) * 32], cs.lists[i][j].scalar.data(), 32);
                }
                if (cs.status[i] != DEC_OK) continue;
                std::vector<Jac1v> scaled;
                for (uint32_t j = 0; j < counts[i]; j++) {
                    Fp x, y;
                    uint32_t w[8];
                    const int32_t pst = g1_decode(&in[(i * k + j) * 48], x, y);
                    cb_scalar(&sc[(i * k + j) * 32], w);
                    scaled.push_back(cb_scale_g1(x, y, w, pst == DEC_OK));
                }
                cb_encode_g1(cb_sum_g1(counts[i], [&](uint32_t j) { return scaled[j]; }), &want[i * 48]);
            }
            std::memset(out_f.get(), 0x5A, n * 48);
            std::memset(out_r.get(), 0x5A, n * 48);
            const int rc_f = msm_points(1, in.get(), sc.get(), counts.get(), k, n, c, nullptr, out_f.get(), st_f.get());
            const int rc_r = msm_points(1, in.get(), sc.get(), counts.get(), k, n, c, reversed.get(), out_r.get(), st_r.get());
            bool ok = rc_f == 0 && rc_r == 0 && std::memcmp(out_f.get(), out_r.get(), n * 48) == 0 && std::memcmp(out_f.get(), want.get(), n * 48) == 0;
            for (uint64_t i = 0; i < n; i++) ok = ok && st_f[i] == cs.status[i] && st_r[i] == cs.status[i];
            std::printf("c %2u %-55s %s\n", c, cs.name, ok ? "ok" : "FAILED");
            failures += !ok;
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
