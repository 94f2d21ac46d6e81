// TEST PROGRAM (stand-alone, built with -fsanitize=address,undefined; run on the CPU only): the run rule and the host stages of
// blsw_verify_groups_shared_batch over the edge shapes. Every array is a heap block of exactly its stated length — the table at n_msgs rows, the
// slot arrays at n — so that a row read for an index beyond the table, or a slot touched beyond a group, is a heap overflow the sanitizer reports.
//   edges_main      prints one line per case, exits 0 iff every verdict, status, run count and GT comparison is as expected
#include <cstdio>
#include <memory>
#include "shim.cpp"

static const uint32_t R_WORDS[8] = BLSW_R_WORDS;
struct Triple {
    uint8_t pk[48], sig[96];
};
// (sk g1, sk H(msg)); negate: the key r - sk
static Triple mint(uint32_t sk, bool negate, const uint8_t* msg, uint32_t msg_len) {
    uint32_t k[8] = {sk, 0, 0, 0, 0, 0, 0, 0};
    if (negate) {
        uint64_t borrow = 0;
        for (int i = 0; i < 8; i++) {
            const uint64_t d = (uint64_t)R_WORDS[i] - k[i] - borrow;
            k[i] = (uint32_t)d;
            borrow = (d >> 32) & 1;
        }
    }
    Triple t;
    Fp x, y;
    g1_mul_affine(K_G1_GEN_X(), fp_neg(K_G1_GEN_NEG_Y()), k, x, y);
    g1_encode(x, y, false, t.pk);
    Fp2 hx, hy, sx, sy;
    bool inf;
    hash_to_g2_affine(msg, msg_len, hx, hy, inf);
    g2_mul_affine(hx, hy, k, sx, sy);
    g2_encode(sx, sy, false, t.sig);
    return t;
}

struct Case {
    const char* name;
    uint32_t msg_len, n_msgs, group;
    std::vector<uint32_t> key;     // per instance: which secret key (bit 31: its negation)
    std::vector<uint32_t> signs;   // per instance: the table row the signature is over
    std::vector<uint32_t> index;   // per instance: msg_index
    std::vector<uint64_t> scalar;  // per instance
    std::vector<int32_t> want;     // per group
    std::vector<uint32_t> runs;    // per group
};

static int run_rule() {
    int failures = 0;
    const std::vector<std::vector<uint32_t>> arrays = {{0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 1, 1, 2, 2, 2}, {5, 5, 7, 7, 7, 7, 7, 7, 7, 7, 7, 5}};
    for (const auto& a : arrays)
        for (uint32_t group = 1; group <= 12; group++)
            for (uint32_t tile : {1u, 2u, 5u, 64u}) {
                const uint64_t n = a.size(), G = vg_groups(n, group);
                const uint32_t cpg = vg_chunks_per_group(n, group, 2);
                std::unique_ptr<uint32_t[]> idx(new uint32_t[n]), lead(new uint32_t[n]), len(new uint32_t[n]), runs(new uint32_t[G]), cc(new uint32_t[G * cpg]);
                std::unique_ptr<uint8_t[]> leader(new uint8_t[n]), bad(new uint8_t[n]), cw(new uint8_t[G * cpg]);
                std::unique_ptr<uint64_t[]> cf(new uint64_t[G * cpg]);
                for (uint64_t i = 0; i < n; i++) idx[i] = a[i], lead[i] = len[i] = 0xffffffffu;
                bool ok = vshared_rule(n, group, 2, tile, idx.get(), 6, leader.get(), lead.get(), len.get(), runs.get(), bad.get(), cf.get(), cc.get(), cw.get()) == (int32_t)cpg;
                for (uint64_t g = 0; g < G && ok; g++) {  // the slots tile the group, in order
                    uint64_t at = g * group;
                    for (uint32_t k = 0; k < runs[g]; k++) {
                        ok = ok && lead[g * group + k] == at && len[g * group + k] >= 1;
                        at += len[g * group + k];
                    }
                    ok = ok && at == g * group + vs_group_size(n, group, g);
                    for (uint32_t k = runs[g]; k < vs_group_size(n, group, g); k++) ok = ok && lead[g * group + k] == 0xffffffffu && len[g * group + k] == 0xffffffffu;
                }
                if (!ok) std::printf("rule: array of %zu, group %u, tile %u FAILED\n", a.size(), group, tile);
                failures += !ok;
            }
    std::printf("rule: %d failures\n", failures);
    return failures;
}

int main() {
    int failures = run_rule();
    const uint32_t NEG = 0x80000000u;
    const uint64_t MAX = ~0ull;
    const std::vector<Case> cases = {
        {"one run per instance", 32, 9, 9, {1, 2, 3, 4, 5, 6, 7, 8, 9}, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {0, 1, 2, 3, 4, 5, 6, 7, 8}, {3, MAX, 1, 5, 7, 9, 11, 13, 1ull << 63}, {1}, {9}},
        {"a run of 9", 32, 1, 9, {1, 2, 3, 4, 5, 6, 7, 8, 9}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}, {3, MAX, 1, 5, 7, 9, 11, 13, 1ull << 63}, {1}, {1}},
        {"A B A, and a tampered index in the second group", 65, 3, 3, {1, 2, 3, 4, 5, 6}, {0, 1, 0, 2, 2, 2}, {0, 1, 0, 2, 1, 2}, {3, 5, 7, 9, 11, 13}, {1, 0}, {3, 3}},
        {"a run never crosses a group", 32, 2, 4, {1, 2, 3, 4, 5, 6, 7}, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {3, 5, 7, 9, 11, 13, 15}, {0, 1}, {3, 1}},
        {"an index at n_msgs and one at 0xffffffff", 32, 2, 2, {1, 2, 3, 4, 5, 6}, {0, 0, 1, 1, 0, 1}, {0, 2, 1, 0xffffffffu, 0, 1}, {3, 5, 7, 9, 11, 13}, {0, 0, 1}, {2, 2, 2}},
        {"the same key and scalar twice in a run", 0, 1, 3, {1, 1, 2}, {0, 0, 0}, {0, 0, 0}, {9, 9, 5}, {1}, {1}},
        {"sk and r - sk: a group with no pair", 32, 1, 2, {7, 7 | NEG}, {0, 0}, {0, 0}, {7, 7}, {1}, {1}},
        {"the cancelling pair and a tampered third", 32, 2, 3, {7, 7 | NEG, 3}, {0, 0, 0}, {0, 0, 1}, {7, 7, 5}, {0}, {2}},
        {"a zero scalar inside a run", 32, 1, 4, {1, 2, 3, 4}, {0, 0, 0, 0}, {0, 0, 0, 0}, {3, 0, 5, 7}, {0}, {1}},
    };
    for (const Case& c : cases) {
        const uint32_t n = (uint32_t)c.key.size();
        const uint64_t G = vg_groups(n, c.group);
        std::unique_ptr<uint8_t[]> table(new uint8_t[c.msg_len * c.n_msgs ? c.msg_len * c.n_msgs : 1]), pk(new uint8_t[48 * n]), sig(new uint8_t[96 * n]);
        for (uint32_t b = 0; b < c.msg_len * c.n_msgs; b++) table[b] = (uint8_t)(0x40 + b / c.msg_len + 7 * (b % c.msg_len));
        std::unique_ptr<uint32_t[]> idx(new uint32_t[n]), runs(new uint32_t[G]);
        std::unique_ptr<uint64_t[]> sc(new uint64_t[n]), fs(new uint64_t[72 * G]), fp(new uint64_t[72 * G]);
        std::unique_ptr<int32_t[]> st_s(new int32_t[2 * n]), st_p(new int32_t[2 * n]), rs(new int32_t[G]), rp(new int32_t[G]), same(new int32_t[G]);
        for (uint32_t i = 0; i < n; i++) {
            const Triple t = mint(c.key[i] & ~NEG, (c.key[i] & NEG) != 0, table.get() + c.msg_len * c.signs[i], c.msg_len);
            std::memcpy(pk.get() + 48 * i, t.pk, 48);
            std::memcpy(sig.get() + 96 * i, t.sig, 96);
            idx[i] = c.index[i];
            sc[i] = c.scalar[i];
        }
        for (uint32_t chunk : {8u, 2u})
            for (uint32_t tile : {64u, 2u}) {
                const int64_t rc = vshared_groups(pk.get(), sig.get(), table.get(), c.msg_len, c.n_msgs, idx.get(), sc.get(), n, c.group, chunk, tile, st_s.get(), st_p.get(), rs.get(),
                                                  rp.get(), runs.get(), fs.get(), fp.get(), same.get());
                bool ok = rc == (int64_t)G;
                for (uint64_t g = 0; g < G && ok; g++) ok = rs[g] == c.want[g] && rp[g] == c.want[g] && runs[g] == c.runs[g] && same[g] == 1;
                for (uint32_t i = 0; i < n && ok; i++)
                    ok = st_s[2 * i] == (c.index[i] >= c.n_msgs ? VS_BAD_INDEX : DEC_OK) && st_s[2 * i + 1] == DEC_OK && st_p[2 * i] == DEC_OK && st_p[2 * i + 1] == DEC_OK;
                std::printf("%-52s chunk %u tile %2u rc %lld %s\n", c.name, chunk, tile, (long long)rc, ok ? "ok" : "FAILED");
                failures += !ok;
            }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
