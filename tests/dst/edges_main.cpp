// TEST PROGRAM (stand-alone, built with -fsanitize=address,undefined; run on the CPU only): the host construction of the tag argument and the
// lane function of k_sha_values_dst (csrc/sha.hpp) at the boundary tags — every tag length at which b_i gains a block, crossed with the message
// lengths that put b_0's end one byte below, on and one byte above a block boundary. Every message is a heap block of exactly msg_len bytes and the
// argument a heap block of exactly its size, so a read beyond either is a heap overflow the sanitizer reports. The expected bytes come from a
// byte-oriented expand_message_xmd written here (msg_prime built as bytes, padded, hashed block by block).
//   edges_main      prints one line per case, exits 0 iff every word is as expected
#include <cstdio>
#include <memory>
#include <vector>
#include "shim.cpp"

static void sha256_bytes(const std::vector<uint8_t>& m, uint8_t out[32]) {
    constexpr uint32_t H0[8] = BLSW_SHA_H0;
    std::vector<uint8_t> p(m);
    p.push_back(0x80);
    while (p.size() % 64 != 56) p.push_back(0);
    for (int k = 7; k >= 0; k--) p.push_back((uint8_t)(((uint64_t)m.size() * 8) >> (8 * k)));
    uint32_t st[8];
    for (int i = 0; i < 8; i++) st[i] = H0[i];
    for (size_t b = 0; b < p.size(); b += 64) {
        uint32_t w[16];
        for (int j = 0; j < 16; j++) w[j] = ((uint32_t)p[b + 4 * j] << 24) | ((uint32_t)p[b + 4 * j + 1] << 16) | ((uint32_t)p[b + 4 * j + 2] << 8) | p[b + 4 * j + 3];
        sha256_compress_plain(st, w);
    }
    for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(st[i] >> (24 - 8 * k));
}
static void expand_bytes(const uint8_t* msg, uint32_t msg_len, const std::vector<uint8_t>& dst, uint32_t words[64]) {
    std::vector<uint8_t> dp(dst), mp(64, 0);
    dp.push_back((uint8_t)dst.size());
    mp.insert(mp.end(), msg, msg + msg_len);
    mp.push_back(0x01);
    mp.push_back(0x00);
    mp.push_back(0x00);
    mp.insert(mp.end(), dp.begin(), dp.end());
    uint8_t b0[32], b[32];
    sha256_bytes(mp, b0);
    for (uint32_t i = 1; i <= 8; i++) {
        std::vector<uint8_t> in(32);
        for (int k = 0; k < 32; k++) in[k] = i == 1 ? b0[k] : (uint8_t)(b0[k] ^ b[k]);
        in.push_back((uint8_t)i);
        in.insert(in.end(), dp.begin(), dp.end());
        sha256_bytes(in, b);
        for (int k = 0; k < 8; k++) words[8 * (i - 1) + k] = ((uint32_t)b[4 * k] << 24) | ((uint32_t)b[4 * k + 1] << 16) | ((uint32_t)b[4 * k + 2] << 8) | b[4 * k + 3];
    }
}

int main() {
    const uint32_t tag_lens[] = {1, 2, 21, 22, 43, 85, 86, 149, 150, 213, 214, 254, 255};
    const uint8_t fill[] = {0x00, 0x80, 0xff, 0x41};
    int failures = 0, cases = 0;
    for (uint32_t L : tag_lens) {
        std::vector<uint8_t> dst(L);
        for (uint32_t k = 0; k < L; k++) dst[k] = fill[(k + L) % 4];
        std::vector<uint32_t> lens = {0, 1, 2, 3, 4, 5};
        const uint32_t k0 = (77 + L) / 64 + 1;  // the first block boundaries behind the empty message's end
        for (uint32_t k = k0; k <= k0 + 2; k++)  // 77 + msg_len + L = 64 k - 1, 64 k, 64 k + 1 (the last byte of the length field ends a block at 64 k)
            for (int d = -1; d <= 1; d++) {
                const int64_t m = 64ll * k + d - 77 - L;
                if (m >= 0) lens.push_back((uint32_t)m);
            }
        for (uint32_t msg_len : lens) {
            std::unique_ptr<uint8_t[]> msg(new uint8_t[msg_len ? msg_len : 1]);  // exactly msg_len bytes (none: a one-byte block, never read)
            for (uint32_t k = 0; k < msg_len; k++) msg[k] = (uint8_t)(0xA7 * k + L);
            std::unique_ptr<DstArg> a(new DstArg);
            bool ok = dst_arg_build(a.get(), dst.data(), L, msg_len) == 0;
            ok = ok && a->bi_blocks == (43 + L + 63) / 64 && a->b0_blocks + 1 == (77 + msg_len + L + 63) / 64;
            ok = ok && a->b0_blocks * 16 - a->msg_words <= BLSW_DST_B0_SUFFIX_WORDS && a->bi_blocks * 16 - 8 <= BLSW_DST_BI_TAIL_WORDS;  // what the lanes index
            uint32_t got[64], want[64];
            if (ok) {
                expand_message_values_dst(msg.get(), a.get(), got);
                expand_bytes(msg.get(), msg_len, dst, want);
                ok = std::memcmp(got, want, sizeof(got)) == 0;
            }
            std::printf("L %3u msg_len %3u b_0 blocks %u b_i blocks %u %s\n", L, msg_len, a->b0_blocks + 1, a->bi_blocks, ok ? "ok" : "FAILED");
            failures += !ok;
            cases++;
        }
    }
    // the tag lengths the library refuses, and NULL
    DstArg a;
    const uint8_t one[256] = {1};
    const bool refused = dst_arg_build(&a, one, 0, 32) != 0 && dst_arg_build(&a, one, 256, 32) != 0 && dst_arg_build(&a, nullptr, 4, 32) != 0 && dst_arg_build(nullptr, one, 4, 32) != 0;
    std::printf("tag lengths 0 and 256, NULL arguments refused: %s\n", refused ? "ok" : "FAILED");
    failures += !refused;
    std::printf("%d cases, %d failures\n", cases + 1, failures);
    return failures ? 1 : 0;
}
