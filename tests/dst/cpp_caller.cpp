// TEST PROGRAM: BLS::pop_prove -> BLS::pop_verify and a tagged BLS::sign -> BLS::verify of include/blsw.hpp from a C++ host, linked to the in-tree
// libblsw.so.
//   cpp_caller <secret key hex, big-endian> [...]
// Prints per key "pk proof status verdict" (hex, hex, PopProve's status, PopVerify's verdict), then a line "swapped v v ..." with PopVerify's
// verdicts on each key with its neighbour's proof, then a line "tagged a b c": BLS::verify of signatures made under the tag "cpp_caller" — under
// that tag, under the library's, and under Dst::library() given explicitly for signatures made with no tag (1 0 1 expected, per key all alike).
#include <cstdio>
#include "blsw.hpp"

static void put_hex(const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%02x", b[i]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        std::vector<blsw::SecretKey> sks;
        for (int i = 1; i < argc; i++) sks.push_back(blsw::SecretKey::try_from(argv[i]));
        const size_t n = sks.size();
        const blsw::Parameters params;
        const blsw::BLS::Proved p = blsw::BLS::pop_prove(params, sks);
        const std::vector<bool> ok = blsw::BLS::pop_verify(params, p.public_keys, p.proofs);
        for (size_t i = 0; i < n; i++) {
            put_hex(p.public_keys[i].bytes.data(), 48);
            std::printf(" ");
            put_hex(p.proofs[i].bytes.data(), 96);
            std::printf(" %d %d\n", p.status[i], (int)ok[i]);
        }
        std::vector<blsw::Signature> rot(n);
        for (size_t i = 0; i < n; i++) rot[i] = p.proofs[(i + 1) % n];
        const std::vector<bool> sw = blsw::BLS::pop_verify(params, p.public_keys, rot);
        std::printf("swapped");
        for (size_t i = 0; i < n; i++) std::printf(" %d", (int)sw[i]);
        std::printf("\n");
        const blsw::Dst tag(std::string("cpp_caller"));
        std::vector<std::vector<uint8_t>> msgs(n, std::vector<uint8_t>{'m', 's', 'g'});
        const blsw::BLS::Signed s = blsw::BLS::sign(params, sks, msgs, tag), s0 = blsw::BLS::sign(params, sks, msgs);
        const std::vector<bool> a = blsw::BLS::verify(params, s.public_keys, msgs, s.signatures, nullptr, tag), b = blsw::BLS::verify(params, s.public_keys, msgs, s.signatures),
                                c = blsw::BLS::verify(params, s0.public_keys, msgs, s0.signatures, nullptr, blsw::Dst::library());
        bool all_a = true, any_b = false, all_c = true;
        for (size_t i = 0; i < n; i++) {
            all_a = all_a && a[i];
            any_b = any_b || b[i];
            all_c = all_c && c[i];
        }
        std::printf("tagged %d %d %d\n", (int)all_a, (int)any_b, (int)all_c);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
