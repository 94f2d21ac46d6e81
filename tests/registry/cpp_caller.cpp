// TEST PROGRAM: BLS::KeyRegistry, BLS::fast_aggregate_verify_indexed and its _grouped form of include/blsw.hpp from a C++ host, linked to the in-tree
// libblsw.so.
//   cpp_caller <file> <group> <capacity>
// file: line 1 the registry's keys (hex, space separated; appended in two parts); then one line per set: the indices (comma separated, "-" for
// the empty list), message hex, signature hex.
// Prints per set "verdict grouped_verdict status_key status_sig aggregate_hex", then a line "groups v v v ..." and a line "keys s s s ...".
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "blsw.hpp"

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> b(h.size() / 2);
    for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
    return b;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    try {
        std::ifstream in(argv[1]);
        const uint32_t group = (uint32_t)std::stoul(argv[2]), capacity = (uint32_t)std::stoul(argv[3]);
        std::string line, tok;
        std::getline(in, line);
        std::vector<blsw::PublicKey> keys;
        for (std::istringstream ks(line); ks >> tok;) keys.push_back(blsw::PublicKey::try_from(tok));
        std::vector<std::vector<uint32_t>> lists;
        std::vector<std::vector<uint8_t>> msgs;
        std::vector<blsw::Signature> sigs;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string ix, m, s;
            if (!(ls >> ix >> m >> s)) continue;
            std::vector<uint32_t> list;
            if (ix != "-") {
                std::istringstream is(ix);
                while (std::getline(is, tok, ',')) list.push_back((uint32_t)std::stoul(tok));
            }
            lists.push_back(list);
            msgs.push_back(unhex(m));
            sigs.push_back(blsw::Signature::try_from(s));
        }
        blsw::KeyRegistry registry(capacity);
        const size_t half = keys.size() / 2;
        registry.append(std::vector<blsw::PublicKey>(keys.begin(), keys.begin() + half));
        registry.append(std::vector<blsw::PublicKey>(keys.begin() + half, keys.end()));
        if (registry.size() != keys.size() || registry.capacity() != capacity) return 3;
        const blsw::Parameters params;
        std::vector<int32_t> status;
        std::vector<blsw::PublicKey> agg;
        const std::vector<bool> per = blsw::BLS::fast_aggregate_verify_indexed(params, registry, lists, msgs, sigs, 0, {}, &status, &agg);
        const std::vector<bool> via = blsw::BLS::fast_aggregate_verify_indexed_grouped(params, registry, lists, msgs, sigs, group);
        for (size_t i = 0; i < per.size(); i++) {
            std::printf("%d %d %d %d ", (int)per[i], (int)via[i], status[2 * i], status[2 * i + 1]);
            for (uint8_t b : agg[i].bytes) std::printf("%02x", b);
            std::printf("\n");
        }
        std::printf("groups");
        for (bool g : blsw::BLS::fast_aggregate_verify_indexed(params, registry, lists, msgs, sigs, group)) std::printf(" %d", (int)g);
        std::printf("\nkeys");
        for (int32_t s : registry.key_status()) std::printf(" %d", s);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 10;
    }
    return 0;
}
