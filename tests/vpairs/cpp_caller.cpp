// TEST PROGRAM: BLS::aggregate_verify of include/blsw.hpp from a C++ host, linked to the in-tree libblsw.so.
//   cpp_caller <file>
// file: one line per instance: the keys (hex, comma separated, "-" for the empty list), the messages (hex, comma separated, "-"), signature hex.
// Prints per instance "verdict status_keys status_sig", then a line "keys s s s ..." with the statuses of every key, the padding included.
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
    if (argc != 2) return 2;
    try {
        std::ifstream in(argv[1]);
        std::string line, tok;
        std::vector<std::vector<blsw::PublicKey>> keys;
        std::vector<std::vector<std::vector<uint8_t>>> msgs;
        std::vector<blsw::Signature> sigs;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string k, m, s;
            if (!(ls >> k >> m >> s)) continue;
            std::vector<blsw::PublicKey> kl;
            std::vector<std::vector<uint8_t>> ml;
            if (k != "-") {
                std::istringstream ks(k), ms(m);
                while (std::getline(ks, tok, ',')) kl.push_back(blsw::PublicKey::try_from(tok));
                while (std::getline(ms, tok, ',')) ml.push_back(unhex(tok));
            }
            keys.push_back(kl);
            msgs.push_back(ml);
            sigs.push_back(blsw::Signature::try_from(s));
        }
        std::vector<int32_t> status, key_status;
        const std::vector<bool> r = blsw::BLS::aggregate_verify(blsw::Parameters(), keys, msgs, sigs, &status, &key_status);
        for (size_t i = 0; i < r.size(); i++) std::printf("%d %d %d\n", (int)r[i], status[2 * i], status[2 * i + 1]);
        std::printf("keys");
        for (int32_t s : key_status) std::printf(" %d", s);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
