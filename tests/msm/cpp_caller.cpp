// TEST PROGRAM: BLS::msm of include/blsw.hpp from a C++ host, next to BLS::combine on the same lists, linked to the in-tree libblsw.so.
//   cpp_caller <file> [window_bits]
// file: one line per list: "g1" or "g2", the points (hex, comma separated), the scalars (32-byte little-endian hex, comma separated).
// Prints per list "status_msm msm_hex status_combine combine_hex"; for the g1 lists then a line "r status hex" each: KeyRegistry::msm over a
// registry that holds every key of the file in order, list i naming its own keys.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "blsw.hpp"

using blsw::BLS;

static BLS::Scalar scalar(const std::string& h) {
    BLS::Scalar s;
    if (h.size() != 64) throw std::runtime_error("a scalar is 64 hex digits");
    for (size_t i = 0; i < 32; i++) s[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
    return s;
}
template <class T>
static std::string hex(const T& bytes) {
    std::string o;
    char b[3];
    for (uint8_t v : bytes) {
        std::snprintf(b, sizeof b, "%02x", v);
        o += b;
    }
    return o;
}
template <class POINT>
static void run(const std::vector<std::vector<POINT>>& pts, const std::vector<std::vector<BLS::Scalar>>& scalars, uint32_t window_bits) {
    std::vector<int32_t> st_m, st_c;
    const std::vector<POINT> msm = BLS::msm(pts, scalars, &st_m, window_bits), com = BLS::combine(pts, scalars, &st_c);
    for (size_t i = 0; i < msm.size(); i++) std::printf("%d %s %d %s\n", st_m[i], hex(msm[i].bytes).c_str(), st_c[i], hex(com[i].bytes).c_str());
}

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) return 2;
    try {
        const uint32_t window_bits = argc == 3 ? (uint32_t)std::stoul(argv[2]) : 0;
        std::ifstream in(argv[1]);
        std::string line, tok;
        std::vector<std::vector<blsw::PublicKey>> pks;
        std::vector<std::vector<blsw::Signature>> sigs;
        std::vector<std::vector<BLS::Scalar>> s1, s2;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string g, p, x;
            if (!(ls >> g >> p >> x)) continue;
            std::vector<BLS::Scalar> xs;
            std::istringstream ps(p), is(x);
            while (std::getline(is, tok, ',')) xs.push_back(scalar(tok));
            if (g == "g1") {
                std::vector<blsw::PublicKey> l;
                while (std::getline(ps, tok, ',')) l.push_back(blsw::PublicKey::try_from(tok));
                pks.push_back(l);
                s1.push_back(xs);
            } else {
                std::vector<blsw::Signature> l;
                while (std::getline(ps, tok, ',')) l.push_back(blsw::Signature::try_from(tok));
                sigs.push_back(l);
                s2.push_back(xs);
            }
        }
        if (!pks.empty()) run(pks, s1, window_bits);
        if (!sigs.empty()) run(sigs, s2, window_bits);
        if (!pks.empty()) {
            std::vector<blsw::PublicKey> all;
            std::vector<std::vector<uint32_t>> idx;
            for (const auto& l : pks) {
                idx.emplace_back();
                for (const auto& k : l) {
                    idx.back().push_back((uint32_t)all.size());
                    all.push_back(k);
                }
            }
            blsw::KeyRegistry reg((uint32_t)all.size());
            reg.append(all);
            std::vector<int32_t> st;
            const std::vector<blsw::PublicKey> out = reg.msm(idx, s1, &st, window_bits);
            for (size_t i = 0; i < out.size(); i++) std::printf("r %d %s\n", st[i], hex(out[i].bytes).c_str());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
