// TEST PROGRAM: BLS::combine, BLS::lagrange_coefficients, BLS::recover_signature and BLS::recover_public_key of include/blsw.hpp from a C++ host,
// linked to the in-tree libblsw.so.
//   cpp_caller <file>
// file: one line per list: "g1" or "g2", the points (hex, comma separated), the ids (32-byte little-endian hex, comma separated).
// Prints per list "status_recover recovered_hex status_lagrange status_combine combined_hex": the recovery, and the same sum formed from the
// coefficients by combine (zero scalars where the id list fails).
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
template <class POINT, class RECOVER>
static void run(const std::vector<std::vector<POINT>>& pts, const std::vector<std::vector<BLS::Scalar>>& ids, RECOVER recover) {
    std::vector<int32_t> st_r, st_l, st_c;
    const std::vector<POINT> rec = recover(ids, pts, &st_r);
    std::vector<std::vector<BLS::Scalar>> coeff = BLS::lagrange_coefficients(ids, &st_l);
    for (size_t i = 0; i < coeff.size(); i++)
        if (coeff[i].empty()) coeff[i].assign(ids[i].size(), BLS::Scalar{});
    const std::vector<POINT> com = BLS::combine(pts, coeff, &st_c);
    for (size_t i = 0; i < rec.size(); i++) std::printf("%d %s %d %d %s\n", st_r[i], hex(rec[i].bytes).c_str(), st_l[i], st_c[i], hex(com[i].bytes).c_str());
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    try {
        std::ifstream in(argv[1]);
        std::string line, tok;
        std::vector<std::vector<blsw::PublicKey>> pks;
        std::vector<std::vector<blsw::Signature>> sigs;
        std::vector<std::vector<BLS::Scalar>> ids1, ids2;
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
                ids1.push_back(xs);
            } else {
                std::vector<blsw::Signature> l;
                while (std::getline(ps, tok, ',')) l.push_back(blsw::Signature::try_from(tok));
                sigs.push_back(l);
                ids2.push_back(xs);
            }
        }
        if (!pks.empty()) run(pks, ids1, [](auto& i, auto& p, auto* s) { return BLS::recover_public_key(i, p, s); });
        if (!sigs.empty()) run(sigs, ids2, [](auto& i, auto& p, auto* s) { return BLS::recover_signature(i, p, s); });
    } catch (const std::exception& e) {
        std::fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
