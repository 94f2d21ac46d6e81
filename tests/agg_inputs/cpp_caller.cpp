// TEST PROGRAM: aggregate_verify with every argument allocated as Input through include/blsw.hpp (the C++ host side above the C ABI). Prints one line per
// system for tests/test_agg_inputs_gpu.py:
//   "<result> <count> <n_instance_vars> <n_witness> <digest(instance_assignment)> <digest(witness_assignment)> <which_is_unsatisfied>"
//   cpp_caller <file>   every line "<bitmap of K characters 0/1> <msg hex> <sig96 hex> <pk48 hex> x K", one K and one message length for all lines
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "blsw.hpp"

using namespace blsw;

// position-weighted sum of the assignment's u64 words, mod 2^64
static uint64_t digest(const std::vector<uint64_t>& w) {
    uint64_t h = 0;
    for (size_t k = 0; k < w.size(); k++) h += w[k] * (2 * (uint64_t)k + 1);
    return h;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: cpp_caller <file>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::vector<std::vector<PublicKey>> pks;  // [K][n]
    std::vector<std::vector<bool>> bits;      // [K][n]
    std::vector<Signature> sigs;
    std::vector<std::vector<uint8_t>> msgs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string bm, msg, sig, pk;
        if (!(ss >> bm >> msg >> sig)) continue;
        if (msg == "-") msg.clear();  // empty message
        if (pks.empty()) {
            pks.resize(bm.size());
            bits.resize(bm.size());
        }
        if (bm.size() != pks.size()) {
            fprintf(stderr, "cpp_caller: one K for all lines\n");
            return 2;
        }
        for (size_t k = 0; k < bm.size(); k++) {
            if (!(ss >> pk)) return 2;
            pks[k].push_back(PublicKey::try_from(pk));
            bits[k].push_back(bm[k] == '1');
        }
        sigs.push_back(Signature::try_from(sig));
        msgs.push_back(detail::unhex(msg, msg.size() / 2));
    }
    try {
        const size_t n = sigs.size();
        ConstraintSystem cs(n, (uint32_t)msgs.at(0).size());
        std::vector<PublicKeyVar> keys;
        std::vector<Boolean> bitmap;
        for (size_t k = 0; k < pks.size(); k++) {
            keys.push_back(PublicKeyVar::new_variable(cs, pks[k], AllocationMode::Input));
            bitmap.push_back(Boolean::new_input(cs, bits[k]));
        }
        const MessageVar msg = UInt8::new_input_vec(cs, msgs);
        const SignatureVar sig = SignatureVar::new_variable(cs, sigs, AllocationMode::Input);
        const auto r = BlsSignatureVerifyGadget::aggregate_verify(ParametersVar::new_variable(cs, Parameters{}, AllocationMode::Constant), keys, bitmap, msg, sig);
        const std::vector<int64_t> bad = cs.which_is_unsatisfied();
        for (size_t i = 0; i < n; i++)
            printf("%d %u %llu %llu %llu %llu %lld\n", r.first.value()[i] ? 1 : 0, r.second.value()[i], (unsigned long long)cs.num_instance_variables(),
                   (unsigned long long)cs.num_witness_variables(), (unsigned long long)digest(cs.instance_assignment(i)),
                   (unsigned long long)digest(cs.witness_assignment(i)), (long long)bad[i]);
    } catch (const Error& e) {
        fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
