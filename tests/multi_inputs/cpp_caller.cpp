// TEST PROGRAM: the N+1-pair product with every argument allocated as Input through include/blsw.hpp (the C++ host side above the C ABI). Prints one
// line per system for tests/test_multi_inputs_gpu.py:
//   "<result> <n_instance_vars> <n_witness> <digest(instance_assignment)> <digest(witness_assignment)>"
//   cpp_caller <file>   every line "<sig96 hex> (<pk48 hex> <msg hex>) x K", one K and one message length for all lines
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
    std::vector<std::vector<PublicKey>> pks;             // [K][n]
    std::vector<std::vector<std::vector<uint8_t>>> msgs;  // [K][n]
    std::vector<Signature> sigs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string sig, pk, msg;
        if (!(ss >> sig)) continue;
        sigs.push_back(Signature::try_from(sig));
        size_t j = 0;
        while (ss >> pk >> msg) {
            if (pks.size() <= j) {
                pks.emplace_back();
                msgs.emplace_back();
            }
            pks[j].push_back(PublicKey::try_from(pk));
            msgs[j].push_back(detail::unhex(msg, msg.size() / 2));
            j++;
        }
        if (j != pks.size()) {
            fprintf(stderr, "cpp_caller: one K for all lines\n");
            return 2;
        }
    }
    try {
        const size_t n = sigs.size();
        ConstraintSystem cs(n, (uint32_t)msgs.at(0).at(0).size());
        std::vector<PublicKeyVar> keys;
        std::vector<MessageVar> messages;
        for (size_t j = 0; j < pks.size(); j++) {
            messages.push_back(UInt8::new_input_vec(cs, msgs[j]));
            keys.push_back(PublicKeyVar::new_variable(cs, pks[j], AllocationMode::Input));
        }
        const SignatureVar sig = SignatureVar::new_variable(cs, sigs, AllocationMode::Input);
        const Boolean r = BlsSignatureVerifyGadget::verify_multi(ParametersVar::new_variable(cs, Parameters{}, AllocationMode::Constant), keys, messages, sig);
        for (size_t i = 0; i < n; i++)
            printf("%d %llu %llu %llu %llu\n", r.value()[i] ? 1 : 0, (unsigned long long)cs.num_instance_variables(), (unsigned long long)cs.num_witness_variables(),
                   (unsigned long long)digest(cs.instance_assignment(i)), (unsigned long long)digest(cs.witness_assignment(i)));
    } catch (const Error& e) {
        fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
