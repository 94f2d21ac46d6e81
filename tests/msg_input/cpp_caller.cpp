// TEST PROGRAM: the message allocated with UInt8::new_input_vec through include/blsw.hpp (the C++ host side above the C ABI), with the key as a
// public input and the signature as witnesses. Prints one line per system for tests/test_msg_input_gpu.py:
//   "<result> <n_instance_vars> <n_witness> <digest(instance_assignment)> <digest(witness_assignment)> <which_is_unsatisfied>"
//   cpp_caller <file>   every line "<pk48 hex> <msg hex> <sig96 hex>", one message length for all lines
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
    std::vector<PublicKey> pks;
    std::vector<Signature> sigs;
    std::vector<std::vector<uint8_t>> msgs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string pk, msg, sig;
        if (!(ss >> pk >> msg >> sig)) continue;
        if (msg == "-") msg.clear();  // empty message
        pks.push_back(PublicKey::try_from(pk));
        sigs.push_back(Signature::try_from(sig));
        msgs.push_back(detail::unhex(msg, msg.size() / 2));
    }
    try {
        ConstraintSystem cs(pks.size(), (uint32_t)msgs.at(0).size());
        // one expression: the allocation modes fix the circuit shape whatever order the arguments are evaluated in
        const Boolean r = BlsSignatureVerifyGadget::verify(ParametersVar::new_variable(cs, Parameters{}, AllocationMode::Constant),
                                                           PublicKeyVar::new_variable(cs, pks, AllocationMode::Input), UInt8::new_input_vec(cs, msgs),
                                                           SignatureVar::new_variable(cs, sigs, AllocationMode::Witness));
        const std::vector<int64_t> bad = cs.which_is_unsatisfied();
        for (size_t i = 0; i < pks.size(); i++)
            printf("%d %llu %llu %llu %llu %lld\n", r.value()[i] ? 1 : 0, (unsigned long long)cs.num_instance_variables(), (unsigned long long)cs.num_witness_variables(),
                   (unsigned long long)digest(cs.instance_assignment(i)), (unsigned long long)digest(cs.witness_assignment(i)), (long long)bad[i]);
    } catch (const Error& e) {
        fprintf(stderr, "cpp_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
