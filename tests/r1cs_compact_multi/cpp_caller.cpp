// TEST PROGRAM: a compact step of the N+1-pair product checked through include/blsw.hpp — ConstraintSystem::which_is_unsatisfied(const
// blsw_compact_layout_multi_t&, ..) and ConstraintSystem::pair_families — for tests/test_r1cs_compact_multi_gpu.py. The system is synthesised by
// verify_multi with every argument Input; the step is another engine's, read from a file.
//   cpp_caller <inputs> <compact>   inputs: every line "<sig96 hex> (<pk48 hex> <msg hex>) x K"; compact: the step's buffer, layout.total bytes
// Prints "families <first>:<rows> ..." and "rows <first unsatisfied row of every instance>".
#include <hip/hip_runtime.h>

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "blsw.hpp"

using namespace blsw;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: cpp_caller <inputs> <compact>\n");
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
    }
    void* d_compact = nullptr;
    try {
        const size_t n = sigs.size(), K = pks.size();
        const uint32_t msg_len = (uint32_t)msgs.at(0).at(0).size();
        ConstraintSystem cs(n, msg_len);
        std::vector<PublicKeyVar> keys;
        std::vector<MessageVar> messages;
        for (size_t j = 0; j < K; j++) {
            messages.push_back(UInt8::new_input_vec(cs, msgs[j]));
            keys.push_back(PublicKeyVar::new_variable(cs, pks[j], AllocationMode::Input));
        }
        const SignatureVar sig = SignatureVar::new_variable(cs, sigs, AllocationMode::Input);
        BlsSignatureVerifyGadget::verify_multi(ParametersVar::new_variable(cs, Parameters{}, AllocationMode::Constant), keys, messages, sig);
        blsw_engine_options_t opt;
        blsw_engine_options_default(&opt);
        opt.n_pairs = (uint32_t)K;
        blsw_compact_layout_multi_t lay;
        const int rc = blsw_compact_layout_multi(n, msg_len, &opt, BLSW_MULTI_KEYS_INPUT | BLSW_MULTI_MSG_INPUT | BLSW_MULTI_SIG_INPUT, &lay);
        if (rc) throw Error("blsw_compact_layout_multi", rc);
        std::ifstream cf(argv[2], std::ios::binary);
        std::vector<char> host(lay.total);
        if (!cf.read(host.data(), (std::streamsize)host.size())) throw Error("the compact file is shorter than layout.total", BLSW_ERR_ARG);
        if (hipMalloc(&d_compact, host.size()) != hipSuccess || hipMemcpy(d_compact, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess)
            throw Error("hipMalloc / hipMemcpy", BLSW_ERR_HIP);
        printf("families");
        for (const auto& f : cs.pair_families(lay)) printf(" %llu:%llu", (unsigned long long)f.first, (unsigned long long)f.second);
        printf("\nrows");
        for (int64_t r : cs.which_is_unsatisfied(lay, d_compact)) printf(" %lld", (long long)r);  // the instance vectors this object's verify_multi wrote
        printf("\n");
    } catch (const Error& e) {
        fprintf(stderr, "cpp_caller: %s\n", e.what());
        if (d_compact) (void)hipFree(d_compact);
        return 1;
    }
    (void)hipFree(d_compact);
    return 0;
}
