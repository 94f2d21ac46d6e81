// TEST HARNESS ONLY (never linked into libblsw.so): compiles csrc/sha.hpp's tag-taking expansion for the HOST with g++ — the host-side construction
// of the kernel argument (dst_arg_build) and the function the lanes of k_sha_values_dst run (expand_message_values_dst), which consumes that same
// argument — so that both are checked against hashlib without a GPU (pytest -m "not gpu"; tests/test_dst_ref.py).
#include <cstdint>
#include <cstring>

#include "../../bls-verify-gadget_amd/csrc/sha.hpp"

using namespace blsw;

extern "C" {
uint32_t dst_arg_words(void) { return sizeof(DstArg) / 4; }
// the kernel argument of a call with this tag and message length, as the words the device copies -> 0, or -1 where the library refuses the tag
int dst_arg(const uint8_t* dst, uint32_t dst_len, uint32_t msg_len, uint32_t* out) {
    DstArg a;
    if (dst_arg_build(&a, dst, dst_len, msg_len)) return -1;
    memcpy(out, &a, sizeof(a));
    return 0;
}
// one lane: the argument's words and a message of the length the argument was built for -> uniform_bytes as 64 big-endian words and
// u0.c0, u0.c1, u1.c0, u1.c1 as 12 Montgomery limbs each
void dst_lane(const uint32_t* arg, const uint8_t* msg, uint32_t* uw, uint32_t* u) {
    DstArg a;
    memcpy(&a, arg, sizeof(a));
    expand_message_values_dst(msg, &a, uw);
    for (int j = 0; j < 4; j++) {
        const Fp e = hash_to_field_elem(uw + 16 * j);
        memcpy(u + 12 * j, e.l, 48);
    }
}
// n messages [n][msg_len] under one tag: the argument built ONCE, as a call does -> uw [n][64], u [n][48] (nullable); 0 or -1
int dst_batch(const uint8_t* dst, uint32_t dst_len, const uint8_t* msgs, uint32_t msg_len, uint64_t n, uint32_t* uw, uint32_t* u) {
    DstArg a;
    if (dst_arg_build(&a, dst, dst_len, msg_len)) return -1;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t w[64];
        expand_message_values_dst(msgs + i * msg_len, &a, w);
        memcpy(uw + 64 * i, w, sizeof(w));
        if (u)
            for (int j = 0; j < 4; j++) {
                const Fp e = hash_to_field_elem(w + 16 * j);
                memcpy(u + 48 * i + 12 * j, e.l, 48);
            }
    }
    return 0;
}
}
