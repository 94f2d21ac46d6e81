// TEST HARNESS ONLY (never linked into libblsw.so): the product's message emitter (csrc/msg_input.hpp, the program k_msg_input runs on the
// device) and its layout, compiled for the host with g++, so that the message segment and the message inputs can be checked against the
// shim (libmsgshim.so) without a GPU.
#include <cstring>
#include "../../bls-verify-gadget_amd/csrc/msg_input.hpp"

using namespace blsw;

extern "C" {
// out_segment [msg_input_chunks(msg_len) * SEG_MSG_CHUNK][6] witnesses, out_inputs [msg_input_chunks(msg_len)][6]; Montgomery limbs. Returns the chunk count.
uint32_t msgemit_segment(const uint8_t* msg, uint32_t msg_len, uint64_t* out_segment, uint64_t* out_inputs) {
    Fp* inputs = reinterpret_cast<Fp*>(out_inputs);
    chain_msg_input(Emitter{reinterpret_cast<uint32_t*>(out_segment), 0}, msg, msg_len, [&](uint32_t j, const Fp& v) { inputs[j] = v; });
    return msg_input_chunks(msg_len);
}
int msgemit_layout(uint32_t msg_len, uint32_t msg_mode, uint32_t pk_mode, uint32_t sig_mode, blsw_layout_t* L) {
    make_layout(msg_len, L, 0, 1, false, pk_mode == 1, sig_mode == 1, msg_mode == 1);
    return 0;
}
}
