// TEST HARNESS ONLY (never linked into libblsw.so): the device logic of the N+1-pair product with public inputs, compiled for the host with g++ — the
// instance-index rules of csrc/multi_input.hpp and the Input branches of the key lane (k_g1: multi_key_input, then chain_g1_post) and of the message
// lane (k_msg_input: multi_msg_input) — so that the instance elements and the message / pk_not_zero / prep_pk segments can be checked against the
// shim (libmultishim.so) without a GPU.
#include <cstring>
#include "../../bls-verify-gadget_amd/csrc/multi_input.hpp"

using namespace blsw;

extern "C" {
int multiemit_layout(uint32_t msg_len, uint32_t n_pairs, uint32_t multi_inputs, blsw_layout_t* L) {
    make_layout_multi(msg_len, L, n_pairs, multi_inputs);
    return 0;
}
// the three index rules, for a caller that wants them alone: which = 0 chunk t of pair j, 1 coordinate t of key j, 2 element t of the signature
uint32_t multiemit_index(uint32_t msg_len, uint32_t n_pairs, uint32_t multi_inputs, uint32_t which, uint32_t j, uint32_t t) {
    blsw_layout_t L;
    make_layout_multi(msg_len, &L, n_pairs, multi_inputs);
    return which == 0 ? multi_inst_msg(L, j, t) : (which == 1 ? multi_inst_key(L, j, t) : multi_inst_sig(L, t));
}
// One instance: what the pair lanes write. For every pair j: the message segment and inputs (messages Input), the key's inputs (keys Input) and — on the
// point an Input key allocates — pk_not_zero and prep_pk. out_witness [n_witness][6] at the layout's offsets (zeros elsewhere), out_instance
// [n_instance_vars][6] with element 0 = one; the signature's six elements are left to the caller (the prepare chain writes them on the device).
void multiemit_instance(const uint64_t* pks_xy, const uint8_t* msgs, uint32_t n_pairs, uint32_t msg_len, uint32_t multi_inputs, uint64_t* out_witness,
                        uint64_t* out_instance) {
    blsw_layout_t L;
    make_layout_multi(msg_len, &L, n_pairs, multi_inputs);
    uint32_t* base = reinterpret_cast<uint32_t*>(out_witness);
    Fp* inst = reinterpret_cast<Fp*>(out_instance);
    inst[0] = fp_one();
    const auto put = [&](uint32_t k, const Fp& v) { inst[k] = v; };
    for (uint32_t j = 0; j < n_pairs; j++) {
        if ((multi_inputs & BLSW_MULTI_MSG_INPUT) && msg_len) multi_msg_input(L, j, Emitter{base, L.off_msg + j * L.stride_msg}, msgs + (uint64_t)j * msg_len, put);
        if (multi_inputs & BLSW_MULTI_KEYS_INPUT) {
            const Fp* p = reinterpret_cast<const Fp*>(pks_xy + 12 * (uint64_t)j);
            const Proj<OpsFp> pk = multi_key_input(L, j, p[0], p[1], put);
            chain_g1_post(Emitter{base, L.off_pk_not_zero + j * L.stride_pk_not_zero}, Emitter{base, L.off_prep_pk + j * L.stride_prep_pk}, pk);
        }
    }
}
}
