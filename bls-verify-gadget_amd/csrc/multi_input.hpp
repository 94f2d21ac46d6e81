// The N+1-pair product with public inputs (blsw_layout_multi_inputs): where each Input argument's elements sit in instance_assignment, and the
// Input branch of a pair's key. Allocation order msgs, params Constant, pks, sig (constraints.rs:335-366 with every statement a loop over the K pairs)
// is the order of the instance variables, the selected groups only:
//   [1 | c chunks per message, pair by pair | x, y, z per key, pair by pair | 6 of the signature]
// Every rule counts from an end of the vector that does not depend on which other groups are selected: the messages follow the constant one, the
// signature is last and the keys end where the signature begins. K = 1 is the single-key circuit's rule (blsw_layout_inputs). Shared by the device
// kernels (k_g1.hip, k_msg.hip, k_prepare.hip) and the host test harness.
#pragma once
#include "agg_input.hpp"
#include "msg_input.hpp"

namespace blsw {

// chunk t of pair j's message (the message is Input: UInt8::new_input_vec per pair)
BLSW_HD uint32_t multi_inst_msg(const blsw_layout_t& L, uint32_t j, uint32_t t) { return 1 + j * msg_input_chunks(L.msg_len) + t; }
// the signature's six elements x.c0 .. z.c1 (L.sig_mode): d = 0 .. 5
BLSW_HD uint32_t multi_inst_sig(const blsw_layout_t& L, uint32_t d) { return L.n_instance_vars - 6 + d; }
// coordinate d (x, y, z) of pair j's key (L.pk_mode)
BLSW_HD uint32_t multi_inst_key(const blsw_layout_t& L, uint32_t j, uint32_t d) { return L.n_instance_vars - (L.sig_mode ? 6 : 0) - 3 * L.n_pairs + 3 * j + d; }

// PublicKeyVar::new_variable(Input) of pair j = new_variable_omit_prime_order_check: x, y, z are public inputs, no witnesses, no in-circuit
// prime-order check; the (0, 0) input is the point at infinity (0, 1, 0). put(k, v): instance variable k := v. Returns the allocated point.
template <class PutInput>
BLSW_HD Proj<OpsFp> multi_key_input(const blsw_layout_t& L, uint32_t j, const Fp& x, const Fp& y, const PutInput& put) {
    const Proj<OpsFp> pk = key_input_point(x, y);
    put(multi_inst_key(L, j, 0), pk.x);
    put(multi_inst_key(L, j, 1), pk.y);
    put(multi_inst_key(L, j, 2), pk.z);
    return pk;
}
// UInt8::new_input_vec of pair j's message: its chunks' inputs and the pair's message segment (e: the cursor at off_msg + j * stride_msg)
template <class PutInput>
BLSW_HD void multi_msg_input(const blsw_layout_t& L, uint32_t j, Emitter e, const uint8_t* msg, const PutInput& put) {
    chain_msg_input(e, msg, L.msg_len, [&](uint32_t t, const Fp& v) { put(multi_inst_msg(L, j, t), v); });
}

}  // namespace blsw
