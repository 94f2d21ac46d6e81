// aggregate_verify with public inputs (blsw_layout_aggregate_inputs): the key source of mapped_aggregate for keys allocated with
// PublicKeyVar::new_variable(.., Input) and the element function of the instance writer. An Input key is new_variable_omit_prime_order_check
// (ark-r1cs-std 0.4.0): its x, y, z are instance variables and no witness exists, so the projective point mapped_aggregate selects and adds is
// formed from the step's affine input — (x, y, 1), or (0, 1, 0) for the (0, 0) encoding of the point at infinity — with no allocation chain in
// front. Shared by the device kernels (k_g1.hip: k_agg_sum_in, k_agg_io.hip: k_agg_instance) and the host test harness; LoadFp is how an Fp is
// read (the device states the global address space, the host copies).
#pragma once
#include "chains.hpp"
#include "layout.h"

namespace blsw {

BLSW_HD Proj<OpsFp> key_input_point(const Fp& x, const Fp& y) {
    const bool inf = fp_is_zero(x) && fp_is_zero(y);
    return {inf ? fp_zero() : x, inf ? fp_one() : y, inf ? fp_zero() : fp_one()};
}
// K of chain_mapped_aggregate: key k of one instance from its affine inputs, keys [n_keys][2] Fp (x, y)
template <class LoadFp>
struct KeyInputSrc {
    const Fp* keys;
    LoadFp load;
    BLSW_HD Proj<OpsFp> ld(uint32_t k) const { return key_input_point(load(keys + 2 * (uint64_t)k), load(keys + 2 * (uint64_t)k + 1)); }
};
// how many leading elements of instance_assignment come from the keys and the bitmap: 1 (the constant one) + 3 per Input key + 1 per Input bit.
// The message's and the signature's follow (k_msg_input, the signature's prepare chain).
BLSW_HD uint32_t agg_instance_head(const blsw_layout_t& L) { return agg_inst_msg_base(L); }
// element e < agg_instance_head(L) of one instance's instance_assignment, Montgomery form
template <class LoadFp>
BLSW_HD Fp agg_instance_element(const blsw_layout_t& L, const Fp* keys, const uint8_t* bitmap, uint32_t e, const LoadFp& load) {
    if (e == 0) return fp_one();
    const uint32_t b0 = agg_inst_bitmap_base(L);
    if (e >= b0) return bitmap[e - b0] != 0 ? fp_one() : fp_zero();  // Boolean::new_input: the bit as a field element
    const uint32_t k = (e - 1) / 3, c = (e - 1) - 3 * k;
    const Proj<OpsFp> p = key_input_point(load(keys + 2 * (uint64_t)k), load(keys + 2 * (uint64_t)k + 1));
    return c == 0 ? p.x : (c == 1 ? p.y : p.z);
}

}  // namespace blsw
