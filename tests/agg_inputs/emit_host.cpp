// TEST HARNESS ONLY (never linked into libblsw.so): the device logic of aggregate_verify with public inputs, compiled for the host with g++ — the key
// source of csrc/agg_input.hpp (what k_agg_sum_in reads its operands through), chain_mapped_aggregate and chain_g1_post (the programs that
// kernel runs), and the element function of the instance writer k_agg_instance — so that the count / agg / pk_not_zero / prep_pk segments and the
// instance elements can be checked against the shim (libaggshim.so) without a GPU.
#include <cstring>
#include "../../bls-verify-gadget_amd/csrc/agg_input.hpp"

using namespace blsw;

namespace {
struct LdHost {
    Fp operator()(const Fp* p) const { return *p; }
};
}  // namespace

extern "C" {
int aggemit_layout(uint32_t msg_len, uint32_t n_keys, uint32_t agg_inputs, blsw_layout_t* L) {
    make_layout_aggregate(msg_len, L, n_keys, agg_inputs);
    return 0;
}
// One instance with Input keys: writes the bitmap (if Witness), count, agg, pk_not_zero and prep_pk segments into out_witness [n_witness][6] at the
// layout's offsets and the head of instance_assignment (agg_instance_head elements) into out_instance. Returns count; *head_out = elements written.
uint32_t aggemit_instance(const uint64_t* pks_xy, const uint8_t* bitmap, uint32_t n_keys, uint32_t msg_len, uint32_t agg_inputs, uint64_t* out_witness,
                          uint64_t* out_instance, uint32_t* head_out) {
    blsw_layout_t L;
    make_layout_aggregate(msg_len, &L, n_keys, agg_inputs);
    uint32_t* base = reinterpret_cast<uint32_t*>(out_witness);
    const Fp* keys = reinterpret_cast<const Fp*>(pks_xy);
    Emitter eb = {base, L.off_bitmap};
    for (uint32_t k = 0; k < L.off_msg - L.off_bitmap; k++) eb.put_bool(bitmap[k] != 0);
    KeyInputSrc<LdHost> src = {keys, LdHost()};
    uint32_t count = 0;
    Proj<OpsFp> pk = chain_mapped_aggregate(Emitter{base, L.off_count}, Emitter{base, L.off_agg}, src, bitmap, n_keys, &count);
    chain_g1_post(Emitter{base, L.off_pk_not_zero}, Emitter{base, L.off_prep_pk}, pk);
    const uint32_t head = agg_instance_head(L);
    Fp* inst = reinterpret_cast<Fp*>(out_instance);
    for (uint32_t e = 0; e < head; e++) inst[e] = agg_instance_element(L, keys, bitmap, e, LdHost());
    if (head_out) *head_out = head;
    return count;
}
}
