// Witness-vector segment table (host side). Segment sizes are properties of the circuit shape:
// the SHA-256 segment is obtained by running the mask propagation of sha.hpp in count-only mode
// (no values, no stores); the field segments are the fixed constants below (pinned by tests against
// the CPU oracle's allocation trace).
#pragma once
#include <vector>
#include "../../include/blsw.h"
#include "sha.hpp"

namespace blsw {

enum : uint32_t {
    SEG_PK_ALLOC = 1942,     // 3 + 125 doublings * 11 + 47 additions * 12
    SEG_SIG_ALLOC = 12413,   // 6 + 254 * 30 + 132 * 36 + 35 (enforce_equal)
    SEG_PK_NOT_ZERO = 8,
    SEG_MAP = 5889,
    SEG_ADD = 36,
    SEG_COFACTOR = 8979,
    SEG_PREP_G2 = 1096,      // 18 + 63 * 16 + 5 * 14
    SEG_PREP_PK = 7,
    SEG_MILLER = 6826,       // 62 * 36 + 68 * (30 + 38) - 30
    SEG_FINAL_EXP = 7848,
    SEG_IS_ONE = 35,
    SEG_MSG_CHUNK = 761,     // AllocatedFp::to_bits_le: 381 booleans + 380 AND witnesses of enforce_in_field_le
    MSG_CHUNK_BYTES = 47,    // ToConstraintField<Fq> for [u8]: (MODULUS_BIT_SIZE - 1) / 8 bytes per field element
};
// public inputs of a message of msg_len bytes allocated with UInt8::new_input_vec
BLSW_HD uint32_t msg_input_chunks(uint32_t msg_len) { return (msg_len + MSG_CHUNK_BYTES - 1) / MSG_CHUNK_BYTES; }

// n_keys > 0: the aggregate_verify circuit (constraints.rs:378-441). n_pairs > 1: the N+1-pair product (one signature over
// n_pairs (pk, msg) pairs; every statement of constraints.rs:97-125 becomes a loop over the pairs, allocation order
// msgs, params, pks, sig as in constraints.rs:335-366). n_pairs == 1 is exactly the single-key circuit.
inline uint32_t seg_miller(uint32_t n_pairs) { return 62 * 36 + 68 * 30 - 30 + 68 * 38 * n_pairs; }
// params_witness: ParametersVar::new_variable(Witness) (constraints.rs:198-211), single-key circuit only: the generator's allocation
// segment follows the message (argument order of constraints.rs:346-364), prepare_g1(-g1) emits its to_affine in front of prepare(H),
// and every ell of the (-g1, sig) pair has a variable point: 38 witnesses instead of 30, 2 instead of 0 in the first one (f = 1).
// pk_input / sig_input: PublicKeyVar / SignatureVar::new_variable(Input) (constraints.rs:214-249), single-key circuit with Constant parameters only: the
// point's coordinates are instance variables and its allocation segment is empty (no in-circuit prime-order check for public inputs).
// msg_input: UInt8::new_input_vec (ark-r1cs-std 0.4.0), single-key circuit with Constant parameters only: the message is packed into
// msg_input_chunks(msg_len) public inputs of MSG_CHUNK_BYTES bytes each, allocated before the key's and the signature's, and the message segment
// holds each chunk's AllocatedFp::to_bits_le (SEG_MSG_CHUNK witnesses per chunk) instead of 8 booleans per byte.
// The N+1-pair product (n_pairs > 1) takes the same three flags for its K keys, its K messages and its signature (blsw_layout_multi_inputs): each
// Input argument is the single-key rule K times, the instance variables in allocation order msgs, pks, sig (multi_input.hpp).
// aggregate_verify (n_keys > 0) takes the same three flags for its keys (every key Input: 3 n_keys instance variables, an empty keys segment), its
// message and its signature, and bitmap_input for Boolean::new_input per bit (n_keys instance variables, an empty bitmap segment; the booleanity
// constraints stay). Allocation order keys, bitmap, message, signature (constraints.rs:394-441) is the order of the instance variables.
inline void make_layout(uint32_t msg_len, blsw_layout_t* L, uint32_t n_keys = 0, uint32_t n_pairs = 1, bool params_witness = false, bool pk_input = false,
                        bool sig_input = false, bool msg_input = false, bool bitmap_input = false) {
    std::vector<uint8_t> msg(msg_len ? msg_len : 1, 0);
    BitSink s;
    s.init(nullptr, 0);
    uint32_t uw[64];
    expand_message_w(s, msg.data(), msg_len, false, uw);
    L->msg_len = msg_len;
    const uint32_t msg_chunks = msg_input ? msg_input_chunks(msg_len) : 0;
    const uint32_t K = n_keys ? 1 : (n_pairs ? n_pairs : 1);
    L->n_instance_vars = 1 + msg_chunks * K + (pk_input ? 3 * (n_keys ? n_keys : K) : 0) + (n_keys && bitmap_input ? n_keys : 0) + (sig_input ? 6 : 0);
    L->pk_mode = pk_input ? 1 : 0;
    L->sig_mode = sig_input ? 1 : 0;
    L->sha_bits = (uint32_t)s.nbits;
    uint32_t o = 0;
    L->n_keys = n_keys;
    L->off_keys = L->off_bitmap = L->off_count = L->off_agg = 0;
    if (n_keys) {  // keys, bitmap booleans, msg, sig, count, per-key (select 3 + add 12 (not the first) + addmany 33)
        L->off_keys = o;
        o += pk_input ? 0 : n_keys * SEG_PK_ALLOC;
        L->off_bitmap = o;
        o += bitmap_input ? 0 : n_keys;
    }
    L->n_pairs = K;
    L->stride_msg = msg_input ? SEG_MSG_CHUNK * msg_chunks : 8 * msg_len;
    L->stride_pk_alloc = pk_input ? 0 : SEG_PK_ALLOC;
    L->stride_pk_not_zero = SEG_PK_NOT_ZERO;
    L->stride_hash = L->sha_bits + 2 * SEG_MAP + SEG_ADD + SEG_COFACTOR;
    L->stride_prep_h = SEG_PREP_G2;
    L->stride_prep_pk = SEG_PREP_PK;
    L->off_msg = o;
    o += L->stride_msg * K;
    L->params_mode = params_witness ? 1 : 0;
    L->off_params_alloc = L->off_prep_g1 = 0;
    if (params_witness) {
        L->off_params_alloc = o;
        o += SEG_PK_ALLOC;
    }
    L->off_pk_alloc = o;
    if (!n_keys) o += L->stride_pk_alloc * K;
    L->off_sig_alloc = o;
    o += sig_input ? 0 : SEG_SIG_ALLOC;
    if (n_keys) {
        L->off_count = o;
        o += 32;
        L->off_agg = o;
        o += 48 * n_keys - 12;
    }
    L->off_pk_not_zero = o;
    o += SEG_PK_NOT_ZERO * K;
    // hash_to_g2 of pair j: expand, map0, map1, add, cofactor, contiguous; pair j + 1 follows at + stride_hash
    L->off_expand = o;
    L->off_map0 = L->off_expand + L->sha_bits;
    L->off_map1 = L->off_map0 + SEG_MAP;
    L->off_add = L->off_map1 + SEG_MAP;
    L->off_cofactor = L->off_add + SEG_ADD;
    o += L->stride_hash * K;
    if (params_witness) {
        L->off_prep_g1 = o;
        o += SEG_PREP_PK;
    }
    L->off_prep_h = o;
    o += SEG_PREP_G2 * K;
    L->off_prep_pk = o;
    o += SEG_PREP_PK * K;
    L->off_prep_sig = o;
    o += SEG_PREP_G2;
    L->off_miller = o;
    o += seg_miller(K) + (params_witness ? 67 * 8 + 2 : 0);
    L->off_final_exp = o;
    o += SEG_FINAL_EXP;
    L->off_is_one = o;
    o += SEG_IS_ONE;
    L->n_witness = o;
}
// aggregate_verify with its mask of Input arguments (BLSW_AGG_*_INPUT, include/blsw.h)
inline void make_layout_aggregate(uint32_t msg_len, blsw_layout_t* L, uint32_t n_keys, uint32_t agg_inputs) {
    make_layout(msg_len, L, n_keys, 1, false, (agg_inputs & BLSW_AGG_KEYS_INPUT) != 0, (agg_inputs & BLSW_AGG_SIG_INPUT) != 0, (agg_inputs & BLSW_AGG_MSG_INPUT) != 0,
                (agg_inputs & BLSW_AGG_BITMAP_INPUT) != 0);
}
// the N+1-pair product with its mask of Input arguments (BLSW_MULTI_*_INPUT, include/blsw.h)
inline void make_layout_multi(uint32_t msg_len, blsw_layout_t* L, uint32_t n_pairs, uint32_t multi_inputs) {
    make_layout(msg_len, L, 0, n_pairs, false, (multi_inputs & BLSW_MULTI_KEYS_INPUT) != 0, (multi_inputs & BLSW_MULTI_SIG_INPUT) != 0, (multi_inputs & BLSW_MULTI_MSG_INPUT) != 0);
}
inline bool multi_inputs_ok(uint32_t multi_inputs) { return multi_inputs <= 15 && !(multi_inputs & 2); }
// the instance variables of an aggregate_verify layout: [1 | 3 per key | 1 per bitmap bit | message chunks | 6 of the signature], the selected groups only
BLSW_HD uint32_t agg_bitmap_is_input(const blsw_layout_t& L) { return L.n_keys && L.off_msg == L.off_bitmap; }
BLSW_HD uint32_t agg_inst_bitmap_base(const blsw_layout_t& L) { return 1 + (L.pk_mode ? 3 * L.n_keys : 0); }
BLSW_HD uint32_t agg_inst_msg_base(const blsw_layout_t& L) { return agg_inst_bitmap_base(L) + (agg_bitmap_is_input(L) ? L.n_keys : 0); }

}  // namespace blsw
