// AggregateVerify of the BLS signature draft as VALUES (blsw_verify_pairs_batch): ONE aggregate signature over K (key, message) pairs with their own
// messages,
//     e(-g1, sig) * prod_j e(pk_j, H(m_j)) == 1
// per instance, with one final exponentiation per instance and the squarings of the Miller loop shared by the pairs one team folds. The pieces are
// those of blsw_verify_groups_batch (vgroups.hpp) without its coefficients: nothing is scaled or summed, the keys stay affine. Stages
// (k_vpairs.hip; tests/vpairs runs them on the host for one instance):
//   decode   one lane per point: n * K keys and n signatures
//   hash     the value-only hash to G2 of the n * K messages
//   status   one lane per instance: the rules below, into d_status[i][0]
//   lines    vline_chain of H(m_ij) against the AFFINE pk_ij (two multipliers) and of sig_i against -g1; a pair that is not used, a point that did
//            not decode and every pair of an instance whose status is not OK write nothing
//   fold     six lanes per chunk of <= `chunk` consecutive pairs of one instance: team_miller_groups; the instance's own pair (-g1, sig) rides with
//            its first chunk. Partial products (not conjugated) go to the workspace
//   finish   six lanes per instance: the product of the partials, conj (x < 0), final exponentiation, is_one, AND the two statuses
// Instance i owns cpi = ceil(K / chunk) teams whatever its count: chunk q covers pairs [q * chunk, ..) clipped to the count, and a chunk without a
// used pair is an idle team that writes the partial 1. An instance whose statuses are not both OK folds nothing: its verdict is 0 whatever its
// product would be.
#pragma once
#include "vgroups.hpp"

namespace blsw {

#define DEC_BAD_COUNT 6  // BLSW_ST_BAD_INDEX: a count beyond the pairs the call carries

// pairs instance i uses: its count, all K without counts, 0 for a count beyond K (nothing of such an instance is read)
BLSW_HD uint32_t vp_count_eff(const uint32_t* counts, uint64_t i, uint32_t K) {
    const uint32_t c = counts ? counts[i] : K;
    return c > K ? 0u : c;
}
// d_status[i][0] from the instance's count and the statuses of its K keys, in this order: a count beyond K; an empty list (the draft requires at
// least one pair); the lowest-indexed USED pair whose key is not OK — a well-formed identity key is DEC_IDENTITY here: every key goes through
// KeyValidate, unlike a summand of PublicKey::aggregate; else OK
BLSW_HD int32_t vp_instance_status(const uint32_t* counts, uint64_t i, uint32_t K, const int32_t* key_status) {
    const uint32_t c = counts ? counts[i] : K;
    if (c > K) return DEC_BAD_COUNT;
    if (c == 0) return DEC_IDENTITY;
    for (uint32_t j = 0; j < c; j++)
        if (key_status[i * K + j] != DEC_OK) return key_status[i * K + j];
    return DEC_OK;
}

// chunk q of an instance of K pairs of which the first `count` are used: pairs [first, first + count) of the instance, count 0 for an idle chunk
struct VpChunk {
    uint32_t first, count;
};
BLSW_HD uint32_t vp_chunks_per_instance(uint32_t K, uint32_t chunk) { return (K + chunk - 1) / chunk; }
BLSW_HD VpChunk vp_chunk(uint32_t chunk, uint32_t count, uint32_t q) {
    const uint64_t first = (uint64_t)q * chunk;
    if (first >= count) return {0, 0};
    return {(uint32_t)first, count - (uint32_t)first < chunk ? count - (uint32_t)first : chunk};
}
// the fold's mask of a chunk: bits [0, count) its pairs, bit `count` the instance's own pair (first chunk, a decoded signature); nothing for an
// instance that does not fold
BLSW_HD uint32_t vp_chunk_mask(const VpChunk& c, uint32_t q, bool folds) {
    if (!folds) return 0;
    return ((1u << c.count) - 1u) | (q == 0 ? 1u << c.count : 0u);
}

}  // namespace blsw
