// Grouped verification over a MESSAGE TABLE (blsw_verify_groups_shared_batch, blsw_registry_verify_shared_batch): instance i signs row
// msg_index[i] of d_msgs [n_msgs][msg_len]. Within a group the product is bilinear in the keys,
//     prod_{i in run} e(r_i pk_i, H(m)) = e(sum_{i in run} r_i pk_i, H(m)),
// so the instances of a RUN — adjacent instances of one group with equal indices — cost one hash (of the table row), one line chain and one pair
// of the fold. The rules, for the host and the device alike (k_vgroups.hip; tests/vshared runs them on the host):
//   leader   instance i starts a run iff it is the first of its group or msg_index[i] != msg_index[i - 1]. A function of (n, group, msg_index)
//            alone: statuses and scalars play no part, equal indices that are not adjacent are separate runs, equality is of indices
//   slot     run k of group g lives in compact slot g * group + k: its leader's instance index, its length, and later its key sum and line rows
//   status   msg_index[i] >= n_msgs: status[i][0] = VS_BAD_INDEX in front of every other rule; the instance is excluded and no table row is read
//   merge    R = sum of the run's P_i = r_i pk_i (the identity for an excluded instance) with the general Jacobian addition: equal summands take
//            its doubling branch, opposite ones give the identity. A run whose R is the identity is a SKIPPED pair, as an identity S_g is
//   chunk    chunk q of group g is slots [q * chunk, min(runs[g], (q + 1) * chunk)) of the group; the group has the plain form's
//            vg_chunks_per_group teams whatever its runs, and a chunk without a slot walks the squarings of one and writes the partial 1
// scale, sum and finish are the plain form's stages (vgroups.hpp).
#pragma once
#include "vgroups.hpp"

namespace blsw {

#define VS_BAD_INDEX 6  // BLSW_ST_BAD_INDEX
#define VS_TILE 64u     // the scan walks a group in tiles of one wavefront

BLSW_HD bool vs_bad_index(uint32_t idx, uint64_t n_msgs) { return (uint64_t)idx >= n_msgs; }
BLSW_HD bool vs_is_leader(const uint32_t* msg_index, uint64_t i, uint32_t group) { return i % group == 0 || msg_index[i] != msg_index[i - 1]; }
BLSW_HD uint32_t vs_group_size(uint64_t n, uint32_t group, uint64_t g) {
    const uint64_t first = g * group;
    return (uint32_t)(n - first < group ? n - first : group);
}

// The scan of one group in tiles of `tile` <= 64 instances. `ballot` bit l: instance base + l of the group is a leader (bits at and beyond the
// tile's m instances are clear). The carry between tiles: the runs before the tile and where the run that is still open began.
struct VsCarry {
    uint32_t slots;  // runs that began before this tile
    uint32_t open;   // offset in the group of the last of their leaders
};
BLSW_HD uint64_t vs_bits_upto(uint32_t lane) { return lane >= 63 ? ~0ull : (1ull << (lane + 1)) - 1ull; }  // bits [0, lane]
BLSW_HD uint32_t vs_popc(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
BLSW_HD uint32_t vs_ctz(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }  // v != 0
BLSW_HD uint32_t vs_top(uint64_t v) { return 63u - (uint32_t)__builtin_clzll(v); }  // v != 0
// what lane `lane` < m of the tile stores (slots relative to the group's first)
struct VsLaneOut {
    bool put_leader;  // slot_leader[slot] = the lane's instance
    bool put_len;     // slot_len[slot] = len: the run ends in this tile (or the group does)
    bool put_close;   // slot_len[close_slot] = close_len: this lane ends the run left open by the tiles before
    uint32_t slot, len, close_slot, close_len;
};
BLSW_HD VsLaneOut vs_tile_lane(const VsCarry& c, uint64_t ballot, uint32_t base, uint32_t m, bool last, uint32_t lane) {
    VsLaneOut o = {false, false, false, 0, 0, 0, 0};
    if ((ballot >> lane) & 1ull) {
        o.put_leader = true;
        o.slot = c.slots + vs_popc(ballot & vs_bits_upto(lane)) - 1u;
        const uint64_t rest = lane >= 63 ? 0ull : ballot >> (lane + 1);
        if (rest) {
            o.put_len = true;
            o.len = vs_ctz(rest) + 1u;
        } else if (last) {
            o.put_len = true;
            o.len = m - lane;
        }
    }
    if (c.slots) {  // a run is open: the tile's first leader ends it, or lane 0 of the group's last tile does
        if (ballot ? lane == vs_ctz(ballot) : (last && lane == 0)) {
            o.put_close = true;
            o.close_slot = c.slots - 1u;
            o.close_len = base + (ballot ? lane : m) - c.open;
        }
    }
    return o;
}
BLSW_HD VsCarry vs_tile_carry(const VsCarry& c, uint64_t ballot, uint32_t base) {
    return {c.slots + vs_popc(ballot), ballot ? base + vs_top(ballot) : c.open};
}

// chunk q of group g over its runs: slots [first, first + count) of the arrays, count 0 for a chunk beyond the runs
BLSW_HD VgChunk vs_chunk(uint32_t group, uint32_t chunk, uint64_t g, uint32_t q, uint32_t runs) {
    const uint64_t k0 = (uint64_t)q * chunk;
    if (k0 >= runs) return {g * group, 0};
    return {g * group + k0, (uint32_t)(runs - k0 < chunk ? runs - k0 : chunk)};
}
// Does a team walk the Miller loop? Every team does, as the plain fold's idle teams do: a team whose chunk is empty (and which does not carry the
// group's own pair) walks 63 squarings of one and stores the partial 1. Skipping that walk was measured and is a LOSS: waves in which some teams
// skip and others walk run the walkers about three times slower. -DBLSW_VS_SKIP_EMPTY builds the skipping form for the A/B
// (tools/shared_rate.py): the decision is uniform over a team and idle lanes copy the wave's first team, so the verdicts are the same.
BLSW_HD bool vs_chunk_walks(const VgChunk& c, uint32_t q) {
#ifdef BLSW_VS_SKIP_EMPTY
    return c.count != 0 || q == 0;
#else
    (void)c;
    (void)q;
    return true;
#endif
}

// sum of a run's len Jacobian G1 points, ld(i) -> Jac1v. v1_add takes its doubling branch on equal summands and returns the identity on opposite ones.
template <class LD>
BLSW_HD Jac1v vs_merge(uint32_t len, const LD& ld) {
    Jac1v acc = {fp_one(), fp_one(), fp_zero()};
#pragma unroll 1
    for (uint32_t i = 0; i < len; i++) acc = v1_add(acc, ld(i));
    return acc;
}

}  // namespace blsw
