// fast_aggregate_verify as VALUES over a RESIDENT registry of keys and n index lists (blsw_registry_*, include/blsw.h): the shape of a consensus
// client's signature sets — (validator indices, one message, one aggregate signature) over 10^5 .. 10^6 keys that change only by appending. The keys
// are decoded ONCE, when they are appended, into records that stay in the handle's device buffer; a call sums each list's records with L lanes and
// hands the sums to the two value verifiers unchanged, as committee.hpp does for bitmap rows. Stages (k_registry.hip; tests/registry runs the same
// functions on the host, lane after lane):
//   append   one lane per new key: g1_decode with its subgroup check -> the key's record and its entry of the status array
//   sum      L lanes per set. registry_lane_sum: lane l walks list positions l, l + L, l + 2 L, ...; it checks the index against the registry's
//            size AS OF THE CALL (a kernel argument: a row beyond it is never read, whatever an earlier life of the buffer left there), holds the
//            record of its NEXT position while it adds the current one with v1_add_mixed (a mixed addition is thousands of VALU instructions for 96
//            bytes: one load in flight hides the gather), adds OK keys, lets a well-formed identity key add nothing and remembers the lowest list
//            POSITION whose entry is bad — an index >= size (DEC_BAD_INDEX) or a key whose status is neither OK nor IDENTITY. A repeated index is
//            added as often as it occurs. Then committee_tree and committee_finish, unchanged: CommitteePartial.bad_index is a list position here.
// The record: 128 bytes, 128-byte aligned — x (48 bytes, Montgomery), y (48), the status (4), 28 bytes unused. One lane's gather is one cache line
// (the committee's [2][K] rows make it two), and 2^20 records are 128 MiB.
#pragma once
#include "committee.hpp"

namespace blsw {

#define DEC_BAD_INDEX 6  // BLSW_ST_BAD_INDEX: offsets that do not describe a list, or an index >= the registry's size
// the longest list: positions are CommitteePartial's 32-bit bad_index, and BLSW_COMMITTEE_NO_BAD is no position
#define BLSW_REGISTRY_MAX_LIST 0xfffffffeull

struct alignas(128) RegistryRecord {
    Fp x, y;  // zeros unless the status is OK
    int32_t status;
    uint32_t unused[7];
};
static_assert(sizeof(RegistryRecord) == 128, "one record, one cache line");

// what a lane holds of one list position
struct RegistryEntry {
    Fp x, y;
    int32_t status;
};
// TABLE: load(k) -> the RegistryEntry of key k < size. LIST: at(p) -> the index at list position p
template <class TABLE, class LIST>
BLSW_HD RegistryEntry registry_fetch(const LIST& list, uint64_t pos, uint32_t size, const TABLE& table) {
    const uint32_t k = list.at(pos);
    if (k >= size) return {fp_zero(), fp_zero(), DEC_BAD_INDEX};
    return table.load(k);
}
template <class TABLE, class LIST>
BLSW_HD CommitteePartial registry_lane_sum(const LIST& list, uint64_t len, uint32_t l, uint32_t L, uint32_t size, const TABLE& table) {
    CommitteePartial p = committee_empty();
    uint64_t pos = l;
    if (pos >= len) return p;
    RegistryEntry cur = registry_fetch(list, pos, size, table);
#pragma unroll 1
    for (;;) {
        const uint64_t next_pos = pos + L;
        const bool more = next_pos < len;
        RegistryEntry next = cur;
        if (more) next = registry_fetch(list, next_pos, size, table);  // in flight under the addition below
        p.count++;
        if (cur.status == DEC_OK) {
            p.sum = v1_add_mixed(p.sum, cur.x, cur.y);
        } else if (cur.status != DEC_IDENTITY && p.bad_index == BLSW_COMMITTEE_NO_BAD) {  // pos ascends: the first one met is the lane's lowest
            p.bad_index = (uint32_t)pos;
            p.bad_status = cur.status;
        }
        if (!more) break;
        cur = next;
        pos = next_pos;
    }
    return p;
}
// Set i of a CSR list: [lo, hi) = off[i], off[i + 1]. False when the offsets describe no list inside the n_indices entries (or one beyond
// BLSW_REGISTRY_MAX_LIST): the set's status is DEC_BAD_INDEX then and none of its entries is read.
BLSW_HD bool registry_list_ok(uint64_t lo, uint64_t hi, uint64_t n_indices) { return lo <= hi && hi <= n_indices && hi - lo <= BLSW_REGISTRY_MAX_LIST; }
// lane 0's partial of a set whose offsets are bad: committee_finish turns it into status DEC_BAD_INDEX, zero coordinates and a zero aggregate
BLSW_HD CommitteePartial registry_bad_list() {
    CommitteePartial p = committee_empty();
    p.bad_index = 0;
    p.bad_status = DEC_BAD_INDEX;
    return p;
}

}  // namespace blsw
