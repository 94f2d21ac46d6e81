// TEST HARNESS ONLY (never linked into libblsw.so): compiles registry.hpp (with committee.hpp, vcurve.hpp and decode.hpp) of
// bls-verify-gadget_amd/csrc for the HOST with g++ and runs the stages of blsw_registry_append / blsw_registry_verify_batch — the decode into
// 128-byte records, the lane walks over an index list for a given L, the tree and the affine / status / compression step — lanes one after the
// other, so that the kernels' logic is checked against the CPU oracle without a GPU (pytest -m "not gpu"). edges_main.cpp includes this file.
#include <cstring>
#include <vector>
#include "../../bls-verify-gadget_amd/csrc/registry.hpp"

using namespace blsw;

struct RegistryTableHost {
    const RegistryRecord* records;
    RegistryEntry load(uint32_t k) const { return {records[k].x, records[k].y, records[k].status}; }
};
struct RegistryListHost {
    const uint32_t* indices;  // the set's first entry
    uint32_t at(uint64_t pos) const { return indices[pos]; }
};
// the L partials of one set, every lane the caller's
struct RegistryLanesHost {
    std::vector<CommitteePartial> p;
    void exchange() {}
    uint32_t first() const { return 0; }
    uint32_t step() const { return 1; }
    const CommitteePartial& mine(uint32_t l) const { return p[l]; }
    CommitteePartial other(uint32_t m) const { return p[m]; }
    void set(uint32_t l, const CommitteePartial& v) { p[l] = v; }
};

extern "C" {
// k_registry_append: pks48 [count][48] -> records [first, first + count) of `records` ([capacity][128] bytes, 128-byte aligned) and of key_status
void registry_append(const uint8_t* pks48, uint32_t first, uint32_t count, uint8_t* records, int32_t* key_status) {
    RegistryRecord* rec = reinterpret_cast<RegistryRecord*>(records);
    for (uint32_t t = 0; t < count; t++) {
        RegistryRecord& r = rec[first + t];
        std::memset(&r, 0, sizeof(r));
        r.status = g1_decode(pks48 + 48 * (size_t)t, r.x, r.y);
        key_status[first + t] = r.status;
    }
}
// k_registry_sum for n sets with L lanes each: indices [n_indices], offsets [n + 1] -> pk_xy [n][24 words], status [n] (of the sum), agg48 [n][48]
int registry_sum(const uint8_t* records, uint32_t size, const uint32_t* indices, uint64_t n_indices, const uint64_t* offsets, uint32_t n, uint32_t L, uint32_t* pk_xy,
                 int32_t* status, uint8_t* agg48) {
    if (L == 0 || L > 64 || (L & (L - 1))) return -1;
    const RegistryTableHost tab{reinterpret_cast<const RegistryRecord*>(records)};
    for (uint32_t i = 0; i < n; i++) {
        RegistryLanesHost t;
        t.p.assign(L, committee_empty());
        const uint64_t lo = offsets[i], hi = offsets[i + 1];
        if (registry_list_ok(lo, hi, n_indices)) {
            for (uint32_t l = 0; l < L; l++) t.p[l] = registry_lane_sum(RegistryListHost{indices + lo}, hi - lo, l, L, size, tab);
        } else {
            t.p[0] = registry_bad_list();
        }
        committee_tree(t, L);
        Fp x, y;
        status[i] = committee_finish(t.p[0], x, y, agg48 + 48 * (size_t)i);
        std::memcpy(pk_xy + 24 * (size_t)i, &x, 48);
        std::memcpy(pk_xy + 24 * (size_t)i + 12, &y, 48);
    }
    return 0;
}
}
