// DEVICE ONLY: the LANES argument of committee_tree (committee.hpp) for the L lanes of one instance inside one wave — shared by k_committee_sum
// (k_committee.hip) and k_registry_sum (k_registry.hip), so that the exchange layout of a CommitteePartial lives in one place.
// The operand exchange of the tree goes through LDS, not __shfl: a partial is 39 words, which are ten 16-byte LDS stores and ten loads per lane
// and round against 39 ds_bpermute_b32 (the same LDS crossbar, a word at a time, and every lane of the wave has to take part in each). 64 lanes x
// 160 bytes = 10 KB per wave, far below what would limit the two waves per SIMD the registers allow.
#pragma once
#include "committee.hpp"

namespace blsw {

struct alignas(16) CommitteeSlot {
    uint32_t w[40];
};
struct CommitteeLanesWave {
    CommitteeSlot* slots;  // the instance's L slots
    CommitteePartial p;    // this lane's
    uint32_t l;
    __device__ __forceinline__ void exchange() {
        __syncthreads();  // the reads of the round before
        uint4* d = reinterpret_cast<uint4*>(slots[l].w);
        const Fp &x = p.sum.x, &y = p.sum.y, &z = p.sum.z;
        d[0] = {x.l[0], x.l[1], x.l[2], x.l[3]};
        d[1] = {x.l[4], x.l[5], x.l[6], x.l[7]};
        d[2] = {x.l[8], x.l[9], x.l[10], x.l[11]};
        d[3] = {y.l[0], y.l[1], y.l[2], y.l[3]};
        d[4] = {y.l[4], y.l[5], y.l[6], y.l[7]};
        d[5] = {y.l[8], y.l[9], y.l[10], y.l[11]};
        d[6] = {z.l[0], z.l[1], z.l[2], z.l[3]};
        d[7] = {z.l[4], z.l[5], z.l[6], z.l[7]};
        d[8] = {z.l[8], z.l[9], z.l[10], z.l[11]};
        d[9] = {p.count, p.bad_index, (uint32_t)p.bad_status, 0u};
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t first() const { return l; }
    __device__ __forceinline__ uint32_t step() const { return 64; }  // >= any s: one turn of the loop for a lane below s, none above
    __device__ __forceinline__ const CommitteePartial& mine(uint32_t) const { return p; }
    __device__ __forceinline__ CommitteePartial other(uint32_t m) const {
        const uint4* s = reinterpret_cast<const uint4*>(slots[m].w);
        CommitteePartial r;
        Fp* f[3] = {&r.sum.x, &r.sum.y, &r.sum.z};
#pragma unroll
        for (int c = 0; c < 3; c++) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint4 v = s[3 * c + q];
                f[c]->l[4 * q] = v.x;
                f[c]->l[4 * q + 1] = v.y;
                f[c]->l[4 * q + 2] = v.z;
                f[c]->l[4 * q + 3] = v.w;
            }
        }
        const uint4 v = s[9];
        r.count = v.x;
        r.bad_index = v.y;
        r.bad_status = (int32_t)v.z;
        return r;
    }
    __device__ __forceinline__ void set(uint32_t, const CommitteePartial& v) { p = v; }
};

}  // namespace blsw
