// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_registry_*: keys decoded once into a resident table of 128-byte records, n index lists summed with BLSW_REGISTRY_LANES lanes each
// (registry.hpp has the stages and their reasons); the sums then go to launch_verify_values / launch_verify_groups unchanged.
#include "kcommon.hpp"
#include "registry.hpp"
#include "committee_wave.hpp"  // CommitteeSlot, CommitteeLanesWave: the tree's operand exchange through LDS

namespace blsw {

static_assert(BLSW_REGISTRY_LANES >= 1 && BLSW_REGISTRY_LANES <= 64 && (BLSW_REGISTRY_LANES & (BLSW_REGISTRY_LANES - 1)) == 0,
              "the lanes of a set are a power-of-two slice of one wave");

// append: lane t decodes key first + t into its record and its entry of the status array. The host has checked first + count <= capacity.
__global__ __launch_bounds__(64) void k_registry_append(const uint8_t* __restrict__ pks48, uint32_t first, uint32_t count, RegistryRecord* records, int32_t* key_status) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    Fp x, y;
    const int32_t st = g1_decode(pks48 + t * 48, x, y);
    RegistryRecord* r = records + first + t;
    st_fp(&r->x, x);
    st_fp(&r->y, y);
    blsw_global_u32x4* tail = (blsw_global_u32x4*)&r->status;  // the status and the unused words: the whole record is defined
    tail[0] = blsw_u32x4{(uint32_t)st, 0u, 0u, 0u};
    tail[1] = blsw_u32x4{0u, 0u, 0u, 0u};
    key_status[first + t] = st;
}

struct RegistryTableDev {
    const RegistryRecord* records;
    __device__ __forceinline__ RegistryEntry load(uint32_t k) const {
        const RegistryRecord* r = records + k;
        RegistryEntry e;
        e.x = ld_fp(&r->x);
        e.y = ld_fp(&r->y);
        e.status = r->status;
        return e;
    }
};
struct RegistryListDev {
    const uint32_t* indices;  // the set's first entry
    __device__ __forceinline__ uint32_t at(uint64_t pos) const { return indices[pos]; }
};
struct RegistrySumArgs {
    uint64_t n, n_indices;
    uint32_t size;  // the registry's size as of the call: no record at or beyond it is read
    const RegistryRecord* records;
    const uint32_t* indices;  // [n_indices]
    const uint64_t* offsets;  // [n + 1]
    uint64_t* pk_xy;          // [n][12]
    int32_t* status;          // [n][2]: writes [i][0]
    uint8_t* agg48;           // [n][48] or null
};
// sum: L lanes per set, 64 / L sets per wave, block = one wave. A wave finishes with its longest list. Lanes of a set past n, and the lanes of a
// set whose offsets are bad, walk nothing, but stay for the barriers of the tree.
__global__ __launch_bounds__(64) void k_registry_sum(RegistrySumArgs a) {
    constexpr uint32_t L = BLSW_REGISTRY_LANES;
    __shared__ CommitteeSlot lds[64];
    const uint32_t inst = threadIdx.x / L, l = threadIdx.x % L;
    const uint64_t i = (uint64_t)blockIdx.x * (64 / L) + inst;
    const bool active = i < a.n;
    CommitteeLanesWave t;
    t.slots = lds + inst * L;
    t.l = l;
    t.p = committee_empty();
    if (active) {
        const uint64_t lo = a.offsets[i], hi = a.offsets[i + 1];
        if (registry_list_ok(lo, hi, a.n_indices))
            t.p = registry_lane_sum(RegistryListDev{a.indices + lo}, hi - lo, l, L, a.size, RegistryTableDev{a.records});
        else if (l == 0)
            t.p = registry_bad_list();
    }
    committee_tree(t, L);
    if (!active || l != 0) return;
    Fp x, y;
    a.status[2 * i] = committee_finish(t.p, x, y, a.agg48 ? a.agg48 + i * 48 : nullptr);
    Fp* o = reinterpret_cast<Fp*>(a.pk_xy + i * 12);
    st_fp(o, x);
    st_fp(o + 1, y);
}

void launch_registry_append(const uint8_t* pks48, uint32_t first, uint32_t count, void* records, int32_t* key_status, hipStream_t st) {
    hipLaunchKernelGGL(k_registry_append, dim3((count + 63) / 64), dim3(64), 0, st, pks48, first, count, reinterpret_cast<RegistryRecord*>(records), key_status);
}
void launch_registry_sum(const void* records, uint32_t size, const uint32_t* indices, uint64_t n_indices, const uint64_t* offsets, uint64_t n, uint64_t* pk_xy, int32_t* status,
                         uint8_t* agg48, hipStream_t st) {
    RegistrySumArgs a;
    a.n = n;
    a.n_indices = n_indices;
    a.size = size;
    a.records = reinterpret_cast<const RegistryRecord*>(records);
    a.indices = indices;
    a.offsets = offsets;
    a.pk_xy = pk_xy;
    a.status = status;
    a.agg48 = agg48;
    const uint64_t per_wave = 64 / BLSW_REGISTRY_LANES;
    hipLaunchKernelGGL(k_registry_sum, dim3((unsigned)((n + per_wave - 1) / per_wave)), dim3(64), 0, st, a);
}

}  // namespace blsw
