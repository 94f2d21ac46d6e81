// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_committee_verify_batch: one committee decoded once, n bitmaps summed with BLSW_COMMITTEE_LANES lanes each (committee.hpp has the stages and
// their reasons); the aggregated keys then go to launch_verify_values / launch_verify_groups unchanged.
#include "kcommon.hpp"
#include "committee_wave.hpp"  // CommitteeSlot, CommitteeLanesWave: the tree's operand exchange through LDS

namespace blsw {

static_assert(BLSW_COMMITTEE_LANES >= 1 && BLSW_COMMITTEE_LANES <= 64 && (BLSW_COMMITTEE_LANES & (BLSW_COMMITTEE_LANES - 1)) == 0,
              "the lanes of an instance are a power-of-two slice of one wave");

// decode: lanes [0, K) the committee's keys into the table (x row, y row) and d_key_status; lanes [K, K + n) the signatures, status[i][1]
__global__ __launch_bounds__(64) void k_committee_decode(const uint8_t* __restrict__ pks48, uint32_t K, const uint8_t* __restrict__ sig96, uint64_t n, Fp* table,
                                                         int32_t* key_status, uint64_t* sig_xy, int32_t* status) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K + n) return;
    if (t < K) {
        Fp x, y;
        key_status[t] = g1_decode(pks48 + t * 48, x, y);
        st_fp(table + t, x);
        st_fp(table + K + t, y);
    } else {
        const uint64_t i = t - K;
        Fp2 x, y;
        const int st = g2_decode(sig96 + i * 96, x, y);
        Fp* o = reinterpret_cast<Fp*>(sig_xy + i * 24);
        st_fp(o, x.c0);
        st_fp(o + 1, x.c1);
        st_fp(o + 2, y.c0);
        st_fp(o + 3, y.c1);
        status[2 * i + 1] = st;
    }
}

struct CommitteeTableRows {
    const Fp* xy;  // [2][K]
    const int32_t* status;
    uint32_t K;
    __device__ __forceinline__ Fp x(uint32_t k) const { return ld_fp(xy + k); }
    __device__ __forceinline__ Fp y(uint32_t k) const { return ld_fp(xy + K + k); }
    __device__ __forceinline__ int32_t st(uint32_t k) const { return status[k]; }
};
struct CommitteeSumArgs {
    uint64_t n;
    uint32_t K;
    const uint8_t* bitmap;  // [n][K]
    const Fp* table;        // [2][K]
    const int32_t* key_status;
    uint64_t* pk_xy;  // [n][12]
    int32_t* status;  // [n][2]: writes [i][0]
    uint32_t* count;  // [n] or null
    uint8_t* agg48;   // [n][48] or null
};
// sum: L lanes per instance, 64 / L instances per wave, block = one wave. Lanes of an instance past n walk nothing and write nothing, but
// stay for the barriers of the tree.
__global__ __launch_bounds__(64) void k_committee_sum(CommitteeSumArgs a) {
    constexpr uint32_t L = BLSW_COMMITTEE_LANES;
    __shared__ CommitteeSlot lds[64];
    const uint32_t inst = threadIdx.x / L, l = threadIdx.x % L;
    const uint64_t i = (uint64_t)blockIdx.x * (64 / L) + inst;
    const bool active = i < a.n;
    CommitteeLanesWave t;
    t.slots = lds + inst * L;
    t.l = l;
    t.p = committee_empty();
    if (active) t.p = committee_lane_sum(a.bitmap + i * a.K, a.K, l, L, CommitteeTableRows{a.table, a.key_status, a.K});
    committee_tree(t, L);
    if (!active || l != 0) return;
    Fp x, y;
    a.status[2 * i] = committee_finish(t.p, x, y, a.agg48 ? a.agg48 + i * 48 : nullptr);
    Fp* o = reinterpret_cast<Fp*>(a.pk_xy + i * 12);
    st_fp(o, x);
    st_fp(o + 1, y);
    if (a.count) a.count[i] = t.p.count;
}

void launch_committee_decode(const uint8_t* pks48, uint32_t n_keys, const uint8_t* sig96, uint64_t n, Fp* table, int32_t* key_status, uint64_t* sig_xy, int32_t* status,
                             hipStream_t st) {
    hipLaunchKernelGGL(k_committee_decode, dim3((unsigned)((n_keys + n + 63) / 64)), dim3(64), 0, st, pks48, n_keys, sig96, n, table, key_status, sig_xy, status);
}
void launch_committee_sum(const uint8_t* bitmap, uint32_t n_keys, uint64_t n, const Fp* table, const int32_t* key_status, uint64_t* pk_xy, int32_t* status, uint32_t* count,
                          uint8_t* agg48, hipStream_t st) {
    CommitteeSumArgs a;
    a.n = n;
    a.K = n_keys;
    a.bitmap = bitmap;
    a.table = table;
    a.key_status = key_status;
    a.pk_xy = pk_xy;
    a.status = status;
    a.count = count;
    a.agg48 = agg48;
    const uint64_t per_wave = 64 / BLSW_COMMITTEE_LANES;
    hipLaunchKernelGGL(k_committee_sum, dim3((unsigned)((n + per_wave - 1) / per_wave)), dim3(64), 0, st, a);
}

}  // namespace blsw
