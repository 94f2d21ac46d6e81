// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_combine_points_batch, blsw_lagrange_batch, blsw_recover_points_batch: weighted point sums and Lagrange coefficients at 0 (vcombine.hpp has
// the stages and their reasons). One lane per unit of work, 64-thread workgroups; nothing here shares data between lanes.
#include "kcommon.hpp"
#include "values.hpp"
#include "vcombine.hpp"

namespace blsw {

__device__ __forceinline__ uint64_t cb_lane() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// status: one lane per list, O(k) loads: the list's status goes to status[i], where the scale and sum lanes read it (a lane per term that
// scanned its whole list would read k^2 scalars per list)
__global__ __launch_bounds__(64) void k_combine_status(CombineArgs a) {
    const uint64_t i = cb_lane();
    if (i >= a.n) return;
    const uint64_t first = i * a.k;
    a.status[i] = cb_list_status(cb_count(a.counts, i, a.k), a.k, a.lag ? a.lag[i] : (int32_t)DEC_OK, a.pst + first, a.scalars + 32 * first);
}
// the term's scalar and whether its ladder runs; term_status (nullable) [t][0] the point's, [t][1] the scalar's decode status, used or not
__device__ __forceinline__ bool cb_term(const CombineArgs& a, uint64_t t, uint32_t* w) {
    const uint64_t i = t / a.k;
    const uint32_t j = (uint32_t)(t % a.k);
    const int32_t ss = cb_scalar(a.scalars + 32 * t, w);
    if (a.term_status) {
        a.term_status[2 * t] = a.pst[t];
        a.term_status[2 * t + 1] = ss;
    }
    return a.status[i] == DEC_OK && j < cb_count(a.counts, i, a.k) && a.pst[t] == DEC_OK;
}
// scale: one lane per term, s P as a Jacobian point into the workspace (G1: rows [3][m]; G2: slot 0 of the term's 16 parked points, slots
// 1..15 the table of v_g2_mul_gls, as the signer's)
#ifndef BLSW_COMBINE_G1_WAVES
#define BLSW_COMBINE_G1_WAVES 2  // an A/B build may pass another occupancy (tools/combine_rate.py)
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BLSW_COMBINE_G1_WAVES, BLSW_COMBINE_G1_WAVES))) void k_combine_scale_g1(CombineArgs a) {
    const uint64_t t = cb_lane(), m = a.n * a.k;
    if (t >= m) return;
    uint32_t w[8];
    const bool live = cb_term(a, t, w);
    const Fp* p = a.xy + 2 * t;
    const Jac1v acc = cb_scale_g1(ld_fp(p), ld_fp(p + 1), w, live);
    Fp* o = a.scaled + t;
    st_fp(o, acc.x);
    st_fp(o + m, acc.y);
    st_fp(o + 2 * m, acc.z);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_combine_scale_g2(CombineArgs a) {
    const uint64_t t = cb_lane(), m = a.n * a.k;
    if (t >= m) return;
    uint32_t w[8];
    const bool live = cb_term(a, t, w);
    const Fp* p = a.xy + 4 * t;
    const ParkRows park = {a.scaled + t, m};
    park.st(0, cb_scale_g2(park, {ld_fp(p), ld_fp(p + 1)}, {ld_fp(p + 2), ld_fp(p + 3)}, w, live));
}
// sum: one lane per list. n lanes never fill the device, so the whole register file (as k_vg_sum)
__global__ __launch_bounds__(64) void k_combine_sum(CombineArgs a) {
    const uint64_t i = cb_lane();
    if (i >= a.n) return;
    const uint32_t bytes = a.group == 1 ? 48u : 96u;
    uint8_t* o = a.out + i * bytes;
    if (a.status[i] != DEC_OK) {
        for (uint32_t b = 0; b < bytes; b++) o[b] = 0;
        return;
    }
    const uint64_t first = i * a.k, m = a.n * a.k;
    const uint32_t count = cb_count(a.counts, i, a.k);
    if (a.group == 1) {
        cb_encode_g1(cb_sum_g1(count, [&](uint32_t j) {
                         const Fp* p = a.scaled + first + j;
                         return Jac1v{ld_fp(p), ld_fp(p + m), ld_fp(p + 2 * m)};
                     }),
                     o);
    } else {
        cb_encode_g2(cb_sum_g2(count, [&](uint32_t j) { return ParkRows{a.scaled + first + j, m}.ld(0); }), o);
    }
}
// lagrange: one lane per (list, j), then one lane per list (vcombine.hpp)
__global__ __launch_bounds__(64) void k_lagrange(const uint8_t* __restrict__ ids, const uint32_t* __restrict__ counts, uint32_t k, uint64_t n, uint8_t* coeff) {
    const uint64_t t = cb_lane();
    if (t >= n * k) return;
    const uint64_t i = t / k;
    cb_lagrange_lane(ids + 32 * i * k, cb_count(counts, i, k), k, (uint32_t)(t % k), coeff + 32 * t);
}
__global__ __launch_bounds__(64) void k_lagrange_status(const uint8_t* __restrict__ ids, const uint32_t* __restrict__ counts, uint32_t k, uint64_t n, uint8_t* coeff, int32_t* status) {
    const uint64_t i = cb_lane();
    if (i >= n) return;
    status[i] = cb_lagrange_status(ids + 32 * i * k, cb_count(counts, i, k), k, coeff + 32 * i * k);
}

static unsigned cb_grid(uint64_t lanes) { return (unsigned)((lanes + 63) / 64); }

void launch_lagrange(const uint8_t* ids, const uint32_t* counts, uint32_t k, uint64_t n, uint8_t* coeff, int32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(k_lagrange, dim3(cb_grid(n * k)), dim3(64), 0, st, ids, counts, k, n, coeff);
    hipLaunchKernelGGL(k_lagrange_status, dim3(cb_grid(n)), dim3(64), 0, st, ids, counts, k, n, coeff, status);
}
void launch_combine(const CombineArgs& a, const uint8_t* in, hipStream_t st) {
    const uint64_t m = a.n * a.k;
    hipLaunchKernelGGL(k_decode_points, dim3(cb_grid(m)), dim3(64), 0, st, a.group, in, m, const_cast<Fp*>(a.xy), const_cast<int32_t*>(a.pst));
    hipLaunchKernelGGL(k_combine_status, dim3(cb_grid(a.n)), dim3(64), 0, st, a);
    if (a.group == 1)
        hipLaunchKernelGGL(k_combine_scale_g1, dim3(cb_grid(m)), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(k_combine_scale_g2, dim3(cb_grid(m)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_combine_sum, dim3(cb_grid(a.n)), dim3(64), 0, st, a);
}

}  // namespace blsw
