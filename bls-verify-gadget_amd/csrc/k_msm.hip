// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_msm_points_batch: sum_j s_j P_j for long lists by the bucket method (vmsm.hpp has the stages and their reasons). 64-thread workgroups; every
// kernel walks its units of work with a grid-sized stride, so no shape can ask for more workgroups than a launch takes. The only data lanes
// share are the histogram and the cursor (atomicAdd) and, in the scan, 64 partial sums in LDS.
#include "kcommon.hpp"
#include "values.hpp"
#include "vmsm.hpp"  // registry.hpp with it: the records of the registry form

namespace blsw {

#define BLSW_MSM_MAX_GRID (1u << 20)
__device__ __forceinline__ uint64_t msm_lane() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint64_t msm_stride() { return (uint64_t)gridDim.x * blockDim.x; }

// Jacobian points in element-major rows: point q of `lanes`
template <class G>
struct MsmRows;
template <>
struct MsmRows<MsmG1> {
    Fp* p;
    uint64_t lanes;
    __device__ __forceinline__ Jac1v ld(uint64_t q) const { return {ld_fp(p + q), ld_fp(p + lanes + q), ld_fp(p + 2 * lanes + q)}; }
    __device__ __forceinline__ void st(uint64_t q, const Jac1v& v) const {
        st_fp(p + q, v.x);
        st_fp(p + lanes + q, v.y);
        st_fp(p + 2 * lanes + q, v.z);
    }
};
template <>
struct MsmRows<MsmG2> {
    Fp* p;
    uint64_t lanes;
    __device__ __forceinline__ Jac2 ld(uint64_t q) const { return ParkRows{p + q, lanes}.ld(0); }
    __device__ __forceinline__ void st(uint64_t q, const Jac2& v) const { ParkRows{p + q, lanes}.st(0, v); }
};
__device__ __forceinline__ MsmAff1 msm_point(const MsmG1&, const Fp* xy, uint64_t t) { return {ld_fp(xy + 2 * t), ld_fp(xy + 2 * t + 1)}; }
__device__ __forceinline__ MsmAff2 msm_point(const MsmG2&, const Fp* xy, uint64_t t) {
    const Fp* p = xy + 4 * t;
    return {{ld_fp(p), ld_fp(p + 1)}, {ld_fp(p + 2), ld_fp(p + 3)}};
}

__global__ __launch_bounds__(64) void k_msm_zero(uint32_t* p, uint64_t words) {
    for (uint64_t t = msm_lane(); t < words; t += msm_stride()) p[t] = 0;
}
// 1: one lane per list, as k_combine_status
__global__ __launch_bounds__(64) void k_msm_status(MsmArgs a) {
    for (uint64_t i = msm_lane(); i < a.n; i += msm_stride()) {
        const uint64_t first = i * a.k;
        a.status[i] = cb_list_status(cb_count(a.counts, i, a.k), a.k, DEC_OK, a.pst + first, a.scalars + 32 * first);
    }
}
// 2 and 4: one lane per term. SCATTER false: count the term's non-zero digits; true: place the term in each of their buckets
template <bool SCATTER>
__global__ __launch_bounds__(64) void k_msm_digits(MsmArgs a) {
    const uint64_t m = a.n * a.k;
    const uint32_t W = msm_windows(a.c), B = msm_buckets(a.c);
    for (uint64_t t = msm_lane(); t < m; t += msm_stride()) {
        const uint64_t i = t / a.k;
        const uint32_t j = (uint32_t)(t % a.k);
        if (a.status[i] != DEC_OK) continue;  // also: no scalar of a list whose count lies beyond k is read
        uint32_t w[8];
        if (cb_scalar(a.scalars + 32 * t, w) != DEC_OK || !msm_term_live(DEC_OK, j, cb_count(a.counts, i, a.k), a.pst[t], w)) continue;
#pragma unroll 1
        for (uint32_t win = 0; win < W; win++) {
            const uint32_t d = msm_digit(w, win, a.c);
            if (d == 0) continue;
            const uint64_t q = (i * W + win) * B + d;
            if (SCATTER)
                a.sorted[win * m + i * a.k + atomicAdd(a.cursor + q, 1u)] = (uint32_t)t;  // the cursor stays below the list's count: the scan summed these same digits
            else
                atomicAdd(a.hist + q, 1u);
        }
    }
}
// 3: one workgroup per (list, window) row
__global__ __launch_bounds__(BLSW_MSM_SCAN_LANES) void k_msm_scan(MsmArgs a) {
    __shared__ uint32_t sums[BLSW_MSM_SCAN_LANES];
    const uint32_t B = msm_buckets(a.c), l = threadIdx.x;
    const uint64_t rows = a.n * msm_windows(a.c);
    uint32_t lo, hi;
    msm_scan_slice(B, l, &lo, &hi);
    for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {  // uniform over the workgroup: every lane meets every barrier
        uint32_t* h = a.hist + row * B;
        sums[l] = msm_scan_sum(h, lo, hi);
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t x = 0; x < l; x++) before += sums[x];
        msm_scan_write(h, a.cursor + row * B, lo, hi, before);
        __syncthreads();
    }
}
// 5: one lane per (list, window, bucket); two waves per SIMD as the signer's ladders and k_combine_scale_*
template <class G>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_msm_buckets(MsmArgs a) {
    const uint64_t m = a.n * a.k;
    const uint32_t W = msm_windows(a.c), B = msm_buckets(a.c);
    const uint64_t lanes = a.n * W * B;
    const MsmRows<G> out = {a.buckets, lanes};
    for (uint64_t q = msm_lane(); q < lanes; q += msm_stride()) {
        const uint64_t row = q / B, i = row / W;
        const uint32_t win = (uint32_t)(row % W);
        out.st(q, msm_bucket<G>(a.sorted + win * m + i * a.k, a.hist[q], a.cursor[q], [&](uint32_t t) { return msm_point(G(), a.xy, t); }));
    }
}
// 6: one lane per segment, then one lane per (list, window)
template <class G>
__global__ __launch_bounds__(64) void k_msm_segments(MsmArgs a) {
    const uint32_t B = msm_buckets(a.c), S = msm_segments(a.c);
    const uint64_t rows = a.n * msm_windows(a.c), lanes = rows * S;
    const MsmRows<G> in = {a.buckets, rows * B}, out = {a.segments, lanes};
    for (uint64_t q = msm_lane(); q < lanes; q += msm_stride()) {
        const uint64_t row = q / S;
        out.st(q, msm_segment<G>((uint32_t)(q % S), a.c, [&](uint32_t b) { return in.ld(row * B + b); }));
    }
}
template <class G>
__global__ __launch_bounds__(64) void k_msm_windows(MsmArgs a) {
    const uint32_t S = msm_segments(a.c);
    const uint64_t rows = a.n * msm_windows(a.c);
    const MsmRows<G> in = {a.segments, rows * S}, out = {a.windows, rows};
    for (uint64_t row = msm_lane(); row < rows; row += msm_stride()) out.st(row, msm_window<G>(a.c, [&](uint32_t s) { return in.ld(row * S + s); }));
}
// 7: one lane per list
template <class G>
__global__ __launch_bounds__(64) void k_msm_final(MsmArgs a) {
    const uint32_t W = msm_windows(a.c);
    const MsmRows<G> in = {a.windows, a.n * W};
    for (uint64_t i = msm_lane(); i < a.n; i += msm_stride()) {
        uint8_t* o = a.out + i * G::BYTES;
        if (a.status[i] != DEC_OK) {
            for (uint32_t b = 0; b < G::BYTES; b++) o[b] = 0;
            continue;
        }
        G::encode(msm_final<G>(a.c, [&](uint32_t w) { return in.ld(i * W + w); }), o);
    }
}

// ---- the registry form: its status lane, its term lanes (one per position of d_indices), its point loader and its final lane
__device__ __forceinline__ const RegistryRecord* msm_record(const MsmArgs& a, uint64_t p) { return reinterpret_cast<const RegistryRecord*>(a.records) + a.indices[p]; }
__global__ __launch_bounds__(64) void k_msm_reg_status(MsmArgs a) {
    const RegistryRecord* rec = reinterpret_cast<const RegistryRecord*>(a.records);
    for (uint64_t i = msm_lane(); i < a.n; i += msm_stride()) {
        const uint64_t lo = a.offsets[i], hi = a.offsets[i + 1];
        const int32_t st = msm_registry_status(a.indices, a.scalars, lo, hi, a.n_indices, a.size, [&](uint32_t idx) { return rec[idx].status; });
        a.status[i] = st;
        a.serial[i] = 0;
        if (st != DEC_OK) continue;
        for (uint64_t p = lo; p < hi; p++) {
            atomicAdd(a.claims + p, 1u);
            a.owner[p] = (uint32_t)i;  // read only where the claim count is 1: then this is the one write
        }
    }
}
__global__ __launch_bounds__(64) void k_msm_reg_claims(MsmArgs a) {
    for (uint64_t i = msm_lane(); i < a.n; i += msm_stride()) {
        if (a.status[i] != DEC_OK) continue;
        int32_t shared = 0;
        for (uint64_t p = a.offsets[i]; p < a.offsets[i + 1]; p++) shared |= a.claims[p] != 1u;
        a.serial[i] = shared;
    }
}
template <bool SCATTER>
__global__ __launch_bounds__(64) void k_msm_reg_digits(MsmArgs a) {
    const uint32_t W = msm_windows(a.c), B = msm_buckets(a.c);
    for (uint64_t p = msm_lane(); p < a.n_indices; p += msm_stride()) {
        if (a.claims[p] != 1u) continue;  // no OK list holds it, or several do
        const uint64_t i = a.owner[p];
        if (a.serial[i]) continue;
        uint32_t w[8];
        cb_scalar(a.scalars + 32 * p, w);  // below r: the list is OK
        if (msm_record(a, p)->status != DEC_OK || cb_words_zero(w)) continue;  // an identity key, a zero scalar
        const uint64_t lo = a.offsets[i];
#pragma unroll 1
        for (uint32_t win = 0; win < W; win++) {
            const uint32_t d = msm_digit(w, win, a.c);
            if (d == 0) continue;
            const uint64_t q = (i * W + win) * B + d;
            if (SCATTER)
                a.sorted[win * a.n_indices + lo + atomicAdd(a.cursor + q, 1u)] = (uint32_t)(p - lo);
            else
                atomicAdd(a.hist + q, 1u);
        }
    }
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_msm_reg_buckets(MsmArgs a) {
    const uint32_t W = msm_windows(a.c), B = msm_buckets(a.c);
    const uint64_t lanes = a.n * W * B;
    const MsmRows<MsmG1> out = {a.buckets, lanes};
    for (uint64_t q = msm_lane(); q < lanes; q += msm_stride()) {
        const uint64_t row = q / B, i = row / W;
        const uint32_t win = (uint32_t)(row % W), first = a.hist[q], last = a.cursor[q];
        Jac1v acc = MsmG1::zero();
        if (first != last) {  // only then do the offsets describe a list
            const uint64_t lo = a.offsets[i];
            acc = msm_bucket<MsmG1>(a.sorted + win * a.n_indices + lo, first, last, [&](uint32_t j) {
                const RegistryRecord* r = msm_record(a, lo + j);
                return MsmAff1{ld_fp(&r->x), ld_fp(&r->y)};
            });
        }
        out.st(q, acc);
    }
}
__global__ __launch_bounds__(64) void k_msm_reg_final(MsmArgs a) {
    const uint32_t W = msm_windows(a.c);
    const MsmRows<MsmG1> in = {a.windows, a.n * W};
    for (uint64_t i = msm_lane(); i < a.n; i += msm_stride()) {
        uint8_t* o = a.out + i * 48;
        if (a.status[i] != DEC_OK) {
            for (uint32_t b = 0; b < 48; b++) o[b] = 0;
            continue;
        }
        Jac1v acc = MsmG1::zero();
        if (a.serial[i]) {
#pragma unroll 1
            for (uint64_t p = a.offsets[i]; p < a.offsets[i + 1]; p++) {
                const RegistryRecord* r = msm_record(a, p);
                uint32_t w[8];
                cb_scalar(a.scalars + 32 * p, w);
                acc = v1_add(acc, cb_scale_g1(ld_fp(&r->x), ld_fp(&r->y), w, r->status == DEC_OK));
            }
        } else {
            acc = msm_final<MsmG1>(a.c, [&](uint32_t w) { return in.ld(i * W + w); });
        }
        cb_encode_g1(acc, o);
    }
}

static unsigned msm_grid(uint64_t lanes) {
    const uint64_t g = (lanes + 63) / 64;
    return (unsigned)(g < BLSW_MSM_MAX_GRID ? (g ? g : 1) : BLSW_MSM_MAX_GRID);
}
template <class G>
static void launch_msm_sums(const MsmArgs& a, uint64_t rows, hipStream_t st) {
    hipLaunchKernelGGL(k_msm_buckets<G>, dim3(msm_grid(rows * msm_buckets(a.c))), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_segments<G>, dim3(msm_grid(rows * msm_segments(a.c))), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_windows<G>, dim3(msm_grid(rows)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_final<G>, dim3(msm_grid(a.n)), dim3(64), 0, st, a);
}
void launch_msm(const MsmArgs& a, const uint8_t* in, hipStream_t st) {
    const uint64_t m = a.n * a.k, rows = a.n * msm_windows(a.c);
    hipLaunchKernelGGL(k_decode_points, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, a.group, in, m, const_cast<Fp*>(a.xy), const_cast<int32_t*>(a.pst));
    hipLaunchKernelGGL(k_msm_status, dim3(msm_grid(a.n)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_zero, dim3(msm_grid(rows * msm_buckets(a.c))), dim3(64), 0, st, a.hist, rows * msm_buckets(a.c));
    hipLaunchKernelGGL(k_msm_digits<false>, dim3(msm_grid(m)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_scan, dim3((unsigned)(rows < BLSW_MSM_MAX_GRID ? rows : BLSW_MSM_MAX_GRID)), dim3(BLSW_MSM_SCAN_LANES), 0, st, a);
    hipLaunchKernelGGL(k_msm_digits<true>, dim3(msm_grid(m)), dim3(64), 0, st, a);
    if (a.group == 1)
        launch_msm_sums<MsmG1>(a, rows, st);
    else
        launch_msm_sums<MsmG2>(a, rows, st);
}
void launch_msm_registry(const MsmArgs& a, hipStream_t st) {
    const uint64_t rows = a.n * msm_windows(a.c);
    hipLaunchKernelGGL(k_msm_zero, dim3(msm_grid(rows * msm_buckets(a.c))), dim3(64), 0, st, a.hist, rows * msm_buckets(a.c));
    hipLaunchKernelGGL(k_msm_zero, dim3(msm_grid(a.n_indices)), dim3(64), 0, st, a.claims, a.n_indices);
    hipLaunchKernelGGL(k_msm_reg_status, dim3(msm_grid(a.n)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_reg_claims, dim3(msm_grid(a.n)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_reg_digits<false>, dim3(msm_grid(a.n_indices)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_scan, dim3((unsigned)(rows < BLSW_MSM_MAX_GRID ? rows : BLSW_MSM_MAX_GRID)), dim3(BLSW_MSM_SCAN_LANES), 0, st, a);
    hipLaunchKernelGGL(k_msm_reg_digits<true>, dim3(msm_grid(a.n_indices)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_reg_buckets, dim3(msm_grid(rows * msm_buckets(a.c))), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_segments<MsmG1>, dim3(msm_grid(rows * msm_segments(a.c))), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_windows<MsmG1>, dim3(msm_grid(rows)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_msm_reg_final, dim3(msm_grid(a.n)), dim3(64), 0, st, a);
}

}  // namespace blsw
