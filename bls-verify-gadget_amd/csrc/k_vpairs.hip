// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_verify_pairs_batch: one aggregate signature over K (key, message) pairs per instance (vpairs.hpp has the stages and their reasons).
#include "kcommon.hpp"
#include "team_multi.hpp"
#include "values.hpp"
#include "vpairs.hpp"

namespace blsw {

struct VpArgs {
    uint64_t n, NK;           // instances, n * K pairs
    uint32_t K, chunk, cpi;   // cpi: chunks (teams) per instance
    const uint8_t* pks48;     // [n][K][48]
    const uint8_t* sig96;     // [n][96]
    const uint32_t* counts;   // [n] or null
    Fp* key_xy;               // [NK][2] affine keys
    uint64_t* sig_xy;         // [n][24]
    int32_t* key_status;      // [NK]: the caller's d_key_status, or the workspace's
    int32_t* status;          // [n][2]
    Fp* lines_h;              // [BLSW_VLINE_ROWS][NK]
    Fp* lines_s;              // [BLSW_VLINE_ROWS][n]
    Fp* partials;             // [n * cpi][6] Fp2
    int32_t* result;          // [n]
};

__device__ __forceinline__ bool vp_folds(const VpArgs& a, uint64_t i) { return a.status[2 * i] == DEC_OK && a.status[2 * i + 1] == DEC_OK; }

// decode: lanes [0, NK) the keys, used or not, into key_xy and key_status; lanes [NK, NK + n) the signatures, status[i][1]
__global__ __launch_bounds__(64) void k_vp_decode(VpArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.NK + a.n) return;
    if (t < a.NK) {
        Fp x, y;
        a.key_status[t] = g1_decode(a.pks48 + t * 48, x, y);
        st_fp(a.key_xy + 2 * t, x);
        st_fp(a.key_xy + 2 * t + 1, y);
    } else {
        const uint64_t i = t - a.NK;
        Fp2 x, y;
        const int st = g2_decode(a.sig96 + i * 96, x, y);
        Fp* o = reinterpret_cast<Fp*>(a.sig_xy + i * 24);
        st_fp(o, x.c0);
        st_fp(o + 1, x.c1);
        st_fp(o + 2, y.c0);
        st_fp(o + 3, y.c1);
        a.status[2 * i + 1] = st;
    }
}
// status: one lane per instance
__global__ __launch_bounds__(64) void k_vp_status(VpArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    a.status[2 * i] = vp_instance_status(a.counts, i, a.K, a.key_status);
}
// lines: lanes [0, NK) H(m_ij) (ws.h, homogeneous) against the affine pk_ij; lanes [NK, NK + n) sig_i against -g1. A pair the fold never reads
// writes nothing.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_vp_lines(VpArgs a, Workspace ws) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.NK + a.n) return;
    const uint64_t NK = a.NK;
    if (t < NK) {
        const uint64_t i = t / a.K;
        if (!vp_folds(a, i) || (uint32_t)(t - i * a.K) >= vp_count_eff(a.counts, i, a.K)) return;
        const Proj<OpsFp2> h = ld_proj2(ws.h + t, NK);
        const Fp2 zi = fp2_inv_inl(h.z);
        const Fp* p = a.key_xy + 2 * t;
        vline_chain(fp2_mul_inl(h.x, zi), fp2_mul_inl(h.y, zi), ld_fp(p), ld_fp(p + 1), CoeffStrided{a.lines_h + t, NK});
    } else {
        const uint64_t i = t - NK;
        if (!vp_folds(a, i)) return;
        const Fp* p = reinterpret_cast<const Fp*>(a.sig_xy + i * 24);
        vline_chain({ld_fp(p), ld_fp(p + 1)}, {ld_fp(p + 2), ld_fp(p + 3)}, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), CoeffStrided{a.lines_s + i, a.n});
    }
}
// fold: six lanes per chunk (team T = i * cpi + q), ten chunks per wave, the slot file of k_vg_fold
__global__ __launch_bounds__(64) void k_vp_fold(VpArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint64_t teams = a.n * a.cpi;
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t T0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && T0 < teams;
    const uint64_t T = active ? T0 : (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE;  // idle lanes walk the loop of the wave's first team
    const uint64_t i = T / a.cpi;
    const uint32_t q = (uint32_t)(T % a.cpi);
    const VpChunk c = vp_chunk(a.chunk, vp_count_eff(a.counts, i, a.K), q);
    TeamLanesGroups t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = {nullptr, 0};
    t.coeff_h = {nullptr, 0};
    t.e = {nullptr, 0};
    t.lines_h = a.lines_h;
    t.lines_g = a.lines_s;
    t.partials = nullptr;
    t.n = a.NK;
    t.n_groups = a.n;
    t.first = i * a.K + c.first;
    t.grp = i;
    t.count = c.count;
    t.mask = vp_chunk_mask(c, q, vp_folds(a, i));
    const Fp2 f = team_miller_groups(t, (uint32_t)t.first, c.count + (q == 0 ? 1u : 0u));
    if (active) {
        Fp* o = a.partials + (T * 6 + j) * 2;
        st_fp(o, f.c0);
        st_fp(o + 1, f.c1);
    }
}
// finish: six lanes per instance
__global__ __launch_bounds__(64) void k_vp_finish(VpArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t I0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && I0 < a.n;
    const uint64_t i = active ? I0 : 0;
    TeamLanesGroups t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = {nullptr, 0};
    t.coeff_h = {nullptr, 0};
    t.e = {nullptr, 0};
    t.lines_h = nullptr;
    t.lines_g = nullptr;
    t.partials = a.partials;
    t.n = a.NK;
    t.n_groups = a.n;
    t.first = 0;
    t.grp = i;
    t.count = 0;
    t.mask = 0;
    const bool one = team_groups_finish(t, i * a.cpi, a.cpi);
    if (active && j == 0) a.result[i] = (one && vp_folds(a, i)) ? 1 : 0;
}

void launch_verify_pairs(uint64_t n, uint32_t n_pairs, uint32_t chunk, const Workspace& ws, const uint8_t* pks48, const uint8_t* sig96, const uint32_t* counts, Fp* key_xy,
                         uint64_t* sig_xy, int32_t* key_status, int32_t* status, Fp* lines_h, Fp* lines_s, Fp* partials, int32_t* result, hipStream_t st) {
    VpArgs a;
    a.n = n;
    a.NK = n * n_pairs;
    a.K = n_pairs;
    a.chunk = chunk;
    a.cpi = vp_chunks_per_instance(n_pairs, chunk);
    a.pks48 = pks48;
    a.sig96 = sig96;
    a.counts = counts;
    a.key_xy = key_xy;
    a.sig_xy = sig_xy;
    a.key_status = key_status;
    a.status = status;
    a.lines_h = lines_h;
    a.lines_s = lines_s;
    a.partials = partials;
    a.result = result;
    const uint64_t lanes = a.NK + n, teams = n * a.cpi;
    hipLaunchKernelGGL(k_vp_decode, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vp_status, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vp_lines, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, a, ws);
    hipLaunchKernelGGL(k_vp_fold, dim3((unsigned)((teams + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vp_finish, dim3((unsigned)((n + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a);
}

}  // namespace blsw
