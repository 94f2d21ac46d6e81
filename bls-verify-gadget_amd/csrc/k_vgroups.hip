// libblsw.so, one translation unit per kernel family (see kcommon.hpp, build.py).
// blsw_verify_groups_batch: groups of (pk, msg, sig) triples verified with random coefficients (vgroups.hpp has the stages and their reasons).
#include "kcommon.hpp"
#include "team_multi.hpp"
#include "values.hpp"
#include "vgroups.hpp"
#include "vshared.hpp"

namespace blsw {

struct VgArgs {
    uint64_t n, n_groups;
    uint32_t group, chunk, cpg;  // cpg: chunks (teams) per group
    const uint64_t* pk_xy;
    const uint64_t* sig_xy;
    const int32_t* status;    // [n][2], written by k_decode
    const uint64_t* scalars;  // [n]
    Fp* p_scaled;             // [3][n]  r_i pk_i, Jacobian
    Fp* s_scaled;             // [6][n]  r_i sig_i, Jacobian
    Fp* sum_xy;               // [4][n_groups] S_g affine (zeros: the identity)
    int32_t* gflag;           // [n_groups] VG_FLAG_*
    Fp* lines_h;              // [BLSW_VLINE_ROWS][n]
    Fp* lines_g;              // [BLSW_VLINE_ROWS][n_groups]
    Fp* partials;             // [n_groups * cpg][6] Fp2
    int32_t* result;          // [n_groups]
};

__device__ __forceinline__ bool vg_included_at(const VgArgs& a, uint64_t i) { return vg_included(a.status[2 * i], a.status[2 * i + 1], a.scalars[i]); }

// scale: lanes [0, n) P_i = r_i pk_i, lanes [n, 2 n) S_i = r_i sig_i; the identity (z = 0) for an excluded instance
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_vg_scale(VgArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * a.n) return;
    const uint64_t n = a.n, i = t < n ? t : t - n;
    const uint64_t r = vg_included_at(a, i) ? a.scalars[i] : 0;
    if (t < n) {
        const Fp* p = reinterpret_cast<const Fp*>(a.pk_xy + i * 12);
        const Jac1v acc = vg_scale_g1(ld_fp(p), ld_fp(p + 1), r);
        Fp* o = a.p_scaled + i;
        st_fp(o, acc.x);
        st_fp(o + n, acc.y);
        st_fp(o + 2 * n, acc.z);
    } else {
        const Fp* p = reinterpret_cast<const Fp*>(a.sig_xy + i * 24);
        ParkRows{a.s_scaled + i, n}.st(0, vg_scale_g2({ld_fp(p), ld_fp(p + 1)}, {ld_fp(p + 2), ld_fp(p + 3)}, r));
    }
}
// sum: one lane per group. n / group lanes never fill the device, so the whole register file (at two waves per SIMD the general addition spills 278)
__global__ __launch_bounds__(64) void k_vg_sum(VgArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n_groups) return;
    const uint64_t first = g * a.group;
    const uint32_t m = (uint32_t)(a.n - first < a.group ? a.n - first : a.group);
    bool ok = true;
    for (uint32_t i = 0; i < m; i++) ok = ok && vg_included_at(a, first + i);
    const Jac2 s = vg_sum(m, [&](uint32_t i) { return ParkRows{a.s_scaled + first + i, a.n}.ld(0); });
    Fp2 x, y;
    const bool some = vg_affine2(s, x, y);
    Fp* o = a.sum_xy + g;
    st_fp(o, x.c0);
    st_fp(o + a.n_groups, x.c1);
    st_fp(o + 2 * a.n_groups, y.c0);
    st_fp(o + 3 * a.n_groups, y.c1);
    a.gflag[g] = (ok ? VG_FLAG_OK : 0) | (some ? VG_FLAG_SUM : 0);
}
// lines: lanes [0, n) H(m_i) (ws.h, homogeneous) against the projective P_i; lanes [n, n + n_groups) S_g against -g1. A skipped pair writes nothing:
// the fold never reads its rows.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_vg_lines(VgArgs a, Workspace ws) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n + a.n_groups) return;
    const uint64_t n = a.n;
    if (t < n) {
        if (!vg_included_at(a, t)) return;
        const Proj<OpsFp2> h = ld_proj2(ws.h + t, n);
        const Fp2 zi = fp2_inv_inl(h.z);
        const Fp* p = a.p_scaled + t;
        Fp m0, m1, m2;
        vg_line_multipliers({ld_fp(p), ld_fp(p + n), ld_fp(p + 2 * n)}, m0, m1, m2);
        vline_chain(fp2_mul_inl(h.x, zi), fp2_mul_inl(h.y, zi), m0, m1, m2, CoeffStrided{a.lines_h + t, n});
    } else {
        const uint64_t g = t - n, G = a.n_groups;
        if (!(a.gflag[g] & VG_FLAG_SUM)) return;
        const Fp* p = a.sum_xy + g;
        vline_chain(ld_fp2(p, G), ld_fp2(p + 2 * G, G), K_G1_GEN_X(), K_G1_GEN_NEG_Y(), CoeffStrided{a.lines_g + g, G});
    }
}
// fold: six lanes per chunk (team T = g * cpg + q), ten chunks per wave, the slot file of k_verify_team
__global__ __launch_bounds__(64) void k_vg_fold(VgArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint64_t teams = a.n_groups * a.cpg;
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t T0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && T0 < teams;
    const uint64_t T = active ? T0 : (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE;  // idle lanes walk the loop of the wave's first team
    const uint64_t g = T / a.cpg;
    const uint32_t q = (uint32_t)(T % a.cpg);
    const VgChunk c = vg_chunk(a.n, a.group, a.chunk, g, q);
    TeamLanesGroups t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = {nullptr, 0};
    t.coeff_h = {nullptr, 0};
    t.e = {nullptr, 0};
    t.lines_h = a.lines_h;
    t.lines_g = a.lines_g;
    t.partials = nullptr;
    t.n = a.n;
    t.n_groups = a.n_groups;
    t.first = c.first;
    t.grp = g;
    t.count = c.count;
    uint32_t mask = 0;
    for (uint32_t p = 0; p < c.count; p++) mask |= vg_included_at(a, c.first + p) ? 1u << p : 0u;
    const bool own = q == 0;  // the group's pair (-g1, S_g)
    if (own && (a.gflag[g] & VG_FLAG_SUM)) mask |= 1u << c.count;
    t.mask = mask;
    const Fp2 f = team_miller_groups(t, (uint32_t)c.first, c.count + (own ? 1u : 0u));
    if (active) {
        Fp* o = a.partials + (T * 6 + j) * 2;
        st_fp(o, f.c0);
        st_fp(o + 1, f.c1);
    }
}
// finish: six lanes per group
__global__ __launch_bounds__(64) void k_vg_finish(VgArgs a) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t G0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && G0 < a.n_groups;
    const uint64_t g = active ? G0 : 0;
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
    t.n = a.n;
    t.n_groups = a.n_groups;
    t.first = 0;
    t.grp = g;
    t.count = 0;
    t.mask = 0;
    const bool one = team_groups_finish(t, g * a.cpg, a.cpg);
    if (active && j == 0) a.result[g] = (one && (a.gflag[g] & VG_FLAG_OK)) ? 1 : 0;
}

void launch_verify_groups(uint64_t n, uint32_t group, uint32_t chunk, const Workspace& ws, const uint64_t* pk_xy, const uint64_t* sig_xy, const int32_t* status, const uint64_t* scalars,
                          Fp* p_scaled, Fp* s_scaled, Fp* sum_xy, int32_t* gflag, Fp* lines_h, Fp* lines_g, Fp* partials, int32_t* result, hipStream_t st) {
    VgArgs a;
    a.n = n;
    a.n_groups = vg_groups(n, group);
    a.group = group;
    a.chunk = chunk;
    a.cpg = vg_chunks_per_group(n, group, chunk);
    a.pk_xy = pk_xy;
    a.sig_xy = sig_xy;
    a.status = status;
    a.scalars = scalars;
    a.p_scaled = p_scaled;
    a.s_scaled = s_scaled;
    a.sum_xy = sum_xy;
    a.gflag = gflag;
    a.lines_h = lines_h;
    a.lines_g = lines_g;
    a.partials = partials;
    a.result = result;
    const uint64_t teams = a.n_groups * a.cpg;
    hipLaunchKernelGGL(k_vg_scale, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vg_sum, dim3((unsigned)((a.n_groups + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vg_lines, dim3((unsigned)((n + a.n_groups + 63) / 64)), dim3(64), 0, st, a, ws);
    hipLaunchKernelGGL(k_vg_fold, dim3((unsigned)((teams + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vg_finish, dim3((unsigned)((a.n_groups + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a);
}

// ---- blsw_verify_groups_shared_batch (vshared.hpp): the same groups over a message table. The kernels above run as they are (scale, sum, finish);
// the ones below stand beside k_vg_lines and k_vg_fold and address pairs by compact run slot instead of by instance.
struct VsArgs {
    uint64_t n_msgs;
    const uint32_t* msg_index;  // [n]
    int32_t* status;            // [n][2]: the scan puts VS_BAD_INDEX in front of k_decode's / the registry sum's [i][0]
    uint32_t* slot_leader;      // [n] by slot g * group + k: the instance that leads run k of group g
    uint32_t* slot_len;         // [n] by slot: the run's instances
    uint32_t* runs;             // [n_groups]
    uint32_t* runs_out;         // [n_groups], nullable: the caller's d_group_runs
    Fp* rsum;                   // [3][n] by slot: the line multipliers (Z^3, X Z, Y) of R = sum of the run's P_i
    int32_t* rflag;             // [n] by slot: R is not the identity
};
// scan: one wave per group, tiles of 64 instances, ballot / popcount prefix with a carry between tiles. A group belongs to one wave: no atomics.
__global__ __launch_bounds__(64) void k_vs_scan(VgArgs a, VsArgs s) {
    const uint64_t g = blockIdx.x;
    if (g >= a.n_groups) return;
    const uint64_t first = g * a.group;
    const uint32_t size = vs_group_size(a.n, a.group, g), lane = threadIdx.x;
    VsCarry c = {0, 0};
#pragma unroll 1
    for (uint32_t base = 0; base < size; base += VS_TILE) {
        const uint32_t m = size - base < VS_TILE ? size - base : VS_TILE;
        const bool last = base + m == size, mine = lane < m;
        const uint64_t i = first + base + lane;
        const uint64_t ballot = __ballot(mine && vs_is_leader(s.msg_index, i, a.group));
        if (mine) {
            if (vs_bad_index(s.msg_index[i], s.n_msgs)) s.status[2 * i] = VS_BAD_INDEX;
            const VsLaneOut o = vs_tile_lane(c, ballot, base, m, last, lane);
            if (o.put_leader) s.slot_leader[first + o.slot] = (uint32_t)i;
            if (o.put_len) s.slot_len[first + o.slot] = o.len;
            if (o.put_close) s.slot_len[first + o.close_slot] = o.close_len;
        }
        c = vs_tile_carry(c, ballot, base);
    }
    if (lane == 0) {
        s.runs[g] = c.slots;
        if (s.runs_out) s.runs_out[g] = c.slots;
    }
}
// merge: one lane per slot, a serial sum of the run's scaled keys (a G1 addition is small against the 68-row line chain the run saves)
__global__ __launch_bounds__(64) void k_vs_merge(VgArgs a, VsArgs s) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    if (t % a.group >= s.runs[t / a.group]) return;
    const uint64_t n = a.n, lead = s.slot_leader[t];
    const Jac1v r = vs_merge(s.slot_len[t], [&](uint32_t i) {
        const Fp* p = a.p_scaled + lead + i;
        return Jac1v{ld_fp(p), ld_fp(p + n), ld_fp(p + 2 * n)};
    });
    Fp m0, m1, m2;
    vg_line_multipliers(r, m0, m1, m2);
    Fp* o = s.rsum + t;
    st_fp(o, m0);
    st_fp(o + n, m1);
    st_fp(o + 2 * n, m2);
    s.rflag[t] = fp_is_zero(r.z) ? 0 : 1;
}
// lines: k_vg_lines' body per slot: lanes [0, n) H(row of the run) (ws.h, homogeneous, stride n_msgs) against R; lanes [n, n + n_groups) S_g against
// -g1. A run that is not the identity holds an included instance, so its index is below n_msgs.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_vs_lines(VgArgs a, VsArgs s, Workspace ws) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n + a.n_groups) return;
    const uint64_t n = a.n;
    if (t < n) {
        if (t % a.group >= s.runs[t / a.group] || !s.rflag[t]) return;
        const uint64_t row = s.msg_index[s.slot_leader[t]];
        if (row >= s.n_msgs) return;
        const Proj<OpsFp2> h = ld_proj2(ws.h + row, s.n_msgs);
        const Fp2 zi = fp2_inv_inl(h.z);
        const Fp* p = s.rsum + t;
        vline_chain(fp2_mul_inl(h.x, zi), fp2_mul_inl(h.y, zi), ld_fp(p), ld_fp(p + n), ld_fp(p + 2 * n), CoeffStrided{a.lines_h + t, n});
    } else {
        const uint64_t g = t - n, G = a.n_groups;
        if (!(a.gflag[g] & VG_FLAG_SUM)) return;
        const Fp* p = a.sum_xy + g;
        vline_chain(ld_fp2(p, G), ld_fp2(p + 2 * G, G), K_G1_GEN_X(), K_G1_GEN_NEG_Y(), CoeffStrided{a.lines_g + g, G});
    }
}
// fold: k_vg_fold over slots. A team whose chunk is empty walks its squarings of one like an idle team of the plain fold (vs_chunk_walks has the
// measurement that decided it); idle lanes do what the wave's first team does.
__global__ __launch_bounds__(64) void k_vs_fold(VgArgs a, VsArgs s) {
    __shared__ Fp2 lds[BLSW_TEAMS_PER_WAVE * TS_NSLOTS];
    const uint64_t teams = a.n_groups * a.cpg;
    const uint32_t team = threadIdx.x / 6, j = threadIdx.x % 6;
    const uint64_t T0 = (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE + team;
    const bool active = team < BLSW_TEAMS_PER_WAVE && T0 < teams;
    const uint64_t T = active ? T0 : (uint64_t)blockIdx.x * BLSW_TEAMS_PER_WAVE;  // idle lanes walk the loop of the wave's first team
    const uint64_t g = T / a.cpg;
    const uint32_t q = (uint32_t)(T % a.cpg);
    const VgChunk c = vs_chunk(a.group, a.chunk, g, q, s.runs[g]);
    TeamLanesGroups t;
    t.slots = lds + (active ? team : 0) * TS_NSLOTS;
    t.j = j;
    t.active = active;
    t.coeff_sig = {nullptr, 0};
    t.coeff_h = {nullptr, 0};
    t.e = {nullptr, 0};
    t.lines_h = a.lines_h;
    t.lines_g = a.lines_g;
    t.partials = nullptr;
    t.n = a.n;
    t.n_groups = a.n_groups;
    t.first = c.first;
    t.grp = g;
    t.count = c.count;
    uint32_t mask = 0;
    for (uint32_t p = 0; p < c.count; p++) mask |= s.rflag[c.first + p] ? 1u << p : 0u;
    const bool own = q == 0;  // the group's pair (-g1, S_g)
    if (own && (a.gflag[g] & VG_FLAG_SUM)) mask |= 1u << c.count;
    t.mask = mask;
    const Fp2 f = vs_chunk_walks(c, q) ? team_miller_groups(t, (uint32_t)c.first, c.count + (own ? 1u : 0u)) : t.one();
    if (active) {
        Fp* o = a.partials + (T * 6 + j) * 2;
        st_fp(o, f.c0);
        st_fp(o + 1, f.c1);
    }
}

void launch_verify_groups_shared(uint64_t n, uint32_t group, uint32_t chunk, const Workspace& ws, uint64_t n_msgs, const uint32_t* msg_index, const uint64_t* pk_xy,
                                 const uint64_t* sig_xy, int32_t* status, const uint64_t* scalars, Fp* p_scaled, Fp* s_scaled, Fp* sum_xy, int32_t* gflag, Fp* lines_h, Fp* lines_g,
                                 Fp* partials, uint32_t* slot_leader, uint32_t* slot_len, uint32_t* runs, Fp* rsum, int32_t* rflag, uint32_t* runs_out, int32_t* result,
                                 hipStream_t st) {
    VgArgs a;
    a.n = n;
    a.n_groups = vg_groups(n, group);
    a.group = group;
    a.chunk = chunk;
    a.cpg = vg_chunks_per_group(n, group, chunk);
    a.pk_xy = pk_xy;
    a.sig_xy = sig_xy;
    a.status = status;
    a.scalars = scalars;
    a.p_scaled = p_scaled;
    a.s_scaled = s_scaled;
    a.sum_xy = sum_xy;
    a.gflag = gflag;
    a.lines_h = lines_h;
    a.lines_g = lines_g;
    a.partials = partials;
    a.result = result;
    const VsArgs s = {n_msgs, msg_index, status, slot_leader, slot_len, runs, runs_out, rsum, rflag};
    const uint64_t teams = a.n_groups * a.cpg;
    hipLaunchKernelGGL(k_vs_scan, dim3((unsigned)a.n_groups), dim3(64), 0, st, a, s);  // before the scale: a bad index excludes its instance
    hipLaunchKernelGGL(k_vg_scale, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vg_sum, dim3((unsigned)((a.n_groups + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_vs_merge, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a, s);
    hipLaunchKernelGGL(k_vs_lines, dim3((unsigned)((n + a.n_groups + 63) / 64)), dim3(64), 0, st, a, s, ws);
    hipLaunchKernelGGL(k_vs_fold, dim3((unsigned)((teams + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a, s);
    hipLaunchKernelGGL(k_vg_finish, dim3((unsigned)((a.n_groups + BLSW_TEAMS_PER_WAVE - 1) / BLSW_TEAMS_PER_WAVE)), dim3(64), 0, st, a);
}

}  // namespace blsw
