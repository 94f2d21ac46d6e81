// TEST HARNESS ONLY (never linked into libblsw.so): compiles vgroups.hpp, vpairing.hpp, team.hpp and decode.hpp of bls-verify-gadget_amd/csrc for
// the HOST with g++ and runs the stages of blsw_verify_groups_batch for ONE group, lanes and teams one after the other, so that the kernels' logic
// is checked against the CPU oracle without a GPU (pytest -m "not gpu").
#include <array>
#include <cstring>
#include <vector>
#include "../../bls-verify-gadget_amd/csrc/decode.hpp"
#include "../../bls-verify-gadget_amd/csrc/sha.hpp"
#include "../../bls-verify-gadget_amd/csrc/team.hpp"
#include "../../bls-verify-gadget_amd/csrc/vgroups.hpp"
#include "../../bls-verify-gadget_amd/csrc/vpairing.hpp"

using namespace blsw;

// value-only host team: the six lanes of a team run one after the other per phase
struct TeamHostValues {
    typedef std::array<Fp2, 6> Reg;
    Fp2 slots[TS_NSLOTS];
    Emitter e = {nullptr, 0};
    Reg one() const {
        Reg r;
        r.fill(fp2_zero());
        r[0] = fp2_one();
        return r;
    }
    Reg exec(const TeamOp& T, const Reg& a, const Reg& b) {
        for (uint32_t j = 0; j < 6; j++) {
            team_st(slots, TS_IN0 + j, a[j]);
            team_st(slots, TS_IN1 + j, b[j]);
        }
        for (uint32_t r = 0; r < T.rounds; r++)
            for (uint32_t j = 0; j < 6; j++) team_task(T.task[r][j], slots, e);
        Reg out;
        for (uint32_t j = 0; j < 6; j++) out[j] = team_gather(T.out[j], slots);
        return out;
    }
    Reg exec_hot(const TeamOp& T, const Reg& a, const Reg& b) { return exec(T, a, b); }
    Reg exp_by_x(const Reg& f) { return team_exp_by_x_body(*this, f); }
    Reg conj(const Reg& a) const {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = team_conj(j, a[j]);
        return r;
    }
    Reg frob(const Reg& a, int power) const {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = team_frob(j, a[j], power);
        return r;
    }
    Reg inverse_w(const Reg& a) {
        for (uint32_t j = 0; j < 6; j++) team_st(slots, TS_IN0 + j, a[j]);
        team_inverse_lane0(slots);
        Reg inv;
        for (uint32_t j = 0; j < 6; j++) inv[j] = team_ld(slots, TS_IN1 + j);
        return inv;
    }
    bool is_one_w(const Reg& a, const Emitter& e_one) {
        bool b[6];
        for (uint32_t j = 0; j < 6; j++) b[j] = team_is_one_coeff(j, a[j], e_one);
        return team_is_one_tree(0, b, e_one);
    }
    // the fold's pairs and the finish's partial products (TeamLanesGroups on the device)
    const std::vector<std::vector<Fp>>* lines = nullptr;  // pair p -> its BLSW_VLINE_ROWS coefficients; empty = a skipped pair
    const std::vector<Reg>* partials = nullptr;
    bool load_pair(uint32_t p, uint32_t k) {
        if ((*lines)[p].empty()) return false;
        const CoeffLinear c{const_cast<Fp*>((*lines)[p].data())};
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lines_lane(j, slots, c, k);
        return true;
    }
    Reg load_partial(uint64_t idx) const { return (*partials)[idx]; }
};

static void hash_to_g2_affine(const uint8_t* msg, uint32_t msg_len, Fp2& hx, Fp2& hy, bool& inf) {  // the lanes of launch_values_hash
    uint32_t uw[64];
    expand_message_values(msg, msg_len, uw);
    const Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)}, u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
    const Proj<OpsFp2> q0 = v_map_to_curve(u0), q1 = v_map_to_curve(u1);
    Jac2 r = {q0.x, q0.y, q0.z};
    if (fp2_is_zero(q0.z)) r = {fp2_one(), fp2_one(), fp2_zero()};
    if (!fp2_is_zero(q1.z)) r = v_add_mixed(r, q1.x, q1.y);
    struct Park {
        Jac2* p;
        void st(int slot, const Jac2& v) const { p[slot] = v; }
        Jac2 ld(int slot) const { return p[slot]; }
    };
    Jac2 park[3];
    inf = !vg_affine2(v_clear_cofactor(Park{park}, r), hx, hy);
}

// element-major rows as the device keeps them: element r of lane i at p[r * n + i]
struct RowsHost {
    Fp* p;
    uint64_t n;
    void st(uint32_t idx, const Fp& v) const { p[(uint64_t)idx * n] = v; }
    Fp ld(uint32_t idx) const { return p[(uint64_t)idx * n]; }
};
// a team over the device's arrays (TeamLanesGroups): pairs [first, first + count) from lines_h, pair first + count the group's own from lines_g
struct TeamHostGroups : TeamHostValues {
    Fp* lines_h;
    Fp* lines_g;
    const Fp* parts;
    uint64_t n, n_groups, first, grp;
    uint32_t count, mask;
    bool load_pair(uint64_t p, uint32_t k) {
        const uint32_t rel = (uint32_t)(p - first);
        if (!((mask >> rel) & 1u)) return false;
        const RowsHost c = rel < count ? RowsHost{lines_h + p, n} : RowsHost{lines_g + grp, n_groups};
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lines_lane(j, slots, c, k);
        return true;
    }
    Reg load_partial(uint64_t idx) const {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = {parts[(idx * 6 + j) * 2], parts[(idx * 6 + j) * 2 + 1]};
        return r;
    }
};
static Fp ldf(const uint64_t* p) {
    Fp r;
    memcpy(r.l, p, 48);
    return r;
}

extern "C" {
// one group of m triples: pk48s [m][48], sig96s [m][96], msgs [m][msg_len], scalars [m]; st_out [m][2] decode statuses; -> the group's verdict
int vgroups_group(const uint8_t* pk48s, const uint8_t* sig96s, const uint8_t* msgs, uint32_t msg_len, const uint64_t* scalars, uint32_t m, uint32_t chunk, int32_t* st_out) {
    if (m == 0 || chunk == 0 || chunk > 31) return -1;
    // decode + scale (k_decode, k_vg_scale)
    std::vector<Jac1v> P(m);
    std::vector<Jac2> S(m);
    std::vector<bool> in(m);
    bool ok = true;
    for (uint32_t i = 0; i < m; i++) {
        Fp px, py;
        Fp2 sx, sy;
        st_out[2 * i] = g1_decode(pk48s + 48 * i, px, py);
        st_out[2 * i + 1] = g2_decode(sig96s + 96 * i, sx, sy);
        in[i] = vg_included(st_out[2 * i], st_out[2 * i + 1], scalars[i]);
        ok = ok && in[i];
        const uint64_t r = in[i] ? scalars[i] : 0;
        P[i] = vg_scale_g1(px, py, r);
        S[i] = vg_scale_g2(sx, sy, r);
    }
    // sum (k_vg_sum)
    Fp2 gx, gy;
    const bool some = vg_affine2(vg_sum(m, [&](uint32_t i) { return S[i]; }), gx, gy);
    // lines (k_vg_lines): pair i < m = instance i, pair m = the group's own
    std::vector<std::vector<Fp>> lines(m + 1);
    for (uint32_t i = 0; i < m; i++) {
        if (!in[i]) continue;
        Fp2 hx, hy;
        bool inf;
        hash_to_g2_affine(msgs + (size_t)msg_len * i, msg_len, hx, hy, inf);
        Fp m0, m1, m2;
        vg_line_multipliers(P[i], m0, m1, m2);
        lines[i].resize(BLSW_VLINE_ROWS);
        vline_chain(hx, hy, m0, m1, m2, CoeffLinear{lines[i].data()});
    }
    if (some) {
        lines[m].resize(BLSW_VLINE_ROWS);
        vline_chain(gx, gy, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), CoeffLinear{lines[m].data()});
    }
    // fold (k_vg_fold): chunk q holds instances [first, first + count); the group's pair rides with chunk 0. The device keeps its pairs in two
    // arrays; here pair index m is the group's, so chunk 0 is folded as its instances followed by it
    const uint32_t cpg = vg_chunks_per_group(m, m, chunk);
    std::vector<TeamHostValues::Reg> partials(cpg);
    for (uint32_t q = 0; q < cpg; q++) {
        const VgChunk c = vg_chunk(m, m, chunk, 0, q);
        std::vector<std::vector<Fp>> mine(lines.begin() + c.first, lines.begin() + c.first + c.count);
        if (q == 0) mine.push_back(lines[m]);
        TeamHostValues t;
        t.lines = &mine;
        partials[q] = team_miller_groups(t, 0, (uint32_t)mine.size());
    }
    // finish (k_vg_finish)
    TeamHostValues t;
    t.partials = &partials;
    const bool one = team_groups_finish(t, 0, cpg);
    return (one && ok) ? 1 : 0;
}

// The stages of launch_verify_groups (k_vg_scale, k_vg_sum, k_vg_lines, k_vg_fold, k_vg_finish) over MANY groups, lanes and teams one after the
// other, on the device's arrays, which the caller fills with its sentinel: a stage stores exactly what its kernel stores. Inputs as the kernels
// read them: pk_xy [n][12], sig_xy [n][24] affine Montgomery limbs, h [6][n] elements (ws.h: homogeneous projective), status [n][2], scalars
// [n]. Outputs: p_scaled [3][n], s_scaled [6][n], sum_xy [4][G], gflag [G], lines_h [408][n], lines_g [408][G], partials [G cpg][12], result
// [G] (elements of 6 u64). Returns the number of groups, -1 for arguments out of range.
int64_t vgroups_stages(uint64_t n, uint32_t group, uint32_t chunk, const uint64_t* pk_xy, const uint64_t* sig_xy, const uint64_t* h, const int32_t* status,
                       const uint64_t* scalars, uint64_t* p_scaled_, uint64_t* s_scaled_, uint64_t* sum_xy_, int32_t* gflag, uint64_t* lines_h_, uint64_t* lines_g_,
                       uint64_t* partials_, int32_t* result) {
    if (n == 0 || group == 0 || chunk == 0 || chunk > 31) return -1;
    const uint64_t G = vg_groups(n, group);
    const uint32_t cpg = vg_chunks_per_group(n, group, chunk);
    Fp *p_scaled = reinterpret_cast<Fp*>(p_scaled_), *s_scaled = reinterpret_cast<Fp*>(s_scaled_), *sum_xy = reinterpret_cast<Fp*>(sum_xy_);
    Fp *lines_h = reinterpret_cast<Fp*>(lines_h_), *lines_g = reinterpret_cast<Fp*>(lines_g_), *partials = reinterpret_cast<Fp*>(partials_);
    auto included = [&](uint64_t i) { return vg_included(status[2 * i], status[2 * i + 1], scalars[i]); };
    auto ld_s = [&](uint64_t i) { return Jac2{{s_scaled[i], s_scaled[n + i]}, {s_scaled[2 * n + i], s_scaled[3 * n + i]}, {s_scaled[4 * n + i], s_scaled[5 * n + i]}}; };
    for (uint64_t i = 0; i < n; i++) {  // scale
        const uint64_t r = included(i) ? scalars[i] : 0;
        const Jac1v P = vg_scale_g1(ldf(pk_xy + i * 12), ldf(pk_xy + i * 12 + 6), r);
        p_scaled[i] = P.x;
        p_scaled[n + i] = P.y;
        p_scaled[2 * n + i] = P.z;
        const Jac2 S = vg_scale_g2({ldf(sig_xy + i * 24), ldf(sig_xy + i * 24 + 6)}, {ldf(sig_xy + i * 24 + 12), ldf(sig_xy + i * 24 + 18)}, r);
        const Fp v[6] = {S.x.c0, S.x.c1, S.y.c0, S.y.c1, S.z.c0, S.z.c1};
        for (int k = 0; k < 6; k++) s_scaled[k * n + i] = v[k];
    }
    for (uint64_t g = 0; g < G; g++) {  // sum
        const uint64_t first = g * group;
        const uint32_t m = (uint32_t)(n - first < group ? n - first : group);
        bool ok = true;
        for (uint32_t i = 0; i < m; i++) ok = ok && included(first + i);
        Fp2 x, y;
        const bool some = vg_affine2(vg_sum(m, [&](uint32_t i) { return ld_s(first + i); }), x, y);
        sum_xy[g] = x.c0;
        sum_xy[G + g] = x.c1;
        sum_xy[2 * G + g] = y.c0;
        sum_xy[3 * G + g] = y.c1;
        gflag[g] = (ok ? VG_FLAG_OK : 0) | (some ? VG_FLAG_SUM : 0);
    }
    const Fp* hh = reinterpret_cast<const Fp*>(h);
    for (uint64_t t = 0; t < n + G; t++) {  // lines: a skipped pair writes nothing
        if (t < n) {
            if (!included(t)) continue;
            const Fp2 hx = {hh[t], hh[n + t]}, hy = {hh[2 * n + t], hh[3 * n + t]}, hz = {hh[4 * n + t], hh[5 * n + t]};
            const Fp2 zi = fp2_inv_inl(hz);
            Fp m0, m1, m2;
            vg_line_multipliers({p_scaled[t], p_scaled[n + t], p_scaled[2 * n + t]}, m0, m1, m2);
            vline_chain(fp2_mul_inl(hx, zi), fp2_mul_inl(hy, zi), m0, m1, m2, RowsHost{lines_h + t, n});
        } else {
            const uint64_t g = t - n;
            if (!(gflag[g] & VG_FLAG_SUM)) continue;
            vline_chain(Fp2{sum_xy[g], sum_xy[G + g]}, Fp2{sum_xy[2 * G + g], sum_xy[3 * G + g]}, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), RowsHost{lines_g + g, G});
        }
    }
    for (uint64_t T = 0; T < G * cpg; T++) {  // fold
        const uint64_t g = T / cpg;
        const uint32_t q = (uint32_t)(T % cpg);
        const VgChunk c = vg_chunk(n, group, chunk, g, q);
        TeamHostGroups t;
        t.lines_h = lines_h;
        t.lines_g = lines_g;
        t.parts = nullptr;
        t.n = n;
        t.n_groups = G;
        t.first = c.first;
        t.grp = g;
        t.count = c.count;
        uint32_t mask = 0;
        for (uint32_t p = 0; p < c.count; p++) mask |= included(c.first + p) ? 1u << p : 0u;
        const bool own = q == 0;
        if (own && (gflag[g] & VG_FLAG_SUM)) mask |= 1u << c.count;
        t.mask = mask;
        const TeamHostValues::Reg f = team_miller_groups(t, (uint32_t)c.first, c.count + (own ? 1u : 0u));
        for (uint32_t j = 0; j < 6; j++) {
            partials[(T * 6 + j) * 2] = f[j].c0;
            partials[(T * 6 + j) * 2 + 1] = f[j].c1;
        }
    }
    for (uint64_t g = 0; g < G; g++) {  // finish
        TeamHostGroups t;
        t.parts = partials;
        const bool one = team_groups_finish(t, g * cpg, cpg);
        result[g] = (one && (gflag[g] & VG_FLAG_OK)) ? 1 : 0;
    }
    return (int64_t)G;
}
// The line stage of launch_verify_values (k_vlines) on the device's arrays: lines_sig, lines_h [408][n]; every instance is walked, whatever its status
void vgroups_value_lines(uint64_t n, const uint64_t* pk_xy, const uint64_t* sig_xy, const uint64_t* h, uint64_t* lines_sig_, uint64_t* lines_h_) {
    const Fp* hh = reinterpret_cast<const Fp*>(h);
    for (uint64_t i = 0; i < n; i++) {
        vline_chain(Fp2{ldf(sig_xy + i * 24), ldf(sig_xy + i * 24 + 6)}, Fp2{ldf(sig_xy + i * 24 + 12), ldf(sig_xy + i * 24 + 18)}, K_G1_GEN_X(), K_G1_GEN_NEG_Y(),
                    RowsHost{reinterpret_cast<Fp*>(lines_sig_) + i, n});
        const Fp2 hx = {hh[i], hh[n + i]}, hy = {hh[2 * n + i], hh[3 * n + i]}, hz = {hh[4 * n + i], hh[5 * n + i]};
        const Fp2 zi = fp2_inv_inl(hz);
        vline_chain(fp2_mul_inl(hx, zi), fp2_mul_inl(hy, zi), ldf(pk_xy + i * 12), ldf(pk_xy + i * 12 + 6), RowsHost{reinterpret_cast<Fp*>(lines_h_) + i, n});
    }
}
}
