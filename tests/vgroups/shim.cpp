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
}
