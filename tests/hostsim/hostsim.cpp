// TEST HARNESS ONLY (never linked into libblsw.so): compiles the device headers of
// bls-verify-gadget_amd/csrc for the HOST with g++ and runs the witness chains for ONE instance on one
// "lane", so that kernel logic can be checked against the CPU oracle without a GPU (pytest -m "not gpu").
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../bls-verify-gadget_amd/csrc/chains.hpp"
#include "../../bls-verify-gadget_amd/csrc/decode.hpp"
#include "../../bls-verify-gadget_amd/csrc/layout.h"
#include "../../bls-verify-gadget_amd/csrc/team.hpp"
#include "../../bls-verify-gadget_amd/csrc/vsign.hpp"
#include "../../bls-verify-gadget_amd/csrc/miller_par.hpp"
#include "../../bls-verify-gadget_amd/csrc/cofactor_par.hpp"
#include "../../bls-verify-gadget_amd/csrc/cofactor_vf.hpp"
#include "../../bls-verify-gadget_amd/csrc/prepare_vf.hpp"
#include "../../bls-verify-gadget_amd/csrc/vpairing.hpp"
#include "../../bls-verify-gadget_amd/csrc/r1cs_encode.hpp"
#include "../devfield/ops.hpp"
#include "../devteam/ops.hpp"
#include "../devcurve/ops.hpp"
#include "../devsha/ops.hpp"
#include "../devpair/ops.hpp"
#include <array>

using namespace blsw;

static Fp load_fp(const uint64_t* p) {
    Fp r;
    memcpy(r.l, p, 48);
    return r;
}


// the six-lanes-per-instance program of team.hpp, lanes run one after the other per phase
struct TeamHost {
    typedef std::array<Fp2, 6> Reg;
    Fp2 slots[TS_NSLOTS];
    Emitter e;
    CoeffLinear coeff_sig, coeff_h;
    Reg zero() const {
        Reg r;
        r.fill(fp2_zero());
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
        e.pos += T.n_witness;
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
    void set_consts(const Fp& pkx, const Fp& pky) {
        for (uint32_t j = 0; j < 6; j++) team_set_consts_lane(j, slots, pkx, pky);
    }
    void load_coeffs(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_coeff_lane(j, slots, coeff_sig, coeff_h, k);
    }
    Reg first_f() const {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = team_first_f(j, slots);
        return r;
    }
    // native pairing (vpairing.hpp: team_miller_values)
    Reg one() const {
        Reg r = zero();
        r[0] = fp2_one();
        return r;
    }
    void load_lines(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_lines_lane(j, slots, coeff_sig, coeff_h, k);
    }
    // ParametersVar allocated as witnesses (team_miller_pv)
    Fp pkx, pky;
    void load_pair_sig(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lane(j, slots, coeff_sig, k, K_G1_GEN_X(), K_G1_GEN_NEG_Y());
    }
    void load_pair_h(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lane(j, slots, coeff_h, k, pkx, pky);
    }
    Reg first_f_var() {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = team_first_f_var(j, slots, e);
        e.pos += 2;
        return r;
    }
    // N+1-pair product: per-pair inputs
    const std::vector<std::vector<Fp>>* pair_coeff = nullptr;
    const std::vector<G1ChainOut>* pair_pk = nullptr;
    void load_coeff_sig(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_coeff_sig_lane(j, slots, coeff_sig, k);
    }
    void load_pair(uint32_t jp, uint32_t k) {
        CoeffLinear c{const_cast<Fp*>((*pair_coeff)[jp].data())};
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lane(j, slots, c, k, (*pair_pk)[jp].ax, (*pair_pk)[jp].ay);
    }
    Reg inverse_w(const Reg& a) {
        for (uint32_t j = 0; j < 6; j++) team_st(slots, TS_IN0 + j, a[j]);
        team_inverse_lane0(slots);
        Reg inv;
        for (uint32_t j = 0; j < 6; j++) {
            inv[j] = team_ld(slots, TS_IN1 + j);
            Emitter w = e;
            w.pos += 2 * j;
            w.put(inv[j].c0);
            w.put(inv[j].c1);
        }
        e.pos += 12;
        exec(TEAM_OP_INVCHK, a, inv);
        return inv;
    }
    bool is_one_w(const Reg& a, const Emitter& e_one) {
        bool b[6];
        for (uint32_t j = 0; j < 6; j++) b[j] = team_is_one_coeff(j, a[j], e_one);
        bool res = false;
        for (uint32_t j = 0; j < 6; j++) res = team_is_one_tree(j, b, e_one);
        return res;
    }
    // what the operation table of tests/devteam/ops.hpp adds to the interface: operand blocks in, the six coefficients of a result out
    Fp* out = nullptr;  // [12]
    void set_coeffs(const Fp* c) { coeff_sig = coeff_h = CoeffLinear{const_cast<Fp*>(c)}; }
    void load_pair_lines(uint32_t k) {
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lines_lane(j, slots, coeff_h, k);
    }
    Reg ld(const Fp* p) const {
        Reg r;
        for (uint32_t j = 0; j < 6; j++) r[j] = {p[2 * j], p[2 * j + 1]};
        return r;
    }
    void st(const Reg& r) {
        for (uint32_t j = 0; j < 6; j++) devteam::st2(out + 2 * j, r[j]);
    }
    void st_flag(bool v) { devteam::st_verdict(out, v); }
    // what the table of pairing programs (tests/devpair/ops.hpp) adds: the constant of the pair (-g1, sig) in front of team_miller_multi
    void set_gen_y() { team_st(slots, TS_XYC, {K_G1_GEN_NEG_Y(), fp_zero()}); }
};
// the team of the two group entries of tests/devpair/ops.hpp (TeamLanesGroups on the device): pairs [first, first + count) are the item's
// instance line sets, pair first + count the group's own; a cleared mask bit is a skipped pair; load_partial reads the item's partial products
struct TeamHostGroupsTable : TeamHost {
    const Fp* sets = nullptr;      // [9][408]
    const Fp* partials = nullptr;  // [3][12]
    uint64_t first = 0;
    uint32_t count = 0, mask = 0;
    bool load_pair(uint64_t p, uint32_t k) {
        const uint32_t rel = (uint32_t)(p - first);
        if (!((mask >> rel) & 1u)) return false;
        const CoeffLinear c{const_cast<Fp*>(sets) + rel * BLSW_VLINE_ROWS};
        for (uint32_t j = 0; j < 6; j++) team_load_pair_lines_lane(j, slots, c, k);
        return true;
    }
    Reg load_partial(uint64_t idx) const { return ld(partials + 12 * idx); }
};
static int g_use_team = 0;
static int g_cofactor_par = 0;  // 1: clear_cofactor2 through cofactor_par.hpp (chunks in the order 2, 0, 1, then the join); 2: cofactor_vf.hpp
static uint32_t g_miller_chunk = 2;  // pairs per chunk of the pair-parallel Miller product (mode 2)
// G2 allocation with the scalar multiplication of the subgroup check on the team program (lanes 0..2 own x, y, z)
static void g2_alloc_segment(uint32_t* base, const blsw_layout_t& L, const Fp2& sx, const Fp2& sy) {
    if (!g_use_team) {
        chain_g2_alloc({base, L.off_sig_alloc}, sx, sy);
        return;
    }
    constexpr uint32_t RM1[8] = BLSW_RM1_WORDS;
    bool inf = fp2_is_zero(sx) && fp2_is_zero(sy);
    TeamHost t;
    t.e = {base, L.off_sig_alloc};
    TeamHost::Reg ge = t.zero();
    ge[0] = inf ? fp2_zero() : sx;
    ge[1] = inf ? fp2_one() : sy;
    ge[2] = inf ? fp2_zero() : fp2_one();
    for (int j = 0; j < 3; j++) {
        t.e.put(ge[j].c0);
        t.e.put(ge[j].c1);
    }
    (void)team_g2_mul_bits(t, ge, RM1, BLSW_RM1_NBITS);
    chain_g2_alloc_tail(t.e, {ge[0], ge[1], ge[2]});
}

static bool pairing_segment(uint32_t* base, const blsw_layout_t& L, const Fp& ax, const Fp& ay, Fp* cs, Fp* ch) {
    if (L.params_mode) {  // six-lane program only (k_pairing_team_pv)
        TeamHost t;
        t.coeff_sig = CoeffLinear{cs};
        t.coeff_h = CoeffLinear{ch};
        t.e = {base, L.off_miller};
        t.pkx = ax;
        t.pky = ay;
        TeamHost::Reg f = team_miller_pv(t);
        if (t.e.pos != L.off_final_exp) return false;
        bool r = team_final_exp_is_one(t, f, Emitter{base, L.off_is_one});
        if (t.e.pos != L.off_is_one) return false;
        return r;
    }
    if (!g_use_team) {
        Fp12 fm = chain_miller({base, L.off_miller}, ax, ay, CoeffLinear{cs}, CoeffLinear{ch});
        return chain_final_exp_is_one({base, L.off_final_exp}, {base, L.off_is_one}, fm);
    }
    TeamHost t;
    t.coeff_sig = CoeffLinear{cs};
    t.coeff_h = CoeffLinear{ch};
    t.e = {base, L.off_miller};
    t.set_consts(ax, ay);
    TeamHost::Reg f = team_miller(t);
    if (t.e.pos != L.off_final_exp) return false;
    bool r = team_final_exp_is_one(t, f, Emitter{base, L.off_is_one});
    if (t.e.pos != L.off_is_one) return false;
    return r;
}

static int g_prepare_vf = 0;  // 1: prepare_g2 through prepare_vf.hpp (value chain, then the steps in reverse order)
static void run_prepare(Emitter e, const Proj<OpsFp2>& q, const CoeffLinear& out) {
    if (!g_prepare_vf) {
        chain_prepare_g2(e, q, out);
        return;
    }
    std::vector<Fp> scr(BLSW_PREPV_ELEMS);
    prepv_chain(e, q, CoeffLinear{scr.data()});
    for (int k = BLSW_PREPV_STEPS - 1; k >= 0; k--) prepv_step_w(e, (uint32_t)k, CoeffLinear{scr.data()}, out);
}
struct ParkHost {
    Jac2* p;
    void st(int slot, const Jac2& v) const { p[slot] = v; }
    Jac2 ld(int slot) const { return p[slot]; }
};
static Proj<OpsFp2> run_cofactor(Emitter e_add, Emitter e, const Proj<OpsFp2>& q0, const Proj<OpsFp2>& q1) {
    if (!g_cofactor_par) return chain_cofactor(e_add, e, q0, q1);
    Fp rows[BLSW_COFACTOR_ROWS];
    if (g_cofactor_par == 2) {  // cofactor_vf.hpp: values first, the parallel phases in reverse order of their lanes
        constexpr CofvPlan vp = cofv_plan();
        std::vector<Fp> scr(BLSW_COFV_ELEMS);
        const CoeffLinear S{scr.data()}, R{rows};
        constexpr CofvSeg sg = cofv_seg();
        // the forward doubling chain first (the device's main stream), then each chunk's pipeline (other streams), the chunks in an arbitrary order
        for (int s = 0; s < BLSW_COFV_NSEG; s++)
            cofv_chain_seg(s, e_add, e, [&](Proj<OpsFp2>& a, Proj<OpsFp2>& b) { a = q0; b = q1; }, S, R);
        const int chunk_order[3] = {2, 0, 1};
        for (int k = 0; k < 3; k++)
            for (int s = 0; s < BLSW_COFV_NSEG; s++) {
                if (sg.chunk[s] != chunk_order[k]) continue;
                cofv_bwd(s, S);
                const int hi = sg.bnd[s + 1] < BLSW_H_EFF_NBITS ? sg.bnd[s + 1] : BLSW_H_EFF_NBITS - 1;
                for (int D = hi; D > sg.bnd[s]; D--) cofv_affine((uint32_t)D, S);
                if (s == 0) cofv_affine(0, S);
                cofv_acc_seg(s, S, R);
            }
        for (int c = 0; c < 3; c++) cofv_acc_az(c, S);
        for (int D = BLSW_H_EFF_NBITS - 1; D >= 0; D--) cofv_dbl_w(e, (uint32_t)D, S);  // beside the addition chains on the device
        for (int c = 2; c >= 0; c--)
            for (int j = (int)vp.n_adds[c] - 1; j >= 0; j--) cofv_add_w(e, c, (uint32_t)j, S);
        return cofv_join(e, S, R);
    }
    const int order[3] = {2, 0, 1};  // the chunks do not depend on each other
    for (int k = 0; k < 3; k++) chain_cofactor_chunk(e_add, e, q0, q1, order[k], CoeffLinear{rows});
    return chain_cofactor_join(e, CoeffLinear{rows});
}
extern "C" {
void hostsim_use_team(int on) { g_use_team = on; }
void hostsim_cofactor_par(int on) { g_cofactor_par = on; }
void hostsim_prepare_vf(int on) { g_prepare_vf = on; }
void hostsim_miller_chunk(uint32_t b) { g_miller_chunk = b ? b : 1; }
int hostsim_layout(uint32_t msg_len, blsw_layout_t* L) {
    make_layout(msg_len, L);
    return 0;
}
// out: n_witness * 6 u64. returns gadget result (0/1); seg_ends (optional, 16 u32): cursor after each chain
int hostsim_witness_params(const uint64_t* pk_xy, const uint8_t* msg, uint32_t msg_len, const uint64_t* sig_xy, uint32_t params_mode, uint64_t* out);
int hostsim_witness(const uint64_t* pk_xy, const uint8_t* msg, uint32_t msg_len, const uint64_t* sig_xy, uint64_t* out, uint32_t* seg_ends) {
    (void)seg_ends;
    return hostsim_witness_params(pk_xy, msg, msg_len, sig_xy, 0, out);
}
int hostsim_layout_params(uint32_t msg_len, uint32_t params_mode, blsw_layout_t* L) {
    make_layout(msg_len, L, 0, 1, params_mode == 1);
    return 0;
}
// params_mode 1: ParametersVar::new_variable(Witness) — the statements of k_g1's params lanes and k_pairing_team_pv
int hostsim_witness_params(const uint64_t* pk_xy, const uint8_t* msg, uint32_t msg_len, const uint64_t* sig_xy, uint32_t params_mode, uint64_t* out) {
    blsw_layout_t L;
    make_layout(msg_len, &L, 0, 1, params_mode == 1);
    uint32_t* base = reinterpret_cast<uint32_t*>(out);
    if (L.params_mode) {
        Emitter none = {nullptr, 0};
        Proj<OpsFp> g = chain_g1_alloc_only({base, L.off_params_alloc}, K_G1_GEN_X(), fp_neg(K_G1_GEN_NEG_Y()));
        g.y = fp_neg(g.y);
        G1ChainOut gn = chain_g1_post(none, {base, L.off_prep_g1}, g);
        if (memcmp(gn.ax.l, K_G1_GEN_X().l, 48) || memcmp(gn.ay.l, K_G1_GEN_NEG_Y().l, 48)) return -2;
    }
    // msg bits (UInt8::new_witness_vec)
    Emitter em = {base, L.off_msg};
    for (uint32_t i = 0; i < msg_len; i++)
        for (int j = 0; j < 8; j++) em.put_bool((msg[i] >> j) & 1);
    // G1 / G2 allocation
    Fp pkx = load_fp(pk_xy), pky = load_fp(pk_xy + 6);
    G1ChainOut g1 = chain_g1_alloc({base, L.off_pk_alloc}, {base, L.off_pk_not_zero}, {base, L.off_prep_pk}, pkx, pky);
    Fp2 sx = {load_fp(sig_xy), load_fp(sig_xy + 6)}, sy = {load_fp(sig_xy + 12), load_fp(sig_xy + 18)};
    g2_alloc_segment(base, L, sx, sy);
    // expand_message: bitstream then expansion
    std::vector<uint32_t> bits((L.sha_bits + 31) / 32 + 1, 0);
    BitSink s;
    s.init(bits.data(), 1);
    uint32_t uw[64];
    expand_message_w(s, msg, msg_len, false, uw);
    if (s.nbits != L.sha_bits) return -1;
    Emitter ex = {base, L.off_expand};
    for (uint32_t i = 0; i < L.sha_bits; i++) ex.put_bool((bits[i >> 5] >> (i & 31)) & 1);
    Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)};
    Fp2 u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
    Proj<OpsFp2> q0 = chain_map_to_curve({base, L.off_map0}, u0);
    Proj<OpsFp2> q1 = chain_map_to_curve({base, L.off_map1}, u1);
    Proj<OpsFp2> h = run_cofactor({base, L.off_add}, {base, L.off_cofactor}, q0, q1);
    std::vector<Fp> ch(68 * 4), cs(68 * 4);
    run_prepare({base, L.off_prep_h}, h, CoeffLinear{ch.data()});
    bool sinf = fp2_is_zero(sx) && fp2_is_zero(sy);
    Proj<OpsFp2> sp = {sinf ? fp2_zero() : sx, sinf ? fp2_one() : sy, sinf ? fp2_zero() : fp2_one()};
    run_prepare({base, L.off_prep_sig}, sp, CoeffLinear{cs.data()});
    bool res = pairing_segment(base, L, g1.ax, g1.ay, cs.data(), ch.data());
    return res ? 1 : 0;
}
// PublicKeyVar / SignatureVar allocated as public inputs (constraints.rs:214-249 with AllocationMode::Input): the statements of k_g1's / k_prepare's
// Input paths. out_instance: [n_instance_vars][6] = instance_assignment (element 0 = one)
int hostsim_witness_io(const uint64_t* pk_xy, const uint8_t* msg, uint32_t msg_len, const uint64_t* sig_xy, uint32_t pk_mode, uint32_t sig_mode, uint64_t* out,
                       uint64_t* out_instance) {
    blsw_layout_t L;
    make_layout(msg_len, &L, 0, 1, false, pk_mode == 1, sig_mode == 1);
    uint32_t* base = reinterpret_cast<uint32_t*>(out);
    Fp* inst = reinterpret_cast<Fp*>(out_instance);
    inst[0] = fp_one();
    Emitter em = {base, L.off_msg};
    for (uint32_t i = 0; i < msg_len; i++)
        for (int j = 0; j < 8; j++) em.put_bool((msg[i] >> j) & 1);
    Fp pkx = load_fp(pk_xy), pky = load_fp(pk_xy + 6);
    Proj<OpsFp> pk;
    if (pk_mode) {
        const bool inf = fp_is_zero(pkx) && fp_is_zero(pky);
        pk = {inf ? fp_zero() : pkx, inf ? fp_one() : pky, inf ? fp_zero() : fp_one()};
        inst[1] = pk.x;
        inst[2] = pk.y;
        inst[3] = pk.z;
    } else {
        pk = chain_g1_alloc_only({base, L.off_pk_alloc}, pkx, pky);
    }
    G1ChainOut g1 = chain_g1_post({base, L.off_pk_not_zero}, {base, L.off_prep_pk}, pk);
    Fp2 sx = {load_fp(sig_xy), load_fp(sig_xy + 6)}, sy = {load_fp(sig_xy + 12), load_fp(sig_xy + 18)};
    bool sinf = fp2_is_zero(sx) && fp2_is_zero(sy);
    Proj<OpsFp2> sp = {sinf ? fp2_zero() : sx, sinf ? fp2_one() : sy, sinf ? fp2_zero() : fp2_one()};
    if (sig_mode) {
        const uint32_t k0 = 1 + (pk_mode ? 3 : 0);
        const Fp v[6] = {sp.x.c0, sp.x.c1, sp.y.c0, sp.y.c1, sp.z.c0, sp.z.c1};
        for (int k = 0; k < 6; k++) inst[k0 + k] = v[k];
    } else {
        g2_alloc_segment(base, L, sx, sy);
    }
    std::vector<uint32_t> bits((L.sha_bits + 31) / 32 + 1, 0);
    BitSink s;
    s.init(bits.data(), 1);
    uint32_t uw[64];
    expand_message_w(s, msg, msg_len, false, uw);
    if (s.nbits != L.sha_bits) return -1;
    Emitter ex = {base, L.off_expand};
    for (uint32_t i = 0; i < L.sha_bits; i++) ex.put_bool((bits[i >> 5] >> (i & 31)) & 1);
    Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)};
    Fp2 u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
    Proj<OpsFp2> q0 = chain_map_to_curve({base, L.off_map0}, u0);
    Proj<OpsFp2> q1 = chain_map_to_curve({base, L.off_map1}, u1);
    Proj<OpsFp2> h = run_cofactor({base, L.off_add}, {base, L.off_cofactor}, q0, q1);
    std::vector<Fp> ch(68 * 4), cs(68 * 4);
    run_prepare({base, L.off_prep_h}, h, CoeffLinear{ch.data()});
    run_prepare({base, L.off_prep_sig}, sp, CoeffLinear{cs.data()});
    bool res = pairing_segment(base, L, g1.ax, g1.ay, cs.data(), ch.data());
    return res ? 1 : 0;
}
int hostsim_layout_io(uint32_t msg_len, uint32_t pk_mode, uint32_t sig_mode, blsw_layout_t* L) {
    make_layout(msg_len, L, 0, 1, false, pk_mode == 1, sig_mode == 1);
    return 0;
}
// N+1-pair product circuit for one instance (blsw_verify_multi_batch): pks_xy [K][12], msgs [K][msg_len]
struct HostPairs {
    const std::vector<std::vector<Fp>>* coeff;
    const std::vector<G1ChainOut>* keys;
    void pk(uint32_t j, Fp& x, Fp& y) const {
        x = (*keys)[j].ax;
        y = (*keys)[j].ay;
    }
    CoeffLinear coeff_h(uint32_t j) const { return CoeffLinear{const_cast<Fp*>((*coeff)[j].data())}; }
};
int hostsim_witness_multi(const uint64_t* pks_xy, const uint8_t* msgs, uint32_t msg_len, uint32_t K, const uint64_t* sig_xy, uint64_t* out, blsw_layout_t* Lout) {
    blsw_layout_t L;
    make_layout(msg_len, &L, 0, K);
    if (Lout) *Lout = L;
    if (!out) return 0;
    uint32_t* base = reinterpret_cast<uint32_t*>(out);
    std::vector<G1ChainOut> pk(K);
    std::vector<std::vector<Fp>> ch(K, std::vector<Fp>(68 * 4));
    for (uint32_t j = 0; j < K; j++) {
        const uint8_t* msg = msgs + (size_t)j * msg_len;
        Emitter em = {base, L.off_msg + j * L.stride_msg};
        for (uint32_t i = 0; i < msg_len; i++)
            for (int b = 0; b < 8; b++) em.put_bool((msg[i] >> b) & 1);
        pk[j] = chain_g1_alloc({base, L.off_pk_alloc + j * L.stride_pk_alloc}, {base, L.off_pk_not_zero + j * L.stride_pk_not_zero},
                               {base, L.off_prep_pk + j * L.stride_prep_pk}, load_fp(pks_xy + 12 * j), load_fp(pks_xy + 12 * j + 6));
        std::vector<uint32_t> bits((L.sha_bits + 31) / 32 + 1, 0);
        BitSink s;
        s.init(bits.data(), 1);
        uint32_t uw[64];
        expand_message_w(s, msg, msg_len, false, uw);
        if (s.nbits != L.sha_bits) return -1;
        const uint32_t ho = j * L.stride_hash;
        Emitter ex = {base, L.off_expand + ho};
        for (uint32_t i = 0; i < L.sha_bits; i++) ex.put_bool((bits[i >> 5] >> (i & 31)) & 1);
        Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)};
        Fp2 u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
        Proj<OpsFp2> q0 = chain_map_to_curve({base, L.off_map0 + ho}, u0);
        Proj<OpsFp2> q1 = chain_map_to_curve({base, L.off_map1 + ho}, u1);
        Proj<OpsFp2> h = run_cofactor({base, L.off_add + ho}, {base, L.off_cofactor + ho}, q0, q1);
        run_prepare({base, L.off_prep_h + j * L.stride_prep_h}, h, CoeffLinear{ch[j].data()});
    }
    Fp2 sx = {load_fp(sig_xy), load_fp(sig_xy + 6)}, sy = {load_fp(sig_xy + 12), load_fp(sig_xy + 18)};
    g2_alloc_segment(base, L, sx, sy);
    std::vector<Fp> cs(68 * 4);
    bool sinf = fp2_is_zero(sx) && fp2_is_zero(sy);
    Proj<OpsFp2> sp = {sinf ? fp2_zero() : sx, sinf ? fp2_one() : sy, sinf ? fp2_zero() : fp2_one()};
    run_prepare({base, L.off_prep_sig}, sp, CoeffLinear{cs.data()});
    if (g_use_team == 2) {  // miller_par.hpp: the four phases of the pair-parallel Miller product, tasks run one after the other
        HostPairs hp = {&ch, &pk};
        const uint32_t B = g_miller_chunk, C = miller_chunks(K, B), S = BLSW_MILLER_STEPS;
        std::vector<Fp> cprod(12 * S * C), q(12 * S * C), tt(12 * S), f1(12 * S);
        Fp12Rows Cp = {cprod.data(), (uint64_t)S * C}, Q = {q.data(), (uint64_t)S * C}, T = {tt.data(), S}, F1 = {f1.data(), S};
        for (uint32_t k = 0; k < S; k++)
            for (uint32_t c = 0; c < C; c++) Cp.st((uint64_t)k * C + c, miller_m1(hp, K, B, k, c));
        for (uint32_t k = 0; k < S; k++) miller_m1b(Cp, Q, T, (uint64_t)k * C, k, C);
        Fp12 fm = miller_m2(Emitter{base, L.off_miller}, K, CoeffLinear{cs.data()}, T, F1, 0);
        for (uint32_t k = 0; k < S; k++)
            for (uint32_t c = 0; c < C; c++) miller_m3(Emitter{base, L.off_miller}, hp, K, B, k, c, F1.ld(k), Q, (uint64_t)k * C + c);
        return chain_final_exp_is_one({base, L.off_final_exp}, {base, L.off_is_one}, fm) ? 1 : 0;
    }
    if (!g_use_team) {
        HostPairs hp = {&ch, &pk};
        Fp12 fm = chain_miller_multi({base, L.off_miller}, K, hp, CoeffLinear{cs.data()});
        return chain_final_exp_is_one({base, L.off_final_exp}, {base, L.off_is_one}, fm) ? 1 : 0;
    }
    TeamHost t;
    t.coeff_sig = CoeffLinear{cs.data()};
    t.coeff_h = CoeffLinear{nullptr};
    t.pair_coeff = &ch;
    t.pair_pk = &pk;
    t.e = {base, L.off_miller};
    team_st(t.slots, TS_XYC, {K_G1_GEN_NEG_Y(), fp_zero()});
    TeamHost::Reg f = team_miller_multi(t, K);
    if (t.e.pos != L.off_final_exp) return -2;
    bool r = team_final_exp_is_one(t, f, Emitter{base, L.off_is_one});
    if (t.e.pos != L.off_is_one) return -3;
    return r ? 1 : 0;
}
struct HostKeys {
    const std::vector<Proj<OpsFp>>* v;
    Proj<OpsFp> ld(uint32_t k) const { return (*v)[k]; }
};
// aggregate_verify circuit for one instance: pks_xy [K][12], bitmap [K]
int hostsim_witness_aggregate(const uint64_t* pks_xy, const uint8_t* bitmap, uint32_t K, const uint8_t* msg, uint32_t msg_len, const uint64_t* sig_xy,
                              uint64_t* out, uint32_t* count_out, blsw_layout_t* Lout) {
    blsw_layout_t L;
    make_layout(msg_len, &L, K);
    if (Lout) *Lout = L;
    if (!out) return 0;
    uint32_t* base = reinterpret_cast<uint32_t*>(out);
    std::vector<Proj<OpsFp>> keys;
    for (uint32_t k = 0; k < K; k++)
        keys.push_back(chain_g1_alloc_only({base, L.off_keys + k * SEG_PK_ALLOC}, load_fp(pks_xy + 12 * k), load_fp(pks_xy + 12 * k + 6)));
    Emitter eb = {base, L.off_bitmap};
    for (uint32_t k = 0; k < K; k++) eb.put_bool(bitmap[k] != 0);
    Emitter em = {base, L.off_msg};
    for (uint32_t i = 0; i < msg_len; i++)
        for (int j = 0; j < 8; j++) em.put_bool((msg[i] >> j) & 1);
    Fp2 sx = {load_fp(sig_xy), load_fp(sig_xy + 6)}, sy = {load_fp(sig_xy + 12), load_fp(sig_xy + 18)};
    g2_alloc_segment(base, L, sx, sy);
    HostKeys hk = {&keys};
    Proj<OpsFp> agg = chain_mapped_aggregate({base, L.off_count}, {base, L.off_agg}, hk, bitmap, K, count_out);
    G1ChainOut g1 = chain_g1_post({base, L.off_pk_not_zero}, {base, L.off_prep_pk}, agg);
    std::vector<uint32_t> bits((L.sha_bits + 31) / 32 + 1, 0);
    BitSink s;
    s.init(bits.data(), 1);
    uint32_t uw[64];
    expand_message_w(s, msg, msg_len, false, uw);
    Emitter ex = {base, L.off_expand};
    for (uint32_t i = 0; i < L.sha_bits; i++) ex.put_bool((bits[i >> 5] >> (i & 31)) & 1);
    Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)};
    Fp2 u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
    Proj<OpsFp2> q0 = chain_map_to_curve({base, L.off_map0}, u0);
    Proj<OpsFp2> q1 = chain_map_to_curve({base, L.off_map1}, u1);
    Proj<OpsFp2> hh = run_cofactor({base, L.off_add}, {base, L.off_cofactor}, q0, q1);
    std::vector<Fp> ch(68 * 4), cs(68 * 4);
    chain_prepare_g2({base, L.off_prep_h}, hh, CoeffLinear{ch.data()});
    bool sinf = fp2_is_zero(sx) && fp2_is_zero(sy);
    Proj<OpsFp2> sp = {sinf ? fp2_zero() : sx, sinf ? fp2_one() : sy, sinf ? fp2_zero() : fp2_one()};
    run_prepare({base, L.off_prep_sig}, sp, CoeffLinear{cs.data()});
    Fp12 fm = chain_miller({base, L.off_miller}, g1.ax, g1.ay, CoeffLinear{cs.data()}, CoeffLinear{ch.data()});
    bool res = chain_final_exp_is_one({base, L.off_final_exp}, {base, L.off_is_one}, fm);
    return res ? 1 : 0;
}
int hostsim_g1_decode(const uint8_t* in, uint64_t* out_xy) {
    Fp x, y;
    int st = g1_decode(in, x, y);
    memcpy(out_xy, x.l, 48);
    memcpy(out_xy + 6, y.l, 48);
    return st;
}
int hostsim_g2_decode(const uint8_t* in, uint64_t* out_xy) {
    Fp2 x, y;
    int st = g2_decode(in, x, y);
    memcpy(out_xy, x.c0.l, 48);
    memcpy(out_xy + 6, x.c1.l, 48);
    memcpy(out_xy + 12, y.c0.l, 48);
    memcpy(out_xy + 18, y.c1.l, 48);
    return st;
}
// signer logic (vsign.hpp, what k_sign runs per lane): sk (32 LE bytes), H(msg) affine -> sig96, pk48; returns the SIGN_* status
int hostsim_sign(const uint8_t* sk32, const uint64_t* h_xy, uint8_t* sig96, uint8_t* pk48) {
    uint32_t k[8];
    int st = sk_from_le32(sk32, k);
    Fp2 x = fp2_zero(), y = fp2_zero();
    Fp px = fp_zero(), py = fp_zero();
    bool sinf = true, pinf = true;
    if (st == SIGN_OK) {
        Fp2 hx = {load_fp(h_xy), load_fp(h_xy + 6)}, hy = {load_fp(h_xy + 12), load_fp(h_xy + 18)};
        Jac2 park[16];
        Jac2 acc = v_g2_mul_gls(ParkHost{park}, Jac2{hx, hy, fp2_one()}, k);
        if (!fp2_is_zero(acc.z)) {
            Fp2 zi = fp2_inv(acc.z), zi2 = fp2_sqr(zi);
            x = fp2_mul(acc.x, zi2);
            y = fp2_mul(acc.y, fp2_mul(zi2, zi));
            sinf = false;
        }
        Jac1v a1 = v1_mul_g1_fixed(k);
        if (!fp_is_zero(a1.z)) {
            Fp zi = fp_inv(a1.z), zi2 = fp_sqr(zi);
            px = fp_mul(a1.x, zi2);
            py = fp_mul(a1.y, fp_mul(zi2, zi));
            pinf = false;
        }
    }
    g2_encode(x, y, sinf, sig96);
    g1_encode(px, py, pinf, pk48);
    return st;
}
// R1CS evaluator (test side): checks <A_i, z> * <B_i, z> = <C_i, z> for every constraint with z = [1] ++ witness, matrices in
// the CSR form blsw_matrices_fill writes. Returns the index of the first unsatisfied constraint, or -1.
// z = [instance (n_inst elements, instance[0] = 1) | witness]: ark-relations' column order. instance == nullptr: z = [1 | witness]
int64_t hostsim_r1cs_check_io(uint64_t n_cons, const uint64_t* const* row_ptr, const uint32_t* const* col, const uint64_t* const* val, const uint64_t* witness,
                              uint64_t n_witness, const uint64_t* instance, uint64_t n_inst) {
    if (!instance) n_inst = 1;
    auto dot = [&](int m, uint64_t i) {
        Fp acc = fp_zero();
        for (uint64_t k = row_ptr[m][i]; k < row_ptr[m][i + 1]; k++) {
            const uint32_t c = col[m][k];
            if (c >= n_inst + n_witness) return fp_from_u32(0xdead);  // out of range: forces a mismatch
            Fp z = c == 0 ? fp_one() : (c < n_inst ? load_fp(instance + (uint64_t)c * 6) : load_fp(witness + (uint64_t)(c - n_inst) * 6));
            acc = fp_add(acc, fp_mul(load_fp(val[m] + k * 6), z));
        }
        return acc;
    };
    for (uint64_t i = 0; i < n_cons; i++)
        if (!fp_eq(fp_mul(dot(0, i), dot(1, i)), dot(2, i))) return (int64_t)i;
    return -1;
}
int64_t hostsim_r1cs_check(uint64_t n_cons, const uint64_t* const* row_ptr, const uint32_t* const* col, const uint64_t* const* val, const uint64_t* witness,
                           uint64_t n_witness) {
    return hostsim_r1cs_check_io(n_cons, row_ptr, col, val, witness, n_witness, nullptr, 1);
}
// value-only hash_to_g2 (vcurve.hpp: what blsw_hash_to_g2_batch / blsw_sign_batch run per lane): expand_message values,
// hash_to_field, SSWU + isogeny x 2, Q0 + Q1, psi-based cofactor clearing; affine result (all zero = identity)
void hostsim_hash_to_g2_values(const uint8_t* msg, uint32_t msg_len, uint64_t* out_xy) {
    uint32_t uw[64];
    expand_message_values(msg, msg_len, uw);
    Fp2 u0 = {hash_to_field_elem(uw), hash_to_field_elem(uw + 16)}, u1 = {hash_to_field_elem(uw + 32), hash_to_field_elem(uw + 48)};
    Proj<OpsFp2> q0 = v_map_to_curve(u0), q1 = v_map_to_curve(u1);
    Jac2 r = {q0.x, q0.y, q0.z};
    if (fp2_is_zero(q0.z)) r = {fp2_one(), fp2_one(), fp2_zero()};
    if (!fp2_is_zero(q1.z)) r = v_add_mixed(r, q1.x, q1.y);
    Jac2 park[3];
    Jac2 acc = v_clear_cofactor(ParkHost{park}, r);
    memset(out_xy, 0, 24 * 8);
    if (fp2_is_zero(acc.z)) return;
    Fp2 zi = fp2_inv(acc.z), zi2 = fp2_sqr(zi);
    Fp2 x = fp2_mul(acc.x, zi2), y = fp2_mul(acc.y, fp2_mul(zi2, zi));
    memcpy(out_xy, x.c0.l, 48);
    memcpy(out_xy + 6, x.c1.l, 48);
    memcpy(out_xy + 12, y.c0.l, 48);
    memcpy(out_xy + 18, y.c1.l, 48);
}
// blsw_verify_batch's per-instance logic (k_decode, the value-only hash, k_vlines, k_verify_team): verdict from compressed bytes; st[2] = decode statuses
int hostsim_verify_values(const uint8_t* pk48, const uint8_t* sig96, const uint8_t* msg, uint32_t msg_len, int32_t* st) {
    Fp px, py;
    Fp2 sx, sy;
    st[0] = g1_decode(pk48, px, py);
    st[1] = g2_decode(sig96, sx, sy);
    uint64_t h_xy[24];
    hostsim_hash_to_g2_values(msg, msg_len, h_xy);
    const Fp2 hx = {load_fp(h_xy), load_fp(h_xy + 6)}, hy = {load_fp(h_xy + 12), load_fp(h_xy + 18)};
    std::vector<Fp> ls(BLSW_VLINE_ROWS), lh(BLSW_VLINE_ROWS);
    vline_chain(sx, sy, K_G1_GEN_X(), K_G1_GEN_NEG_Y(), CoeffLinear{ls.data()});
    vline_chain(hx, hy, px, py, CoeffLinear{lh.data()});
    TeamHost t;
    t.coeff_sig = CoeffLinear{ls.data()};
    t.coeff_h = CoeffLinear{lh.data()};
    t.e = {nullptr, 0};
    TeamHost::Reg f = team_miller_values(t);
    const bool one = team_final_exp_is_one(t, f, Emitter{nullptr, 0});
    return (one && st[0] == 0 && st[1] == 0) ? 1 : 0;
}
// clear_cofactor2 of a given pair (Q0, Q1) of affine points (z = 1; all zero = the identity (0, 0, 0)): the serial chain and the
// chunked one write their "add" + "cofactor" segments (36 + 8979 elements each) and results; returns 1 if everything is equal
int hostsim_cofactor_compare(const uint64_t* q0_xy, const uint64_t* q1_xy, uint64_t* out_serial, uint64_t* out_chunked) {
    auto load = [](const uint64_t* p) {
        Proj<OpsFp2> q = {{load_fp(p), load_fp(p + 6)}, {load_fp(p + 12), load_fp(p + 18)}, fp2_one()};
        if (fp2_is_zero(q.x) && fp2_is_zero(q.y)) q.z = fp2_zero();
        return q;
    };
    Proj<OpsFp2> q0 = load(q0_xy), q1 = load(q1_xy);
    Proj<OpsFp2> a = chain_cofactor({reinterpret_cast<uint32_t*>(out_serial), 0}, {reinterpret_cast<uint32_t*>(out_serial), SEG_ADD}, q0, q1);
    Fp rows[BLSW_COFACTOR_ROWS];
    Emitter e_add = {reinterpret_cast<uint32_t*>(out_chunked), 0}, e = {reinterpret_cast<uint32_t*>(out_chunked), SEG_ADD};
    Proj<OpsFp2> b;
    if (g_cofactor_par == 2) {
        b = run_cofactor(e_add, e, q0, q1);  // cofactor_vf.hpp
    } else {
        const int order[3] = {1, 2, 0};
        for (int k = 0; k < 3; k++) chain_cofactor_chunk(e_add, e, q0, q1, order[k], CoeffLinear{rows});
        b = chain_cofactor_join(e, CoeffLinear{rows});
    }
    bool same = fp_eq(a.x.c0, b.x.c0) && fp_eq(a.x.c1, b.x.c1) && fp_eq(a.y.c0, b.y.c0) && fp_eq(a.y.c1, b.y.c1) && fp_eq(a.z.c0, b.z.c0) && fp_eq(a.z.c1, b.z.c1);
    return same && memcmp(out_serial, out_chunked, (size_t)(SEG_ADD + SEG_COFACTOR) * 48) == 0;
}
// field micro-checks
void hostsim_fp_mul(const uint64_t* a, const uint64_t* b, uint64_t* r) {
    Fp z = fp_mul(load_fp(a), load_fp(b));
    memcpy(r, z.l, 48);
}
void hostsim_fp_mul32(const uint64_t* a, const uint64_t* b, uint64_t* r) {
    Fp z = fp_mul32(load_fp(a), load_fp(b));
    memcpy(r, z.l, 48);
}
void hostsim_fp_inv(const uint64_t* a, uint64_t* r) {
    Fp z = fp_inv(load_fp(a));
    memcpy(r, z.l, 48);
}
void hostsim_fp_inv_fermat(const uint64_t* a, uint64_t* r) {
    Fp z = fp_inv_fermat(load_fp(a));
    memcpy(r, z.l, 48);
}
// one operation of the field / tower table (tests/devfield/ops.hpp: the table tests/devfield/devfield.hip runs on the device) on one item:
// a, b [12][6] u64 operand blocks, out [12][6] result elements (the operation's own count written, the rest untouched), wit: room for the
// operation's witnesses, [n][6]. Returns the witness cursor after the operation, -1 for an unknown operation.
int hostsim_field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit) {
    Fp fa[12], fb[12], fo[DEVFIELD_OUT_MAX];
    for (int i = 0; i < 12; i++) {
        fa[i] = load_fp(a + 6 * i);
        fb[i] = load_fp(b + 6 * i);
    }
    Emitter e = {reinterpret_cast<uint32_t*>(wit), 0};
    switch (op) {
#define HOSTSIM_X_RUN(name, n_out, n_wit)                            \
    case devfield::OP_##name:                                        \
        devfield::FieldOp<devfield::OP_##name>::run(fa, fb, fo, e);  \
        break;
        DEVFIELD_OPS(HOSTSIM_X_RUN)
#undef HOSTSIM_X_RUN
        default:
            return -1;
    }
    memcpy(out, fo, (size_t)devfield::op_n_out(op) * 48);
    return (int)e.pos;
}
// the same over n items, with the arrays of devfield_run (one "lane" per item): out [n][12][6], wit [n][wcap][6], npos [n] the cursors
int hostsim_field_op_batch(int op, uint64_t n, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    if (devfield::op_n_out(op) < 0) return -1;
    if ((int64_t)wcap < devfield::op_n_wit(op)) return -2;
    for (uint64_t i = 0; i < n; i++) npos[i] = (uint32_t)hostsim_field_op(op, a + i * 72, b + i * 72, out + i * 72, wit + i * (uint64_t)wcap * 6);
    return 0;
}
const char* hostsim_field_op_name(int op) {
    static const char* const T[devfield::OP_COUNT] = {
#define HOSTSIM_X_NAME(name, n_out, n_wit) #name,
        DEVFIELD_OPS(HOSTSIM_X_NAME)
#undef HOSTSIM_X_NAME
    };
    return (op >= 0 && op < devfield::OP_COUNT) ? T[op] : "";
}
int hostsim_field_op_count() { return devfield::OP_COUNT; }
int hostsim_field_op_n_out(int op) { return devfield::op_n_out(op); }
int hostsim_field_op_n_wit(int op) { return devfield::op_n_wit(op); }
// one entry of the team operation table (tests/devteam/ops.hpp: the table tests/devteam/devteam.hip runs on the device) over n items. form 0: the
// single-lane statement; 1 / 2: the team form through exec / exec_hot on the looped team above (one text on the host). a, b, c [n][12][6] u64 operand
// blocks; out [n][12][6] the six coefficients of the result; wit [n][wcap][6]; npos [n] the cursor after the entry (the team's own cursor, which does
// not pass the entry's tail). Returns 0, -1 for an unknown entry or form, -2 when wcap is below the entry's witness count.
int hostsim_team_op(int form, int op, uint64_t n, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    const int64_t n_wit = devteam::op_n_wit(op, devteam::NwTables());
    if (n_wit < 0 || form < 0 || form > 2) return -1;
    if ((int64_t)wcap < n_wit) return -2;
    for (uint64_t i = 0; i < n; i++) {
        Fp fa[12], fb[12], fc[12], fo[12];
        for (int k = 0; k < 12; k++) {
            fa[k] = load_fp(a + i * 72 + 6 * k);
            fb[k] = load_fp(b + i * 72 + 6 * k);
            fc[k] = load_fp(c + i * 72 + 6 * k);
        }
        Emitter e = {reinterpret_cast<uint32_t*>(wit + i * (uint64_t)wcap * 6), 0};
        TeamHost t;
        memset(t.slots, 0, sizeof(t.slots));
        t.e = e;
        t.out = fo;
        t.pkx = t.pky = fp_zero();
        switch (op) {
#define HOSTSIM_X_TEAM(name, dual, g2, w, tail)                                              \
    case devteam::OP_##name:                                                                 \
        if (form == 0)                                                                       \
            devteam::TeamEntry<devteam::OP_##name>::single(fa, fb, fc, fo, e);               \
        else if (form == 1)                                                                  \
            devteam::TeamEntry<devteam::OP_##name>::team<false>(t, fa, fb, fc, 0);           \
        else                                                                                 \
            devteam::TeamEntry<devteam::OP_##name>::team<true>(t, fa, fb, fc, 0);            \
        break;
            DEVTEAM_OPS(HOSTSIM_X_TEAM)
#undef HOSTSIM_X_TEAM
        }
        memcpy(out + i * 72, fo, sizeof(fo));
        npos[i] = form == 0 ? e.pos : t.e.pos;
    }
    return 0;
}
const char* hostsim_team_op_name(int op) {
    static const char* const T[devteam::OP_COUNT] = {
#define HOSTSIM_X_TNAME(name, dual, g2, w, tail) #name,
        DEVTEAM_OPS(HOSTSIM_X_TNAME)
#undef HOSTSIM_X_TNAME
    };
    return (op >= 0 && op < devteam::OP_COUNT) ? T[op] : "";
}
int hostsim_team_op_count() { return devteam::OP_COUNT; }
int hostsim_team_op_n_wit(int op) { return (int)devteam::op_n_wit(op, devteam::NwTables()); }
int hostsim_team_op_tail(int op) { return (int)devteam::op_tail(op, devteam::NwTables()); }
int hostsim_team_op_dual(int op) { return devteam::op_dual(op); }
// one entry of the table of pairing programs (tests/devpair/ops.hpp: the table tests/devpair/devpair.hip runs on the device) over n items. form 0:
// the single-lane statement; 1: the program on the looped team above. in [n][n_in][6] u64 operand blocks (hostsim_pair_op_n_in(op, K)); out
// [n][n_out][6]; wit [n][wcap][6]; npos [n] the cursor after the entry (form 0: the entry's count, its chains take the cursor by value). Returns 0, -1
// for an unknown entry, form or K, -2 when wcap is below the entry's witness count.
int hostsim_pair_op(int form, int op, uint32_t K, uint64_t n, const uint64_t* in, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    const int forms = devpair::op_forms(op);
    if (forms < 0 || form < 0 || form > 1 || !((forms >> form) & 1) || !devpair::k_ok(op, K)) return -1;
    const int64_t n_wit = devpair::op_n_wit(op, K, devteam::NwTables()), n_in = devpair::op_n_in(op, K), n_out = devpair::op_n_out(op);
    if ((int64_t)wcap < n_wit) return -2;
    for (uint64_t i = 0; i < n; i++) {
        std::vector<Fp> fin(n_in), fo(n_out);
        for (int64_t k = 0; k < n_in; k++) fin[k] = load_fp(in + (i * n_in + k) * 6);
        Emitter e = {reinterpret_cast<uint32_t*>(wit + i * (uint64_t)wcap * 6), 0};
        if (n_wit == 0) e.base = nullptr;
        if (form == 0) {
            devpair::run_single(op, K, fin.data(), fo.data(), e);
            npos[i] = (uint32_t)n_wit;
        } else if (op == devpair::OP_miller_groups || op == devpair::OP_groups_finish) {
            TeamHostGroupsTable t;
            memset(t.slots, 0, sizeof(t.slots));
            t.e = {nullptr, 0};
            if (op == devpair::OP_miller_groups) {
                t.count = fin[0].l[0];
                t.mask = fin[2].l[0];
                t.first = 5 * i;  // any base: the program only forms differences with it
                t.sets = fin.data() + DEVPAIR_GROUPS_HDR;
                const TeamHost::Reg f = devpair::run_team<devpair::OP_miller_groups>(t, fp_zero(), fp_zero(), t.count + (fin[1].l[0] ? 1u : 0u));
                for (uint32_t j = 0; j < 6; j++) devteam::st2(fo.data() + 2 * j, f[j]);
            } else {
                t.partials = fin.data() + 1;
                devteam::st_verdict(fo.data(), devpair::run_team_finish(t, 0, fin[0].l[0]));
            }
            npos[i] = t.e.pos;
        } else {
            const devpair::PairsBlock pairs = {fin.data()};
            std::vector<G1ChainOut> pk(K);
            std::vector<std::vector<Fp>> ch(K);
            for (uint32_t j = 0; j < K && op != devpair::OP_miller_values; j++) {
                pairs.pk(j, pk[j].ax, pk[j].ay);
                ch[j].assign(pairs.coeff_h(j).p, pairs.coeff_h(j).p + DEVPAIR_COEFFS);
            }
            TeamHost t;
            memset(t.slots, 0, sizeof(t.slots));
            t.e = e;
            t.pkx = t.pky = fp_zero();
            t.coeff_sig = CoeffLinear{fin.data()};
            t.coeff_h = op == devpair::OP_miller_values ? CoeffLinear{fin.data() + BLSW_VLINE_ROWS} : (op == devpair::OP_miller_multi ? CoeffLinear{nullptr} : CoeffLinear{ch[0].data()});
            t.pair_coeff = &ch;
            t.pair_pk = &pk;
            TeamHost::Reg f;
            switch (op) {
                case devpair::OP_miller: f = devpair::run_team<devpair::OP_miller>(t, pk[0].ax, pk[0].ay, K); break;
                case devpair::OP_miller_pv: f = devpair::run_team<devpair::OP_miller_pv>(t, pk[0].ax, pk[0].ay, K); break;
                case devpair::OP_miller_multi: f = devpair::run_team<devpair::OP_miller_multi>(t, pk[0].ax, pk[0].ay, K); break;
                default: f = devpair::run_team<devpair::OP_miller_values>(t, fp_zero(), fp_zero(), K); break;
            }
            for (uint32_t j = 0; j < 6; j++) devteam::st2(fo.data() + 2 * j, f[j]);
            npos[i] = t.e.pos;
        }
        memcpy(out + i * n_out * 6, fo.data(), (size_t)n_out * sizeof(Fp));
    }
    return 0;
}
const char* hostsim_pair_op_name(int op) {
    static const char* const T[devpair::OP_COUNT] = {
#define HOSTSIM_X_PNAME(name, sdev, team, nin, nout, wit) #name,
        DEVPAIR_OPS(HOSTSIM_X_PNAME)
#undef HOSTSIM_X_PNAME
    };
    return (op >= 0 && op < devpair::OP_COUNT) ? T[op] : "";
}
int hostsim_pair_op_count() { return devpair::OP_COUNT; }
int hostsim_pair_op_forms(int op) { return devpair::op_forms(op); }
int64_t hostsim_pair_op_n_wit(int op, uint32_t K) { return devpair::k_ok(op, K) ? devpair::op_n_wit(op, K, devteam::NwTables()) : -1; }
int64_t hostsim_pair_op_n_in(int op, uint32_t K) { return devpair::k_ok(op, K) ? devpair::op_n_in(op, K) : -1; }
int64_t hostsim_pair_op_n_out(int op) { return devpair::op_n_out(op); }
// the two statements of the Miller segment's fixed part: as miller_step_info() places it, and from the op tables' counts
uint32_t hostsim_pair_spine_witnesses(int from_tables) { return from_tables ? devpair::spine_from_tables(devteam::NwTables()) : devpair::spine_witnesses(); }
// the four phases of miller_par.hpp (m1, m1b, the single-lane spine m2, m3) over n items of K pairs in chunks of B, the tasks one after the other, on
// the arrays of the device's launch (element-major Fp12Rows over ALL items): in [n][272 + 274 K][6] operand blocks of miller_multi; ffinal [12][n];
// f1, t [12][n 68]; q [12][n 68 C], item (i 68 + k) C + c (the caller's sentinel stays where nothing is stored); wit [n][wcap][6]: the Miller
// segment at cursor 0. Returns 0, -1 for K or B out of range, -2 when wcap is below the segment's length.
int hostsim_pair_par(uint32_t K, uint32_t B, uint64_t n, const uint64_t* in, uint64_t* ffinal, uint64_t* wit, uint32_t wcap, uint64_t* f1, uint64_t* t, uint64_t* q) {
    if (K < 1 || K > DEVPAIR_K_MAX || B < 1) return -1;
    const int64_t n_wit = devpair::op_n_wit(devpair::OP_miller_multi, K, devteam::NwTables()), n_in = devpair::op_n_in(devpair::OP_miller_multi, K);
    if ((int64_t)wcap < n_wit) return -2;
    const uint32_t C = miller_chunks(K, B), S = BLSW_MILLER_STEPS;
    const uint64_t steps = n * S, tasks = steps * C;
    std::vector<Fp> cprod(12 * tasks);
    const Fp12Rows Cp = {cprod.data(), tasks}, Q = {reinterpret_cast<Fp*>(q), tasks}, T = {reinterpret_cast<Fp*>(t), steps}, F1 = {reinterpret_cast<Fp*>(f1), steps};
    const Fp12Rows FF = {reinterpret_cast<Fp*>(ffinal), n};
    for (uint64_t i = 0; i < n; i++) {
        std::vector<Fp> fin(n_in);
        for (int64_t k = 0; k < n_in; k++) fin[k] = load_fp(in + (i * n_in + k) * 6);
        const devpair::PairsBlock hp = {fin.data()};
        const Emitter e = {reinterpret_cast<uint32_t*>(wit + i * (uint64_t)wcap * 6), 0};
        for (uint32_t k = 0; k < S; k++)
            for (uint32_t c = 0; c < C; c++) Cp.st((i * S + k) * C + c, miller_m1(hp, K, B, k, c));
        for (uint32_t k = 0; k < S; k++) miller_m1b(Cp, Q, T, (i * S + k) * C, i * S + k, C);
        FF.st(i, miller_m2(e, K, CoeffLinear{fin.data()}, T, F1, i * S));
        for (uint32_t k = 0; k < S; k++)
            for (uint32_t c = 0; c < C; c++) miller_m3(e, hp, K, B, k, c, F1.ld(i * S + k), Q, (i * S + k) * C + c);
    }
    return 0;
}
// the 272 line coefficients of an affine G2 point (not the identity) by chain_prepare_g2, value only: the operands of the witness entries
void hostsim_pair_prepare(const uint64_t* q_xy, uint64_t* coeff) {
    const Proj<OpsFp2> q = {{load_fp(q_xy), load_fp(q_xy + 6)}, {load_fp(q_xy + 12), load_fp(q_xy + 18)}, fp2_one()};
    chain_prepare_g2(Emitter{nullptr, 0}, q, CoeffLinear{reinterpret_cast<Fp*>(coeff)});
}
// one operation of the curve table (tests/devcurve/ops.hpp: the table tests/devcurve/devcurve.hip runs on the device) on one item, with the
// arrays of hostsim_field_op; the PARK of v_clear_cofactor and v_g2_mul_gls is an array. Returns the witness cursor after the operation, -1 for an
// unknown operation.
int hostsim_curve_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit) {
    Fp fa[12], fb[12], fo[DEVCURVE_OUT_MAX];
    for (int i = 0; i < 12; i++) {
        fa[i] = load_fp(a + 6 * i);
        fb[i] = load_fp(b + 6 * i);
    }
    Jac2 park[DEVCURVE_PARK_SLOTS];
    Emitter e = {reinterpret_cast<uint32_t*>(wit), 0};
    switch (op) {
#define HOSTSIM_X_CRUN(name, n_out, n_wit, quad)                                      \
    case devcurve::OP_##name:                                                        \
        devcurve::CurveOp<devcurve::OP_##name>::run(fa, fb, fo, e, ParkHost{park});  \
        break;
        DEVCURVE_OPS(HOSTSIM_X_CRUN)
#undef HOSTSIM_X_CRUN
        default:
            return -1;
    }
    memcpy(out, fo, (size_t)devcurve::op_n_out(op) * 48);
    return (int)e.pos;
}
// the same over n items, with the arrays of devcurve_run (one "lane" per item): out [n][12][6], wit [n][wcap][6], npos [n] the cursors
int hostsim_curve_op_batch(int op, uint64_t n, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t* wit, uint32_t wcap, uint32_t* npos) {
    if (devcurve::op_n_out(op) < 0) return -1;
    if ((int64_t)wcap < devcurve::op_n_wit(op)) return -2;
    for (uint64_t i = 0; i < n; i++) npos[i] = (uint32_t)hostsim_curve_op(op, a + i * 72, b + i * 72, out + i * 72, wit + i * (uint64_t)wcap * 6);
    return 0;
}
const char* hostsim_curve_op_name(int op) {
    static const char* const T[devcurve::OP_COUNT] = {
#define HOSTSIM_X_CNAME(name, n_out, n_wit, quad) #name,
        DEVCURVE_OPS(HOSTSIM_X_CNAME)
#undef HOSTSIM_X_CNAME
    };
    return (op >= 0 && op < devcurve::OP_COUNT) ? T[op] : "";
}
int hostsim_curve_op_count() { return devcurve::OP_COUNT; }
int hostsim_curve_op_n_out(int op) { return devcurve::op_n_out(op); }
int hostsim_curve_op_n_wit(int op) { return devcurve::op_n_wit(op); }
int hostsim_curve_op_quad(int op) { return devcurve::op_quad(op); }
// the device R1CS evaluator's encoder (r1cs_encode.hpp: what blsw_r1cs_device_bytes / blsw_r1cs_create run). codes[m]: nnz[m] entry codes;
// table: room for nnz[0] + nnz[1] + nnz[2] elements of 6 u64, *table_size written; blk: room for n_constraints + 1 block starts, *n_blk = the
// number of blocks (blk[n_blk] = n_constraints). Returns encode()'s code, the outputs written only on BLSW_OK.
int hostsim_r1cs_encode(uint64_t n_cons, uint64_t n_inst, uint64_t n_wit, const uint64_t* nnz, const uint64_t* const* row_ptr, const uint32_t* const* col,
                        const uint64_t* const* val, uint32_t* const* codes, uint64_t* table, uint64_t* table_size, uint64_t* blk, uint64_t* n_blk, uint64_t* bytes) {
    blsw_matrices_info_t info;
    blsw_matrices_t m;
    memset(&info, 0, sizeof(info));
    memset(&m, 0, sizeof(m));
    info.n_constraints = n_cons;
    info.n_instance_vars = n_inst;
    info.n_witness = n_wit;
    for (int k = 0; k < 3; k++) {
        info.nnz[k] = nnz[k];
        m.row_ptr[k] = const_cast<uint64_t*>(row_ptr[k]);
        m.col[k] = const_cast<uint32_t*>(col[k]);
        m.val[k] = const_cast<uint64_t*>(val[k]);
    }
    r1cs::Encoded e;
    const int rc = r1cs::encode(&info, &m, &e);
    if (rc) return rc;
    for (int k = 0; k < 3; k++)
        for (uint64_t j = 0; j < nnz[k]; j++) {
            if (e.ent[k][j].x != col[k][j]) return -1;  // an entry keeps its column
            codes[k][j] = e.ent[k][j].y;
        }
    if (e.table.size()) memcpy(table, e.table.data(), e.table.size() * sizeof(Fp));
    *table_size = e.table.size();
    memcpy(blk, e.blk.data(), e.blk.size() * 8);
    *n_blk = e.blk.size() - 1;
    *bytes = e.bytes;
    return rc;
}
// REDC(<row, z>) of one encoded matrix row by the kernel's own functions (r1cs_row.hpp: row_term per entry, then redc14): count entries
// (col, code), the table of hostsim_r1cs_encode, z = [n_z][6] stored integers (any value below 2^384: the kernel does not reduce its input)
void hostsim_r1cs_row(const uint32_t* col, const uint32_t* code, uint64_t count, const uint64_t* table, const uint64_t* z, uint64_t* out) {
    r1cs::Acc x;
    for (int j = 0; j < 14; j++) x.l[j] = 0;
    for (uint64_t k = 0; k < count; k++) r1cs::row_term(x, load_fp(z + (uint64_t)col[k] * 6), code[k], reinterpret_cast<const Fp*>(table));
    const Fp r = r1cs::redc14(x);
    memcpy(out, r.l, 48);
}
// sha.hpp's host BitSink alone, on the script tests/devstream/devstream.hip's k_devstream_sink runs on the device: entry i = (op, n), op 0 =
// push(data[i], n), op 1 = push32(data[i]); one flush at the end. words [cap] receives the stream; returns the word count (widx), or -1 when the
// stream does not fit; *nbits = the sink's bit count.
int64_t hostsim_sink_script(const uint32_t* script, uint32_t n_ops, const uint32_t* data, uint32_t* words, uint64_t cap, uint64_t* nbits) {
    uint64_t need = 0;
    for (uint32_t i = 0; i < n_ops; i++) need += script[2 * i] == 0 ? script[2 * i + 1] : 32;
    if ((need + 31) / 32 > cap) return -1;
    BitSink s;
    s.init(words, 1);
    for (uint32_t i = 0; i < n_ops; i++) {
        if (script[2 * i] == 0)
            s.push(data[i], script[2 * i + 1]);
        else
            s.push32(data[i]);
    }
    s.flush();
    *nbits = s.nbits;
    return (int64_t)s.widx;
}
// one entry of the SHA gadget table (tests/devsha/ops.hpp: the table tests/devsha/devsha.hip runs on the device) on one item: in
// [DEVSHA_IN_MAX] u32 operands, msg [msg_len], out [DEVSHA_OUT_MAX] u32 (the entry's own count written), words [cap] the entry's bit stream through
// sha.hpp's host BitSink (flushed), *nbits its bit count. Returns the word count, -1 for an unknown entry, -2 when the stream does not fit cap
// (the entry is run on a counting sink first).
int64_t hostsim_sha_op(int op, const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, uint32_t* words, uint64_t cap, uint64_t* nbits) {
    uint32_t scratch[DEVSHA_OUT_MAX];
    for (int pass = 0; pass < 2; pass++) {
        BitSink s;
        s.init(pass ? words : nullptr, 1);
        uint32_t* o = pass ? out : scratch;
        switch (op) {
#define HOSTSIM_X_SRUN(name, n_in, n_out, m, fl)                          \
    case devsha::OP_##name:                                               \
        devsha::ShaOp<devsha::OP_##name>::run(in, msg, msg_len, o, s);    \
        break;
            DEVSHA_OPS(HOSTSIM_X_SRUN)
#undef HOSTSIM_X_SRUN
            default:
                return -1;
        }
        if (!devsha::op_flushes(op)) s.flush();
        if (!pass && (s.nbits + 31) / 32 > cap) return -2;
        if (pass) {
            *nbits = s.nbits;
            return (int64_t)s.widx;
        }
    }
    return -1;
}
// the same over n items: in [n][DEVSHA_IN_MAX], msg [n][msg_len], out [n][DEVSHA_OUT_MAX], words [n][cap], nwords [n], nbits [n]
int hostsim_sha_op_batch(int op, uint64_t n, const uint32_t* in, const uint8_t* msg, uint32_t msg_len, uint32_t* out, uint32_t* words, uint64_t cap, uint32_t* nwords,
                         uint64_t* nbits) {
    if (devsha::op_n_out(op) < 0) return -1;
    for (uint64_t i = 0; i < n; i++) {
        const int64_t r = hostsim_sha_op(op, in + i * DEVSHA_IN_MAX, msg + i * (uint64_t)msg_len, msg_len, out + i * DEVSHA_OUT_MAX, words + i * cap, cap, nbits + i);
        if (r < 0) return (int)r;
        nwords[i] = (uint32_t)r;
    }
    return 0;
}
const char* hostsim_sha_op_name(int op) {
    static const char* const T[devsha::OP_COUNT] = {
#define HOSTSIM_X_SNAME(name, n_in, n_out, m, fl) #name,
        DEVSHA_OPS(HOSTSIM_X_SNAME)
#undef HOSTSIM_X_SNAME
    };
    return (op >= 0 && op < devsha::OP_COUNT) ? T[op] : "";
}
int hostsim_sha_op_count() { return devsha::OP_COUNT; }
int hostsim_sha_op_n_in(int op) { return devsha::op_n_in(op); }
int hostsim_sha_op_n_out(int op) { return devsha::op_n_out(op); }
int hostsim_sha_op_msg(int op) { return devsha::op_msg(op); }
// the "hash.expand" segment of one message alone, as hostsim_witness_params emits it: bits [cap] one byte per boolean witness in allocation
// order, uniform [256] the bytes of b1 .. b8. Returns the segment's length (the layout's sha_bits), -1 when it differs from the layout's or
// does not fit cap.
int64_t hostsim_hash_expand(const uint8_t* msg, uint32_t msg_len, uint8_t* bits, uint64_t cap, uint8_t* uniform) {
    blsw_layout_t L;
    make_layout(msg_len, &L);
    std::vector<uint32_t> w((L.sha_bits + 31) / 32 + 1, 0);
    BitSink s;
    s.init(w.data(), 1);
    uint32_t uw[64];
    expand_message_w(s, msg, msg_len, false, uw);
    if (s.nbits != L.sha_bits || s.nbits > cap) return -1;
    for (uint32_t i = 0; i < L.sha_bits; i++) bits[i] = (w[i >> 5] >> (i & 31)) & 1;
    for (int i = 0; i < 64; i++)
        for (int b = 0; b < 4; b++) uniform[4 * i + b] = (uint8_t)(uw[i] >> (8 * (3 - b)));
    return (int64_t)L.sha_bits;
}
}
