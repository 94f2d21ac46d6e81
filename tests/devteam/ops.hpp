// TEST HARNESS ONLY (never linked into libblsw.so): one table of the operations of the six-lane team executor (csrc/team.hpp, team_tables.hpp,
// team_multi.hpp, the team parts of vpairing.hpp), each written twice from the same operand blocks:
//   team    against the TEAM interface of team.hpp: tests/hostsim/hostsim.cpp runs it on its looped team (TeamHost), tests/devteam/devteam.hip on
//           the device's TeamLanes, one kernel per entry, shaped like the library's team kernels
//   single  the single-lane statement the team form claims to equal, values and witness stream (host only: tests/devfield covers it on the device)
// Operand blocks of an item: a, b = an Fp12 as twelve stored elements (a G2 point: x, y, z in the first six); c = up to twelve elements, line
// coefficients and a G1 point. The result of every entry is six Fp2, coefficient j owned by lane j of the team: an Fp12, a G2 point on lanes 0..2
// (zero on 3..5), or a verdict (the flag as the integer 0 / 1 in limb 0 of c0, the same on all six lanes).
// What the TEAM interface gains for this table (test side only): set_coeffs(c), load_pair_lines(k), ld(block) -> Reg, st(Reg), st_flag(bool).
#pragma once
#include "chains.hpp"
#include "team.hpp"
#include "vpairing.hpp"

namespace devteam {
using namespace blsw;

enum TableId { T_MUL, T_SQR, T_CYC, T_ELLC, T_ELLV, T_ELLGS, T_ELLGH, T_G2DBL, T_G2ADD, T_INVCHK, T_COUNT };
#define DEVTEAM_IS_ONE_WITNESSES 35u  // 2 x (3 x fp2_is_eq_w (5) + 2 ANDs) + the final AND: no table states it, the single-lane cursor is asserted against it

// X(name, dual, g2, witnesses, tail). dual: the library runs the op through exec and through exec_hot, so the entry has a kernel for each.
// g2: the LDS file of k_g2_alloc_team (TS_P + 12 slots per team). witnesses: the length of the stream as a function of the TABLES' counts
// (nw(T_x) = TEAM_OP_x.n_witness), never a second literal; the single-lane form's cursor is asserted against it. tail: how many of them are written
// through the second cursor (e_one), which the team's own cursor does not pass.
#define DEVTEAM_EXP_BY_X_W (64u * nw(T_CYC) + 5u * nw(T_MUL))
#define DEVTEAM_INVERSE_W (12u + nw(T_INVCHK))
#define DEVTEAM_OPS(X)                                                                                                           \
    X(MUL, 1, 0, nw(T_MUL), 0u)                                                                                                  \
    X(SQR, 1, 0, nw(T_SQR), 0u)                                                                                                  \
    X(CYC, 1, 0, nw(T_CYC), 0u)                                                                                                  \
    X(ELLC, 1, 0, nw(T_ELLC), 0u)                                                                                                \
    X(ELLV, 1, 0, nw(T_ELLV), 0u)                                                                                                \
    X(ELLGS, 1, 0, nw(T_ELLGS), 0u)                                                                                              \
    X(ELLGH, 1, 0, nw(T_ELLGH), 0u)                                                                                              \
    X(G2DBL, 1, 1, nw(T_G2DBL), 0u)                                                                                              \
    X(G2ADD, 1, 1, nw(T_G2ADD), 0u)                                                                                              \
    X(inverse_w, 0, 0, DEVTEAM_INVERSE_W, 0u)                                                                                    \
    X(is_one_w, 0, 0, DEVTEAM_IS_ONE_WITNESSES, DEVTEAM_IS_ONE_WITNESSES)                                                        \
    X(conj, 0, 0, 0u, 0u)                                                                                                        \
    X(frob_1, 0, 0, 0u, 0u)                                                                                                      \
    X(frob_2, 0, 0, 0u, 0u)                                                                                                      \
    X(frob_3, 0, 0, 0u, 0u)                                                                                                      \
    X(first_f, 0, 0, 0u, 0u)                                                                                                     \
    X(first_f_var, 0, 0, 2u, 0u)                                                                                                 \
    X(exp_by_x, 0, 0, DEVTEAM_EXP_BY_X_W, 0u)                                                                                    \
    X(final_exp_is_one, 0, 0, DEVTEAM_INVERSE_W + 12u * nw(T_MUL) + 2u * nw(T_CYC) + 5u * DEVTEAM_EXP_BY_X_W + DEVTEAM_IS_ONE_WITNESSES, \
      DEVTEAM_IS_ONE_WITNESSES)                                                                                                  \
    X(seq, 1, 0, 2u * nw(T_SQR) + nw(T_ELLC) + nw(T_ELLV) + 2u * nw(T_MUL) + nw(T_CYC), 0u)

enum OpId {
#define DEVTEAM_X_ENUM(name, dual, g2, wit, tail) OP_##name,
    DEVTEAM_OPS(DEVTEAM_X_ENUM)
#undef DEVTEAM_X_ENUM
        OP_COUNT
};
// the stream length / the tail of entry `op`; nw(T_x) supplies the tables' counts (read directly where the tables are host data, copied from the
// device's symbols where they are constant memory)
template <class NW>
inline int64_t op_n_wit(int op, const NW& nw) {
    switch (op) {
#define DEVTEAM_X_WIT(name, dual, g2, wit, tail) \
    case OP_##name:                              \
        return (int64_t)(wit);
        DEVTEAM_OPS(DEVTEAM_X_WIT)
#undef DEVTEAM_X_WIT
    }
    return -1;
}
template <class NW>
inline int64_t op_tail(int op, const NW& nw) {
    (void)nw;
    switch (op) {
#define DEVTEAM_X_TAIL(name, dual, g2, wit, tail) \
    case OP_##name:                               \
        return (int64_t)(tail);
        DEVTEAM_OPS(DEVTEAM_X_TAIL)
#undef DEVTEAM_X_TAIL
    }
    return -1;
}
inline int op_dual(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVTEAM_X_DUAL(name, dual, g2, wit, tail) dual,
        DEVTEAM_OPS(DEVTEAM_X_DUAL)
#undef DEVTEAM_X_DUAL
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}
BLSW_HD const TeamOp& table(int id) {
    switch (id) {
        case T_MUL: return TEAM_OP_MUL;
        case T_SQR: return TEAM_OP_SQR;
        case T_CYC: return TEAM_OP_CYC;
        case T_ELLC: return TEAM_OP_ELLC;
        case T_ELLV: return TEAM_OP_ELLV;
        case T_ELLGS: return TEAM_OP_ELLGS;
        case T_ELLGH: return TEAM_OP_ELLGH;
        case T_G2DBL: return TEAM_OP_G2DBL;
        case T_G2ADD: return TEAM_OP_G2ADD;
        default: return TEAM_OP_INVCHK;
    }
}
// the tables' counts where the tables can be read in place: host data (g++), constant memory (device code). NOT the host pass of a HIP unit.
struct NwTables {
    BLSW_HD uint32_t operator()(int id) const { return table(id).n_witness; }
};
// witnesses of the final exponentiation in front of the is_one tail: where the second cursor of final_exp_is_one starts
BLSW_HD uint32_t final_exp_witnesses() {
    const NwTables nw;
    return DEVTEAM_INVERSE_W + 12u * nw(T_MUL) + 2u * nw(T_CYC) + 5u * DEVTEAM_EXP_BY_X_W;
}

BLSW_HD Fp2 ld2(const Fp* p) { return {p[0], p[1]}; }
BLSW_HD Fp6 ld6(const Fp* p) { return {ld2(p), ld2(p + 2), ld2(p + 4)}; }
BLSW_HD Fp12 ld12(const Fp* p) { return {ld6(p), ld6(p + 6)}; }
BLSW_HD void st2(Fp* p, const Fp2& v) {
    p[0] = v.c0;
    p[1] = v.c1;
}
BLSW_HD void st12(Fp* p, const Fp12& v) {
    st2(p, v.c0.c0);
    st2(p + 2, v.c0.c1);
    st2(p + 4, v.c0.c2);
    st2(p + 6, v.c1.c0);
    st2(p + 8, v.c1.c1);
    st2(p + 10, v.c1.c2);
}
BLSW_HD void st_point(Fp* p, const Proj<OpsFp2>& v) {  // lanes 0..2 hold x, y, z; the outputs of lanes 3..5 are the empty combination
    st2(p, v.x);
    st2(p + 2, v.y);
    st2(p + 4, v.z);
    for (int i = 6; i < 12; i++) p[i] = fp_zero();
}
BLSW_HD Fp fp_of_bool(bool b) {  // a flag as a result element: the integer 0 or 1 in limb 0 (not Montgomery)
    Fp r = fp_zero();
    r.l[0] = b ? 1u : 0u;
    return r;
}
BLSW_HD void st_verdict(Fp* p, bool v) {
    for (int j = 0; j < 6; j++) st2(p + 2 * j, {fp_of_bool(v), fp_zero()});
}
// what csrc/ has no single-lane text for, stated with single-lane functions
BLSW_HD Fp12 sparse_014(const Fp* c) { return {{ld2(c), ld2(c + 2), fp2_zero()}, {fp2_zero(), ld2(c + 4), fp2_zero()}}; }
BLSW_HD Fp12 mul_value(const Fp12& a, const Fp12& b) {
    Emitter none = {nullptr, 0};
    return fp12_mul_w(none, a, b);
}

// The op of a team form is chosen at run time, as at the library's call sites (team_miller: `ph == 0 ? TEAM_OP_SQR : ...`): `alt` is a kernel
// argument that is always 0. A table known at compile time would let the compiler fold the descriptors the executor fetches from constant memory.
BLSW_HD const TeamOp& pick(uint32_t alt, const TeamOp& T, const TeamOp& other) { return alt ? other : T; }
template <bool HOT, class TEAM>
BLSW_HD typename TEAM::Reg run(TEAM& t, const TeamOp& T, const typename TEAM::Reg& a, const typename TEAM::Reg& b) {
    if constexpr (HOT)
        return t.exec_hot(T, a, b);
    else
        return t.exec(T, a, b);
}

template <int OP>
struct TeamEntry;
#define DEVTEAM_X_TRAITS(name, dual_, g2_, wit, tail) \
    template <>                                       \
    struct TeamEntry<OP_##name> {                     \
        static constexpr bool dual = dual_, g2 = g2_; \
        template <bool HOT, class TEAM>               \
        static BLSW_HD void team(TEAM& t, const Fp* a, const Fp* b, const Fp* c, uint32_t alt); \
        static inline void single(const Fp* a, const Fp* b, const Fp* c, Fp* out, Emitter& e);  \
    };
DEVTEAM_OPS(DEVTEAM_X_TRAITS)
#undef DEVTEAM_X_TRAITS
#define DEVTEAM_TEAM(name)          \
    template <bool HOT, class TEAM> \
    BLSW_HD void TeamEntry<OP_##name>::team(TEAM& t, const Fp* a, const Fp* b, const Fp* c, uint32_t alt)
#define DEVTEAM_SINGLE(name) inline void TeamEntry<OP_##name>::single(const Fp* a, const Fp* b, const Fp* c, Fp* out, Emitter& e)
#define DEVTEAM_UNUSED(...) (void)sizeof(devteam_unused(__VA_ARGS__))
template <class... A>
BLSW_HD int devteam_unused(const A&...) { return 0; }

// ---- the op tables on Fp12 operands
DEVTEAM_TEAM(MUL) {
    DEVTEAM_UNUSED(c);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_MUL, TEAM_OP_SQR), t.ld(a), t.ld(b)));
}
DEVTEAM_SINGLE(MUL) {
    DEVTEAM_UNUSED(c);
    st12(out, fp12_mul_w(e, ld12(a), ld12(b)));
}
DEVTEAM_TEAM(SQR) {
    DEVTEAM_UNUSED(b, c);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_SQR, TEAM_OP_MUL), f, f));
}
DEVTEAM_SINGLE(SQR) {
    DEVTEAM_UNUSED(b, c);
    st12(out, fp12_sqr_w(e, ld12(a)));
}
DEVTEAM_TEAM(CYC) {
    DEVTEAM_UNUSED(b, c);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_CYC, TEAM_OP_MUL), f, f));
}
DEVTEAM_SINGLE(CYC) {
    DEVTEAM_UNUSED(b, c);
    st12(out, fp12_cyclotomic_square_w(e, ld12(a)));
}
// ---- the ell ops. c = (c0.c0, c0.c1, c1.c0, c1.c1, p.x, p.y): one step of prepare_g2's coefficients and the pair's G1 point
DEVTEAM_TEAM(ELLC) {  // the pair (-g1, sig) as team_miller loads it: set_consts once, load_coeffs per step (c1 times g1.x, TS_XYC)
    DEVTEAM_UNUSED(b);
    t.set_coeffs(c);
    t.set_consts(c[4], c[5]);
    t.load_coeffs(0);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_ELLC, TEAM_OP_ELLV), f, f));
}
DEVTEAM_SINGLE(ELLC) {
    DEVTEAM_UNUSED(b);
    st12(out, ell_const_p_w(e, ld12(a), CoeffLinear{const_cast<Fp*>(c)}, 0, false));
}
DEVTEAM_TEAM(ELLV) {  // the pair (pk, H(m)) as team_miller_pv / team_miller_multi load it: team_load_pair_lane
    DEVTEAM_UNUSED(b);
    t.set_coeffs(c);
    t.pkx = c[4];
    t.pky = c[5];
    t.load_pair_h(0);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_ELLV, TEAM_OP_SQR), f, f));
}
DEVTEAM_SINGLE(ELLV) {
    DEVTEAM_UNUSED(b);
    st12(out, ell_var_p_w(e, ld12(a), CoeffLinear{const_cast<Fp*>(c)}, 0, c[4], c[5]));
}
// the native pairing's ell: c = (c0, c1, c4), three general Fp2 coefficients, null cursor (value-only kinds, no witnesses)
DEVTEAM_TEAM(ELLGS) {  // team_load_lines_lane: lanes 0..2 fill XS0, XS1, XYC (lanes 3..5 the other pair's slots, from the same triple)
    DEVTEAM_UNUSED(b);
    t.set_coeffs(c);
    t.e.base = nullptr;
    t.load_lines(0);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_ELLGS, TEAM_OP_ELLGH), f, f));
}
DEVTEAM_SINGLE(ELLGS) {
    DEVTEAM_UNUSED(b, e);
    st12(out, mul_value(ld12(a), sparse_014(c)));
}
DEVTEAM_TEAM(ELLGH) {  // team_load_pair_lines_lane: lanes 0..2 fill XH0, XH1, XYV
    DEVTEAM_UNUSED(b);
    t.set_coeffs(c);
    t.e.base = nullptr;
    t.load_pair_lines(0);
    const typename TEAM::Reg f = t.ld(a);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_ELLGH, TEAM_OP_SQR), f, f));
}
DEVTEAM_SINGLE(ELLGH) {
    DEVTEAM_UNUSED(b, e);
    st12(out, mul_value(ld12(a), sparse_014(c)));
}
// ---- G2 points on lanes 0..2: a = P, b = Q as (x, y, z)
DEVTEAM_TEAM(G2DBL) {
    DEVTEAM_UNUSED(c);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_G2DBL, TEAM_OP_G2ADD), t.ld(a), t.ld(b)));
}
DEVTEAM_SINGLE(G2DBL) {
    DEVTEAM_UNUSED(b, c);
    st_point(out, proj_double_w<OpsFp2>(e, {ld2(a), ld2(a + 2), ld2(a + 4)}));
}
DEVTEAM_TEAM(G2ADD) {
    DEVTEAM_UNUSED(c);
    t.st(run<HOT>(t, pick(alt, TEAM_OP_G2ADD, TEAM_OP_G2DBL), t.ld(a), t.ld(b)));
}
DEVTEAM_SINGLE(G2ADD) {
    DEVTEAM_UNUSED(c);
    st_point(out, proj_add_w<OpsFp2, 0>(e, {ld2(a), ld2(a + 2), ld2(a + 4)}, {ld2(b), ld2(b + 2), ld2(b + 4)}));
}
// ---- routines
DEVTEAM_TEAM(inverse_w) {
    DEVTEAM_UNUSED(b, c, alt);
    t.st(t.inverse_w(t.ld(a)));
}
DEVTEAM_SINGLE(inverse_w) {
    DEVTEAM_UNUSED(b, c);
    st12(out, fp12_inv_w(e, ld12(a)));
}
DEVTEAM_TEAM(is_one_w) {  // the 35 witnesses go through the second cursor: the team's own stays where it is
    DEVTEAM_UNUSED(b, c, alt);
    const Emitter e_one = t.e;
    t.st_flag(t.is_one_w(t.ld(a), e_one));
}
DEVTEAM_SINGLE(is_one_w) {  // the tail of chain_final_exp_is_one
    DEVTEAM_UNUSED(b, c);
    const Fp12 v = ld12(a), one = fp12_one();
    const bool b0 = fp6_is_eq_w(e, one.c0, v.c0);
    const bool b1 = fp6_is_eq_w(e, one.c1, v.c1);
    const bool res = b0 && b1;
    e.put_bool(res);
    st_verdict(out, res);
}
DEVTEAM_TEAM(conj) {
    DEVTEAM_UNUSED(b, c, alt);
    t.st(t.conj(t.ld(a)));
}
DEVTEAM_SINGLE(conj) {
    DEVTEAM_UNUSED(b, c, e);
    st12(out, fp12_conj(ld12(a)));
}
#define DEVTEAM_FROB(k)                        \
    DEVTEAM_TEAM(frob_##k) {                   \
        DEVTEAM_UNUSED(b, c, alt);             \
        t.st(t.frob(t.ld(a), k));              \
    }                                          \
    DEVTEAM_SINGLE(frob_##k) {                 \
        DEVTEAM_UNUSED(b, c, e);               \
        st12(out, fp12_frobenius<k>(ld12(a))); \
    }
DEVTEAM_FROB(1)
DEVTEAM_FROB(2)
DEVTEAM_FROB(3)
#undef DEVTEAM_FROB
DEVTEAM_TEAM(first_f) {  // team_miller: the first ell, on the constant f = 1, is a linear combination of the loaded slots
    DEVTEAM_UNUSED(a, b, alt);
    t.set_coeffs(c);
    t.set_consts(c[4], c[5]);
    t.load_coeffs(0);
    t.st(t.first_f());
}
DEVTEAM_SINGLE(first_f) {
    DEVTEAM_UNUSED(a, b);
    st12(out, ell_const_p_w(e, fp12_one(), CoeffLinear{const_cast<Fp*>(c)}, 0, true));
}
DEVTEAM_TEAM(first_f_var) {  // team_miller_pv: the allocated generator's pair, two product witnesses
    DEVTEAM_UNUSED(a, b, alt);
    t.set_coeffs(c);
    t.load_pair_sig(0);
    t.st(t.first_f_var());
}
DEVTEAM_SINGLE(first_f_var) {  // ell with a variable point on the constant f = 1: c1.c0 * p.x, c1.c1 * p.x are products of variables, the rest is linear
    DEVTEAM_UNUSED(a, b);
    const Fp k0 = fp_mul_w(e, c[2], K_G1_GEN_X());
    const Fp k1 = fp_mul_w(e, c[3], K_G1_GEN_X());
    st12(out, fp12_mul_by_014_const_f(fp12_one(), ld2(c), {k0, k1}, K_G1_GEN_NEG_Y()));
}
DEVTEAM_TEAM(exp_by_x) {
    DEVTEAM_UNUSED(b, c, alt);
    t.st(team_exp_by_x(t, t.ld(a)));
}
DEVTEAM_SINGLE(exp_by_x) {
    DEVTEAM_UNUSED(b, c);
    st12(out, fp12_exp_by_x_w(e, ld12(a)));
}
DEVTEAM_TEAM(final_exp_is_one) {  // the team's cursor runs over the final exponentiation, the second one over the is_one tail behind it
    DEVTEAM_UNUSED(b, c, alt);
    Emitter e_one = t.e;
    e_one.pos += final_exp_witnesses();
    t.st_flag(team_final_exp_is_one(t, t.ld(a), e_one));
}
DEVTEAM_SINGLE(final_exp_is_one) {  // chain_final_exp_is_one takes its cursors by value: the stream and the sentinel behind it state its count
    DEVTEAM_UNUSED(b, c);
    Emitter e_one = e;
    e_one.pos += final_exp_witnesses();
    st_verdict(out, chain_final_exp_is_one(e, e_one, ld12(a)));
    e.pos += final_exp_witnesses() + DEVTEAM_IS_ONE_WITNESSES;
}
// SQR -> ELLC -> ELLV -> SQR -> MUL -> CYC -> MUL on one running f. c = step 0's and step 1's coefficients (four elements each), p.x, p.y at 8, 9;
// the pair slots are loaded as team_miller does (set_consts once, load_coeffs before an ell), step 1's between the two ells
DEVTEAM_TEAM(seq) {
    typedef typename TEAM::Reg R;
    t.set_coeffs(c);
    t.set_consts(c[8], c[9]);
    R f = t.ld(a);
    const R g = t.ld(b);
    f = run<HOT>(t, pick(alt, TEAM_OP_SQR, TEAM_OP_MUL), f, f);
    t.load_coeffs(0);
    f = run<HOT>(t, pick(alt, TEAM_OP_ELLC, TEAM_OP_ELLV), f, f);
    t.load_coeffs(1);
    f = run<HOT>(t, pick(alt, TEAM_OP_ELLV, TEAM_OP_ELLC), f, f);
    f = run<HOT>(t, pick(alt, TEAM_OP_SQR, TEAM_OP_CYC), f, f);
    f = run<HOT>(t, pick(alt, TEAM_OP_MUL, TEAM_OP_CYC), f, g);
    f = run<HOT>(t, pick(alt, TEAM_OP_CYC, TEAM_OP_MUL), f, f);
    f = run<HOT>(t, pick(alt, TEAM_OP_MUL, TEAM_OP_SQR), f, g);
    t.st(f);
}
DEVTEAM_SINGLE(seq) {
    const CoeffLinear C = {const_cast<Fp*>(c)};
    const Fp12 g = ld12(b);
    Fp12 f = fp12_sqr_w(e, ld12(a));
    f = ell_const_p_w(e, f, C, 0, false);
    f = ell_var_p_w(e, f, C, 1, c[8], c[9]);
    f = fp12_sqr_w(e, f);
    f = fp12_mul_w(e, f, g);
    f = fp12_cyclotomic_square_w(e, f);
    f = fp12_mul_w(e, f, g);
    st12(out, f);
}

#undef DEVTEAM_TEAM
#undef DEVTEAM_SINGLE

}  // namespace devteam
