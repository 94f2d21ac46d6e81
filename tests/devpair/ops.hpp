// TEST HARNESS ONLY (never linked into libblsw.so): one table of the PROGRAMS that sequence the team / field ops into a pairing (csrc/chains.hpp:
// chain_miller, chain_miller_multi; team.hpp: team_miller, team_miller_pv, team_miller_multi; vpairing.hpp: both vline_chain forms,
// team_miller_values, team_miller_groups; vgroups.hpp: team_groups_finish), each from the same operand block of an item:
//   single  the single-lane statement (form 0): tests/hostsim/hostsim.cpp runs it on the host; tests/devpair/devpair.hip runs the ones the library
//           ships on a lane (chain_miller: k_pairing; vline_chain: k_vlines, k_vg_lines) with one thread per item
//   team    the program against the TEAM interface of team.hpp (form 1): hostsim on its looped team, devpair.hip on the library's own device
//           teams (TeamLanes, TeamLanesPv, TeamLanesMulti, TeamLanesValues, TeamLanesGroups), ten teams per wave
// Operand block of an item, `n_in` stored elements:
//   miller, miller_pv, miller_multi   coeff_sig [272], then per pair j < K: coeff_h_j [272], pk_j.x, pk_j.y   (K = 1 for the first two)
//   vlines2                           q.x (2), q.y (2), p.x, p.y
//   vlines3                           q.x (2), q.y (2), p0, p.x, p.y
//   miller_values                     lines_sig [408], lines_h [408]
//   miller_groups                     count, own, mask (integers in limb 0), then nine line sets [408]: sets 0 .. count - 1 are the chunk's instance pairs,
//                                     set `count` the group's own pair if own != 0; bit p of mask = pair p is folded. The result is the partial product
//   groups_finish                     n (1 .. 3, integer in limb 0), then three partial products [12]. The result is the verdict, as devteam's st_verdict
// Result: a Miller value as twelve elements, the 408 line rows, or a verdict. Witness counts are functions of the op tables' counts and of miller_step_info().
#pragma once
#include "chains.hpp"
#include "miller_par.hpp"
#include "team.hpp"
#include "vpairing.hpp"
#include "decode.hpp"
#include "vgroups.hpp"
#include "../devteam/ops.hpp"

namespace devpair {
using namespace blsw;
using devteam::T_ELLC;
using devteam::T_ELLV;
using devteam::T_SQR;

#define DEVPAIR_COEFFS (4u * BLSW_MILLER_STEPS)  // prepare_g2's coefficients of one G2 point
#define DEVPAIR_PAIR (DEVPAIR_COEFFS + 2u)       // one variable pair of an item: its coefficients and its G1 point
#define DEVPAIR_K_MAX 25u
#define DEVPAIR_GROUPS_SETS 9u      // line sets of a miller_groups item: `count` instance pairs, then (own != 0) the group's own pair
#define DEVPAIR_GROUPS_HDR 3u       // count, own, mask as the integers in limb 0 of the block's first three elements
#define DEVPAIR_FINISH_PARTIALS 3u  // partial products of a groups_finish item; the integer in limb 0 of element 0 says how many are used

constexpr uint32_t n_squares() {
    const MillerStepInfo m = miller_step_info();
    uint32_t s = 0;
    for (uint32_t k = 0; k < BLSW_MILLER_STEPS; k++) s += m.dbl[k];
    return s;
}
// witnesses of the Miller segment that belong to no variable pair, as miller_step_info() places them
constexpr uint32_t spine_witnesses() { return miller_step_info().base[BLSW_MILLER_STEPS]; }
// the same from the op tables: every square, and every ell of the constant pair but the first (a linear combination of constants)
template <class NW>
inline uint32_t spine_from_tables(const NW& nw) { return n_squares() * nw(T_SQR) + (BLSW_MILLER_STEPS - 1u) * nw(T_ELLC); }

// X(name, single on the device, has a team form, n_in(K), n_out, witnesses(K, nw))
#define DEVPAIR_OPS(X)                                                                                                             \
    X(miller, 1, 1, DEVPAIR_COEFFS + DEVPAIR_PAIR, 12u, spine_from_tables(nw) + BLSW_MILLER_STEPS * nw(T_ELLV))                    \
    X(miller_pv, 0, 1, DEVPAIR_COEFFS + DEVPAIR_PAIR, 12u, n_squares() * nw(T_SQR) + 2u + (2u * BLSW_MILLER_STEPS - 1u) * nw(T_ELLV)) \
    X(miller_multi, 0, 1, DEVPAIR_COEFFS + K * DEVPAIR_PAIR, 12u, spine_from_tables(nw) + K * BLSW_MILLER_STEPS * nw(T_ELLV))      \
    X(vlines2, 1, 0, 6u, BLSW_VLINE_ROWS, 0u)                                                                                     \
    X(vlines3, 1, 0, 7u, BLSW_VLINE_ROWS, 0u)                                                                                     \
    X(miller_values, 0, 1, 2u * BLSW_VLINE_ROWS, 12u, 0u)                                                                        \
    X(miller_groups, 0, 1, DEVPAIR_GROUPS_HDR + DEVPAIR_GROUPS_SETS * BLSW_VLINE_ROWS, 12u, 0u)                                    \
    X(groups_finish, 0, 1, 1u + DEVPAIR_FINISH_PARTIALS * 12u, 12u, 0u)

enum OpId {
#define DEVPAIR_X_ENUM(name, sdev, team, nin, nout, wit) OP_##name,
    DEVPAIR_OPS(DEVPAIR_X_ENUM)
#undef DEVPAIR_X_ENUM
        OP_COUNT
};
inline bool k_ok(int op, uint32_t K) { return op == OP_miller_multi ? (K >= 1 && K <= DEVPAIR_K_MAX) : K == 1; }
template <class NW>
inline int64_t op_n_wit(int op, uint32_t K, const NW& nw) {
    (void)K;
    (void)nw;
    switch (op) {
#define DEVPAIR_X_WIT(name, sdev, team, nin, nout, wit) \
    case OP_##name:                                     \
        return (int64_t)(wit);
        DEVPAIR_OPS(DEVPAIR_X_WIT)
#undef DEVPAIR_X_WIT
    }
    return -1;
}
inline int64_t op_n_in(int op, uint32_t K) {
    (void)K;
    switch (op) {
#define DEVPAIR_X_IN(name, sdev, team, nin, nout, wit) \
    case OP_##name:                                    \
        return (int64_t)(nin);
        DEVPAIR_OPS(DEVPAIR_X_IN)
#undef DEVPAIR_X_IN
    }
    return -1;
}
inline int64_t op_n_out(int op) {
    switch (op) {
#define DEVPAIR_X_OUT(name, sdev, team, nin, nout, wit) \
    case OP_##name:                                     \
        return (int64_t)(nout);
        DEVPAIR_OPS(DEVPAIR_X_OUT)
#undef DEVPAIR_X_OUT
    }
    return -1;
}
// bit 0: the entry has a single-lane form; bit 1: a team form; bit 2: the single-lane form also runs on the device
inline int op_forms(int op) {
    switch (op) {
#define DEVPAIR_X_FORMS(name, sdev, team, nin, nout, wit) \
    case OP_##name:                                       \
        return (OP_##name == OP_miller_values ? 0 : 1) | (team ? 2 : 0) | (sdev ? 4 : 0);  // miller_values has no other statement than its team form
        DEVPAIR_OPS(DEVPAIR_X_FORMS)
#undef DEVPAIR_X_FORMS
    }
    return -1;
}

// ---- the single-lane statements. C: a coefficient accessor (CoeffLinear on the host, CoeffStrided on the device)
// team_miller_pv's: ParametersVar allocated as witnesses, so the pair (-g1, sig) has a variable point too. Its first ell, on the constant f = 1,
// leaves the two products of variables c1.c0 g1.x, c1.c1 g1.x as witnesses; every other ell is ell_var_p_w.
template <class C>
BLSW_FN Fp12 chain_miller_pv(Emitter e, const Fp& pkx, const Fp& pky, const C& coeff_sig, const C& coeff_h) {
    const Fp gx = K_G1_GEN_X(), gy = K_G1_GEN_NEG_Y();
    Fp12 f = fp12_one();
    uint32_t k = 0;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        const int reps = ((BLSW_X_ABS >> i) & 1) ? 2 : 1;
        for (int rep = 0; rep < reps; rep++) {
            if (rep == 0 && i != 62) f = fp12_sqr_w(e, f);
            if (k == 0) {
                const Fp k0 = fp_mul_w(e, coeff_sig.ld(2), gx);
                const Fp k1 = fp_mul_w(e, coeff_sig.ld(3), gx);
                f = fp12_mul_by_014_const_f(f, {coeff_sig.ld(0), coeff_sig.ld(1)}, {k0, k1}, gy);
            } else {
                f = ell_var_p_w(e, f, coeff_sig, k, gx, gy);
            }
            f = ell_var_p_w(e, f, coeff_h, k, pkx, pky);
            k++;
        }
    }
    return fp12_conj(f);
}
// the pairs of one item's operand block, for chain_miller_multi
struct PairsBlock {
    const Fp* in;
    void pk(uint32_t j, Fp& x, Fp& y) const {
        x = in[DEVPAIR_COEFFS + j * DEVPAIR_PAIR + DEVPAIR_COEFFS];
        y = in[DEVPAIR_COEFFS + j * DEVPAIR_PAIR + DEVPAIR_COEFFS + 1];
    }
    CoeffLinear coeff_h(uint32_t j) const { return CoeffLinear{const_cast<Fp*>(in) + DEVPAIR_COEFFS + j * DEVPAIR_PAIR}; }
};
// team_miller_groups' single-lane statement: per line index one square (doubling steps below the top bit), then the dense product with the
// embedded line (c0, c1, c4) of every pair whose mask bit is set, in pair order. Not conjugated.
inline Fp12 chain_miller_groups(const Fp* in) {
    const uint32_t count = in[0].l[0], own = in[1].l[0], mask = in[2].l[0], n_pairs = count + (own ? 1u : 0u);
    const MillerStepInfo info = miller_step_info();
    Fp12 f = fp12_one();
    for (uint32_t k = 0; k < BLSW_MILLER_STEPS; k++) {
        if (info.dbl[k]) f = devteam::mul_value(f, f);
        for (uint32_t p = 0; p < n_pairs; p++)
            if ((mask >> p) & 1u) f = devteam::mul_value(f, devteam::sparse_014(in + DEVPAIR_GROUPS_HDR + p * BLSW_VLINE_ROWS + 6 * k));
    }
    return f;
}
// team_groups_finish's: the product of the first n partials, conjugated, through the single-lane final exponentiation and is_one on null cursors
inline bool chain_groups_finish(const Fp* in) {
    const uint32_t n = in[0].l[0];
    Fp12 f = devteam::ld12(in + 1);
    for (uint32_t q = 1; q < n; q++) f = devteam::mul_value(f, devteam::ld12(in + 1 + 12 * q));
    return chain_final_exp_is_one(Emitter{nullptr, 0}, Emitter{nullptr, 0}, fp12_conj(f));
}
// host only: one item's single-lane form. The chains take their cursor by value: the stream and the sentinel behind it state the count.
inline void run_single(int op, uint32_t K, const Fp* in, Fp* out, Emitter e) {
    const PairsBlock pairs = {in};
    const CoeffLinear cs = {const_cast<Fp*>(in)};
    Fp px, py;
    pairs.pk(0, px, py);
    switch (op) {
        case OP_miller: devteam::st12(out, chain_miller(e, px, py, cs, pairs.coeff_h(0))); break;
        case OP_miller_pv: devteam::st12(out, chain_miller_pv(e, px, py, cs, pairs.coeff_h(0))); break;
        case OP_miller_multi: devteam::st12(out, chain_miller_multi(e, K, pairs, cs)); break;
        case OP_vlines2: vline_chain(Fp2{in[0], in[1]}, Fp2{in[2], in[3]}, in[4], in[5], CoeffLinear{out}); break;
        case OP_vlines3: vline_chain(Fp2{in[0], in[1]}, Fp2{in[2], in[3]}, in[4], in[5], in[6], CoeffLinear{out}); break;
        case OP_miller_groups: devteam::st12(out, chain_miller_groups(in)); break;
        case OP_groups_finish: devteam::st_verdict(out, chain_groups_finish(in)); break;
        default: break;
    }
}

// ---- the team forms. The harness has bound the team to its item's operands (coefficient accessors, pair loaders, cursor); (px, py) is pair 0's point.
// TEAM provides set_gen_y(): the constant -g1.y into TS_XYC, as k_pairing_team_multi does in front of team_miller_multi.
template <int OP, class TEAM>
BLSW_HD typename TEAM::Reg run_team(TEAM& t, const Fp& px, const Fp& py, uint32_t K) {
    (void)px;
    (void)py;
    (void)K;
    if constexpr (OP == OP_miller) {
        t.set_consts(px, py);
        return team_miller(t);
    } else if constexpr (OP == OP_miller_pv) {
        t.pkx = px;
        t.pky = py;
        return team_miller_pv(t);
    } else if constexpr (OP == OP_miller_multi) {
        t.set_gen_y();
        return team_miller_multi(t, K);
    } else if constexpr (OP == OP_miller_values) {
        t.e = {nullptr, 0};
        return team_miller_values(t);
    } else {
        // the harness has bound first / count / mask (TeamLanesGroups' fields) to the item: pairs [first, first + n_pairs), K = n_pairs here
        static_assert(OP == OP_miller_groups, "no team form that returns a value");
        t.e = {nullptr, 0};
        return team_miller_groups(t, (uint32_t)t.first, K);
    }
}
// groups_finish returns a verdict: partials [first_partial, first_partial + n)
template <class TEAM>
BLSW_HD bool run_team_finish(TEAM& t, uint64_t first_partial, uint32_t n) {
    t.e = {nullptr, 0};
    return team_groups_finish(t, first_partial, n);
}

}  // namespace devpair
