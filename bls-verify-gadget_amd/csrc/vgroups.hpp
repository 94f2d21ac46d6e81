// Batch verification of GROUPS of (pk, msg, sig) triples with caller-chosen 64-bit coefficients r_i (blsw_verify_groups_batch):
//     prod_i e(r_i pk_i, H(m_i)) * e(-g1, sum_i r_i sig_i) == 1
// decides a whole group with ONE final exponentiation, one line chain per instance (the signatures are summed before their pair is walked) and
// squarings of the Miller loop shared by the pairs one team folds. Stages (k_vgroups.hip; tests/vgroups runs them on the host for one group):
//   scale    one lane per point: P_i = r_i pk_i (Jacobian over Fp), S_i = r_i sig_i (Jacobian over Fp2); an excluded instance — a decode status
//            that is not OK, or a zero coefficient — is the identity in both
//   sum      one lane per group: S_g = sum_i S_i, to affine (one inversion per group), and the group's flags
//   lines    vline_chain of H(m_i) against the PROJECTIVE P_i (three Fp multipliers, vpairing.hpp) and of S_g against -g1
//   fold     six lanes per chunk of <= `chunk` consecutive instances of one group: team_miller_groups; the group's own pair (-g1, S_g) rides with
//            the group's first chunk. Partial products (not conjugated) go to the workspace
//   finish   six lanes per group: the product of the partials, conj (x < 0), final exponentiation, is_one, AND the group's flags
// An excluded instance and an identity S_g are SKIPPED pairs (factor 1), never zero lines folded into f: two valid signatures that cancel
// (sk and r - sk on one message) make S_g the identity of a group that must pass.
#pragma once
#include "vpairing.hpp"

namespace blsw {

enum : int32_t { VG_FLAG_OK = 1, VG_FLAG_SUM = 2 };  // every instance included; S_g is not the identity

BLSW_HD bool vg_included(int32_t st_pk, int32_t st_sig, uint64_t r) { return st_pk == DEC_OK && st_sig == DEC_OK && r != 0; }

// r * (px, py), 64-bit double-and-add from the top set bit; r = 0 gives the identity (z = 0)
BLSW_HD Jac1v vg_scale_g1(const Fp& px, const Fp& py, uint64_t r) {
    Jac1v acc = {fp_one(), fp_one(), fp_zero()};
    bool started = false;
#pragma unroll 1
    for (int i = 63; i >= 0; i--) {
        if (started) acc = v1_dbl(acc);
        if ((r >> i) & 1) {
            acc = v1_add_mixed(acc, px, py);
            started = true;
        }
    }
    return acc;
}
BLSW_HD Jac2 vg_scale_g2(const Fp2& qx, const Fp2& qy, uint64_t r) {
    Jac2 acc = {fp2_one(), fp2_one(), fp2_zero()};
    bool started = false;
#pragma unroll 1
    for (int i = 63; i >= 0; i--) {
        if (started) acc = v_dbl(acc);
        if ((r >> i) & 1) {
            acc = v_add_mixed(acc, qx, qy);
            started = true;
        }
    }
    return acc;
}
// sum of m Jacobian points, ld(i) -> Jac2. v_add takes its doubling branch on equal summands and returns the identity on opposite ones.
template <class LD>
BLSW_HD Jac2 vg_sum(uint32_t m, const LD& ld) {
    Jac2 acc = {fp2_one(), fp2_one(), fp2_zero()};
#pragma unroll 1
    for (uint32_t i = 0; i < m; i++) acc = v_add(acc, ld(i));
    return acc;
}
// (X / Z^2, Y / Z^3); false (and zeros) for the identity
BLSW_HD bool vg_affine2(const Jac2& s, Fp2& x, Fp2& y) {
    const bool inf = fp2_is_zero(s.z);
    const Fp2 zi = fp2_inv_inl(s.z), zi2 = v_sqr(zi);  // the inverse of 0 is 0
    x = inf ? fp2_zero() : fp2_mul_inl(s.x, zi2);
    y = inf ? fp2_zero() : fp2_mul_inl(s.y, fp2_mul_inl(zi2, zi));
    return !inf;
}
// the three line multipliers of a Jacobian G1 point (vpairing.hpp): (Z^3, X Z, Y) = Z^3 (1, x, y)
BLSW_HD void vg_line_multipliers(const Jac1v& p, Fp& m0, Fp& m1, Fp& m2) {
    m0 = fp_mul(fp_sqr(p.z), p.z);
    m1 = fp_mul(p.x, p.z);
    m2 = p.y;
}

// chunks of a group: instances [first, first + count) of chunk q of group g; count may be 0 in the last, short group
struct VgChunk {
    uint64_t first;
    uint32_t count;
};
BLSW_HD uint32_t vg_group_eff(uint64_t n, uint32_t group) { return (uint64_t)group < n ? group : (uint32_t)n; }
BLSW_HD uint32_t vg_chunks_per_group(uint64_t n, uint32_t group, uint32_t chunk) { return (vg_group_eff(n, group) + chunk - 1) / chunk; }
BLSW_HD uint64_t vg_groups(uint64_t n, uint32_t group) { return (n + group - 1) / group; }
BLSW_HD VgChunk vg_chunk(uint64_t n, uint32_t group, uint32_t chunk, uint64_t g, uint32_t q) {
    const uint64_t g0 = g * group, g1 = g0 + group < n ? g0 + group : n;
    const uint64_t first = g0 + (uint64_t)q * chunk;
    if (first >= g1) return {g0, 0};
    return {first, (uint32_t)(g1 - first < chunk ? g1 - first : chunk)};
}

// the group's verdict from its partial products [first_partial, first_partial + n_partials). TEAM provides load_partial(idx) -> Reg
template <class TEAM>
BLSW_HD bool team_groups_finish(TEAM& t, uint64_t first_partial, uint32_t n_partials) {
    typename TEAM::Reg f = t.load_partial(first_partial);
#pragma unroll 1
    for (uint32_t q = 1; q < n_partials; q++) f = t.exec_hot(TEAM_OP_MUL, f, t.load_partial(first_partial + q));
    return team_final_exp_is_one(t, t.conj(f), Emitter{nullptr, 0});
}

}  // namespace blsw
