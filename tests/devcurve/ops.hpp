// TEST HARNESS ONLY (never linked into libblsw.so): one table of the curve operations of csrc/decode.hpp, vcurve.hpp, curve.hpp, vsign.hpp and
// vgroups.hpp, each as a function of two operand blocks. tests/hostsim/hostsim.cpp compiles it for the host (hostsim_curve_op),
// tests/devcurve/devcurve.hip three times for the device (programs out of line, inlined, inlined on quads), one kernel per operation. An operation
// reads up to twelve elements of `a` and of `b`, writes its result elements to `out` and emits its witnesses through `e`; what it does not name it
// does not touch. Flags, status codes and digits are results with the integer in the low limbs (not Montgomery). Raw bytes ride in element slots:
// a 48-byte record is one slot, a 96-byte record two, a 32-byte scalar or a 64-bit coefficient the low limbs of one. `park` is the PARK of
// v_clear_cofactor and v_g2_mul_gls (DEVCURVE_PARK_SLOTS Jacobian points of the item).
#pragma once
#include "vgroups.hpp"
#include "vsign.hpp"

namespace devcurve {
using namespace blsw;

#define DEVCURVE_OUT_MAX 12     // result elements of an operation
#define DEVCURVE_PARK_SLOTS 16  // v_g2_mul_gls: slots 1..15
// X(name, result elements, witnesses, in the quad build). The quad build carries the entries whose code has a BLSW_QUAD_DEV path or that
// cofactor_vf.hpp / prepare_vf.hpp / chains.hpp call; the library compiles decode, encode, sign, scale and map code only without quads.
#define DEVCURVE_OPS(X)                 \
    X(fp_from_be48_1f, 2, 0, 0)         \
    X(fp_from_be48_ff, 2, 0, 0)         \
    X(fp_sqrt, 2, 0, 0)                 \
    X(fp2_sqrt, 3, 0, 0)                \
    X(fp_lex_largest, 1, 0, 0)          \
    X(fp2_lex_largest, 1, 0, 0)         \
    X(g1_decode, 3, 0, 0)               \
    X(g2_decode, 5, 0, 0)               \
    X(g1_encode, 1, 0, 0)               \
    X(g2_encode, 2, 0, 0)               \
    X(sk_from_le32, 2, 0, 0)            \
    X(g1_in_subgroup, 1, 0, 0)          \
    X(g2_in_subgroup, 1, 0, 0)          \
    X(g1_in_subgroup_ladder, 1, 0, 0)   \
    X(g2_in_subgroup_ladder, 1, 0, 0)   \
    X(jac1_dbl, 3, 0, 1)                \
    X(jac1_add_mixed, 3, 0, 1)          \
    X(jac1v_dbl, 3, 0, 0)               \
    X(jac1v_add_mixed, 3, 0, 0)         \
    X(jac2_dbl, 6, 0, 0)                \
    X(jac2_add_mixed, 6, 0, 0)          \
    X(v1_dbl, 3, 0, 0)                  \
    X(v1_add_mixed, 3, 0, 0)            \
    X(v_sqr, 2, 0, 1)                   \
    X(v_dbl, 6, 0, 1)                   \
    X(v_dbl_inplace, 6, 0, 1)           \
    X(v_add_mixed, 6, 0, 1)             \
    X(v_add, 6, 0, 1)                   \
    X(v_neg, 6, 0, 0)                   \
    X(v_psi, 6, 0, 0)                   \
    X(v_psi2, 6, 0, 0)                  \
    X(g1_mul_affine, 3, 0, 0)           \
    X(g2_mul_affine, 5, 0, 0)           \
    X(v_pow_c1, 2, 0, 0)                \
    X(v_sgn0, 1, 0, 0)                  \
    X(v_poly, 2, 0, 0)                  \
    X(v_map_to_curve, 6, 0, 0)          \
    X(v_clear_cofactor, 6, 0, 0)        \
    X(v_digits_x, 4, 0, 0)              \
    X(v_g2_mul_gls, 6, 0, 0)            \
    X(v1_mul_g1_fixed, 3, 0, 0)         \
    X(vg_scale_g1, 3, 0, 0)             \
    X(vg_scale_g2, 6, 0, 0)             \
    X(vg_sum2, 6, 0, 0)                 \
    X(vg_sum3, 6, 0, 0)                 \
    X(vg_affine2, 5, 0, 1)              \
    X(vg_line_multipliers, 3, 0, 0)     \
    X(proj_double_w_fp, 3, 11, 1)       \
    X(proj_double_w_fp2, 6, 30, 1)      \
    X(proj_add_w_fp_z0, 3, 12, 1)       \
    X(proj_add_w_fp_z1, 3, 11, 1)       \
    X(proj_add_w_fp_z2, 3, 11, 1)       \
    X(proj_add_w_fp2_z0, 6, 36, 1)      \
    X(proj_add_w_fp2_z1, 6, 33, 1)      \
    X(proj_add_w_fp2_z2, 6, 33, 1)      \
    X(nz_double_w, 4, 10, 1)            \
    X(nz_add_unchecked_w, 4, 8, 1)      \
    X(nz_double_pre_w, 4, 10, 1)        \
    X(nz_add_unchecked_pre_w, 4, 8, 1)  \
    X(nz_double_pre_inl, 4, 10, 1)      \
    X(nz_add_unchecked_pre_inl, 4, 8, 1)

enum OpId {
#define DEVCURVE_X_ENUM(name, n_out, n_wit, quad) OP_##name,
    DEVCURVE_OPS(DEVCURVE_X_ENUM)
#undef DEVCURVE_X_ENUM
        OP_COUNT
};
inline int op_n_out(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVCURVE_X_OUT(name, n_out, n_wit, quad) n_out,
        DEVCURVE_OPS(DEVCURVE_X_OUT)
#undef DEVCURVE_X_OUT
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}
inline int op_n_wit(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVCURVE_X_WIT(name, n_out, n_wit, quad) n_wit,
        DEVCURVE_OPS(DEVCURVE_X_WIT)
#undef DEVCURVE_X_WIT
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}
inline int op_quad(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVCURVE_X_QUAD(name, n_out, n_wit, quad) quad,
        DEVCURVE_OPS(DEVCURVE_X_QUAD)
#undef DEVCURVE_X_QUAD
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}

BLSW_HD Fp2 ld2(const Fp* p) { return {p[0], p[1]}; }
BLSW_HD void st2(Fp* p, const Fp2& v) {
    p[0] = v.c0;
    p[1] = v.c1;
}
BLSW_HD Jac2 ldj2(const Fp* p) { return {ld2(p), ld2(p + 2), ld2(p + 4)}; }
BLSW_HD void st3(Fp* p, const Fp& x, const Fp& y, const Fp& z) {
    p[0] = x;
    p[1] = y;
    p[2] = z;
}
BLSW_HD void st6(Fp* p, const Fp2& x, const Fp2& y, const Fp2& z) {
    st2(p, x);
    st2(p + 2, y);
    st2(p + 4, z);
}
BLSW_HD Fp fp_of_u64(uint64_t v) {  // an integer as a result element: limbs 0 and 1 (not Montgomery)
    Fp r = fp_zero();
    r.l[0] = (uint32_t)v;
    r.l[1] = (uint32_t)(v >> 32);
    return r;
}
BLSW_HD uint64_t u64_of(const Fp& a) { return a.l[0] | ((uint64_t)a.l[1] << 32); }
BLSW_HD const uint8_t* bytes_of(const Fp* p) { return reinterpret_cast<const uint8_t*>(p); }
// eight scalar words out of the operand (the kernels hold their scalars in registers)
struct Words8 {
    uint32_t w[8];
};
BLSW_HD Words8 words_of(const Fp& a) {
    Words8 k;
    for (int i = 0; i < 8; i++) k.w[i] = a.l[i];
    return k;
}

template <int OP>
struct CurveOp;
#define DEVCURVE_DEF(name)                                                                                  \
    template <>                                                                                             \
    struct CurveOp<OP_##name> {                                                                             \
        template <class PARK>                                                                               \
        static BLSW_HD void run(const Fp* a, const Fp* b, Fp* out, Emitter& e, const PARK& park);           \
    };                                                                                                      \
    template <class PARK>                                                                                   \
    BLSW_HD void CurveOp<OP_##name>::run(const Fp* a, const Fp* b, Fp* out, Emitter& e, const PARK& park)
#define DEVCURVE_UNUSED (void)a, (void)b, (void)e, (void)park

// ---- bytes and square roots (decode.hpp)
DEVCURVE_DEF(fp_from_be48_1f) {
    DEVCURVE_UNUSED;
    Fp r = fp_zero();  // untouched when the value is not below p
    out[0] = fp_of_u64(fp_from_be48(bytes_of(a), 0x1f, r));
    out[1] = r;
}
DEVCURVE_DEF(fp_from_be48_ff) {
    DEVCURVE_UNUSED;
    Fp r = fp_zero();
    out[0] = fp_of_u64(fp_from_be48(bytes_of(a), 0xff, r));
    out[1] = r;
}
DEVCURVE_DEF(fp_sqrt) {
    DEVCURVE_UNUSED;
    Fp r;
    out[0] = fp_of_u64(fp_sqrt(a[0], r));
    out[1] = r;  // a^((p + 1) / 4) also when a is no square
}
DEVCURVE_DEF(fp2_sqrt) {
    DEVCURVE_UNUSED;
    Fp2 r = fp2_zero();  // untouched when a is no square
    out[0] = fp_of_u64(fp2_sqrt(ld2(a), r));
    st2(out + 1, r);
}
DEVCURVE_DEF(fp_lex_largest) { DEVCURVE_UNUSED, out[0] = fp_of_u64(fp_lex_largest(a[0])); }
DEVCURVE_DEF(fp2_lex_largest) { DEVCURVE_UNUSED, out[0] = fp_of_u64(fp2_lex_largest(ld2(a))); }
DEVCURVE_DEF(g1_decode) {
    DEVCURVE_UNUSED;
    Fp x, y;
    out[0] = fp_of_u64((uint64_t)g1_decode(bytes_of(a), x, y));
    out[1] = x;
    out[2] = y;
}
DEVCURVE_DEF(g2_decode) {
    DEVCURVE_UNUSED;
    Fp2 x, y;
    out[0] = fp_of_u64((uint64_t)g2_decode(bytes_of(a), x, y));
    st2(out + 1, x);
    st2(out + 3, y);
}
DEVCURVE_DEF(g1_encode) { DEVCURVE_UNUSED, g1_encode(a[0], a[1], (a[2].l[0] & 1u) != 0, reinterpret_cast<uint8_t*>(out)); }  // infinity: bit 0 of a[2]
DEVCURVE_DEF(g2_encode) { DEVCURVE_UNUSED, g2_encode(ld2(a), ld2(a + 2), (a[4].l[0] & 1u) != 0, reinterpret_cast<uint8_t*>(out)); }
DEVCURVE_DEF(sk_from_le32) {
    DEVCURVE_UNUSED;
    Fp w = fp_zero();
    out[0] = fp_of_u64((uint64_t)sk_from_le32(bytes_of(a), w.l));
    out[1] = w;  // the words are read whatever the status
}
DEVCURVE_DEF(g1_in_subgroup) { DEVCURVE_UNUSED, out[0] = fp_of_u64(g1_in_subgroup(a[0], a[1])); }
DEVCURVE_DEF(g2_in_subgroup) { DEVCURVE_UNUSED, out[0] = fp_of_u64(g2_in_subgroup(ld2(a), ld2(a + 2))); }
DEVCURVE_DEF(g1_in_subgroup_ladder) { DEVCURVE_UNUSED, out[0] = fp_of_u64(g1_in_subgroup_ladder(a[0], a[1])); }
DEVCURVE_DEF(g2_in_subgroup_ladder) { DEVCURVE_UNUSED, out[0] = fp_of_u64(g2_in_subgroup_ladder(ld2(a), ld2(a + 2))); }
// ---- Jacobian values: the point is a[0..2] (a[0..5] over Fp2), the affine or Jacobian second operand starts at b[0]
DEVCURVE_DEF(jac1_dbl) {
    DEVCURVE_UNUSED;
    const Jac1 r = jac1_dbl({a[0], a[1], a[2]});
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(jac1_add_mixed) {
    DEVCURVE_UNUSED;
    const Jac1 r = jac1_add_mixed({a[0], a[1], a[2]}, b[0], b[1]);
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(jac1v_dbl) {
    DEVCURVE_UNUSED;
    const Jac1v r = jac1v_dbl({a[0], a[1], a[2]});
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(jac1v_add_mixed) {
    DEVCURVE_UNUSED;
    const Jac1v r = jac1v_add_mixed({a[0], a[1], a[2]}, b[0], b[1]);
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(jac2_dbl) {
    DEVCURVE_UNUSED;
    const Jac2 r = jac2_dbl(ldj2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(jac2_add_mixed) {
    DEVCURVE_UNUSED;
    const Jac2 r = jac2_add_mixed(ldj2(a), ld2(b), ld2(b + 2));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v1_dbl) {
    DEVCURVE_UNUSED;
    const Jac1v r = v1_dbl({a[0], a[1], a[2]});
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v1_add_mixed) {
    DEVCURVE_UNUSED;
    const Jac1v r = v1_add_mixed({a[0], a[1], a[2]}, b[0], b[1]);
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_sqr) { DEVCURVE_UNUSED, st2(out, v_sqr(ld2(a))); }
DEVCURVE_DEF(v_dbl) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_dbl(ldj2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_dbl_inplace) {
    DEVCURVE_UNUSED;
    Jac2 r = ldj2(a);
    v_dbl_inplace(r.x, r.y, r.z);
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_add_mixed) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_add_mixed(ldj2(a), ld2(b), ld2(b + 2));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_add) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_add(ldj2(a), ldj2(b));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_neg) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_neg(ldj2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_psi) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_psi(ldj2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_psi2) {
    DEVCURVE_UNUSED;
    const Jac2 r = v_psi2(ldj2(a));
    st6(out, r.x, r.y, r.z);
}
// the scalar is the eight low words of b[0]; results: flag (false: the identity), then the affine point (zero when the flag is false)
DEVCURVE_DEF(g1_mul_affine) {
    DEVCURVE_UNUSED;
    const Words8 k = words_of(b[0]);
    Fp x = fp_zero(), y = fp_zero();
    out[0] = fp_of_u64(g1_mul_affine(a[0], a[1], k.w, x, y));
    out[1] = x;
    out[2] = y;
}
DEVCURVE_DEF(g2_mul_affine) {
    DEVCURVE_UNUSED;
    const Words8 k = words_of(b[0]);
    Fp2 x = fp2_zero(), y = fp2_zero();
    out[0] = fp_of_u64(g2_mul_affine(ld2(a), ld2(a + 2), k.w, x, y));
    st2(out + 1, x);
    st2(out + 3, y);
}
// ---- programs (vcurve.hpp, vsign.hpp, vgroups.hpp)
DEVCURVE_DEF(v_pow_c1) { DEVCURVE_UNUSED, st2(out, v_pow_c1(ld2(a))); }
DEVCURVE_DEF(v_sgn0) { DEVCURVE_UNUSED, out[0] = fp_of_u64(v_sgn0(ld2(a))); }
DEVCURVE_DEF(v_poly) {  // x = a[0..1], up to five coefficients a[2..11], their number (1..5) in b[0]
    DEVCURVE_UNUSED;
    Fp2 k[5];
    for (int i = 0; i < 5; i++) k[i] = ld2(a + 2 + 2 * i);
    const uint32_t n = b[0].l[0] < 1u ? 1u : (b[0].l[0] > 5u ? 5u : b[0].l[0]);
    st2(out, v_poly(k, (int)n, ld2(a)));
}
DEVCURVE_DEF(v_map_to_curve) {
    DEVCURVE_UNUSED;
    const Proj<OpsFp2> r = v_map_to_curve(ld2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_clear_cofactor) {
    (void)b, (void)e;
    const Jac2 r = v_clear_cofactor(park, ldj2(a));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v_digits_x) {
    DEVCURVE_UNUSED;
    const Words8 k = words_of(a[0]);
    uint64_t d[4];
    v_digits_x(k.w, d);
    for (int i = 0; i < 4; i++) out[i] = fp_of_u64(d[i]);
}
DEVCURVE_DEF(v_g2_mul_gls) {
    (void)e;
    const Words8 k = words_of(b[0]);
    const Jac2 r = v_g2_mul_gls(park, ldj2(a), k.w);
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(v1_mul_g1_fixed) {
    DEVCURVE_UNUSED;
    const Words8 k = words_of(a[0]);
    const Jac1v r = v1_mul_g1_fixed(k.w);
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(vg_scale_g1) {
    DEVCURVE_UNUSED;
    const Jac1v r = vg_scale_g1(a[0], a[1], u64_of(b[0]));
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(vg_scale_g2) {
    DEVCURVE_UNUSED;
    const Jac2 r = vg_scale_g2(ld2(a), ld2(a + 2), u64_of(b[0]));
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(vg_sum2) {  // the summands: a[0..5], b[0..5]
    DEVCURVE_UNUSED;
    const Jac2 r = vg_sum(2, [&](uint32_t i) { return ldj2(i == 0 ? a : b); });
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(vg_sum3) {  // the summands: a[0..5], a[6..11], b[0..5]
    DEVCURVE_UNUSED;
    const Jac2 r = vg_sum(3, [&](uint32_t i) { return ldj2(i == 0 ? a : (i == 1 ? a + 6 : b)); });
    st6(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(vg_affine2) {
    DEVCURVE_UNUSED;
    Fp2 x, y;
    out[0] = fp_of_u64(vg_affine2(ldj2(a), x, y));
    st2(out + 1, x);
    st2(out + 3, y);
}
DEVCURVE_DEF(vg_line_multipliers) {
    DEVCURVE_UNUSED;
    Fp m0, m1, m2;
    vg_line_multipliers({a[0], a[1], a[2]}, m0, m1, m2);
    st3(out, m0, m1, m2);
}
// ---- witness programs (curve.hpp)
DEVCURVE_DEF(proj_double_w_fp) {
    (void)b, (void)park;
    const Proj<OpsFp> r = proj_double_w<OpsFp>(e, {a[0], a[1], a[2]});
    st3(out, r.x, r.y, r.z);
}
DEVCURVE_DEF(proj_double_w_fp2) {
    (void)b, (void)park;
    const Proj<OpsFp2> r = proj_double_w<OpsFp2>(e, {ld2(a), ld2(a + 2), ld2(a + 4)});
    st6(out, r.x, r.y, r.z);
}
#define DEVCURVE_DEF_ADD(mode)                                                                                                   \
    DEVCURVE_DEF(proj_add_w_fp_z##mode) {                                                                                        \
        (void)park;                                                                                                              \
        const Proj<OpsFp> r = proj_add_w<OpsFp, mode>(e, {a[0], a[1], a[2]}, {b[0], b[1], b[2]});                                \
        st3(out, r.x, r.y, r.z);                                                                                                 \
    }                                                                                                                            \
    DEVCURVE_DEF(proj_add_w_fp2_z##mode) {                                                                                       \
        (void)park;                                                                                                              \
        const Proj<OpsFp2> r = proj_add_w<OpsFp2, mode>(e, {ld2(a), ld2(a + 2), ld2(a + 4)}, {ld2(b), ld2(b + 2), ld2(b + 4)});  \
        st6(out, r.x, r.y, r.z);                                                                                                 \
    }
DEVCURVE_DEF_ADD(0)
DEVCURVE_DEF_ADD(1)
DEVCURVE_DEF_ADD(2)
#undef DEVCURVE_DEF_ADD
// the affine steps: p = a[0..3], q = b[0..3], the supplied inverse of the slope's denominator a[4..5]
BLSW_HD void st_aff(Fp* p, const Aff2& r) {
    st2(p, r.x);
    st2(p + 2, r.y);
}
DEVCURVE_DEF(nz_double_w) {
    (void)b, (void)park;
    st_aff(out, nz_double_w(e, {ld2(a), ld2(a + 2)}));
}
DEVCURVE_DEF(nz_add_unchecked_w) {
    (void)park;
    st_aff(out, nz_add_unchecked_w(e, {ld2(a), ld2(a + 2)}, {ld2(b), ld2(b + 2)}));
}
DEVCURVE_DEF(nz_double_pre_w) {
    (void)b, (void)park;
    st_aff(out, nz_double_pre_w(e, {ld2(a), ld2(a + 2)}, ld2(a + 4)));
}
DEVCURVE_DEF(nz_add_unchecked_pre_w) {
    (void)park;
    st_aff(out, nz_add_unchecked_pre_w(e, {ld2(a), ld2(a + 2)}, {ld2(b), ld2(b + 2)}, ld2(a + 4)));
}
DEVCURVE_DEF(nz_double_pre_inl) {
    (void)b, (void)park;
    st_aff(out, nz_double_pre_inl(e, {ld2(a), ld2(a + 2)}, ld2(a + 4)));
}
DEVCURVE_DEF(nz_add_unchecked_pre_inl) {
    (void)park;
    st_aff(out, nz_add_unchecked_pre_inl(e, {ld2(a), ld2(a + 2)}, {ld2(b), ld2(b + 2)}, ld2(a + 4)));
}

#undef DEVCURVE_DEF
#undef DEVCURVE_UNUSED

}  // namespace devcurve
