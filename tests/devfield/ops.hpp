// TEST HARNESS ONLY (never linked into libblsw.so): one table of the field and tower operations of csrc/fp.hpp, gadgets.hpp and tower.hpp, each
// as a function of two operand blocks. tests/hostsim/hostsim.cpp compiles it for the host (hostsim_field_op), tests/devfield/devfield.hip three
// times for the device (programs out of line, inlined, inlined on quads), one kernel per operation. An operation reads up to twelve elements of
// `a` and of `b`, writes its result elements to `out` and emits its witnesses through `e`; what it does not name it does not touch.
#pragma once
#include "tower.hpp"

namespace devfield {
using namespace blsw;

#define DEVFIELD_OUT_MAX 12  // result elements of an operation (an Fp12)
// X(name, result elements, witnesses): the witness count of every operation is independent of its operands
#define DEVFIELD_OPS(X)              \
    X(fp_add, 1, 0)                  \
    X(fp_sub, 1, 0)                  \
    X(fp_neg, 1, 0)                  \
    X(fp_dbl, 1, 0)                  \
    X(fp_mul, 1, 0)                  \
    X(fp_mul32, 1, 0)                \
    X(fp_sqr, 1, 0)                  \
    X(fp_inv, 1, 0)                  \
    X(fp_inv_fermat, 1, 0)           \
    X(fp_to_canonical, 1, 0)         \
    X(fp_from_u32, 1, 0)             \
    X(fp_is_eq_w, 1, 2)              \
    X(fp_to_bits_le_w, 1, 761)       \
    X(fp2_mul, 2, 0)                 \
    X(fp2_sqr, 2, 0)                 \
    X(fp2_mul_fp, 2, 0)              \
    X(fp2_mul_xi, 2, 0)              \
    X(fp2_inv, 2, 0)                 \
    X(fp2_inv2, 4, 0)                \
    X(fp2_mul_w, 2, 3)               \
    X(fp2_sqr_w, 2, 2)               \
    X(fp2_inv_w, 2, 3)               \
    X(fp2_div_w, 2, 3)               \
    X(fp2_is_eq_w, 1, 5)             \
    X(fp2_select_w, 2, 2)            \
    X(fp6_mul_w, 6, 18)              \
    X(fp6_mul_by_c0_c1_0_w, 6, 15)   \
    X(fp12_mul_by_014_w_yvar, 12, 36)  \
    X(fp12_mul_by_014_w_yconst, 12, 30) \
    X(fp12_sqr_w, 12, 36)            \
    X(fp12_mul_w, 12, 54)            \
    X(fp12_cyclotomic_square_w, 12, 18) \
    X(fp12_inv_w, 12, 54)            \
    X(fp12_frobenius_1, 12, 0)       \
    X(fp12_frobenius_2, 12, 0)       \
    X(fp12_frobenius_3, 12, 0)

enum OpId {
#define DEVFIELD_X_ENUM(name, n_out, n_wit) OP_##name,
    DEVFIELD_OPS(DEVFIELD_X_ENUM)
#undef DEVFIELD_X_ENUM
        OP_COUNT
};
inline int op_n_out(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVFIELD_X_OUT(name, n_out, n_wit) n_out,
        DEVFIELD_OPS(DEVFIELD_X_OUT)
#undef DEVFIELD_X_OUT
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}
inline int op_n_wit(int op) {
    constexpr int T[OP_COUNT] = {
#define DEVFIELD_X_WIT(name, n_out, n_wit) n_wit,
        DEVFIELD_OPS(DEVFIELD_X_WIT)
#undef DEVFIELD_X_WIT
    };
    return (op >= 0 && op < OP_COUNT) ? T[op] : -1;
}

BLSW_HD Fp2 ld2(const Fp* p) { return {p[0], p[1]}; }
BLSW_HD Fp6 ld6(const Fp* p) { return {ld2(p), ld2(p + 2), ld2(p + 4)}; }
BLSW_HD Fp12 ld12(const Fp* p) { return {ld6(p), ld6(p + 6)}; }
BLSW_HD void st2(Fp* p, const Fp2& v) {
    p[0] = v.c0;
    p[1] = v.c1;
}
BLSW_HD void st6(Fp* p, const Fp6& v) {
    st2(p, v.c0);
    st2(p + 2, v.c1);
    st2(p + 4, v.c2);
}
BLSW_HD void st12(Fp* p, const Fp12& v) {
    st6(p, v.c0);
    st6(p + 6, v.c1);
}
BLSW_HD Fp fp_of_bool(bool b) {  // a flag as a result element: the integer 0 or 1 in limb 0 (not Montgomery)
    Fp r = fp_zero();
    r.l[0] = b ? 1u : 0u;
    return r;
}

template <int OP>
struct FieldOp;
#define DEVFIELD_DEF(name)                                                           \
    template <>                                                                      \
    struct FieldOp<OP_##name> {                                                      \
        static BLSW_HD void run(const Fp* a, const Fp* b, Fp* out, Emitter& e);      \
    };                                                                               \
    BLSW_HD void FieldOp<OP_##name>::run(const Fp* a, const Fp* b, Fp* out, Emitter& e)
#define DEVFIELD_UNUSED (void)a, (void)b, (void)e

// ---- Fp
DEVFIELD_DEF(fp_add) { DEVFIELD_UNUSED, out[0] = fp_add(a[0], b[0]); }
DEVFIELD_DEF(fp_sub) { DEVFIELD_UNUSED, out[0] = fp_sub(a[0], b[0]); }
DEVFIELD_DEF(fp_neg) { DEVFIELD_UNUSED, out[0] = fp_neg(a[0]); }
DEVFIELD_DEF(fp_dbl) { DEVFIELD_UNUSED, out[0] = fp_dbl(a[0]); }
DEVFIELD_DEF(fp_mul) { DEVFIELD_UNUSED, out[0] = fp_mul(a[0], b[0]); }
DEVFIELD_DEF(fp_mul32) { DEVFIELD_UNUSED, out[0] = fp_mul32(a[0], b[0]); }
DEVFIELD_DEF(fp_sqr) { DEVFIELD_UNUSED, out[0] = fp_sqr(a[0]); }
DEVFIELD_DEF(fp_inv) { DEVFIELD_UNUSED, out[0] = fp_inv(a[0]); }
DEVFIELD_DEF(fp_inv_fermat) { DEVFIELD_UNUSED, out[0] = fp_inv_fermat(a[0]); }
DEVFIELD_DEF(fp_to_canonical) { DEVFIELD_UNUSED, out[0] = fp_to_canonical(a[0]); }
DEVFIELD_DEF(fp_from_u32) { DEVFIELD_UNUSED, out[0] = fp_from_u32(a[0].l[0]); }  // the integer is limb 0 of a[0]
DEVFIELD_DEF(fp_is_eq_w) { out[0] = fp_of_bool(fp_is_eq_w(e, a[0], b[0])); }
DEVFIELD_DEF(fp_to_bits_le_w) {
    (void)b;
    out[0] = fp_of_bool(fp_to_bits_le_w(e, a[0]));
}
// ---- Fp2
DEVFIELD_DEF(fp2_mul) { DEVFIELD_UNUSED, st2(out, fp2_mul(ld2(a), ld2(b))); }
DEVFIELD_DEF(fp2_sqr) { DEVFIELD_UNUSED, st2(out, fp2_sqr(ld2(a))); }
DEVFIELD_DEF(fp2_mul_fp) { DEVFIELD_UNUSED, st2(out, fp2_mul_fp(ld2(a), b[0])); }
DEVFIELD_DEF(fp2_mul_xi) { DEVFIELD_UNUSED, st2(out, fp2_mul_xi(ld2(a))); }
DEVFIELD_DEF(fp2_inv) { DEVFIELD_UNUSED, st2(out, fp2_inv(ld2(a))); }
DEVFIELD_DEF(fp2_inv2) {
    (void)e;
    Fp2 ai, bi;
    fp2_inv2(ld2(a), ld2(b), ai, bi);
    st2(out, ai);
    st2(out + 2, bi);
}
DEVFIELD_DEF(fp2_mul_w) { st2(out, fp2_mul_w(e, ld2(a), ld2(b))); }
DEVFIELD_DEF(fp2_sqr_w) {
    (void)b;
    st2(out, fp2_sqr_w(e, ld2(a)));
}
DEVFIELD_DEF(fp2_inv_w) {
    (void)b;
    st2(out, fp2_inv_w(e, ld2(a)));
}
DEVFIELD_DEF(fp2_div_w) { st2(out, fp2_div_w(e, ld2(a), ld2(b))); }
DEVFIELD_DEF(fp2_is_eq_w) { out[0] = fp_of_bool(fp2_is_eq_w(e, ld2(a), ld2(b))); }
DEVFIELD_DEF(fp2_select_w) { st2(out, fp2_select_w(e, (a[2].l[0] & 1u) != 0, ld2(a), ld2(b))); }  // the condition is bit 0 of a[2]
// ---- tower
DEVFIELD_DEF(fp6_mul_w) { st6(out, fp6_mul_w(e, ld6(a), ld6(b))); }
DEVFIELD_DEF(fp6_mul_by_c0_c1_0_w) { st6(out, fp6_mul_by_c0_c1_0_w(e, ld6(a), ld2(b), ld2(b + 2))); }
DEVFIELD_DEF(fp12_mul_by_014_w_yvar) { st12(out, fp12_mul_by_014_w<true>(e, ld12(a), ld2(b), ld2(b + 2), b[4])); }
DEVFIELD_DEF(fp12_mul_by_014_w_yconst) { st12(out, fp12_mul_by_014_w<false>(e, ld12(a), ld2(b), ld2(b + 2), b[4])); }
DEVFIELD_DEF(fp12_sqr_w) {
    (void)b;
    st12(out, fp12_sqr_w(e, ld12(a)));
}
DEVFIELD_DEF(fp12_mul_w) { st12(out, fp12_mul_w(e, ld12(a), ld12(b))); }
DEVFIELD_DEF(fp12_cyclotomic_square_w) {
    (void)b;
    st12(out, fp12_cyclotomic_square_w(e, ld12(a)));
}
DEVFIELD_DEF(fp12_inv_w) {
    (void)b;
    st12(out, fp12_inv_w(e, ld12(a)));
}
DEVFIELD_DEF(fp12_frobenius_1) { DEVFIELD_UNUSED, st12(out, fp12_frobenius<1>(ld12(a))); }
DEVFIELD_DEF(fp12_frobenius_2) { DEVFIELD_UNUSED, st12(out, fp12_frobenius<2>(ld12(a))); }
DEVFIELD_DEF(fp12_frobenius_3) { DEVFIELD_UNUSED, st12(out, fp12_frobenius<3>(ld12(a))); }

#undef DEVFIELD_DEF
#undef DEVFIELD_UNUSED

}  // namespace devfield
