"""A plain big-integer reference of the curve operation table of tests/devcurve/ops.hpp (csrc/decode.hpp, vcurve.hpp, curve.hpp, vsign.hpp,
vgroups.hpp). Python integers on top of tests/field_ref.py (Fp2, the witness layouts of the Fp2 gadgets) and the affine g2_add / g2_mul of
tests/team_ref.py. Two tiers; `reference` returns the tier-2 value after asserting that it has the tier-1 meaning, so an expected value that is
compared bit for bit has been held to both.

Tier 1, MEANING, independent of the formulas the code uses: affine chord-and-tangent arithmetic with None as the identity, pow(., -1, p) for
inverses, Euler's criterion and the norm map for "is a square", divmod for the digits, [k]P by an affine ladder for every scalar multiplication
([h_eff]P for v_clear_cofactor, [-|x|]P for v_psi on G2 points, [r]P is None for the subgroup tests), a straight RFC 9380 simplified SWU onto
y^2 = x^3 + 240u x + 1012(1 + u) with a generic Fp2 square root, and the 3-isogeny from this file's own copy of the published coefficients,
proven before use (prove_isogeny). Affine results and field elements are unique, so tier 1 fixes their bits.

Tier 2, BITS, for the results whose representative is a choice: dbl-2009-l, madd-2007-bl and add-2007-bl with the branch rules of the code's
comments, Renes-Costello-Batina for a = 0 in the order of proj_double_inl / proj_add_inl (the order fixes the witness stream), the affine slope
steps, the step programs of v_clear_cofactor, v_g2_mul_gls, v1_mul_g1_fixed, vg_scale_* and vg_sum over those formulas, and fp2_sqrt's algorithm
with its sign choice. Every stored element is a reduced residue, so a formula fixes the bits whatever the order of its field operations.

Conventions on degenerate inputs (each stated where the reference applies it):
  * fp_inv(0) = 0 makes vg_affine2 of the identity (0, 0) with a false flag (vgroups.hpp: "the inverse of 0 is 0"; k_vg_sum stores these zeros).
  * The Jacobian identity that an addition PRODUCES is (1, 1, 0); an identity operand of an addition returns the other operand unchanged.
  * A decode with the infinity flag is DEC_IDENTITY whatever the body (ark-bls12-381 0.4 read_g1_compressed returns zero before it reads x).
  * fp_sqrt returns a^((p + 1) / 4) also for a non-square; fp_from_be48, fp2_sqrt and g*_mul_affine leave their outputs alone on failure (the
    table presets them to zero), sk_from_le32 has read its words whatever the status.
Elements travel as stored integers (Montgomery form); an operation's expected value is (result elements, witness stream)."""
import random

from tests import field_ref as F
from tests import team_ref as T
from tests.field_edges import P
from tests.field_ref import dec, enc

X_ABS = T.X_ABS
R_ORDER = T.R_ORDER
G1_GEN, G2_GEN = T.G1_GEN, T.G2_GEN
H_EFF = 0xBC69F08F2EE75B3584C6A0EA91B352888E2A8E9145AD7689986FF031508FFE1329C2F178731DB956D82BF015D1212B02EC0EC69D7477C1AE954CBC06689F6A359894C0ADEBBF6B4E8020005AAA95551
DEC_OK, DEC_BAD_ENCODING, DEC_NOT_ON_CURVE, DEC_NOT_IN_SUBGROUP, DEC_IDENTITY = 0, 1, 2, 3, 4
SIGN_OK, SIGN_BAD_ENCODING, SIGN_INVALID_SECRET_KEY = 0, 1, 5


# ---------------------------------------------------------------- the two fields behind one interface (canonical integers / pairs of them)
class K1:
    zero, one, b = 0, 1, 4
    n = 1  # stored elements per field element
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    neg = staticmethod(lambda a: (-a) % P)
    inv = staticmethod(F.inv)
    scale = staticmethod(lambda a, k: a * k % P)
    mul3b = staticmethod(lambda a: a * 12 % P)
    k3b = 12
    st = staticmethod(lambda a: [enc(a)])
    ld = staticmethod(lambda s, i=0: dec(s[i]))

    @staticmethod
    def mul_w(w, a, b):  # fp_mul_w: the product
        w.append(enc(a * b))
        return a * b % P

    @staticmethod
    def sqr_w(w, a):  # OpsFp::sqr_w is fp_mul_w(a, a)
        return K1.mul_w(w, a, a)


class K2:
    zero, one, b = (0, 0), (1, 0), (4, 4)
    n = 2
    add, sub, mul, neg, inv = staticmethod(F.f2_add), staticmethod(F.f2_sub), staticmethod(F.f2_mul), staticmethod(F.f2_neg), staticmethod(F.f2_inv)
    scale = staticmethod(T.f2_scale)
    mul3b = staticmethod(lambda a: T.f2_scale(F.f2_mul(a, F.XI), 12))
    k3b = (12, 12)
    st = staticmethod(F.e2)
    ld = staticmethod(F.d2)

    @staticmethod
    def mul_w(w, x, y):  # fp2_mul_w (field_ref.reference: "fp2_mul_w")
        w += [enc(x[0] * y[0]), enc(x[1] * y[1]), enc((x[0] + x[1]) * (y[0] + y[1]))]
        return F.f2_mul(x, y)

    @staticmethod
    def sqr_w(w, x):  # fp2_sqr_w
        w += [enc(x[0] * x[1]), enc((x[0] - x[1]) * (x[0] + x[1]))]
        return F.f2_mul(x, x)


def f_sqr(K, a):
    return K.mul(a, a)


# ---------------------------------------------------------------- tier 1: affine arithmetic, None = the identity
def on_curve(K, pt, a=None, b=None):
    if pt is None:
        return True
    rhs = K.add(K.mul(f_sqr(K, pt[0]), pt[0]), K.b if b is None else b)
    if a is not None:
        rhs = K.add(rhs, K.mul(a, pt[0]))
    return f_sqr(K, pt[1]) == rhs


def aff_neg(K, pt):
    return None if pt is None else (pt[0], K.neg(pt[1]))


def aff_add(K, p, q, a=None):
    """the chord-and-tangent law on y^2 = x^3 + a x + b (a = 0 on the curves of the library)"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if K.add(p[1], q[1]) == K.zero:
            return None
        num = K.scale(f_sqr(K, p[0]), 3)
        if a is not None:
            num = K.add(num, a)
        lam = K.mul(num, K.inv(K.scale(p[1], 2)))
    else:
        lam = K.mul(K.sub(q[1], p[1]), K.inv(K.sub(q[0], p[0])))
    x3 = K.sub(K.sub(f_sqr(K, lam), p[0]), q[0])
    return (x3, K.sub(K.mul(lam, K.sub(p[0], x3)), p[1]))


def aff_mul(K, k, pt):
    if K is K2:
        return T.g2_mul(k, pt)  # the same law (team_ref.g2_add)
    acc = None
    while k:
        if k & 1:
            acc = aff_add(K, acc, pt)
        pt = aff_add(K, pt, pt)
        k >>= 1
    return acc


def jac_affine(K, j):
    """(X / Z^2, Y / Z^3); Z = 0 is the identity whatever X, Y"""
    if j[2] == K.zero:
        return None
    zi = K.inv(j[2])
    zi2 = f_sqr(K, zi)
    return (K.mul(j[0], zi2), K.mul(j[1], K.mul(zi2, zi)))


def proj_affine(K, h):
    if h[2] == K.zero:
        return None
    zi = K.inv(h[2])
    return (K.mul(h[0], zi), K.mul(h[1], zi))


def jac_rep(K, pt, lam):
    """the representative (l^2 x, l^3 y, l) of an affine point"""
    l2 = f_sqr(K, lam)
    return (K.mul(pt[0], l2), K.mul(pt[1], K.mul(l2, lam)), lam)


def fp_is_square(a):
    """Euler's criterion"""
    return a % P == 0 or pow(a, (P - 1) // 2, P) == 1


def fp2_is_square(a):
    """a is a square in Fp2 iff its norm is one in Fp"""
    return fp_is_square((a[0] * a[0] + a[1] * a[1]) % P)


def fp2_sqrt_generic(a):
    """a square root in Fp2 for p = 3 (mod 4) by Adj and Rodriguez-Henriquez' power method (eprint 2012/685 alg. 9), which shares nothing with the
    norm-and-halving method of decode.hpp's fp2_sqrt; None for a non-square"""
    if a == (0, 0):
        return (0, 0)
    a1 = F.f2_pow(a, (P - 3) // 4)
    x0 = F.f2_mul(a1, a)
    alpha = F.f2_mul(a1, x0)
    if F.f2_mul(F.f2_conj(alpha), alpha) == ((P - 1), 0):
        return None
    if alpha == (P - 1, 0):
        r = F.f2_mul((0, 1), x0)
    else:
        r = F.f2_mul(F.f2_pow(F.f2_add(F.F2_ONE, alpha), (P - 1) // 2), x0)
    assert F.f2_mul(r, r) == a
    return r


def lex_largest(K, a):
    """a > -a as canonical integers; over Fp2 c1 decides and c0 breaks the tie (ark-serialize's flag)"""
    if K is K1:
        return a > (P - a) % P
    if a[1] != (P - a[1]) % P:
        return a[1] > (P - a[1]) % P
    return a[0] > (P - a[0]) % P


def sgn0(a):
    """RFC 9380 4.1 for m = 2"""
    return bool((a[0] & 1) or (a[0] == 0 and (a[1] & 1)))


# ---------------------------------------------------------------- tier 2: the representative the code's formulas give
JAC_IDENTITY = lambda K: (K.one, K.one, K.zero)  # what an addition returns for P + (-P)


def jac_dbl(K, p):
    """dbl-2009-l, a = 0"""
    X, Y, Z = p
    A, B = f_sqr(K, X), f_sqr(K, Y)
    C = f_sqr(K, B)
    D = K.scale(K.sub(K.sub(f_sqr(K, K.add(X, B)), A), C), 2)
    Ee = K.scale(A, 3)
    x3 = K.sub(f_sqr(K, Ee), K.scale(D, 2))
    return (x3, K.sub(K.mul(Ee, K.sub(D, x3)), K.scale(C, 8)), K.scale(K.mul(Y, Z), 2))


def jac_add_mixed(K, p, q, branches=True):
    """madd-2007-bl -> (point, branch). With the branch rules of jac2_add_mixed / v_add_mixed: an identity p gives (qx, qy, 1), p = q the
    doubling of p, p = -q the identity (1, 1, 0). branches=False is jac1_add_mixed, which has none."""
    X, Y, Z = p
    if branches and Z == K.zero:
        return (q[0], q[1], K.one), "identity"
    z1z1 = f_sqr(K, Z)
    u2, s2 = K.mul(q[0], z1z1), K.mul(K.mul(q[1], Z), z1z1)
    h, rr = K.sub(u2, X), K.scale(K.sub(s2, Y), 2)
    if branches and h == K.zero:
        if rr == K.zero:
            return jac_dbl(K, p), "doubling"
        return JAC_IDENTITY(K), "cancelling"
    hh = f_sqr(K, h)
    i = K.scale(hh, 4)
    j, v = K.mul(h, i), K.mul(X, i)
    x3 = K.sub(K.sub(f_sqr(K, rr), j), K.scale(v, 2))
    y3 = K.sub(K.mul(rr, K.sub(v, x3)), K.scale(K.mul(Y, j), 2))
    z3 = K.sub(K.sub(f_sqr(K, K.add(Z, h)), z1z1), hh)
    return (x3, y3, z3), "general"


def jac_add(K, p, q):
    """add-2007-bl with v_add's rules: an identity operand returns the other operand as it is -> (point, branch)"""
    if p[2] == K.zero:
        return q, "identity"
    if q[2] == K.zero:
        return p, "identity"
    z1z1, z2z2 = f_sqr(K, p[2]), f_sqr(K, q[2])
    u1, u2 = K.mul(p[0], z2z2), K.mul(q[0], z1z1)
    s1, s2 = K.mul(K.mul(p[1], q[2]), z2z2), K.mul(K.mul(q[1], p[2]), z1z1)
    h, rr = K.sub(u2, u1), K.scale(K.sub(s2, s1), 2)
    if h == K.zero:
        if rr == K.zero:
            return jac_dbl(K, p), "doubling"
        return JAC_IDENTITY(K), "cancelling"
    i = f_sqr(K, K.scale(h, 2))
    j, v = K.mul(h, i), K.mul(u1, i)
    x3 = K.sub(K.sub(f_sqr(K, rr), j), K.scale(v, 2))
    y3 = K.sub(K.mul(rr, K.sub(v, x3)), K.scale(K.mul(s1, j), 2))
    z3 = K.mul(K.sub(K.sub(f_sqr(K, K.add(p[2], q[2])), z1z1), z2z2), h)
    return (x3, y3, z3), "general"


def jac_neg(K, p):
    return (p[0], K.neg(p[1]), p[2])


def proj_double(K, w, p):
    """Renes-Costello-Batina doubling for a = 0 in the order of proj_double_inl: 3 squarings and 8 products"""
    x, y, z = p
    xx, yy, zz = K.sqr_w(w, x), K.sqr_w(w, y), K.sqr_w(w, z)
    xy2 = K.scale(K.mul_w(w, x, y), 2)
    xz2 = K.scale(K.mul_w(w, x, z), 2)
    bzz3 = K.mul3b(zz)
    yy_m, yy_p = K.sub(yy, bzz3), K.add(yy, bzz3)
    y_frag = K.mul_w(w, yy_p, yy_m)
    x_frag = K.mul_w(w, yy_m, xy2)
    bxz3 = K.mul3b(xz2)
    xx3 = K.scale(xx, 3)
    t = K.mul_w(w, xx3, bxz3)
    yz2 = K.scale(K.mul_w(w, y, z), 2)
    t2 = K.mul_w(w, bxz3, yz2)
    z3 = K.scale(K.mul_w(w, yz2, yy), 4)
    return (K.sub(x_frag, t2), K.add(y_frag, t), z3)


def proj_add(K, w, mode, a, b):
    """Renes-Costello-Batina addition for a = 0 in the order of proj_add_inl. mode 0: both z variable; 1: b.z is the constant one (zz = a.z, no
    product); 2: both are (zz = 1, 3 b zz a constant)"""
    xx = K.mul_w(w, a[0], b[0])
    yy = K.mul_w(w, a[1], b[1])
    zz = K.mul_w(w, a[2], b[2]) if mode == 0 else (a[2] if mode == 1 else K.one)
    xy = K.sub(K.mul_w(w, K.add(a[0], a[1]), K.add(b[0], b[1])), K.add(xx, yy))
    xz = K.sub(K.mul_w(w, K.add(a[0], a[2]), K.add(b[0], b[2])), K.add(xx, zz))
    yz = K.sub(K.mul_w(w, K.add(a[1], a[2]), K.add(b[1], b[2])), K.add(yy, zz))
    bzz3 = K.k3b if mode == 2 else K.mul3b(zz)
    yy_m, yy_p = K.sub(yy, bzz3), K.add(yy, bzz3)
    xx3, bxz3 = K.scale(xx, 3), K.mul3b(xz)
    m0 = K.mul_w(w, yy_m, xy)
    m1 = K.mul_w(w, yz, bxz3)
    m2 = K.mul_w(w, yy_p, yy_m)
    m3 = K.mul_w(w, xx3, bxz3)
    m4 = K.mul_w(w, yy_p, yz)
    m5 = K.mul_w(w, xy, xx3)
    return (K.sub(m0, m1), K.add(m2, m3), K.add(m4, m5))


def _div_w(w, num, den, den_inv):
    """fp2_div_w / fp2_div_pre_w / fp2_div_pre_inl: r = num den^-1 (c0, c1), then r.c1 den.c1 (field_ref.reference: "fp2_div_w")"""
    r = F.f2_mul(num, F.f2_inv(den) if den_inv is None else den_inv)
    w += F.e2(r) + [enc(r[1] * den[1])]
    return r


def nz_double(w, p, den_inv=None):
    """NonZeroAffineVar::double: the tangent's slope as a quotient witness"""
    x1_sqr = K2.sqr_w(w, p[0])
    lam = _div_w(w, T.f2_scale(x1_sqr, 3), T.f2_scale(p[1], 2), den_inv)
    x3 = F.f2_sub(K2.sqr_w(w, lam), T.f2_scale(p[0], 2))
    return (x3, F.f2_sub(K2.mul_w(w, lam, F.f2_sub(p[0], x3)), p[1]))


def nz_add(w, p, q, den_inv=None):
    lam = _div_w(w, F.f2_sub(q[1], p[1]), F.f2_sub(q[0], p[0]), den_inv)
    x3 = F.f2_sub(F.f2_sub(K2.sqr_w(w, lam), p[0]), q[0])
    return (x3, F.f2_sub(K2.mul_w(w, lam, F.f2_sub(p[0], x3)), p[1]))


def fp_sqrt(a):
    """(a is a square, a^((p + 1) / 4))"""
    r = pow(a, (P + 1) // 4, P)
    return r * r % P == a % P, r


def fp2_sqrt(a):
    """decode.hpp's fp2_sqrt restated -> (flag, root or None, exit). The sign of the root is the algorithm's: the principal a^((p + 1) / 4) of the
    first delta that is a square, x1 = c1 / (2 x0)."""
    if a == (0, 0):
        return True, (0, 0), "zero"
    if a[1] == 0:
        ok, r = fp_sqrt(a[0])
        if ok:
            return True, (r, 0), "c1 = 0, c0 a square"
        ok, r = fp_sqrt((-a[0]) % P)
        assert ok  # -1 is a non-residue: one of c0, -c0 is a square
        return True, (0, r), "c1 = 0, c0 a non-square"
    ok, alpha = fp_sqrt((a[0] * a[0] + a[1] * a[1]) % P)
    if not ok:
        return False, None, "not a square"
    half = (P + 1) // 2
    ok, x0 = fp_sqrt((a[0] + alpha) * half % P)
    which = "first delta a square"
    if not ok:
        ok, x0 = fp_sqrt((a[0] - alpha) * half % P)
        which = "second delta a square"
        assert ok  # the two deltas multiply to -c1^2 / 4, a non-residue: exactly one is a square
    r = (x0, a[1] * F.inv(2 * x0) % P)
    assert F.f2_mul(r, r) == a
    return True, r, which


# psi = untwist-Frobenius-twist on y^2 = x^3 + 4(1 + u): (x, y) -> (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)); psi^2 = (x / 2^((p-1)/3), -y)
PSI_C1 = F.f2_inv(F.f2_pow(F.XI, (P - 1) // 3))
PSI_C2 = F.f2_inv(F.f2_pow(F.XI, (P - 1) // 2))
PSI2_C1 = F.inv(pow(2, (P - 1) // 3, P))


def jac_psi(p):
    return (F.f2_mul(F.f2_conj(p[0]), PSI_C1), F.f2_mul(F.f2_conj(p[1]), PSI_C2), F.f2_conj(p[2]))


def jac_psi2(p):
    return (T.f2_scale(p[0], PSI2_C1), F.f2_neg(p[1]), p[2])


def _ladder_x(K, base, add):
    """acc = [|x|] base by 63 doublings from base, additions at the set bits"""
    acc = base
    for i in range(62, -1, -1):
        acc = jac_dbl(K, acc)
        if (X_ABS >> i) & 1:
            acc = add(acc, base)
    return acc


def clear_cofactor_program(p):
    """v_clear_cofactor's step table over v_dbl / v_add: [x^2 - x - 1] P + [x - 1] psi(P) + psi^2(2 P), x = -|x| (Budroni-Pintore)"""
    add = lambda a, b: jac_add(K2, a, b)[0]
    t1 = jac_neg(K2, _ladder_x(K2, p, add))  # x P
    t2 = add(t1, jac_psi(p))  # x P + psi(P)
    t2 = jac_neg(K2, _ladder_x(K2, t2, add))  # x (x P + psi(P))
    acc = jac_psi2(jac_dbl(K2, p))
    acc = add(acc, jac_neg(K2, jac_psi(p)))
    acc = add(acc, t2)
    acc = add(acc, jac_neg(K2, t1))
    return add(acc, jac_neg(K2, p))


def digits_x(k):
    """k = d0 + d1 |x| + d2 |x|^2 + d3 |x|^3"""
    d = []
    for _ in range(3):
        k, r = divmod(k, X_ABS)
        d.append(r)
    return d + [k]


def g2_mul_gls_program(q, k):
    """v_g2_mul_gls: Straus over the bases q, |x| q = -psi(q), |x|^2 q = psi^2(q), |x|^3 q = -psi(psi^2(q)); the table entry of a subset is the
    entry of the subset without its lowest base plus that base; 64 steps of doubling and one table addition from (1, 1, 0)"""
    add = lambda a, b: jac_add(K2, a, b)[0]
    d = digits_x(k)
    tab = {1: q, 2: jac_neg(K2, jac_psi(q)), 4: jac_psi2(q)}
    tab[8] = jac_neg(K2, jac_psi(tab[4]))
    for s in range(3, 16):
        if s & (s - 1):
            low = s & -s
            tab[s] = add(tab[s ^ low], tab[low])
    acc = JAC_IDENTITY(K2)
    for i in range(63, -1, -1):
        acc = jac_dbl(K2, acc)
        idx = sum(((d[j] >> i) & 1) << j for j in range(4))
        if idx:
            acc = add(acc, tab[idx])
    return acc


def g1_window_table():
    """[w][d - 1] = d 16^w g1, affine, by tier-1 arithmetic (what csrc/g1_table.hpp is generated to hold)"""
    def make():
        tab, base = [], G1_GEN
        for _ in range(64):
            row, acc = [], None
            for _ in range(15):
                acc = aff_add(K1, acc, base)
                row.append(acc)
            tab.append(row)
            base = aff_add(K1, row[14], base)
        return tab
    return F._memo("curve_g1_table", make)


def mul_g1_fixed_program(k):
    acc = JAC_IDENTITY(K1)
    tab = g1_window_table()
    for w in range(64):
        dgt = (k >> (4 * w)) & 15
        if dgt:
            acc = jac_add_mixed(K1, acc, tab[w][dgt - 1])[0]
    return acc


def scale_program(K, pt, r):
    """vg_scale_*: double-and-add from the top set bit, from (1, 1, 0); r = 0 gives that identity"""
    acc, started = JAC_IDENTITY(K), False
    for i in range(63, -1, -1):
        if started:
            acc = jac_dbl(K, acc)
        if (r >> i) & 1:
            acc = jac_add_mixed(K, acc, pt)[0]
            started = True
    return acc


def sum_program(points):
    acc = JAC_IDENTITY(K2)
    for q in points:
        acc = jac_add(K2, acc, q)[0]
    return acc


# ---------------------------------------------------------------- hash-to-curve: RFC 9380 8.8.2, own copy of the published numbers
SSWU_A, SSWU_B, SSWU_Z = (0, 240), (1012, 1012), (P - 2, P - 1)
_H = lambda s: int(s, 16)
ISO_XNUM = [
    (_H("5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97d6"),) * 2,
    (0, _H("11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71a")),
    (_H("11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71e"),
     _H("8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38d")),
    (_H("171d6541fa38ccfaed6dea691f5fb614cb14b4e7f4e810aa22d6108f142b85757098e38d0f671c7188e2aaaaaaaa5ed1"), 0),
]
ISO_XDEN = [(0, P - 72), (12, P - 12), (1, 0)]
ISO_YNUM = [
    (_H("1530477c7ab4113b59a4c18b076d11930f7da5d4a07f649bf54439d87d27e500fc8c25ebf8c92f6812cfc71c71c6d706"),) * 2,
    (0, _H("5c759507e8e333ebb5b7a9a47d7ed8532c52d39fd3a042a88b58423c50ae15d5c2638e343d9c71c6238aaaaaaaa97be")),
    (_H("11560bf17baa99bc32126fced787c88f984f87adf7ae0c7f9a208c6b4f20a4181472aaa9cb8d555526a9ffffffffc71c"),
     _H("8ab05f8bdd54cde190937e76bc3e447cc27c3d6fbd7063fcd104635a790520c0a395554e5c6aaaa9354ffffffffe38f")),
    (_H("124c9ad43b6cf79bfbf7043de3811ad0761b0f37a1e26286b0e977c69aa274524e79097a56dc4bd9e1b371c71c718b10"), 0),
]
ISO_YDEN = [(P - 432, P - 432), (0, P - 216), (18, P - 18), (1, 0)]


def poly(k, x):
    """sum k[i] x^i by Horner's rule"""
    r = F.F2_ZERO
    for c in reversed(k):
        r = F.f2_add(F.f2_mul(r, x), c)
    return r


def iso_map(pt):
    x, y = pt
    return (F.f2_mul(poly(ISO_XNUM, x), F.f2_inv(poly(ISO_XDEN, x))), F.f2_mul(y, F.f2_mul(poly(ISO_YNUM, x), F.f2_inv(poly(ISO_YDEN, x)))))


def sswu_curve_point(rng):
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = fp2_sqrt_generic(F.f2_add(F.f2_add(F.f2_mul(F.f2_mul(x, x), x), F.f2_mul(SSWU_A, x)), SSWU_B))
        if y is not None:
            return (x, y)


def prove_isogeny(pairs=4):
    """the sixteen coefficients above are a homomorphism from the SSWU curve onto y^2 = x^3 + 4(1 + u): images of random points lie on that curve
    and the map is additive on random pairs (a rational map between the two curves with these properties is an isogeny; a typo in one coefficient
    breaks both)"""
    def prove():
        rng = random.Random(0x150)
        for _ in range(pairs):
            a, b = sswu_curve_point(rng), sswu_curve_point(rng)
            assert on_curve(K2, a, SSWU_A, SSWU_B) and on_curve(K2, b, SSWU_A, SSWU_B) and a[0] != b[0]
            ia, ib = iso_map(a), iso_map(b)
            assert on_curve(K2, ia) and on_curve(K2, ib)
            assert iso_map(aff_add(K2, a, b, SSWU_A)) == aff_add(K2, ia, ib)
            assert iso_map(aff_add(K2, a, a, SSWU_A)) == aff_add(K2, ia, ia)
        return True
    return F._memo("curve_iso_proven", prove)


def sswu(u):
    """RFC 9380 6.6.2, the straight-line statement with inversions -> (point of the SSWU curve, gx1 is a square)"""
    A, B, Z = SSWU_A, SSWU_B, SSWU_Z
    u2 = F.f2_mul(u, u)
    zu2 = F.f2_mul(Z, u2)
    tv1 = F.f2_inv(F.f2_add(F.f2_mul(zu2, zu2), zu2))  # inv0
    nba = F.f2_mul(F.f2_neg(B), F.f2_inv(A))
    x1 = F.f2_mul(B, F.f2_inv(F.f2_mul(Z, A))) if tv1 == F.F2_ZERO else F.f2_mul(nba, F.f2_add(F.F2_ONE, tv1))
    g = lambda x: F.f2_add(F.f2_add(F.f2_mul(F.f2_mul(x, x), x), F.f2_mul(A, x)), B)
    gx1 = g(x1)
    first = fp2_is_square(gx1)
    x = x1 if first else F.f2_mul(zu2, x1)
    y = fp2_sqrt_generic(g(x))
    assert y is not None
    if sgn0(u) != sgn0(y):
        y = F.f2_neg(y)
    return (x, y), first


def map_to_curve(u):
    assert prove_isogeny()
    pt, first = sswu(u)
    return iso_map(pt), first


C1_EXP = (P * P - 9) // 16


# ---------------------------------------------------------------- bytes
def be48(x, flags=0):
    return bytes([(x >> 376) & 0xFF | flags]) + (x & ((1 << 376) - 1)).to_bytes(47, "big")


def g1_compress(pt, sort=None):
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    s = lex_largest(K1, pt[1]) if sort is None else sort
    return be48(pt[0], 0x80 | (0x20 if s else 0))


def g2_compress(pt, sort=None):
    if pt is None:
        return bytes([0xC0]) + bytes(95)
    s = lex_largest(K2, pt[1]) if sort is None else sort
    return be48(pt[0][1], 0x80 | (0x20 if s else 0)) + be48(pt[0][0])


def decode(kind, data):
    """(status, x, y) of a compressed record, from the bytes by the rules of ark-bls12-381 0.4 (curves/util.rs) and the definition of the
    subgroup: flags, x < p per component (the first 48 bytes masked with 0x1f, the second 48 of a G2 record with nothing: its top bits must be
    clear for it to be below p), a square right-hand side, the y the sort flag names, [r]P = O"""
    K = K1 if kind == "g1" else K2
    c, inf, sort = data[0] >> 7, (data[0] >> 6) & 1, (data[0] >> 5) & 1
    zero = (K.zero, K.zero)
    if not c or (sort and inf):
        return (DEC_BAD_ENCODING,) + zero
    if inf:
        return (DEC_IDENTITY,) + zero
    first = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:48], "big")
    if first >= P:
        return (DEC_BAD_ENCODING,) + zero
    if kind == "g1":
        x = first
        ok, y = fp_sqrt((x * x * x + 4) % P)
        y = y if ok else None
    else:
        second = int.from_bytes(data[48:96], "big")
        if second >= P:
            return (DEC_BAD_ENCODING,) + zero
        x = (second, first)
        y = fp2_sqrt_generic(F.f2_add(F.f2_mul(F.f2_mul(x, x), x), K2.b))
    if y is None:
        return (DEC_NOT_ON_CURVE,) + zero
    if lex_largest(K, y) != bool(sort):
        y = K.neg(y)
    if aff_mul(K, R_ORDER, (x, y)) is not None:
        return (DEC_NOT_IN_SUBGROUP,) + zero
    return (DEC_OK, x, y)


# ---------------------------------------------------------------- the table
# name -> (result elements, witnesses, in the quad build), in the order of DEVCURVE_OPS. The witness counts of the curve.hpp programs are formed
# below from the field table's (WITNESS_COUNTS) and asserted against this column and the compiled one by the test.
OPS = {
    "fp_from_be48_1f": (2, 0, 0), "fp_from_be48_ff": (2, 0, 0), "fp_sqrt": (2, 0, 0), "fp2_sqrt": (3, 0, 0), "fp_lex_largest": (1, 0, 0),
    "fp2_lex_largest": (1, 0, 0), "g1_decode": (3, 0, 0), "g2_decode": (5, 0, 0), "g1_encode": (1, 0, 0), "g2_encode": (2, 0, 0),
    "sk_from_le32": (2, 0, 0), "g1_in_subgroup": (1, 0, 0), "g2_in_subgroup": (1, 0, 0), "g1_in_subgroup_ladder": (1, 0, 0),
    "g2_in_subgroup_ladder": (1, 0, 0),
    "jac1_dbl": (3, 0, 1), "jac1_add_mixed": (3, 0, 1), "jac1v_dbl": (3, 0, 0), "jac1v_add_mixed": (3, 0, 0), "jac2_dbl": (6, 0, 0),
    "jac2_add_mixed": (6, 0, 0), "v1_dbl": (3, 0, 0), "v1_add_mixed": (3, 0, 0), "v_sqr": (2, 0, 1), "v_dbl": (6, 0, 1), "v_dbl_inplace": (6, 0, 1),
    "v_add_mixed": (6, 0, 1), "v_add": (6, 0, 1), "v_neg": (6, 0, 0), "v_psi": (6, 0, 0), "v_psi2": (6, 0, 0), "g1_mul_affine": (3, 0, 0),
    "g2_mul_affine": (5, 0, 0),
    "v_pow_c1": (2, 0, 0), "v_sgn0": (1, 0, 0), "v_poly": (2, 0, 0), "v_map_to_curve": (6, 0, 0), "v_clear_cofactor": (6, 0, 0), "v_digits_x": (4, 0, 0),
    "v_g2_mul_gls": (6, 0, 0), "v1_mul_g1_fixed": (3, 0, 0), "vg_scale_g1": (3, 0, 0), "vg_scale_g2": (6, 0, 0), "vg_sum2": (6, 0, 0),
    "vg_sum3": (6, 0, 0), "vg_affine2": (5, 0, 1), "vg_line_multipliers": (3, 0, 0),
    "proj_double_w_fp": (3, 11, 1), "proj_double_w_fp2": (6, 30, 1), "proj_add_w_fp_z0": (3, 12, 1), "proj_add_w_fp_z1": (3, 11, 1),
    "proj_add_w_fp_z2": (3, 11, 1), "proj_add_w_fp2_z0": (6, 36, 1), "proj_add_w_fp2_z1": (6, 33, 1), "proj_add_w_fp2_z2": (6, 33, 1),
    "nz_double_w": (4, 10, 1), "nz_add_unchecked_w": (4, 8, 1), "nz_double_pre_w": (4, 10, 1), "nz_add_unchecked_pre_w": (4, 8, 1),
    "nz_double_pre_inl": (4, 10, 1), "nz_add_unchecked_pre_inl": (4, 8, 1),
}
OP_NAMES = list(OPS)
PARK_OPS = ("v_clear_cofactor", "v_g2_mul_gls")
ADDITIONS = ("jac1v_add_mixed", "jac2_add_mixed", "v1_add_mixed", "v_add_mixed", "v_add")  # the additions with the four branches


def witness_counts():
    """the witness counts of the curve.hpp programs, formed from the field table's counts (fp_mul_w 1; fp2_mul_w, fp2_sqr_w, fp2_div_w from
    field_ref.OPS) and the products each program makes"""
    mul = {K1: 1, K2: F.OPS["fp2_mul_w"][1]}
    sqr = {K1: 1, K2: F.OPS["fp2_sqr_w"][1]}  # OpsFp::sqr_w is a product
    div = F.OPS["fp2_div_w"][1]
    out = {}
    for K, tag in ((K1, "fp"), (K2, "fp2")):
        out["proj_double_w_" + tag] = 3 * sqr[K] + 8 * mul[K]
        out["proj_add_w_%s_z0" % tag] = 12 * mul[K]
        out["proj_add_w_%s_z1" % tag] = out["proj_add_w_%s_z2" % tag] = 11 * mul[K]
    for sfx in ("_w", "_pre_w", "_pre_inl"):
        out["nz_double" + sfx] = 2 * sqr[K2] + div + mul[K2]
        out["nz_add_unchecked" + sfx] = div + sqr[K2] + mul[K2]
    return out


def _rec(block, n):
    """the first n bytes of an operand block (slots hold their 48 little-endian bytes)"""
    return b"".join(x.to_bytes(48, "little") for x in block[:(n + 47) // 48])[:n]


def _slots(data):
    return [int.from_bytes(data[i:i + 48], "little") for i in range(0, len(data), 48)]


def _st(K, xs):
    return [s for x in xs for s in K.st(x)]


def _ldn(K, blk, count, at=0):
    return tuple(K.ld(blk, at + K.n * i) for i in range(count))


def reference(op, a, b):
    """(result elements, witness stream, branch label or None) of operation `op` on the operand blocks a, b (twelve stored integers each). The
    branch label names the path the REFERENCE says the operation takes (coverage conditions, the per-branch launches)."""
    K = K1 if op.startswith(("jac1", "v1_", "g1_", "fp_", "vg_scale_g1", "vg_line")) or op.endswith("_fp") or "_fp_z" in op else K2
    if op in ("fp_from_be48_1f", "fp_from_be48_ff"):
        raw = _rec(a, 48)
        v = int.from_bytes(bytes([raw[0] & (0x1F if op.endswith("1f") else 0xFF)]) + raw[1:], "big")
        return ([1, enc(v)] if v < P else [0, 0]), [], "below p" if v < P else "not below p"
    if op == "fp_sqrt":
        ok, r = fp_sqrt(dec(a[0]))
        assert ok == fp_is_square(dec(a[0]))
        return [int(ok), enc(r)], [], "square" if ok else "non-square"
    if op == "fp2_sqrt":
        x = F.d2(a)
        ok, r, which = fp2_sqrt(x)
        assert ok == fp2_is_square(x) == (fp2_sqrt_generic(x) is not None)
        return [int(ok)] + F.e2(r if ok else (0, 0)), [], which
    if op == "fp_lex_largest":
        v = dec(a[0])
        assert lex_largest(K1, v) == (v > (P - 1) // 2)
        return [int(lex_largest(K1, v))], [], None
    if op == "fp2_lex_largest":
        return [int(lex_largest(K2, F.d2(a)))], [], None
    if op in ("g1_decode", "g2_decode"):
        st, x, y = decode(op[:2], _rec(a, 48 * K.n))
        return [st] + _st(K, [x, y]), [], "status %d" % st
    if op in ("g1_encode", "g2_encode"):
        pt = None if a[2 * K.n] & 1 else _ldn(K, a, 2)
        return _slots((g1_compress if K is K1 else g2_compress)(pt)), [], None
    if op == "sk_from_le32":
        v = int.from_bytes(_rec(a, 32), "little")
        st = SIGN_BAD_ENCODING if v >= R_ORDER else (SIGN_INVALID_SECRET_KEY if v == 0 else SIGN_OK)
        return [st, v], [], "status %d" % st
    if op.endswith(("_in_subgroup", "_in_subgroup_ladder")):
        pt = _ldn(K, a, 2)
        assert on_curve(K, pt)
        inside = aff_mul(K, R_ORDER, pt) is None
        return [int(inside)], [], subgroup_exit(K, pt) if op.endswith("_in_subgroup") else ("inside" if inside else "outside")
    if op in ("jac1_dbl", "jac1v_dbl", "jac2_dbl", "v1_dbl", "v_dbl", "v_dbl_inplace"):
        p = _ldn(K, a, 3)
        r = jac_dbl(K, p)
        want = jac_affine(K, p)
        assert jac_affine(K, r) == aff_add(K, want, want)
        return _st(K, r), [], None
    if op in ("jac1_add_mixed",) + ADDITIONS:
        p, q = _ldn(K, a, 3), _ldn(K, b, 3 if op == "v_add" else 2)
        r, branch = jac_add(K, p, q) if op == "v_add" else jac_add_mixed(K, p, q, op != "jac1_add_mixed")
        assert jac_affine(K, r) == aff_add(K, jac_affine(K, p), jac_affine(K, q) if op == "v_add" else q), (op, branch)
        return _st(K, r), [], branch
    if op == "v_sqr":
        x = F.d2(a)
        return F.e2(F.f2_mul(x, x)), [], None
    if op in ("v_neg", "v_psi", "v_psi2"):
        p = _ldn(K2, a, 3)
        r = {"v_neg": lambda: jac_neg(K2, p), "v_psi": lambda: jac_psi(p), "v_psi2": lambda: jac_psi2(p)}[op]()
        pt = jac_affine(K2, p)
        assert on_curve(K2, jac_affine(K2, r))
        if op == "v_neg":
            assert jac_affine(K2, r) == aff_neg(K2, pt)
        elif _in_g2(pt):  # on the subgroup psi is multiplication by x = -|x| (off it, it is only an endomorphism: checked by the test)
            assert jac_affine(K2, r) == aff_mul(K2, (R_ORDER - X_ABS if op == "v_psi" else X_ABS * X_ABS) % R_ORDER, pt)
        return _st(K2, r), [], None
    if op in ("g1_mul_affine", "g2_mul_affine"):
        pt, k = _ldn(K, a, 2), b[0] & ((1 << 256) - 1)
        assert k < (1 << 255)
        r = aff_mul(K, k, pt)
        return [int(r is not None)] + _st(K, r if r is not None else (K.zero, K.zero)), [], "identity" if r is None else "point"
    if op == "v_pow_c1":
        return F.e2(F.f2_pow(F.d2(a), C1_EXP)), [], None
    if op == "v_sgn0":
        return [int(sgn0(F.d2(a)))], [], None
    if op == "v_poly":
        n = min(max(b[0] & 0xFFFFFFFF, 1), 5)
        return F.e2(poly([F.d2(a, 2 + 2 * i) for i in range(n)], F.d2(a))), [], None
    if op == "v_map_to_curve":
        u = F.d2(a)
        pt, first = map_to_curve(u)
        assert on_curve(K2, pt)
        if u != F.F2_ZERO:  # the map is odd: sgn0(-u) != sgn0(u) picks the other root
            assert map_to_curve(F.f2_neg(u))[0] == aff_neg(K2, pt)
        return _st(K2, [pt[0], pt[1], K2.one]), [], "gx1 a square" if first else "gx1 a non-square"
    if op == "v_clear_cofactor":
        p = _ldn(K2, a, 3)
        r = clear_cofactor_program(p)
        assert jac_affine(K2, r) == aff_mul(K2, H_EFF, jac_affine(K2, p))
        return _st(K2, r), [], None
    if op == "v_digits_x":
        k = a[0] & ((1 << 256) - 1)
        d = digits_x(k)
        assert k < X_ABS ** 4 and all(x < X_ABS for x in d) and sum(x * X_ABS ** i for i, x in enumerate(d)) == k
        return d, [], None
    if op == "v_g2_mul_gls":
        q, k = _ldn(K2, a, 3), b[0] & ((1 << 256) - 1)
        r = g2_mul_gls_program(q, k)
        assert _in_g2(jac_affine(K2, q)) and jac_affine(K2, r) == aff_mul(K2, k, jac_affine(K2, q))
        return _st(K2, r), [], None
    if op == "v1_mul_g1_fixed":
        k = a[0] & ((1 << 256) - 1)
        r = mul_g1_fixed_program(k)
        assert jac_affine(K1, r) == aff_mul(K1, k % R_ORDER, G1_GEN)
        return _st(K1, r), [], None
    if op in ("vg_scale_g1", "vg_scale_g2"):
        pt, k = _ldn(K, a, 2), b[0] & ((1 << 64) - 1)
        r = scale_program(K, pt, k)
        assert jac_affine(K, r) == aff_mul(K, k, pt)
        return _st(K, r), [], None
    if op in ("vg_sum2", "vg_sum3"):
        pts = [_ldn(K2, a, 3)] + ([_ldn(K2, a, 3, 6)] if op == "vg_sum3" else []) + [_ldn(K2, b, 3)]
        r = sum_program(pts)
        want = None
        for q in pts:
            want = aff_add(K2, want, jac_affine(K2, q))
        assert jac_affine(K2, r) == want
        return _st(K2, r), [], "identity sum" if want is None else "point"
    if op == "vg_affine2":
        pt = jac_affine(K2, _ldn(K2, a, 3))
        return [int(pt is not None)] + _st(K2, pt if pt is not None else (K2.zero, K2.zero)), [], "identity" if pt is None else "point"
    if op == "vg_line_multipliers":
        x, y, z = _ldn(K1, a, 3)
        m = (pow(z, 3, P), x * z % P, y)
        pt = jac_affine(K1, (x, y, z))
        assert pt is None or (m[1], m[2]) == (pt[0] * m[0] % P, pt[1] * m[0] % P)  # Z^3 (1, x, y)
        return _st(K1, m), [], None
    if op.startswith("proj_double_w"):
        w = []
        p = _ldn(K, a, 3)
        r = proj_double(K, w, p)
        want = proj_affine(K, p)
        assert proj_affine(K, r) == aff_add(K, want, want)
        return _st(K, r), w, None
    if op.startswith("proj_add_w"):
        w = []
        p, q, mode = _ldn(K, a, 3), _ldn(K, b, 3), int(op[-1])
        r = proj_add(K, w, mode, p, q)
        if not ((mode < 1 or q[2] == K.one) and (mode < 2 or p[2] == K.one)):
            return _st(K, r), w, "off contract"  # a z the mode takes for the constant one is not: the formula alone (it tells the modes apart)
        pa, qa = proj_affine(K, p), proj_affine(K, q)
        want = aff_add(K, pa, qa)
        assert proj_affine(K, r) == want
        branch = "identity" if pa is None or qa is None else ("cancelling" if want is None else ("doubling" if pa == qa else "general"))
        return _st(K, r), w, branch
    if op.startswith("nz_double"):
        w = []
        p = _ldn(K2, a, 2)
        r = nz_double(w, p, None if op == "nz_double_w" else F.d2(a, 4))
        if on_curve(K2, p):  # off the curve the step is only its formula
            assert r == aff_add(K2, p, p)
        return _st(K2, r), w, None
    if op.startswith("nz_add_unchecked"):
        w = []
        p, q = _ldn(K2, a, 2), _ldn(K2, b, 2)
        r = nz_add(w, p, q, None if op == "nz_add_unchecked_w" else F.d2(a, 4))
        if on_curve(K2, p) and on_curve(K2, q):
            assert r == aff_add(K2, p, q)
        return _st(K2, r), w, None
    raise KeyError(op)


def _in_g2(pt):
    return F._memo(("curve_in_g2", pt), lambda: pt is not None and on_curve(K2, pt) and T.g2_mul(R_ORDER, pt) is None)


def subgroup_exit(K, pt):
    """the exit of g1_in_subgroup / g2_in_subgroup that the point takes, from multiples computed by the affine ladder"""
    t = aff_mul(K, X_ABS, pt)
    if t is None:
        return "[|x|]P = O"
    if K is K2:
        return "psi(P) = [x]P" if aff_mul(K, R_ORDER, pt) is None else "psi(P) != [x]P"
    if t[0] == pt[0]:
        return "[|x|]P = +-P"
    if aff_mul(K, X_ABS, t) is None:
        return "[x^2]P = O"
    return "phi(P) = -[x^2]P" if aff_mul(K, R_ORDER, pt) is None else "phi(P) != -[x^2]P"


def expected(op, items):
    """[(results, stream, branch)] per item, computed once per distinct operand pair"""
    memo = F._CACHE.setdefault(("curve_expected", op), {})
    out = []
    for a, b in items:
        if (a, b) not in memo:
            res, w, branch = reference(op, a, b)
            assert len(res) == OPS[op][0] and len(w) == OPS[op][1], (op, len(res), len(w))
            memo[(a, b)] = (res, w, branch)
        out.append(memo[(a, b)])
    return out
