"""What a Miller value IS: the textbook optimal-ate pairing on BLS12-381 in Python integers, on top of tests/field_ref.py and tests/curve_ref.py.
Nothing here restates csrc/ or oracle/: no prepared coefficients, no projective steps, no sparse products, no hard-part addition chain.

  E: y^2 = x^3 + 4 over Fp;  the twist E': y^2 = x^3 + 4 (1 + u) over Fp2;  Fp12 = Fp2[w] / (w^6 - (1 + u)).
  The untwist E' -> E(Fp12) is (x, y) -> (x / w^2, y / w^3). The line through T (slope s on the twist, s / w after the untwist) at P = (xP, yP):
      l = yP - (s / w) xP + (s xT - yT) / w^3.
  It is used multiplied by w^3: l w^3 = (s xT - yT) + (-s xP) w^2 + yP w^3, a dense Fp12 element multiplied with F.f12_mul.
  miller_ref: affine double-and-add on the twist over the bits of |x| = 0xd201000000010000 below the top one (f <- f^2 l_{T,T}(P), T <- 2 T; on
  a set bit f <- f l_{T,Q}(P), T <- T + Q); x < 0, so the inverse of f at the end. Vertical lines are left out.
  gt(f) = f^((p^12 - 1) / r), one plain f12_pow.

Every normalisation above is legitimate because gt kills any factor from a proper subfield of Fp12 ((p^k - 1) divides (p^12 - 1) / r for k = 1, 2,
4, 6): w^3 lies in Fp4 ((w^3)^2 = 1 + u), a vertical line x_P - x_T / w^2 in Fp6, and so do the Fp2 factors by which the code's projective lines
differ from these and the factor f^(p^6 + 1) between a final conjugation and a final inverse. So a comparison of MEANING is always
gt(code's Miller value) == gt-side expression of e_ref, both through this file's gt; never through the code's final exponentiation.

prove() is the reference's own proof (non-degeneracy, order r, bilinearity in both arguments, additivity in the second), run by the host test
before anything is compared with it. The reference is a function of arbitrary curve points whose line values are nonzero: a key off the subgroup
(the order-3 point (0, 2) of tests/chain_edges.py) is a legitimate first argument."""
from tests import curve_ref as C
from tests import field_ref as F
from tests.curve_ref import K1, K2, R_ORDER, X_ABS
from tests.field_edges import P
from tests.team_ref import G1_GEN, G2_GEN

GT_EXP = (P ** 12 - 1) // R_ORDER
assert GT_EXP * R_ORDER == P ** 12 - 1


def _w_poly(c0, c2, c3):
    """c0 + c2 w^2 + c3 w^3 as an Fp12 element: the coefficient of w^i is a[i % 2][i // 2] (field_ref.f12_frobenius)"""
    return ((c0, c2, F.F2_ZERO), (F.F2_ZERO, c3, F.F2_ZERO))


def line_steps(p, q):
    """the 68 lines of the walk, in order: [(doubling step?, l w^3 as (c0, c2, c3))], c0 = s xT - yT, c2 = -s xP, c3 = yP in Fp2"""
    assert C.on_curve(K1, p) and C.on_curve(K2, q) and p is not None and q is not None
    out, t = [], q
    for i in range(X_ABS.bit_length() - 2, -1, -1):
        assert t[1] != F.F2_ZERO, "the tangent at a point of order 2"
        s = F.f2_mul(C.T.f2_scale(F.f2_mul(t[0], t[0]), 3), F.f2_inv(C.T.f2_scale(t[1], 2)))
        out.append((True, (F.f2_sub(F.f2_mul(s, t[0]), t[1]), F.f2_neg(C.T.f2_scale(s, p[0])), (p[1] % P, 0))))
        t = C.aff_add(K2, t, t)
        if (X_ABS >> i) & 1:
            assert t is not None and t[0] != q[0], "the chord through t = +-q"
            s = F.f2_mul(F.f2_sub(t[1], q[1]), F.f2_inv(F.f2_sub(t[0], q[0])))
            out.append((False, (F.f2_sub(F.f2_mul(s, t[0]), t[1]), F.f2_neg(C.T.f2_scale(s, p[0])), (p[1] % P, 0))))
            t = C.aff_add(K2, t, q)
    return out


def miller_ref(p, q):
    """the Miller function f_{|x|, q}(p), inverted for x < 0. p: an affine point of E(Fp); q: an affine point of the twist; neither the identity"""
    f = F.F12_ONE
    for dbl, (c0, c2, c3) in line_steps(p, q):
        if dbl:
            f = F.f12_mul(f, f)
        f = F.f12_mul(f, _w_poly(c0, c2, c3))
    assert f != (F.F6_ZERO, F.F6_ZERO), "a line through p: the reference is not defined on this pair"
    return F.f12_inv(f)


def gt(f):
    """f^((p^12 - 1) / r), once per distinct value"""
    return F._memo(("pairing_ref.gt", f), lambda: F.f12_pow(f, GT_EXP))


def e_ref(p, q):
    return F._memo(("pairing_ref.e", p, q), lambda: gt(miller_ref(p, q)))


def product(values):
    out = F.F12_ONE
    for v in values:
        out = F.f12_mul(out, v)
    return out


def gt_of_block(block):
    """gt of a Miller value that travels as twelve stored integers"""
    return gt(F.d12(list(block)))


NEG_G1 = C.aff_neg(K1, G1_GEN)


def prove():
    """the properties that make e_ref a pairing, on the generators: a failure here means there is no reference to compare with"""
    def run():
        g1, g2 = G1_GEN, G2_GEN
        e = e_ref(g1, g2)
        assert e != F.F12_ONE, "e(g1, g2) = 1"
        assert F.f12_pow(e, R_ORDER) == F.F12_ONE, "e(g1, g2)^r != 1"
        for a, b in [(a, b) for a in (2, 3, R_ORDER - 1) for b in (2, 3, R_ORDER - 1)]:
            lhs = e_ref(C.aff_mul(K1, a, g1), C.aff_mul(K2, b, g2))
            assert lhs == F.f12_pow(e, a * b % R_ORDER), "e(%d g1, %d g2) != e(g1, g2)^(ab)" % (a, b)
        q1, q2 = C.aff_mul(K2, 5, g2), C.aff_mul(K2, 7, g2)
        p = NEG_G1
        assert e_ref(p, C.aff_add(K2, q1, q2)) == F.f12_mul(e_ref(p, q1), e_ref(p, q2)), "e(P, Q1 + Q2) != e(P, Q1) e(P, Q2)"
        return True
    return F._memo("pairing_ref.proved", run)
