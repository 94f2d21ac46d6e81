"""Operands of the table of pairing programs (tests/devpair/ops.hpp), shared by the host test (test_pairing_ref.py) and the device test
(test_pairing_device_gpu.py). A case is (name, P, Q_sig, Q_h, kind): the programs compute the Miller value of the two pairs (-g1, Q_sig), (P, Q_h).
Points are built by the affine arithmetic of tests/curve_ref.py, never by the code under test, and travel as stored integers (Montgomery form).

Signature RELATIONS (Q_sig = [sk] Q_h, P = [sk] g1: the product of the two pairings is 1, or "something else" for the tampered one) and at least as
many NON-relations, whose product is a generic GT element: the cases in which twelve coefficients are compared instead of one bit. Most G2
operands are the small multiples of g2 on which pairing_ref.prove() has evaluated the reference already, so a case costs no new reference value
unless it is there for a seeded multiple."""
import random

from tests import curve_ref as C
from tests import field_ref as F
from tests.curve_ref import K1, K2, R_ORDER
from tests.field_edges import P
from tests.field_ref import enc
from tests.pairing_ref import NEG_G1
from tests.team_ref import G1_GEN, G2_GEN

ORDER3 = (0, 2)  # chain_edges.g1_operands(): "order 3: (0, 2)", the key with x = 0
KINDS = ("relation", "tampered", "generic", "off-subgroup")


def g1(k):
    return C.aff_mul(K1, k % R_ORDER, G1_GEN)


def g2(k):
    return C.aff_mul(K2, k % R_ORDER, G2_GEN)


def seeds():
    rng = random.Random(0x9A1C)
    return rng.randrange(2, R_ORDER), rng.randrange(2, R_ORDER)


def cases():
    """[(name, P, Q_sig, Q_h, kind)]"""
    def make():
        s, h = seeds()
        out = [
            ("sk = 1: sig = H = g2", g1(1), g2(1), g2(1), "relation"),
            ("sk = r - 1: pk = -g1, sig = -g2", g1(-1), g2(-1), g2(1), "relation"),
            ("valid: seeded sk and H", g1(s), g2(s * h), g2(h), "relation"),
            ("tampered: pk = [2]g1, H = [3]g2, sig = [7]g2", g1(2), g2(7), g2(3), "tampered"),
            ("generic: [2]g1, -g2, [2]g2", g1(2), g2(-1), g2(2), "generic"),
            ("generic: -g1, Q_h = Q_sig = [3]g2", g1(-1), g2(3), g2(3), "generic"),
            ("generic: [3]g1, [5]g2, -g2", g1(3), g2(5), g2(-1), "generic"),
            ("generic: g1, [2]g2, g2", g1(1), g2(2), g2(1), "generic"),
            ("order-3 key (0, 2), [12]g2, g2", ORDER3, g2(12), g2(1), "off-subgroup"),
        ]
        for name, p, qs, qh, _ in out:
            assert C.on_curve(K1, p) and C.on_curve(K2, qs) and C.on_curve(K2, qh) and None not in (p, qs, qh), name
        return out
    return F._memo("pairing_edges.cases", make)


def value_cases():
    """the cases of the value entries: the key off the subgroup is an operand of the witness entries only"""
    return [c for c in cases() if c[4] != "off-subgroup"]


def expected_gt(p, q_sig, q_h):
    """e_ref(-g1, Q_sig) e_ref(P, Q_h)"""
    from tests import pairing_ref as R
    return F.f12_mul(R.e_ref(NEG_G1, q_sig), R.e_ref(p, q_h))


# which cases' MEANING is checked where (every kind of operand has its meaning checked in one program at least; the bit-for-bit comparisons of the
# forms run on every case). The cut is the cost of the reference: one f12_pow per distinct Miller value.
WITNESS_MEANING = (0, 2, 8)
VALUES_MEANING = (1, 3, 4)
JACOBIAN_MEANING_CASE = 4


def multi_pool():
    """[(pk_j, Q_j)]: the pairs of the miller_multi items, a prefix of K of them per item; Q_sig of these items is [5]g2"""
    c = cases()
    return [(c[3][1], c[3][3]), (c[0][1], c[0][3]), (c[5][1], c[5][3]), (c[4][1], c[4][3]), (c[2][1], c[2][3])]


MULTI_K = (1, 2, 3, 5)
MULTI_MEANING_K = (2, 3, 5)  # K = 1 is miller, bit for bit
MULTI_QSIG = 5


def jacobian_zs():
    """Z of the Jacobian representatives (X, Y, Z) = (x Z^2, y Z^3, Z) of P for the three-multiplier lines: 1, 2, p - 1, a seeded value"""
    return [1, 2, P - 1, random.Random(0x7AC0).randrange(3, P - 1)]


def jacobian_multipliers(p, z):
    """(p0, px, py) = (Z^3, X Z, Y) of the representative with that Z (vpairing.hpp: the whole line times Z^3)"""
    x, y = p[0] * z * z % P, p[1] * z * z * z % P
    return (z * z * z % P, x * z % P, y)


# ---------------------------------------------------------------- stored operands
def st_g2(q):
    return F.e2(q[0]) + F.e2(q[1])


def st_g1(p):
    return [enc(p[0]), enc(p[1])]
