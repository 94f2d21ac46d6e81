"""Keys and signatures off the prime-order subgroup for the witness chains (csrc/chains.hpp, prepare_vf.hpp, the kernels that run them), shared by
the host test (test_chain_edges.py) and the device test (test_chain_edges_gpu.py). The witness entry points take decoded points and make no
subgroup check, and the reference circuit accepts them too (its G2 prime-order check compares `ge` with itself), so these are inputs a caller can
submit. Points are built by the affine arithmetic of tests/curve_ref.py and curve_edges.curve_point, never by the code under test, and travel as
Montgomery limbs (x 2^384 mod p, little-endian u64); an all-zero pair is the identity, as everywhere in the library.

Which exceptional steps an operand meets is computed here from its order alone, by integer arithmetic on the prefixes of the two fixed scalars:
  * the prepare chain (G2PreparedVar::from_group_var) walks |x| = 0xd201000000010000 from below its top bit: double, and add q at a set bit.
    Its steps are affine with zero-hint inverses, so only the FIRST exceptional step is a statement about group elements: what follows is the
    circuit's arithmetic on a pair that is no curve point any more (prepare_reference restates exactly that).
  * the native [h1^-1 mod r] pk before the G1 allocation is a Jacobian double-and-add from pk: every step is a group operation, all events count.
"""
import random

import numpy as np

from tests import curve_edges as X
from tests import curve_ref as C
from tests import field_ref as F
from tests.curve_ref import K1, K2, R_ORDER, X_ABS
from tests.field_edges import P
from tests.field_ref import enc

_x = -X_ABS
H1 = (_x - 1) ** 2 // 3
H2 = (_x ** 8 - 4 * _x ** 7 + 5 * _x ** 6 - 4 * _x ** 4 + 6 * _x ** 3 - 4 * _x ** 2 - 4 * _x + 13) // 9
H1_INV = pow(H1, -1, R_ORDER)
H1_FACTORS = {3: 1, 11: 2, 10177: 2, 859267: 2, 52437899: 2}
H2_BIG = 402096035359507321594726366720466575392706800671181159425656785868777272553337714697862511267018014931937703598282857976535744623203249
H2_FACTORS = {13: 2, 23: 2, 2713: 1, 11953: 1, 262069: 1, H2_BIG: 1}

PREP_EVENTS = ("doubling of O", "addition r = q", "addition r = -q")
G1_EVENTS = ("acc = O", "acc = pk", "acc = -pk")


def _prod(f):
    out = 1
    for q, e in f.items():
        out *= q ** e
    return out


assert _prod(H1_FACTORS) == H1 and _prod(H2_FACTORS) == H2 and H1 * H1_INV % R_ORDER == 1


def exact_order(K, pt):
    """the order of a curve point, from the factorisation of the group order h r (the identity has order 1)"""
    fac = dict(H1_FACTORS if K is K1 else H2_FACTORS)
    fac[R_ORDER] = 1
    n = _prod(fac)
    assert C.aff_mul(K, n, pt) is None
    for q, e in fac.items():
        for _ in range(e):
            if C.aff_mul(K, n // q, pt) is None:
                n //= q
    return n


def prepare_events(n):
    """[(event, step)] the prepare chain meets on a point of order n: empty, or the one first event (see the module's docstring). The identity
    (n = 1) arrives as the pair (0, 0): its first doubling is the doubling of O."""
    acc, k = 1, 0
    for i in range(62, -1, -1):
        if acc % n == 0:
            return [("doubling of O", k)]
        acc, k = 2 * acc, k + 1
        if (X_ABS >> i) & 1:
            if acc % n == 1:
                return [("addition r = q", k)]
            if (acc + 1) % n == 0:
                return [("addition r = -q", k)]
            acc, k = acc + 1, k + 1
    return []


def g1_ladder_events(n):
    """({event: count}, (h1^-1 mod r) mod n) of the ladder acc = pk; per lower bit of h1^-1 mod r: acc = 2 acc; on a set bit acc += pk, for a key
    of order n > 1. "acc = O": the accumulator is the identity when a doubling or an addition reads it; "acc = pk" / "acc = -pk": at an addition."""
    acc, ev = 1, dict.fromkeys(G1_EVENTS, 0)
    for i in range(H1_INV.bit_length() - 2, -1, -1):
        ev["acc = O"] += acc % n == 0
        acc *= 2
        if (H1_INV >> i) & 1:
            ev["acc = O"] += acc % n == 0
            ev["acc = pk"] += acc % n == 1
            ev["acc = -pk"] += (acc + 1) % n == 0 and n > 2
            acc += 1
    assert acc == H1_INV
    return ev, acc % n


def small_divisors():
    """every divisor of h2 r below 2^64 + 2: the divisors of 13^2 23^2 2713 11953 262069 (r and the last prime factor of h2 exceed 2^64)"""
    divs = [1]
    for q, e in H2_FACTORS.items():
        if q != H2_BIG:
            divs = [d * q ** j for d in divs for j in range(e + 1)]
    assert min(R_ORDER, H2_BIG) > (1 << 64) + 2 and max(divs) < 1 << 64
    return sorted(divs)


def _torsion_of_order(K, d, rng, tries=8):
    """a point of exact order d (a prime with d^e the exact power in h): the d-primary part [r h / d^e] Q of a random Q, multiplied by d until
    the next multiple is O. (Both curves' small torsion may be non-cyclic, so [r h / d] Q alone can be O for every Q.)"""
    h = H1 if K is K1 else H2
    e = (H1_FACTORS if K is K1 else H2_FACTORS)[d]
    for _ in range(tries):
        pt = C.aff_mul(K, R_ORDER * h // d ** e, X.curve_point(K, rng))
        while pt is not None:
            nxt = C.aff_mul(K, d, pt)
            if nxt is None:
                return pt
            pt = nxt
    raise AssertionError("no point of order %d found" % d)


def g1_operands():
    """[(name, affine point or None, order)]"""
    def make():
        pts = X.points(K1)
        rng = random.Random(0xC4A1)
        out = [("identity", None)]
        out += [("subgroup[%d]" % i, q) for i, q in enumerate(pts["subgroup"])]  # G, 2G, 3G, 5G, [r - 1]G
        out += [("random", pts["random"][0]), ("[r]Q", pts["torsion"][0]), ("order 3: (0, 2)", (0, 2)), ("order 3: (0, p - 2)", (0, P - 2))]
        small = {}
        for d in (11, 10177):
            small[d] = _torsion_of_order(K1, d, rng)
            out.append(("order %d" % d, small[d]))
        out += [("subgroup + order 3", C.aff_add(K1, pts["subgroup"][2], (0, 2))), ("subgroup + order 11", C.aff_add(K1, pts["subgroup"][3], small[11]))]
        res = []
        for name, q in out:
            assert C.on_curve(K1, q), name
            res.append((name, q, exact_order(K1, q)))
        return res
    return F._memo("chain_edges_g1", make)


def g2_operands():
    """[(name, affine point or None, order)]. An order-169 point exists only if the 13-part of the twist's group is cyclic; the search below
    settles it for the points it tries and the host test asserts what it found."""
    def make():
        pts = X.points(K2)
        rng = random.Random(0xC4A2)
        out = [("identity", None)]
        out += [("subgroup[%d]" % i, q) for i, q in enumerate(pts["subgroup"])]
        out += [("random", pts["random"][0]), ("[r]Q", pts["torsion"][0])]
        small = {}
        for d in (13, 23):
            small[d] = _torsion_of_order(K2, d, rng)
            out += [("order %d" % d, small[d]), ("-(order %d)" % d, C.aff_neg(K2, small[d]))]
        for _ in range(4):  # [r h2 / 169] Q has order 1, 13 or 169
            q = C.aff_mul(K2, R_ORDER * H2 // 169, X.curve_point(K2, rng))
            if q is not None and C.aff_mul(K2, 13, q) is not None:
                out += [("order 169", q), ("-(order 169)", C.aff_neg(K2, q))]
                break
        out += [("subgroup + order 13", C.aff_add(K2, pts["subgroup"][2], small[13])), ("subgroup + order 23", C.aff_add(K2, pts["subgroup"][3], small[23]))]
        res = []
        for name, q in out:
            assert C.on_curve(K2, q), name
            res.append((name, q, exact_order(K2, q)))
        return res
    return F._memo("chain_edges_g2", make)


# ---------------------------------------------------------------- the encoder
def _limbs(v):
    return np.frombuffer(int(v).to_bytes(48, "little"), dtype=np.uint64)


def enc_g1(pt):
    """[12] uint64: x, y as Montgomery limbs; the identity is all zero"""
    if pt is None:
        return np.zeros(12, dtype=np.uint64)
    return np.concatenate([_limbs(enc(pt[0])), _limbs(enc(pt[1]))])


def enc_g2(pt):
    """[24] uint64: x.c0, x.c1, y.c0, y.c1"""
    if pt is None:
        return np.zeros(24, dtype=np.uint64)
    return np.concatenate([_limbs(enc(c)) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1])])


def el(row):
    """one stored witness element ([6] uint64) as an integer"""
    return int.from_bytes(np.ascontiguousarray(row, dtype=np.uint64).tobytes(), "little")


def els(rows):
    return [el(r) for r in rows]


# ---------------------------------------------------------------- the meaning tier of the three segments where these inputs bite
def _is_zero2_w(w, a):
    """Fp2Var::is_zero = is_eq(zero): per component [is_not_equal, multiplier], then the AND of the two"""
    e0, w0 = F.w_is_eq(0, a[0])  # zero.is_eq(a): the multiplier inverts 0 - a
    e1, w1 = F.w_is_eq(0, a[1])
    w += w0 + w1 + [F.w_bool(e0 and e1)]
    return e0 and e1


def _inv2_w(w, a):
    """QuadExtVar::inverse: the inverse (0 for 0) as a witness pair, then mul_equals' product a.c1 inv.c1"""
    i = F.f2_inv(a)
    w += F.e2(i) + [enc(a[1] * i[1])]
    return i


def prepare_reference(pt):
    """(1 096 stored witnesses, 272 stored coefficients) of G2PreparedVar::from_group_var on an affine point (None: the identity (0, 1, 0)), by
    SURVEY App. A.7 over Python integers: to_affine (is_zero(z), z^-1 or 0, z^-1 z, x z^-1, y z^-1, the two selects), then per bit of |x| below
    the top one a doubling step and, on a set bit, an addition step. A step's witnesses follow its statements: the inverse (3), then each
    product (3) or square (2) in the order A.7 writes them. An inverse of 0 is 0, so a degenerate step goes on with slope 0."""
    w, coeff = [], []
    x, y, z = ((0, 0), (1, 0), (0, 0)) if pt is None else (pt[0], pt[1], (1, 0))
    inf = _is_zero2_w(w, z)
    zi = F.f2_inv(z)
    w += F.e2(zi) + [enc(zi[1] * z[1])]
    nzx, nzy = K2.mul_w(w, x, zi), K2.mul_w(w, y, zi)
    q = ((0, 0) if inf else nzx, (0, 0) if inf else nzy)
    w += F.e2(q[0]) + F.e2(q[1])
    assert len(w) == 18
    rx, ry = q
    half = pow(2, -1, P)
    for i in range(62, -1, -1):
        a = _inv2_w(w, ry)  # double: a = 1 / r.y; b = r.x^2; b = b / 2 + b; c = a b; x3 = c^2 - 2 x; e = c x - y; y3 = e - c x3; pair (e, -c)
        b = K2.sqr_w(w, rx)
        b = F.f2_add(C.T.f2_scale(b, half), b)
        c = K2.mul_w(w, a, b)
        x3 = F.f2_sub(K2.sqr_w(w, c), C.T.f2_scale(rx, 2))
        e = F.f2_sub(K2.mul_w(w, c, rx), ry)
        y3 = F.f2_sub(e, K2.mul_w(w, c, x3))
        coeff += F.e2(e) + F.e2(F.f2_neg(c))
        rx, ry = x3, y3
        if (X_ABS >> i) & 1:
            a = _inv2_w(w, F.f2_sub(q[0], rx))  # add: a = 1 / (q.x - r.x); c = a (q.y - r.y); x3 = c^2 - (r.x + q.x); e = (r.x - x3) c; y3 = e - r.y; g = c r.x - r.y
            c = K2.mul_w(w, a, F.f2_sub(q[1], ry))
            x3 = F.f2_sub(K2.sqr_w(w, c), F.f2_add(rx, q[0]))
            e = K2.mul_w(w, F.f2_sub(rx, x3), c)
            g = F.f2_sub(K2.mul_w(w, c, rx), ry)
            coeff += F.e2(g) + F.e2(F.f2_neg(c))
            rx, ry = x3, F.f2_sub(e, ry)
    assert len(w) == 1096 and len(coeff) == 272
    return w, coeff


def prepare_coefficients_of(seg):
    """the 272 coefficients as the 1 096 stored witnesses of a prepare segment determine them: a product's witnesses (v0, v1, v2) give
    (v0 - v1, v2 - v0 - v1); a doubling's pair is (c x - y, -c) with y = (c x)' - (c x3)' of the step before, an addition's (c r.x - r.y, -c)"""
    d = lambda i: F.dec(seg[i])
    mul = lambda i: ((d(i) - d(i + 1)) % P, (d(i + 2) - d(i) - d(i + 1)) % P)
    ry = (d(16), d(17))
    coeff, pos = [], 18
    for i in range(62, -1, -1):
        c, cx, cx3 = mul(pos + 5), mul(pos + 10), mul(pos + 13)
        e = F.f2_sub(cx, ry)
        coeff += F.e2(e) + F.e2(F.f2_neg(c))
        ry = F.f2_sub(e, cx3)
        pos += 16
        if (X_ABS >> i) & 1:
            c, e, cr = mul(pos + 3), mul(pos + 8), mul(pos + 11)
            coeff += F.e2(F.f2_sub(cr, ry)) + F.e2(F.f2_neg(c))
            ry = F.f2_sub(e, ry)
            pos += 14
    assert pos == 1096
    return coeff


def proj_is(K, xyz, pt):
    """the homogeneous triple (canonical values) is the affine point pt (None: z = 0)"""
    if pt is None:
        return xyz[2] == K.zero
    return xyz[2] != K.zero and K.mul(pt[0], xyz[2]) == xyz[0] and K.mul(pt[1], xyz[2]) == xyz[1]
