"""A plain big-integer reference of the team operation table of tests/devteam/ops.hpp (csrc/team.hpp, team_tables.hpp, the team parts of
vpairing.hpp), and the table's test cases. Python integers on top of tests/field_ref.py.

An item is three operand blocks (a, b, c) of twelve stored integers: a, b an Fp12 (a G2 point: x, y, z in the first six), c line coefficients and
a G1 point. An entry's expected value is (six Fp2 coefficients as twelve stored integers, witness stream). VALUES are computed here, independently
of the code under test: dense products of embedded sparse elements for every ell, f12_inv, the Frobenius maps, f12_pow for exp_by_x and for the
verdict of the final exponentiation, the is_one flags from w_is_eq. The G2 entries are held to the GROUP LAW instead of a restated formula
(g2_law_holds: the result is projectively the affine sum of on-curve operands built from the generator); their bits, like every Fp12 witness
stream, are the single-lane host form's (devteam_lib.expected), which the oracle parity tests pin to the circuit."""
import random

from tests import field_edges as E
from tests import field_ref as F
from tests.field_edges import ONE, P

X_ABS = 0xD201000000010000
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_GEN = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
          0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2_GEN = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
           0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
          (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
           0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))
B2 = (4, 4)  # the twist: y^2 = x^3 + 4 (1 + u)
IS_ONE_WITNESSES = 35

# name -> (has an exec and an exec_hot kernel, runs on the G2 slot file), in the order of DEVTEAM_OPS; the witness counts are the compiled table's
OPS = {
    "MUL": (1, 0), "SQR": (1, 0), "CYC": (1, 0), "ELLC": (1, 0), "ELLV": (1, 0), "ELLGS": (1, 0), "ELLGH": (1, 0), "G2DBL": (1, 1), "G2ADD": (1, 1),
    "inverse_w": (0, 0), "is_one_w": (0, 0), "conj": (0, 0), "frob_1": (0, 0), "frob_2": (0, 0), "frob_3": (0, 0), "first_f": (0, 0),
    "first_f_var": (0, 0), "exp_by_x": (0, 0), "final_exp_is_one": (0, 0), "seq": (1, 0),
}
OP_NAMES = list(OPS)
G2_OPS = ("G2DBL", "G2ADD")
VERDICT_OPS = ("is_one_w", "final_exp_is_one")
ITEM_COUNTS = (1, 9, 10, 11, 19, 20, 21, 60, 64, 100)  # a one-team wave, full waves, one team spilling into a new wave (ten teams per wave)
LONG_OPS = ("exp_by_x", "final_exp_is_one")  # hundreds to thousands of table passes per item: cut in item count, not in kinds of operand
LONG_ITEM_COUNTS = (1, 9, 10, 11, 19, 20, 21)
TEAMS = 10


# ---------------------------------------------------------------- values
def sparse_014(c0, c1, c4):
    return ((c0, c1, F.F2_ZERO), (F.F2_ZERO, c4, F.F2_ZERO))


def f2_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def line_const_p(c, k=0):
    """the factor of ell for the pair (-g1, sig): (c0, c1 g1.x, (-g1.y, 0))"""
    return sparse_014(F.d2(c, 4 * k), f2_scale(F.d2(c, 4 * k + 2), G1_GEN[0]), ((-G1_GEN[1]) % P, 0))


def line_var_p(c, px, py, k=0):
    return sparse_014(F.d2(c, 4 * k), f2_scale(F.d2(c, 4 * k + 2), px), (py, 0))


def f12_cyc_formula(a):
    """fp12_cyclotomic_square_w's map on ANY element (the square only on the cyclotomic subgroup): with the three Fp4 squares
    (za + zb s)^2 = (za^2 + xi zb^2) + (2 za zb) s of (z0, z1), (z2, z3), (z4, z5) it is 3 t - 2 z on the even parts and 3 t + 2 z on the odd ones"""
    z0, z4, z3 = a[0]
    z2, z1, z5 = a[1]

    def fp4_sqr(za, zb):
        return F.f2_add(F.f2_mul(za, za), F.f2_mul(F.XI, F.f2_mul(zb, zb))), f2_scale(F.f2_mul(za, zb), 2)

    t0, t1 = fp4_sqr(z0, z1)
    t2, t3 = fp4_sqr(z2, z3)
    t4, t5 = fp4_sqr(z4, z5)
    m = lambda t, z: F.f2_sub(f2_scale(t, 3), f2_scale(z, 2))
    p = lambda t, z: F.f2_add(f2_scale(t, 3), f2_scale(z, 2))
    return ((m(t0, z0), m(t2, z4), m(t4, z3)), (p(F.f2_mul(F.XI, t5), z2), p(t1, z1), p(t3, z5)))


def is_cyclotomic(a):
    """a^(p^4 - p^2 + 1) = 1, as a^(p^4) a = a^(p^2)"""
    return a != (F.F6_ZERO, F.F6_ZERO) and F.f12_mul(F.f12_frobenius(F.f12_frobenius(a, 2), 2), a) == F.f12_frobenius(a, 2)


def final_exp_is_one(a):
    return F._memo(("team_fe_verdict", a), lambda: F.f12_pow(a, (P ** 12 - 1) // R_ORDER) == F.F12_ONE)


def item_counts(op):
    return LONG_ITEM_COUNTS if op in LONG_OPS else ITEM_COUNTS


def is_one_stream(a):
    """one.is_eq(a) componentwise: per Fp6 half three fp2_is_eq_w (two is_neq pairs and their AND) and two ANDs, then the final AND -> (verdict, stream)"""
    flat = F.flat12(a)
    w, halves = [], []
    for h in range(2):
        b = []
        for k in range(3):
            i = 2 * (3 * h + k)
            e0, w0 = F.w_is_eq(1 if i == 0 else 0, flat[i])
            e1, w1 = F.w_is_eq(0, flat[i + 1])
            w += w0 + w1 + [F.w_bool(e0 and e1)]
            b.append(e0 and e1)
        w += [F.w_bool(b[0] and b[1]), F.w_bool(b[0] and b[1] and b[2])]
        halves.append(all(b))
    w.append(F.w_bool(all(halves)))
    assert len(w) == IS_ONE_WITNESSES
    return all(halves), w


def verdict_block(v):
    return [int(v), 0] * 6


def reference(op, a, b, c):
    """(the twelve result elements or None, the witness stream or None) of entry `op` on one item; None = taken from the single-lane host form"""
    if op in G2_OPS:
        return None, None
    x = F.d12(a)
    if op == "MUL":
        return F.e12(F.f12_mul(x, F.d12(b))), None
    if op == "SQR":
        return F.e12(F.f12_mul(x, x)), None
    if op == "CYC":
        assert is_cyclotomic(x), "CYC is given cyclotomic elements only"
        return F.e12(F.f12_mul(x, x)), None
    if op == "ELLC":
        return F.e12(F.f12_mul(x, line_const_p(c))), None
    if op == "ELLV":
        return F.e12(F.f12_mul(x, line_var_p(c, F.dec(c[4]), F.dec(c[5])))), None
    if op in ("ELLGS", "ELLGH"):
        return F.e12(F.f12_mul(x, sparse_014(F.d2(c, 0), F.d2(c, 2), F.d2(c, 4)))), []
    if op == "inverse_w":
        return F.e12(F.f12_inv(x)), None
    if op == "is_one_w":
        v, w = is_one_stream(x)
        return verdict_block(v), w
    if op == "conj":
        return F.e12(F.f12_conj(x)), []
    if op.startswith("frob_"):
        return F.e12(F.f12_frobenius(x, int(op[-1]))), []
    if op == "first_f":
        return F.e12(line_const_p(c)), []
    if op == "first_f_var":  # the allocated generator's pair: the two products c1.c0 g1.x, c1.c1 g1.x are the witnesses
        c1 = F.d2(c, 2)
        return F.e12(line_const_p(c)), [F.enc(c1[0] * G1_GEN[0]), F.enc(c1[1] * G1_GEN[0])]
    if op == "exp_by_x":  # x is negative: the power by |x|, conjugated (an inverse on the cyclotomic subgroup)
        assert x == (F.F6_ZERO, F.F6_ZERO) or is_cyclotomic(x), "exp_by_x is given cyclotomic elements (and 0) only"
        return F.e12(F.f12_conj(F.f12_pow(x, X_ABS))), None
    if op == "final_exp_is_one":
        return verdict_block(final_exp_is_one(x)), None
    if op == "seq":
        g = F.d12(b)
        f = F.f12_mul(x, x)
        f = F.f12_mul(f, line_const_p(c, 0))
        f = F.f12_mul(f, line_var_p(c, F.dec(c[8]), F.dec(c[9]), 1))
        f = F.f12_mul(f, f)
        f = F.f12_mul(f, g)
        f = f12_cyc_formula(f)
        return F.e12(F.f12_mul(f, g)), None
    raise KeyError(op)


# ---------------------------------------------------------------- G2: affine arithmetic on the twist, None = the identity
def g2_on_curve(pt):
    return pt is None or F.f2_mul(pt[1], pt[1]) == F.f2_add(F.f2_mul(pt[0], F.f2_mul(pt[0], pt[0])), B2)


def g2_neg(pt):
    return None if pt is None else (pt[0], F.f2_neg(pt[1]))


def g2_add(p, q):
    """the chord-and-tangent law in affine coordinates"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if F.f2_add(p[1], q[1]) == F.F2_ZERO:
            return None
        lam = F.f2_mul(f2_scale(F.f2_mul(p[0], p[0]), 3), F.f2_inv(f2_scale(p[1], 2)))
    else:
        lam = F.f2_mul(F.f2_sub(q[1], p[1]), F.f2_inv(F.f2_sub(q[0], p[0])))
    x3 = F.f2_sub(F.f2_sub(F.f2_mul(lam, lam), p[0]), q[0])
    return (x3, F.f2_sub(F.f2_mul(lam, F.f2_sub(p[0], x3)), p[1]))


def g2_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, pt)
        pt = g2_add(pt, pt)
        k >>= 1
    return acc


def g2_proj(pt, lam=F.F2_ONE):
    """homogeneous coordinates (x lam, y lam, lam); the identity is (0, lam, 0)"""
    if pt is None:
        return (F.F2_ZERO, lam, F.F2_ZERO)
    return (F.f2_mul(pt[0], lam), F.f2_mul(pt[1], lam), lam)


def g2_block(xyz):
    return F.blk(F.e2(xyz[0]) + F.e2(xyz[1]) + F.e2(xyz[2]))


def g2_affine_of_block(blk):
    x, y, z = F.d2(blk, 0), F.d2(blk, 2), F.d2(blk, 4)
    if z == F.F2_ZERO:
        assert x == F.F2_ZERO and y != F.F2_ZERO
        return None
    zi = F.f2_inv(z)
    return (F.f2_mul(x, zi), F.f2_mul(y, zi))


def g2_law_holds(op, a, b, result):
    """the result block of a G2 entry is projectively the affine sum of its operands: X3 z = x Z3 and Y3 z = y Z3 against the affine (x, y, 1), the
    identity as (0, y != 0, 0); lanes 3..5 of the team own nothing of a point and return zero"""
    p, q = g2_affine_of_block(a), g2_affine_of_block(b)
    assert g2_on_curve(p) and g2_on_curve(q)
    want = g2_add(p, p) if op == "G2DBL" else g2_add(p, q)
    X, Y, Z = F.d2(result, 0), F.d2(result, 2), F.d2(result, 4)
    if any(result[6:]):
        return False
    if want is None:
        return X == F.F2_ZERO and Z == F.F2_ZERO and Y != F.F2_ZERO
    return Z != F.F2_ZERO and X == F.f2_mul(want[0], Z) and Y == F.f2_mul(want[1], Z)


# ---------------------------------------------------------------- the cases
def _rng_f2(rng):
    return (rng.randrange(P), rng.randrange(P))


def lines4():
    """stored (c0, c1) pairs: the sparse sets of fp12_mul_by_014_w_*'s cases, then c0 = 0, c1 = 0, both zero (what k_vlines writes for an identity
    point), all p - 1"""
    def make():
        f2 = E.fp2_operand_set() + E.fp2_random(4, 0xF2F2)
        rng = random.Random(0x11AE5)
        out = [x + y for x in f2[::13] for y in f2[4::17]]
        out += [(0, 0) + _rng_f2(rng), _rng_f2(rng) + (0, 0), (0, 0, 0, 0), (P - 1,) * 4]
        return out
    return F._memo("team_lines4", make)


def g1_coords():
    return F._memo("team_g1", lambda: [0, 1, P - 1, ONE, random.Random(0x61C0).randrange(P)])


def lines_var():
    """(c0, c1, px, py): every line with one (px, py) pair of {0, 1, p - 1, ONE, random}, the pairs walking through all 25 combinations"""
    g = g1_coords()
    return [ln + (g[i % 5], g[(i // 5 + i) % 5]) for i, ln in enumerate(lines4() + lines4()[:1])] + \
        [lines4()[5] + (x, y) for x in g for y in g]


def lines6():
    """(c0, c1, c4) triples of the native pairing: the sparse pairs with c4 walking through 0, 1, p - 1, ONE, (p-1, p-1), random; c0 = 0, c1 = 0,
    c4 = 0 alone, all zero, all p - 1"""
    def make():
        rng = random.Random(0x11AE6)
        c4s = [(0, 0), (1, 0), (P - 1, 0), (ONE, 0), (P - 1, P - 1), (0, ONE), _rng_f2(rng), _rng_f2(rng)]
        out = [ln + c4s[i % len(c4s)] for i, ln in enumerate(lines4()[:20])]
        r = lambda: _rng_f2(rng)
        out += [(0, 0) + r() + r(), r() + (0, 0) + r(), r() + r() + (0, 0), (0,) * 6, (P - 1,) * 6]
        return out
    return F._memo("team_lines6", make)


def g2_points():
    """three affine on-curve points [k] G (k small, so that sums and doubles stay distinct non-identity points)"""
    def make():
        assert g2_on_curve(G2_GEN) and g2_mul(R_ORDER, G2_GEN) is None
        return [g2_mul(k, G2_GEN) for k in (1, 5, 7)]
    return F._memo("team_g2", make)


def _g2_cases(op):
    rng = random.Random(0x62C5)
    g, p5, p7 = g2_points()
    lam, mu, m1 = _rng_f2(rng), _rng_f2(rng), (P - 1, 0)
    one = F.F2_ONE
    if op == "G2DBL":
        pts = [(g, one), (p5, one), (p7, lam), (p5, m1), (g, (0, P - 1)), (None, one), (None, lam), (None, m1), (g2_neg(p7), mu)]
        return [(g2_block(g2_proj(p, s)), g2_block(g2_proj(p7, mu)), F.ZERO_BLK) for p, s in pts]
    pairs = [
        (p5, one, p7, one), (p7, one, p5, one), (g, one, p5, one),  # P + Q
        (p5, one, p5, one), (p5, lam, p5, mu), (g, m1, g, one),  # P + P through the addition
        (p5, one, g2_neg(p5), one), (p7, lam, g2_neg(p7), mu), (g, one, g2_neg(g), m1),  # P + (-P)
        (None, one, p7, one), (p7, one, None, one), (None, one, None, one), (None, lam, p5, mu), (p5, mu, None, lam), (None, m1, None, lam),  # identities
        (p5, lam, p7, mu), (p5, m1, p7, one), (p5, one, p7, m1), (p5, m1, p7, m1), (g, (0, 1), p7, (P - 1, P - 1)),  # Z != 1
    ]
    return [(g2_block(g2_proj(p, s)), g2_block(g2_proj(q, u)), F.ZERO_BLK) for p, s, q, u in pairs]


def is_one_elements():
    """1, 0, a random element, and 1 with each of its twelve Fp coordinates in turn off by +1 and replaced by p - 1: exactly one false flag in every
    position of the AND tree"""
    one = list(F.flat12(F.F12_ONE))
    out = [one, [0] * 12, [random.Random(0x150E).randrange(P) for _ in range(12)]]
    for k in range(12):
        out.append(one[:k] + [(one[k] + 1) % P] + one[k + 1:])
        out.append(one[:k] + [P - 1] + one[k + 1:])
    return [F.blk(F.enc(v) for v in el) for el in out]


def final_exp_elements():
    """[(block, verdict)]: 1; an element of Fp2 and one of Fp6 embedded in Fp12 (the easy part sends both to 1); g^r for a random cyclotomic g; two
    random elements (false). Not 0: its inverse hint is not what is under test here."""
    def make():
        rng = random.Random(0xF1E7)
        z = F.F2_ZERO
        f2 = ((_rng_f2(rng), z, z), F.F6_ZERO)
        f6 = ((_rng_f2(rng), _rng_f2(rng), _rng_f2(rng)), F.F6_ZERO)
        gr = F.f12_pow(F.d12(F.cyclotomic_elements()[2]), R_ORDER)
        assert gr != F.F12_ONE
        rnd = [F.d12([rng.randrange(P) for _ in range(12)]) for _ in range(2)]
        return [(F.blk(F.e12(x)), v) for x, v in [(F.F12_ONE, True), (f2, True), (f6, True), (gr, True), (rnd[0], False), (rnd[1], False)]]
    return F._memo("team_fe", make)


def cyclotomic_with_conjugates():
    cyc = F.cyclotomic_elements()
    return cyc + [F.blk(F.e12(F.f12_conj(F.d12(x)))) for x in cyc[1:]]


def _pad(vals):
    return F.blk(vals)


def cases(op):
    """[(a, b, c)]: every edge item of entry `op`"""
    return F._memo(("team_cases", op), lambda: _cases(op))


def _cases(op):
    Z = F.ZERO_BLK
    fp12, cyc = F.fp12_elements(), F.cyclotomic_elements()
    if op == "MUL":
        return [(x, y, Z) for x in fp12 for y in fp12]  # the diagonal: a is b
    if op in ("SQR", "inverse_w", "conj", "frob_1", "frob_2", "frob_3"):
        return [(x, Z, Z) for x in fp12 + cyc]
    if op == "CYC":
        return [(x, Z, Z) for x in cyc]
    if op == "ELLC":
        return [(x, Z, _pad(ln)) for x in fp12 for ln in lines4()]
    if op == "ELLV":
        return [(x, Z, _pad(ln)) for x in fp12 for ln in lines_var()]
    if op in ("ELLGS", "ELLGH"):
        return [(x, Z, _pad(ln)) for x in fp12 for ln in lines6()]
    if op in G2_OPS:
        return _g2_cases(op)
    if op == "is_one_w":
        return [(x, Z, Z) for x in is_one_elements()]
    if op in ("first_f", "first_f_var"):
        return [(Z, Z, _pad(ln)) for ln in lines4()]
    if op == "exp_by_x":
        return [(x, Z, Z) for x in cyclotomic_with_conjugates()]
    if op == "final_exp_is_one":
        return [(x, Z, Z) for x, _ in final_exp_elements()]
    if op == "seq":
        g = g1_coords()
        lv = lines4()
        # the running f meets two lines and a second operand: every Fp12 operand kind against a walk through the lines and the G1 coordinates
        return [(x, fp12[(3 * i + 1) % len(fp12)], _pad(lv[i % len(lv)] + lv[(5 * i + 2) % len(lv)] + (g[i % 5], g[(i // 5 + 2 * i + 1) % 5]))) for i, x in enumerate(fp12 + cyc)]
    raise KeyError(op)


def mixed_wave(op):
    """seq and exp_by_x: a wave whose ten teams hold ten different operand kinds, 0 and 1 among them"""
    if op == "exp_by_x":
        cyc = cyclotomic_with_conjugates()
        items = [(F.ZERO_BLK, F.ZERO_BLK, F.ZERO_BLK)] + [(x, F.ZERO_BLK, F.ZERO_BLK) for x in cyc[:9]]
    else:
        src = cases(op)
        items = [src[i] for i in (0, 1, 2, 5, 8, 13, 14, 15, 16, len(src) - 1)]  # 0, 1, single coefficients, all p - 1, the stress values, random, cyclotomic
    assert len(items) == TEAMS and len(set(it[0] for it in items)) == TEAMS
    return items


def launches(op):
    """[(arrangement, items)]: every launch of entry `op`, the same for the host test and for the device. "edges": all edge items; "shift3",
    "shift9": the same behind 3 and 9 filler items; "teams": every edge item in a wave of its own at team 0, at an inner team and at team 9 (beside
    the idle lanes), fillers between; "n=K": the first K items of a walk through the edge items (item_counts); "mixed" (seq, exp_by_x)."""
    src = cases(op)
    filler = src[len(src) // 2]
    out = [("edges", src), ("shift3", [filler] * 3 + src), ("shift9", [filler] * 9 + src)]
    teams = []
    for it in src:
        teams += [it] + [filler] * 3 + [it] + [filler] * 4 + [it]
    out.append(("teams", teams))
    step = next(s for s in (37, 41, 43, 47, 53) if len(src) % s) if len(src) > 1 else 1
    walk = [src[i * step % len(src)] for i in range(max(item_counts(op)))]
    out += [("n=%d" % n, walk[:n]) for n in item_counts(op)]
    if op in ("seq", "exp_by_x"):
        out.append(("mixed", mixed_wave(op)))
    return out
