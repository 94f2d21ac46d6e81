"""The operand sets of the curve operation table (tests/devcurve/ops.hpp), shared by the host test (test_curve_ref.py) and the device test
(test_curve_device_gpu.py). Points are built by the reference's affine arithmetic (tests/curve_ref.py), never taken from the code under test;
field elements come from tests/field_edges.py. cases(op) is the list of (a, b) operand blocks of twelve stored integers; raw bytes ride in slots
as the little-endian integer of their 48 bytes."""
import random

from tests import curve_ref as C
from tests import field_edges as E
from tests import field_ref as F
from tests.curve_ref import K1, K2, R_ORDER, X_ABS
from tests.field_edges import ONE, P
from tests.field_ref import blk, enc

ITEM_COUNTS = (1, 63, 64, 65, 100)  # one lane, a partial last wave, a full wave, a wave with one item; 63 and 65 make the PARK's row stride odd
WAVE = 64
ZERO_BLK = blk([])


def _memo(key, fn):
    return F._memo(("curve_edges", key), fn)


def _rand_el(K, rng):
    return rng.randrange(P) if K is K1 else (rng.randrange(P), rng.randrange(P))


def _sqrt(K, a):
    if K is K2:
        return C.fp2_sqrt_generic(a)
    ok, r = C.fp_sqrt(a)
    return r if ok else None


def curve_point(K, rng):
    """a curve point from a random x"""
    while True:
        x = _rand_el(K, rng)
        y = _sqrt(K, K.add(K.mul(K.mul(x, x), x), K.b))
        if y is not None:
            return (x, y)


def points(K):
    """{kind: [affine points]}: multiples of the generator ([r - 1]G among them), random curve points outside the subgroup, cofactor-torsion points
    [r]Q, sums of a subgroup and a torsion point, and on E(Fp) the order-3 points (0, +-2). (The twist has no point with x = 0: 4(1 + u) is a
    square only if its norm 32 is one, and 2 is a non-residue for p = 3 (mod 8).)"""
    def make():
        gen = C.G1_GEN if K is K1 else C.G2_GEN
        rng = random.Random(0xC0DE + K.n)
        sub = [C.aff_mul(K, k, gen) for k in (1, 2, 3, 5, R_ORDER - 1)]
        rnd = [curve_point(K, rng) for _ in range(3)]
        tors = [C.aff_mul(K, R_ORDER, q) for q in rnd[:2]]
        assert all(C.on_curve(K, q) for q in sub + rnd + tors) and all(C.aff_mul(K, R_ORDER, q) is not None for q in rnd + tors)
        out = {"subgroup": sub, "random": rnd, "torsion": tors, "mixed": [C.aff_add(K, s, t) for s, t in zip(sub[1:], tors)]}
        if K is K1:
            out["order3"] = [(0, 2), (0, P - 2)]
            assert C.aff_mul(K1, 3, (0, 2)) is None and not C.fp_is_square(2)
        return out
    return _memo(("points", K.n), make)


def all_points(K):
    return [q for group in points(K).values() for q in group]


def lams(K):
    """the factors l of the representatives (l^2 X, l^3 Y, l Z): 1, 2, p - 1, a random value"""
    rng = random.Random(0x1A + K.n)
    if K is K1:
        return [1, 2, P - 1, rng.randrange(1, P)]
    return [(1, 0), (2, 0), (P - 1, 0), (rng.randrange(P), rng.randrange(1, P))]


def identities(K):
    """the Jacobian identity as (1, 1, 0), as (x, y, 0) with arbitrary x, y, and as the doubling of that"""
    rng = random.Random(0x1D + K.n)
    xy0 = (_rand_el(K, rng), _rand_el(K, rng), K.zero)
    return [(K.one, K.one, K.zero), xy0, C.jac_dbl(K, xy0)]


def jblk(K, *els):
    """field elements -> an operand block"""
    return blk([s for x in els for s in K.st(x)])


def jac_operands(K):
    """every point in every representative, then the identities"""
    return _memo(("jac", K.n), lambda: [C.jac_rep(K, q, l) for q in all_points(K) for l in lams(K)] + identities(K))


def mixed_pairs(K, domain_only=False):
    """[(Jacobian p, affine q)]: P + Q, P + P, P + (-P), P + 2P, 2P + P for every point in every representative (an order-3 point makes the last
    two cancel), and the identities + Q. domain_only: jac1_add_mixed's contract (p no identity, p != +-q)"""
    def make():
        pts, ls, out = all_points(K), lams(K), []
        for i, pt in enumerate(pts):
            other, two = pts[(i + 1) % len(pts)], C.aff_add(K, pt, pt)
            for j, l in enumerate(ls):
                out.append((C.jac_rep(K, pt, l), other))
                for q in (pt, C.aff_neg(K, pt), two):
                    out.append((C.jac_rep(K, pt, l), q))
                out.append((C.jac_rep(K, two, ls[(j + 1) % 4]), pt))
        out += [(o, q) for o in identities(K) for q in pts[:3]]
        if domain_only:
            out = [(p, q) for p, q in out if p[2] != K.zero and C.jac_affine(K, p)[0] != q[0]]
        return out
    return _memo(("mixed", K.n, domain_only), make)


def jac_pairs():
    """[(Jacobian p, Jacobian q)] over Fp2 for v_add: every mixed pair with q in a representative with Z != 1 as well (and Z = 1 for some), then
    P + identity and identity + identity"""
    def make():
        ls, out = lams(K2), []
        for i, (p, q) in enumerate(mixed_pairs(K2)):
            out.append((p, C.jac_rep(K2, q, ls[(i + 1 + i // 4) % 4])))
        ids = identities(K2)
        out += [(C.jac_rep(K2, q, ls[i % 4]), ids[i % 3]) for i, q in enumerate(all_points(K2))]
        out += [(x, y) for x in ids for y in ids]
        return out
    return _memo("jacpairs", make)


def proj_rep(K, pt, lam):
    return (K.zero, lam, K.zero) if pt is None else (K.mul(pt[0], lam), K.mul(pt[1], lam), lam)


def proj_pairs(K, mode):
    """[(homogeneous a, homogeneous b)] for the complete addition in Z mode `mode`: the pair kinds of mixed_pairs; mode 0 with both operands
    scaled and with the identity (0, 1, 0) on either side and both; mode 1 with b.z = 1 (a any, the identity among them); mode 2 with both z = 1;
    modes 1 and 2 also on a few operands off their contract"""
    def make():
        pts, ls, out = all_points(K), lams(K), []
        for i, pt in enumerate(pts):
            other, two = pts[(i + 1) % len(pts)], C.aff_add(K, pt, pt)
            for j, q in enumerate((other, pt, C.aff_neg(K, pt), two)):
                la, lb = (ls[(i + j) % 4], ls[(i + 2 * j + 1) % 4]) if mode == 0 else ((ls[(i + j) % 4], K.one) if mode == 1 else (K.one, K.one))
                out.append((proj_rep(K, pt, la), proj_rep(K, q, lb)))
            out.append((proj_rep(K, two, K.one if mode == 2 else ls[i % 4]), proj_rep(K, pt, ls[(i + 1) % 4] if mode == 0 else K.one)))
        if mode < 2:
            out += [(proj_rep(K, None, l), proj_rep(K, q, K.one if mode else ls[2])) for l in ls for q in pts[:2]]
        if mode:  # off the mode's contract, where only the formula speaks: z operands that are not the one the mode takes them for
            out += [(proj_rep(K, pts[i], ls[1 + i % 3]), proj_rep(K, pts[i + 1], ls[1 + (i + 1) % 3] if mode == 1 else K.one)) for i in range(4)]
            out += [(proj_rep(K, pts[i], ls[1 + i % 3]), proj_rep(K, pts[i], ls[3 - i % 3])) for i in range(2)]
        if mode == 0:
            out += [(proj_rep(K, q, l), proj_rep(K, None, K.one)) for l in ls for q in pts[:2]]
            out += [(proj_rep(K, None, K.one), proj_rep(K, None, l)) for l in ls]
        return out
    return _memo(("proj", K.n, mode), make)


def scalars():
    """0, 1, 2, 15, 16, |x| - 1, |x|, |x| + 1, |x|^2, |x|^2 - 1, |x|^3, |x|^3 + |x|^2 + |x| + 1, r - 2, r - 1, 2^254 + 1, and single set bits at
    every word border (bits 31, 32, 63, 64, ... 224, 254); all below 2^255 and below |x|^4"""
    x = X_ABS
    s = [0, 1, 2, 15, 16, x - 1, x, x + 1, x * x, x * x - 1, x ** 3, x ** 3 + x * x + x + 1, R_ORDER - 2, R_ORDER - 1, (1 << 254) + 1]
    s += [1 << b for w in range(1, 8) for b in (32 * w - 1, 32 * w)] + [1 << 254]
    assert all(k < x ** 4 and k < (1 << 255) for k in s)
    return s


def flag_records(n, valid_body):
    """all eight settings of the three flag bits over a valid body, a zero body, and a non-zero body that is no valid x (all 0xff below the flags:
    with the infinity flag it is the non-zero body the identity rule ignores)"""
    out = []
    for body in (valid_body, bytes(n), bytes([0x1F]) + b"\xff" * (n - 1)):
        out += [bytes([(body[0] & 0x1F) | (f << 5)]) + body[1:] for f in range(8)]
    return out


X_EDGES = (0, 1, P - 1, P, P + 1, (1 << 381) - 1)


def g1_records():
    def make():
        pts = points(K1)
        recs = flag_records(48, C.g1_compress(C.G1_GEN))
        recs += [C.be48(x, 0x80 | s) for x in X_EDGES for s in (0, 0x20)]
        for q in all_points(K1):  # both sort flags of every point (the flag picks between P and -P), so also the round trip of either
            recs += [C.g1_compress(q, False), C.g1_compress(q, True)]
        rng = random.Random(0x6101)
        recs += [C.be48(rng.randrange(P), 0x80 | (0x20 if i & 1 else 0)) for i in range(24)]  # about half off the curve, the rest outside the subgroup
        recs += [C.be48(rng.randrange(P), 0xC0) for _ in range(6)]  # the identity over arbitrary bodies
        assert len(pts["order3"]) == 2
        return list(dict.fromkeys(recs))
    return _memo("g1rec", make)


def g2_records():
    def make():
        gx = C.G2_GEN[0]
        recs = flag_records(96, C.g2_compress(C.G2_GEN))
        for x in X_EDGES:  # each half at its edges with the other half the generator's
            recs += [C.be48(x, 0x80 | s) + C.be48(gx[0]) for s in (0, 0x20)] + [C.be48(gx[1], 0x80 | s) + C.be48(x) for s in (0, 0x20)]
        recs += [C.be48(gx[1], 0x80) + C.be48(gx[0], f << 5) for f in range(1, 8)]  # the second half is not masked: any of its top three bits rejects
        recs += [C.be48(gx[1], 0x80) + bytes([0xFF]) * 48, C.be48(0, 0x80) + C.be48(0), C.be48(0, 0xA0) + C.be48(1)]
        for q in all_points(K2):
            recs += [C.g2_compress(q, False), C.g2_compress(q, True)]
        rng = random.Random(0x6202)
        recs += [C.be48(rng.randrange(P), 0x80 | (0x20 if i & 1 else 0)) + C.be48(rng.randrange(P)) for i in range(24)]
        recs += [C.be48(rng.randrange(P), 0xC0) + C.be48(rng.randrange(1 << 384)) for _ in range(6)]
        return list(dict.fromkeys(recs))
    return _memo("g2rec", make)


def rec_blk(data):
    return blk(C._slots(data))


def fp2_sqrt_operands():
    """canonical Fp2 values: zero; c1 = 0 with c0 a square and a non-square (p - 1, the edge values); random elements and squares of random
    elements, which the reference splits into first delta / second delta / not a square"""
    rng = random.Random(0x5912)
    fe = [0, 1, 4, 9, P - 1, P - 4, 2, P - 2, (P - 1) // 2, (P + 1) // 2, 5, P - 5] + [rng.randrange(P) for _ in range(4)]
    out = [(0, 0)] * 4 + [(v, 0) for v in fe if v]  # zero has one operand: given four times, so that its exit fills lanes like the others
    rnd = [(rng.randrange(P), rng.randrange(1, P)) for _ in range(28)]
    out += rnd + [F.f2_mul(x, x) for x in rnd[:12]] + [(0, 1), (0, P - 1), (1, 1), (P - 1, P - 1), (P - 1, 1)]
    return out


LEX_VALUES = (0, 1, (P - 1) // 2, (P + 1) // 2, P - 1)


def unary(vals):
    return [(blk(v if isinstance(v, (tuple, list)) else [v]), ZERO_BLK) for v in vals]


def cases(op):
    """[(a, b)] operand blocks of operation `op`, in a fixed order"""
    return _memo(("cases", op), lambda: _cases(op))


def _cases(op):
    K = K1 if op.startswith(("jac1", "v1_", "g1_", "vg_scale_g1", "vg_line")) or op.endswith("_fp") or "_fp_z" in op else K2
    rng = random.Random(sum(map(ord, op)))
    f2 = E.fp2_operand_set()
    if op in ("fp_from_be48_1f", "fp_from_be48_ff"):
        vals = list(X_EDGES) + [P - 2, (1 << 384) - 1, 1 << 380, 1 << 381, 1 << 382, 1 << 383, (1 << 383) + 5] + [rng.randrange(P) for _ in range(6)]
        recs = [v.to_bytes(48, "big") for v in vals] + [bytes([(f << 5) | 0x0A]) + b"\x11" * 47 for f in range(8)] + [bytes([(f << 5) | 0x1A]) + b"\x01" * 47 for f in range(8)]
        return [(rec_blk(r), ZERO_BLK) for r in recs]
    if op == "fp_sqrt":
        vals = [enc(v) for v in (0, 1, 4, P - 1, 2, 9, P - 4)] + E.field_edge_values() + [enc(v * v) for v in (P - 1, (P - 1) // 2, rng.randrange(P), rng.randrange(P))]
        return unary(vals)
    if op == "fp2_sqrt":
        return unary([tuple(F.e2(x)) for x in fp2_sqrt_operands()])
    if op == "fp_lex_largest":
        return unary([enc(v) for v in LEX_VALUES] + [enc(rng.randrange(P)) for _ in range(4)])
    if op == "fp2_lex_largest":
        r = rng.randrange(P)
        return unary([tuple(F.e2((c0, 0))) for c0 in LEX_VALUES] + [tuple(F.e2((c0, c1))) for c1 in LEX_VALUES for c0 in (r, 0, P - 1)])
    if op == "g1_decode":
        return [(rec_blk(r), ZERO_BLK) for r in g1_records()]
    if op == "g2_decode":
        return [(rec_blk(r), ZERO_BLK) for r in g2_records()]
    if op in ("g1_encode", "g2_encode"):
        pts = all_points(K) + [C.aff_neg(K, q) for q in all_points(K)]
        out = [(jblk(K, q[0], q[1]), ZERO_BLK) for q in pts]
        out += [(blk(K.st(q[0]) + K.st(q[1]) + [1]), ZERO_BLK) for q in pts[:2]]  # the infinity flag over arbitrary coordinates
        edge = [(0, 2), (1, 1), (P - 1, (P - 1) // 2), (P - 1, (P + 1) // 2)] if K is K1 else [((0, 0), (1, 0)), ((P - 1, P - 1), (0, (P - 1) // 2)), ((1, P - 1), ((P + 1) // 2, 0))]
        return out + [(jblk(K, x, y), ZERO_BLK) for x, y in edge]  # encode reads x and the sign of y: no curve equation
    if op == "sk_from_le32":
        vals = [0, 1, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, 1 << 255, 1 << 32, R_ORDER - (1 << 32)] + [rng.randrange(R_ORDER) for _ in range(3)]
        return unary(vals)
    if op.endswith(("_in_subgroup", "_in_subgroup_ladder")):
        return [(jblk(K, q[0], q[1]), ZERO_BLK) for q in all_points(K) + [C.aff_neg(K, q) for q in all_points(K)[:6]]]
    if op in ("jac1_dbl", "jac1v_dbl", "jac2_dbl", "v1_dbl", "v_dbl", "v_dbl_inplace", "v_neg", "v_psi", "v_psi2", "vg_affine2", "vg_line_multipliers"):
        return [(jblk(K, *p), ZERO_BLK) for p in jac_operands(K)]
    if op == "jac1_add_mixed":
        return [(jblk(K, *p), jblk(K, *q)) for p, q in mixed_pairs(K, True)]
    if op in ("jac1v_add_mixed", "jac2_add_mixed", "v1_add_mixed", "v_add_mixed"):
        return [(jblk(K, *p), jblk(K, *q)) for p, q in mixed_pairs(K)]
    if op == "v_add":
        return [(jblk(K2, *p), jblk(K2, *q)) for p, q in jac_pairs()]
    if op == "v_sqr":
        return unary(f2)
    if op in ("g1_mul_affine", "g2_mul_affine"):
        pts = points(K)
        sel = [pts["subgroup"][0], pts["subgroup"][2], pts["random"][0], pts["torsion"][0]] + (pts["order3"][:1] if K is K1 else [])
        out = [(jblk(K, *q), blk([k])) for q in sel[:2] for k in scalars() + [R_ORDER]]  # [r]P: the identity, the flag false
        return out + [(jblk(K, *q), blk([k])) for q in sel[2:] for k in (0, 1, 2, 3, 16, X_ABS, X_ABS + 1, R_ORDER, (1 << 254) + 1)]
    if op == "v_pow_c1":
        vals = [(0, 0), (1, 0), (P - 1, 0), (2, 0), (rng.randrange(P), 0), (0, 1), (0, P - 1), (0, rng.randrange(P))] + [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        return unary([tuple(F.e2(x)) for x in vals])
    if op == "v_sgn0":
        vals = [(c0, c1) for c0 in (0, 1, 2, P - 1, P - 2) for c1 in (0, 1, 2, P - 1)] + [(rng.randrange(P), rng.randrange(P)) for _ in range(4)]
        return unary([tuple(F.e2(x)) for x in vals])
    if op == "v_poly":
        xs = [(0, 0), (ONE, 0), (P - 1, P - 1), (rng.randrange(P), rng.randrange(P))]
        coeff = [[0] * 10, [P - 1] * 10, [rng.randrange(P) for _ in range(10)], [ONE, 0] * 5, [rng.randrange(P) if i % 4 < 2 else 0 for i in range(10)]]
        return [(blk(list(x) + k), blk([n])) for x in xs for k in coeff for n in (1, 2, 3, 4, 5)] + [(blk(list(xs[3]) + coeff[2]), blk([n])) for n in (0, 6, 1 << 31)]
    if op == "v_map_to_curve":
        us = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (1, 1), (0, P - 1), (0, 2), (0, rng.randrange(P))] + [(rng.randrange(P), rng.randrange(P)) for _ in range(28)]
        return unary([tuple(F.e2(u)) for u in us])
    if op == "v_clear_cofactor":
        ls = lams(K2)
        return [(jblk(K2, *C.jac_rep(K2, q, ls[(i + j) % 4])), ZERO_BLK) for i, q in enumerate(all_points(K2)) for j in (0, 1)] + [(jblk(K2, *o), ZERO_BLK) for o in identities(K2)]
    if op == "v_digits_x":
        return unary(scalars() + [X_ABS ** 4 - 1, X_ABS ** 2 + X_ABS - 1, (X_ABS - 1) * (X_ABS ** 3 + X_ABS ** 2 + X_ABS + 1)] + [rng.randrange(R_ORDER) for _ in range(6)])
    if op == "v_g2_mul_gls":
        ls, sub = lams(K2), points(K2)["subgroup"]
        reps = [C.jac_rep(K2, sub[0], ls[0]), C.jac_rep(K2, sub[2], ls[3]), C.jac_rep(K2, sub[4], ls[2])]
        return [(jblk(K2, *q), blk([k])) for i, k in enumerate(scalars() + [rng.randrange(R_ORDER) for _ in range(4)]) for q in (reps[i % 3], reps[(i + 1) % 3])]
    if op == "v1_mul_g1_fixed":
        ks = [d << (4 * w) for w in range(64) for d in (1, 15)] + [(1 << 256) - 1] + scalars() + [rng.randrange(1 << 256) for _ in range(4)]
        return unary(ks)
    if op in ("vg_scale_g1", "vg_scale_g2"):
        pts = points(K)
        sel = [pts["subgroup"][0], pts["subgroup"][3], pts["random"][1], pts["mixed"][0]] + (pts["order3"][:1] if K is K1 else [])
        rs = [0, 1, 2, 3, 1 << 32, 1 << 63, (1 << 64) - 1, X_ABS, rng.randrange(1 << 64)]
        return [(jblk(K, *q), blk([r])) for q in sel for r in rs]
    if op == "vg_sum2":
        return [(jblk(K2, *p), jblk(K2, *q)) for p, q in jac_pairs()[::2] + jac_pairs()[-12:]]
    if op == "vg_sum3":
        ls, out = lams(K2), []
        ids = identities(K2)
        for i, pt in enumerate(all_points(K2)):
            other = all_points(K2)[(i + 3) % len(all_points(K2))]
            rep = lambda q, j: C.jac_rep(K2, q, ls[(i + j) % 4])
            back = C.aff_neg(K2, C.aff_add(K2, pt, other))
            for trio in ((rep(pt, 0), rep(other, 1), rep(back, 2)), (rep(pt, 0), rep(C.aff_neg(K2, pt), 1), rep(other, 2)), (rep(pt, 1), rep(pt, 2), rep(pt, 3)),
                         (rep(pt, 0), ids[i % 3], rep(pt, 1)), (ids[i % 3], rep(pt, 2), rep(other, 0))):
                out.append((blk(list(jblk(K2, *trio[0])[:6]) + list(jblk(K2, *trio[1])[:6])), jblk(K2, *trio[2])))
        out.append((blk(list(jblk(K2, *ids[0])[:6]) + list(jblk(K2, *ids[1])[:6])), jblk(K2, *ids[2])))
        return out
    if op.startswith("proj_double_w"):
        return [(jblk(K, *proj_rep(K, q, l)), ZERO_BLK) for q in all_points(K) for l in lams(K)] + [(jblk(K, *proj_rep(K, None, l)), ZERO_BLK) for l in lams(K)]
    if op.startswith("proj_add_w"):
        return [(jblk(K, *x), jblk(K, *y)) for x, y in proj_pairs(K, int(op[-1]))]
    if op.startswith("nz_"):
        pts = all_points(K2)
        beta = pow(2, (P - 1) // 3, P)  # (beta x, y) is a curve point with the same y: the chord's numerator is 0
        edge = [((0, 0), (P - 1, P - 1)), ((P - 1, 0), (0, P - 1)), ((1, P - 1), (P - 1, 1)), ((0, P - 1), (1, 0))]  # no curve points: the steps are formulas
        if op.startswith("nz_double"):
            ps = pts + [C.aff_neg(K2, q) for q in pts[:4]] + edge
            return [(blk(F.e2(p[0]) + F.e2(p[1]) + F.e2(F.f2_inv(C.T.f2_scale(p[1], 2)))), ZERO_BLK) for p in ps]
        pairs = [(p, pts[(i + 1) % len(pts)]) for i, p in enumerate(pts)] + [(p, pts[(i + 5) % len(pts)]) for i, p in enumerate(pts)]
        pairs += [(p, C.aff_add(K2, p, p)) for p in pts[:6]] + [(p, (C.T.f2_scale(p[0], beta), p[1])) for p in pts[:6]]
        pairs += [(edge[i], edge[(i + 1) % 4]) for i in range(4)] + [(edge[0], pts[0]), (pts[1], edge[1])]
        return [(blk(F.e2(p[0]) + F.e2(p[1]) + F.e2(F.f2_inv(F.f2_sub(q[0], p[0])))), blk(F.e2(q[0]) + F.e2(q[1]))) for p, q in pairs]
    raise KeyError(op)


def launches(op):
    """[(name, items)]: every launch of operation `op`, the same for the host test and for each device build. "order": every case once;
    "shuffled": the same in a seeded random order, so that every wave mixes branches, statuses and exits; "branch: ...": for an operation whose
    reference names branches, the cases of one branch repeated over a whole wave (four waves on quads), so that all lanes take that path
    together; "n=...": the first n items of the shuffled order repeated to 100, for n in ITEM_COUNTS."""
    def make():
        cs = cases(op)
        labels = [x[2] for x in C.expected(op, cs)]
        sh = list(cs)
        random.Random(0x5AFE).shuffle(sh)
        out = [("order", cs), ("shuffled", sh)]
        for label in dict.fromkeys(l for l in labels if l is not None):
            mine = [c for c, l in zip(cs, labels) if l == label]
            out.append(("branch: " + label, [mine[i % len(mine)] for i in range(WAVE * ((len(mine) + WAVE - 1) // WAVE))]))
        walk = [sh[i % len(sh)] for i in range(max(ITEM_COUNTS))]
        return out + [("n=%d" % n, walk[:n]) for n in ITEM_COUNTS]
    return _memo(("launches", op), make)


def branch_counts(op):
    """{branch: cases} as the reference reports them"""
    cs = cases(op)
    out = {}
    for x in C.expected(op, cs):
        out[x[2]] = out.get(x[2], 0) + 1
    return out
