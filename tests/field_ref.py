"""A plain big-integer reference of the operation table of tests/devfield/ops.hpp (csrc/fp.hpp, gadgets.hpp, tower.hpp), and the table's test cases.

Python integers mod p. Fp2 = Fp[u]/(u^2 + 1), Fp6 = Fp2[v]/(v^3 - (1 + u)), Fp12 = Fp6[w]/(w^2 - v); products are schoolbook, inverses come
from pow(x, -1, p) and the norm maps, the inverse of zero is zero. The sparse products and the cyclotomic square are the dense product (square)
of the embedded operands; the Frobenius maps are conjugations and powers of (1 + u)^((p^k - 1) / 6) computed here. Elements travel as stored
integers (Montgomery form, R = 2^384); an operation's expected value is (result elements, witness stream), both lists of stored integers.

The witness streams of the Fp and Fp2 operations are stated here directly; fp_to_bits_le_w's restates ark-r1cs-std's to_bits_le and
Boolean::enforce_in_field_le. For the Fp6 / Fp12 operations `reference` returns None as the stream: its expected value is the
host compilation's stream (hostsim_field_op), which the pipeline tests pin to the oracle."""
import random

from tests import field_edges as E
from tests.field_edges import ONE, P, R

R_INV = pow(R, -1, P)
SENTINEL = 0xA5A5A5A5A5A5A5A5


def enc(x):
    return x * R % P


def dec(m):
    return m * R_INV % P


def inv(x):
    return pow(x, -1, P) if x % P else 0


# ---------------------------------------------------------------- Fp2, Fp6, Fp12 on canonical integers: tuples (c0, c1), 3-tuples of Fp2, 2-tuples of Fp6
XI = (1, 1)
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_conj(a):
    return (a[0], (-a[1]) % P)


def f2_inv(a):
    n = inv((a[0] * a[0] + a[1] * a[1]) % P)
    return (a[0] * n % P, (-a[1]) * n % P)


def f2_pow(a, e):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


def poly_mul_mod(a, b, shift):
    """schoolbook product of two polynomials over Fp2 of the same degree bound n, reduced by X^n = shift"""
    n = len(a)
    t = [F2_ZERO] * (2 * n - 1)
    for i in range(n):
        for j in range(n):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    for k in range(2 * n - 2, n - 1, -1):
        t[k - n] = f2_add(t[k - n], f2_mul(t[k], shift))
    return tuple(t[:n])


F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)


def f6_mul(a, b):
    return poly_mul_mod(a, b, XI)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul_v(a):
    return (f2_mul(a[2], XI), a[0], a[1])


def f6_inv(a):
    """a^-1 = (a^p2 a^p4) / N(a) would need Frobenius maps; the adjugate of the multiplication-by-a map does not: with the norm to Fp2
    N = a0 t0 + xi (a2 t1 + a1 t2), t0 = a0^2 - xi a1 a2, t1 = xi a2^2 - a0 a1, t2 = a1^2 - a0 a2, the inverse is (t0, t1, t2) / N"""
    a0, a1, a2 = a
    t0 = f2_sub(f2_mul(a0, a0), f2_mul(XI, f2_mul(a1, a2)))
    t1 = f2_sub(f2_mul(XI, f2_mul(a2, a2)), f2_mul(a0, a1))
    t2 = f2_sub(f2_mul(a1, a1), f2_mul(a0, a2))
    n = f2_add(f2_mul(a0, t0), f2_mul(XI, f2_add(f2_mul(a2, t1), f2_mul(a1, t2))))
    ni = f2_inv(n)
    r = (f2_mul(t0, ni), f2_mul(t1, ni), f2_mul(t2, ni))
    assert n == F2_ZERO or f6_mul(a, r) == F6_ONE
    return r


F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):
    """schoolbook over Fp6 with w^2 = v"""
    return (f6_add(f6_mul(a[0], b[0]), f6_mul_v(f6_mul(a[1], b[1]))), f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_conj(a):
    return (a[0], f6_neg(a[1]))


def f12_inv(a):
    """conjugate over the norm to Fp6: (a0 - a1 w) / (a0^2 - v a1^2)"""
    n = f6_sub(f6_mul(a[0], a[0]), f6_mul_v(f6_mul(a[1], a[1])))
    ni = f6_inv(n)
    return (f6_mul(a[0], ni), f6_neg(f6_mul(a[1], ni)))


def f12_pow(a, e):
    r = F12_ONE
    while e:
        if e & 1:
            r = f12_mul(r, a)
        a = f12_mul(a, a)
        e >>= 1
    return r


_GAMMA = {}


def f12_frobenius(a, k):
    """a^(p^k): with a = sum of c_i w^i over Fp2 (w^6 = xi; c_i = a[i % 2][i // 2]), conj^k(c_i) gamma^i w^i, gamma = xi^((p^k - 1) / 6)"""
    if k not in _GAMMA:
        _GAMMA[k] = f2_pow(XI, (P ** k - 1) // 6)
    out = [[None] * 3, [None] * 3]
    for i in range(6):
        c = a[i % 2][i // 2]
        if k & 1:
            c = f2_conj(c)
        out[i % 2][i // 2] = f2_mul(c, f2_pow(_GAMMA[k], i))
    return (tuple(out[0]), tuple(out[1]))


def f12_to_cyclotomic(a):
    """the easy part of the final exponentiation: a^((p^6 - 1)(p^2 + 1))"""
    g = f12_mul(f12_conj(a), f12_inv(a))
    return f12_mul(f12_frobenius(g, 2), g)


# ---------------------------------------------------------------- blocks of stored integers <-> elements
def blk(vals):
    """up to twelve stored integers -> an operand block of twelve"""
    vals = list(vals)
    return tuple(vals + [0] * (12 - len(vals)))


def d2(s, i=0):
    return (dec(s[i]), dec(s[i + 1]))


def d6(s, i=0):
    return (d2(s, i), d2(s, i + 2), d2(s, i + 4))


def d12(s):
    return (d6(s, 0), d6(s, 6))


def e2(a):
    return [enc(a[0]), enc(a[1])]


def e6(a):
    return e2(a[0]) + e2(a[1]) + e2(a[2])


def e12(a):
    return e6(a[0]) + e6(a[1])


def flat12(a):
    return tuple(x for f6 in a for f2 in f6 for x in f2)


# ---------------------------------------------------------------- witness streams
def w_bool(b):
    return ONE if b else 0


def w_is_eq(s, o):
    """AllocatedFp::is_neq(self, other): [is_not_equal, multiplier = (self - other)^-1 if unequal else 1]; -> (is_eq, stream)"""
    d = (s - o) % P
    return d == 0, [w_bool(d != 0), enc(inv(d)) if d else ONE]


class _Bool:
    """a Boolean of the constraint system: a constant or an allocated variable"""

    def __init__(self, value, const):
        self.value, self.const = bool(value), const


def w_to_bits_le(c):
    """FpVar::to_bits_le on a variable with canonical value c: the 381 bits as boolean witnesses, LSB first, then enforce_in_field_le =
    enforce_smaller_or_equal_than_le(bits, p - 1). That function walks the bits of p - 1 from the top beside the value's: a one of p - 1 appends
    the value's bit to the current run; a zero closes a non-empty run with last_run = kary_and(run + [last_run]) and then enforces
    nand(last_run, bit), which is kary_and([last_run, bit]) constrained to be zero. kary_and folds from the left with Boolean::and, and an `and`
    allocates its result as a witness unless an operand is a constant (true: the other operand is returned; last_run starts as the constant true)."""
    out = []

    def and_(x, y):
        if x.const:
            return y if x.value else x
        if y.const:
            return x if y.value else y
        r = _Bool(x.value and y.value, False)
        out.append(w_bool(r.value))
        return r

    def kary_and(bs):
        cur = bs[0]
        for nxt in bs[1:]:
            cur = and_(cur, nxt)
        return cur

    bits = [_Bool((c >> i) & 1, False) for i in range(381)]
    out += [w_bool(b.value) for b in bits]
    last_run, run = _Bool(True, True), []
    for i in range(380, -1, -1):
        if ((P - 1) >> i) & 1:
            run.append(bits[i])
        else:
            if run:
                run.append(last_run)
                last_run = kary_and(run)
                run = []
            kary_and([last_run, bits[i]])
    return out


TO_BITS_WITNESSES = 761  # independent of the value: 381 bits + 380 ANDs (one per bit of p - 1 below the first run's start, bar the first run's own)

# name -> (result elements, witnesses), in the order of DEVFIELD_OPS
OPS = {
    "fp_add": (1, 0), "fp_sub": (1, 0), "fp_neg": (1, 0), "fp_dbl": (1, 0), "fp_mul": (1, 0), "fp_mul32": (1, 0), "fp_sqr": (1, 0), "fp_inv": (1, 0),
    "fp_inv_fermat": (1, 0), "fp_to_canonical": (1, 0), "fp_from_u32": (1, 0), "fp_is_eq_w": (1, 2), "fp_to_bits_le_w": (1, TO_BITS_WITNESSES),
    "fp2_mul": (2, 0), "fp2_sqr": (2, 0), "fp2_mul_fp": (2, 0), "fp2_mul_xi": (2, 0), "fp2_inv": (2, 0), "fp2_inv2": (4, 0), "fp2_mul_w": (2, 3),
    "fp2_sqr_w": (2, 2), "fp2_inv_w": (2, 3), "fp2_div_w": (2, 3), "fp2_is_eq_w": (1, 5), "fp2_select_w": (2, 2),
    "fp6_mul_w": (6, 18), "fp6_mul_by_c0_c1_0_w": (6, 15), "fp12_mul_by_014_w_yvar": (12, 36), "fp12_mul_by_014_w_yconst": (12, 30),
    "fp12_sqr_w": (12, 36), "fp12_mul_w": (12, 54), "fp12_cyclotomic_square_w": (12, 18), "fp12_inv_w": (12, 54),
    "fp12_frobenius_1": (12, 0), "fp12_frobenius_2": (12, 0), "fp12_frobenius_3": (12, 0),
}
OP_NAMES = list(OPS)
INVERSION_OPS = ("fp_inv", "fp_is_eq_w", "fp2_inv", "fp2_inv2", "fp2_inv_w", "fp2_div_w", "fp2_is_eq_w", "fp12_inv_w")
HOST_STREAM_OPS = tuple(n for n in OP_NAMES if n.startswith(("fp6_", "fp12_")) and OPS[n][1])


def reference(op, a, b):
    """(result elements, witness stream or None) of operation `op` on the operand blocks a, b (twelve stored integers each)"""
    if op == "fp_add":
        return [(a[0] + b[0]) % P], []
    if op == "fp_sub":
        return [(a[0] - b[0]) % P], []
    if op == "fp_neg":
        return [(-a[0]) % P], []
    if op == "fp_dbl":
        return [2 * a[0] % P], []
    if op in ("fp_mul", "fp_mul32"):
        return [a[0] * b[0] * R_INV % P], []
    if op == "fp_sqr":
        return [a[0] * a[0] * R_INV % P], []
    if op in ("fp_inv", "fp_inv_fermat"):
        return [enc(inv(dec(a[0])))], []
    if op == "fp_to_canonical":
        return [dec(a[0])], []
    if op == "fp_from_u32":
        return [enc(a[0] & 0xFFFFFFFF)], []
    if op == "fp_is_eq_w":
        eq, w = w_is_eq(dec(a[0]), dec(b[0]))
        return [int(eq)], w
    if op == "fp_to_bits_le_w":
        c = dec(a[0])
        return [c & 1], w_to_bits_le(c)
    if op.startswith("fp2_"):
        x, y = d2(a), d2(b)
        if op == "fp2_mul":
            return e2(f2_mul(x, y)), []
        if op == "fp2_sqr":
            return e2(f2_mul(x, x)), []
        if op == "fp2_mul_fp":
            return e2((x[0] * y[0] % P, x[1] * y[0] % P)), []
        if op == "fp2_mul_xi":
            return e2(f2_mul(x, XI)), []
        if op == "fp2_inv":
            return e2(f2_inv(x)), []
        if op == "fp2_inv2":
            return e2(f2_inv(x)) + e2(f2_inv(y)), []
        if op == "fp2_mul_w":
            return e2(f2_mul(x, y)), [enc(x[0] * y[0]), enc(x[1] * y[1]), enc((x[0] + x[1]) * (y[0] + y[1]))]
        if op == "fp2_sqr_w":
            return e2(f2_mul(x, x)), [enc(x[0] * x[1]), enc((x[0] - x[1]) * (x[0] + x[1]))]
        if op == "fp2_inv_w":
            i = f2_inv(x)
            return e2(i), e2(i) + [enc(x[1] * i[1])]
        if op == "fp2_div_w":
            r = f2_mul(x, f2_inv(y))
            return e2(r), e2(r) + [enc(r[1] * y[1])]
        if op == "fp2_is_eq_w":
            e0, w0 = w_is_eq(x[0], y[0])
            e1, w1 = w_is_eq(x[1], y[1])
            return [int(e0 and e1)], w0 + w1 + [w_bool(e0 and e1)]
        if op == "fp2_select_w":
            r = e2(x if a[2] & 1 else y)
            return r, list(r)
    if op == "fp6_mul_w":
        return e6(f6_mul(d6(a), d6(b))), None
    if op == "fp6_mul_by_c0_c1_0_w":
        return e6(f6_mul(d6(a), (d2(b, 0), d2(b, 2), F2_ZERO))), None
    if op in ("fp12_mul_by_014_w_yvar", "fp12_mul_by_014_w_yconst"):
        other = ((d2(b, 0), d2(b, 2), F2_ZERO), (F2_ZERO, (dec(b[4]), 0), F2_ZERO))
        return e12(f12_mul(d12(a), other)), None
    if op in ("fp12_sqr_w", "fp12_cyclotomic_square_w"):
        x = d12(a)
        return e12(f12_mul(x, x)), None
    if op == "fp12_mul_w":
        return e12(f12_mul(d12(a), d12(b))), None
    if op == "fp12_inv_w":
        return e12(f12_inv(d12(a))), None
    if op.startswith("fp12_frobenius_"):
        return e12(f12_frobenius(d12(a), int(op[-1]))), []
    raise KeyError(op)


# ---------------------------------------------------------------- the cases: lists of (a, b) operand blocks per operation
def tower_elements(n):
    """stored Fp2 coefficient lists of length n (3: Fp6, 6: Fp12): 0, 1, a single non-zero coefficient in each position (an edge value, a random
    one), every coefficient p - 1, the inversion stress values spread over the coefficients, and three seeded random elements"""
    rng = random.Random(0x70E8 + n)
    rnd2 = lambda: (rng.randrange(P), rng.randrange(P))
    z = (0, 0)
    out = [[z] * n, [(ONE, 0)] + [z] * (n - 1)]
    singles = [(P - 1, 0), (0, P - 1), (1, 0), (0, ONE), (P - 1, P - 1), (E.INV_SLOW, E.INV_FAST)]
    for i in range(n):
        out.append([z] * i + [singles[i % len(singles)]] + [z] * (n - 1 - i))
        out.append([z] * i + [rnd2()] + [z] * (n - 1 - i))
    out.append([(P - 1, P - 1)] * n)
    out.append([(E.INV_SLOW, 0), (0, E.INV_FAST), (E.INV_SLOW_EDGE, P - 1)] * (n // 3))
    out += [[rnd2() for _ in range(n)] for _ in range(3)]
    return [blk(x for c in el for x in c) for el in out]


_CACHE = {}


def _memo(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def fp6_elements():
    return _memo("fp6", lambda: tower_elements(3))


def fp12_elements():
    return _memo("fp12", lambda: tower_elements(6))


def cyclotomic_elements():
    """1 and five seeded random elements pushed into the cyclotomic subgroup by the easy part of the final exponentiation (their product with
    their conjugate is 1: checked)"""
    def make():
        rng = random.Random(0xC1C10)
        out = [blk(e12(F12_ONE))]
        for _ in range(5):
            g = f12_to_cyclotomic(d12([rng.randrange(P) for _ in range(12)]))
            assert g != F12_ONE and f12_mul(g, f12_conj(g)) == F12_ONE
            out.append(blk(e12(g)))
        return out
    return _memo("cyc", make)


ZERO_BLK = blk([])


def _fp_pattern():
    """what an interleaved wave holds side by side: 0, 1, p - 1, the slowest and the fastest inversion found, random values"""
    rng = random.Random(0x1A7E)
    return [0, 1, P - 1, E.INV_SLOW, E.INV_FAST, ONE, E.INV_SLOW_EDGE] + [rng.randrange(P) for _ in range(6)]


def _fp2_pattern():
    f = _fp_pattern()
    return [(0, 0), (1, 0), (P - 1, P - 1), (E.INV_SLOW, E.INV_FAST), (E.INV_FAST, 0), (0, E.INV_SLOW), (ONE, 0), (0, 1)] + E.fp2_random(5, 0x1A7F) + [(f[7], 0), (f[8], (P - f[8]) % P)]


def cases(op):
    """{arrangement: [(a, b)]} for operation `op`. "edges": every edge operand, in one launch. "interleaved" (inversion-bearing operations): 0, 1,
    p - 1, the stress values and random values side by side in every wave. "uniform" (the same): every edge operand 64 times, a wave (four waves
    on quads) to itself. The launches over the item counts ITEM_COUNTS take their items from the front of "interleaved", or of a stride through
    "edges" (item_count_cases)."""
    return _memo(("cases", op), lambda: _cases(op))


def _cases(op):
    fv = E.field_edge_values() + [v for v, _ in E.INV_STRESS]
    f2 = E.fp2_operand_set() + E.fp2_random(4, 0xF2F2)
    unary = lambda vals: [(blk(v if isinstance(v, tuple) else [v]), ZERO_BLK) for v in vals]
    pairs = lambda xs, ys: [(blk(x if isinstance(x, tuple) else [x]), blk(y if isinstance(y, tuple) else [y])) for x in xs for y in ys]
    c = {}
    if op in ("fp_add", "fp_sub", "fp_mul", "fp_mul32"):
        c["edges"] = pairs(fv, fv)
    elif op in ("fp_neg", "fp_dbl", "fp_sqr", "fp_inv_fermat", "fp_to_canonical"):
        c["edges"] = unary(fv)
    elif op == "fp_inv":
        c["edges"] = unary(fv)
        c["uniform"] = E.uniform_waves(unary(fv))
        c["interleaved"] = E.interleaved(unary(_fp_pattern()))
    elif op == "fp_from_u32":
        c["edges"] = unary([0, 1, 2, 0xFFFF, 0x10000, 0x0FFFFFFF, 0x10000000, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 0xDEADBEEF])
    elif op == "fp_is_eq_w":
        c["edges"] = pairs(fv, fv)  # the diagonal: equal operands
        red = E.fp_reduced_edges()
        c["uniform"] = E.uniform_waves(pairs(red, [0]) + pairs(red, [P - 1]) + [(blk([x]), blk([x])) for x in red])
        pat = _fp_pattern()
        c["interleaved"] = E.interleaved([(blk([x]), blk([y])) for x, y in zip(pat, pat[:2] + pat[3:] + [pat[2]])])  # 0 == 0, 1 == 1, the rest unequal
    elif op == "fp_to_bits_le_w":
        c["edges"] = unary([enc(v) for v in E.to_bits_canonical_values()])
    elif op in ("fp2_mul", "fp2_mul_w"):
        c["edges"] = pairs(f2, f2)
    elif op in ("fp2_sqr", "fp2_sqr_w", "fp2_mul_xi"):
        c["edges"] = unary(f2)
    elif op == "fp2_mul_fp":
        c["edges"] = pairs(f2, E.fp_reduced_edges() + [2, (P + 1) // 2])
    elif op in ("fp2_inv", "fp2_inv_w"):
        c["edges"] = unary(f2)
        c["uniform"] = E.uniform_waves(unary(f2))
        c["interleaved"] = E.interleaved(unary(_fp2_pattern()))
    elif op in ("fp2_inv2", "fp2_div_w"):
        c["edges"] = pairs(f2, f2)  # first operand zero, second zero, both zero, a = b among them
        sel = [(0, 0), (1, 0), (P - 1, P - 1), (E.INV_SLOW, E.INV_FAST), (0, E.INV_SLOW_EDGE), f2[-1]]
        c["uniform"] = E.uniform_waves(pairs(sel, sel))
        pat = _fp2_pattern()
        c["interleaved"] = E.interleaved(pairs(pat, pat)[::7], 4 * E.WAVE)  # a stride coprime to the pattern's length: all combinations of zero / non-zero
    elif op == "fp2_is_eq_w":
        c["edges"] = pairs(f2, f2)  # equal operands on the diagonal; operands differing in c0 only, in c1 only and in both off it
        sel = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (E.INV_SLOW, E.INV_FAST), f2[-1]]
        c["uniform"] = E.uniform_waves(pairs(sel, sel) + [(blk(x), blk((x[0], y[1]))) for x in sel for y in sel[3:]] + [(blk(x), blk((y[0], x[1]))) for x in sel for y in sel[3:]])
        pat = _fp2_pattern()
        mixed = []
        for i, x in enumerate(pat):
            y = pat[(i + 1) % len(pat)]
            mixed += [(blk(x), blk(x)), (blk(x), blk((y[0], x[1]))), (blk(x), blk((x[0], y[1]))), (blk(x), blk(y))]
        c["interleaved"] = E.interleaved(mixed, 4 * E.WAVE)
    elif op == "fp2_select_w":
        sel = f2[::3]
        c["edges"] = [(blk(x + (k,)), blk(y)) for x in sel for y in sel for k in (0, 1)] + [(blk(f2[5] + (k,)), blk(f2[6])) for k in (2, 3, P - 1, 1 << 32, (1 << 32) + 1)]
    elif op == "fp6_mul_w":
        c["edges"] = [(x, y) for x in fp6_elements() for y in fp6_elements()]
    elif op == "fp6_mul_by_c0_c1_0_w":
        sparse = [blk(x + y) for x in f2[::9] for y in f2[4::11]]
        c["edges"] = [(x, y) for x in fp6_elements() for y in sparse]
    elif op in ("fp12_mul_by_014_w_yvar", "fp12_mul_by_014_w_yconst"):
        ys = [0, 1, P - 1, ONE, E.INV_SLOW]
        sparse = [blk(x + y + (ys[(i + j) % len(ys)],)) for i, x in enumerate(f2[::13]) for j, y in enumerate(f2[4::17])]
        c["edges"] = [(x, y) for x in fp12_elements() for y in sparse]
    elif op in ("fp12_sqr_w", "fp12_frobenius_1", "fp12_frobenius_2", "fp12_frobenius_3"):
        c["edges"] = [(x, ZERO_BLK) for x in fp12_elements() + cyclotomic_elements()]
    elif op == "fp12_mul_w":
        c["edges"] = [(x, y) for x in fp12_elements() for y in fp12_elements()]
    elif op == "fp12_cyclotomic_square_w":
        c["edges"] = [(x, ZERO_BLK) for x in cyclotomic_elements()]
    elif op == "fp12_inv_w":
        els = [(x, ZERO_BLK) for x in fp12_elements() + cyclotomic_elements()]  # 0 among them
        c["edges"] = els
        c["uniform"] = E.uniform_waves(els)
        c["interleaved"] = E.interleaved(els)
    else:
        raise KeyError(op)
    assert (op in INVERSION_OPS) == ("uniform" in c) == ("interleaved" in c)
    return c


def item_count_cases(op):
    """[(n, items)] for n in ITEM_COUNTS: the first n items of the interleaved arrangement (inversion-bearing operations) or of a walk through
    the edge cases with a stride coprime to their number (so that a short launch still mixes the operand kinds)"""
    c = cases(op)
    if "interleaved" in c:
        src = c["interleaved"]
        walk = [src[i % len(src)] for i in range(max(E.ITEM_COUNTS))]
    else:
        src = c["edges"]
        step = next(s for s in (37, 41, 43, 47, 53) if len(src) % s) if len(src) > 1 else 1
        walk = [src[i * step % len(src)] for i in range(max(E.ITEM_COUNTS))]
    return [(n, walk[:n]) for n in E.ITEM_COUNTS]


def all_launches(op):
    """[(arrangement name, items)]: every launch of operation `op`, the same for the host test and for each device build"""
    return list(cases(op).items()) + [("n=%d" % n, items) for n, items in item_count_cases(op)]


def expected(op, items, host_stream=None):
    """[(results, stream)] per item, computed once per distinct operand pair. host_stream(op, a, b) supplies the streams the reference does not state
    (HOST_STREAM_OPS)."""
    memo = _CACHE.setdefault(("expected", op), {})
    out = []
    for a, b in items:
        if (a, b) not in memo:
            res, w = reference(op, a, b)
            if w is None:
                w = host_stream(op, a, b)
            assert len(res) == OPS[op][0] and len(w) == OPS[op][1], op
            memo[(a, b)] = (res, w)
        out.append(memo[(a, b)])
    return out
