"""Operands, message lengths and launches for the SHA gadget operation table (tests/devsha/ops.hpp), shared by tests/test_sha_ref.py (host) and
tests/test_sha_device_gpu.py (device). A case is (operand words, message); a launch is a list of cases with one message length."""
import random

from tests import sha_ref as S

M32 = 0xFFFFFFFF
ITEM_COUNTS = (1, 63, 64, 65, 70)
LANES = 70

_rng = random.Random(0x5A256)
WORDS = [0, 1, 0x80000000, M32, 0x55555555, 0xAAAAAAAA, 1 << 0, 1 << 7, 1 << 8, 1 << 31] + [_rng.getrandbits(32) for _ in range(6)]
ROTR_COUNTS = (2, 6, 7, 11, 13, 17, 18, 19, 22, 25)  # every rotation of the gadget
SHR_COUNTS = (3, 10)
PEXT_MASKS = [0, M32, 1, 0xFF, 0xFFFF, 0x7FFFFFFF, 1 << 7, 1 << 31, 0x55555555, 0xAAAAAAAA, 0xFF00FF00, 0x00FFFF00] + [_rng.getrandbits(32) for _ in range(6)]

# every msg_len in 0 .. 130 (each residue mod 64 twice; the block count (msg_len + 183) // 64 changes at 9, 73, 137), the later borders, long
# messages, and the first lengths whose bit length has a third byte (msg_len + 111 >= 8192)
STREAM_LENGTHS = list(range(0, 131)) + [136, 137, 183, 184, 185, 247, 248, 249, 1000, 8080, 8081]
VALUE_ONLY_LENGTHS = [65535]
LENGTHS = STREAM_LENGTHS + VALUE_ONLY_LENGTHS


def messages(msg_len, lanes=LANES):
    """`lanes` different messages of one length: all 0x00, all 0xFF, a counter pattern, then random bytes"""
    rng = random.Random(msg_len * 1000003 + lanes)
    out = [bytes(msg_len), b"\xff" * msg_len, bytes((i * 7 + 1) & 0xFF for i in range(msg_len))]
    while len(out) < lanes:
        out.append(rng.getrandbits(8 * msg_len).to_bytes(msg_len, "little") if msg_len else b"")
    return out[:lanes]


# ---------------------------------------------------------------- mask triples
def triple(kinds):
    """32 bit kinds (indices into sha_ref.KIND_NAMES, bit 0 first) -> (v, cm, nm)"""
    v = sum((k & 1) << i for i, k in enumerate(kinds))
    cm = sum(1 << i for i, k in enumerate(kinds) if k < 2)
    nm = sum(1 << i for i, k in enumerate(kinds) if k >= 4)
    return (v, cm, nm)


def kind_pair_triples():
    """pairs of triples in which every ordered pair of the six bit kinds meets at bit 0, at bit 31 and spread over a word"""
    out = []
    for fill in ((2, 2), (0, 3)):  # the other bits: variables, then constants
        for a in range(6):
            for b in range(6):
                for pos in (0, 31):
                    ka, kb = [fill[0]] * 32, [fill[1]] * 32
                    ka[pos], kb[pos] = a, b
                    out.append((triple(ka), triple(kb)))
    for shift in range(6):  # spread: bit i holds the pair (i % 6, (i // 6 + i + shift) % 6): 36 pairs over the six words
        ka = [i % 6 for i in range(32)]
        kb = [(i // 6 + i + shift) % 6 for i in range(32)]
        out.append((triple(ka), triple(kb)))
    return out


def shape_triples():
    """all-constant, all-variable, all-negated, one variable bit, one constant bit, byte-wise mixtures as b0_byte makes them, random"""
    rng = random.Random(77)
    out = []
    for v in (0, M32, 0x12345678):
        out += [(v, M32, 0), (v, 0, 0), (v, 0, M32), (v, M32 ^ (1 << 5), 0), (v, 1 << 31, 0), (v, 1 << 0, M32 ^ 1)]
        out += [(v, cm, 0) for cm in (0xFF000000, 0x00FFFFFF, 0xFFFF0000, 0x0000FFFF, 0xFF0000FF, 0x00FF0000, 0xFFFFFF00)]
    for _ in range(8):
        cm = rng.getrandbits(32)
        out.append((rng.getrandbits(32), cm, rng.getrandbits(32) & ~cm & M32))
    return out


def _flat(*triples):
    return tuple(x for t in triples for x in t)


def addmany_operands(k):
    """value lists for k operands: all 0xffffffff (the largest carry), sums of exactly 2^32, 2^33, 2^34 and one below each (where k operands
    reach them), all zero, every carry value 0 .. k - 1, random"""
    rng = random.Random(k)
    out = [[M32] * k, [0] * k]
    for total in (1 << 32, (1 << 32) - 1, 1 << 33, (1 << 33) - 1, 1 << 34, (1 << 34) - 1):
        if total <= k * M32:
            vals, rest = [], total
            for i in range(k):
                v = min(M32, rest) if i < k - 1 else rest
                v = min(v, M32)
                vals.append(v)
                rest -= v
            assert rest == 0 and sum(vals) == total
            out.append(vals)
            out.append(vals[::-1])
    for carry in range(k):
        out.append([M32] * carry + [1 if carry else 0] + [0] * (k - carry - 1))
    out += [[rng.getrandbits(32) for _ in range(k)] for _ in range(6)]
    return out


_CASES = {}


def cases(op, msg_len=0):
    """the cases of an entry without a message -> list of (operand words, b"")"""
    if op not in _CASES:
        _CASES[op] = [(tuple(w), b"") for w in _build(op)]
    return _CASES[op]


def _build(op):
    rng = random.Random(len("sha_block" if op.startswith("sha_block") else op) * 31 + 5)  # the two block entries share their cases
    var = lambda v: (v, 0, 0)
    con = lambda v: (v, M32, 0)
    pairs = kind_pair_triples()
    shapes = shape_triples()
    if op in ("w_xor", "w_and"):
        out = [_flat(a, b) for a, b in pairs]
        out += [_flat(a, b) for a in shapes[::3] for b in shapes[1::4]]
        out += [_flat(var(a), var(b)) for a in WORDS[:10] for b in WORDS[:10:3]]
        return out
    if op == "w_not":
        return [_flat(t) for t in shapes] + [_flat(var(w)) for w in WORDS]
    if op in ("w_rotr", "w_shr"):
        counts = ROTR_COUNTS if op == "w_rotr" else SHR_COUNTS + (1, 31)
        return [_flat(t) + (n,) for t in shapes for n in counts]
    if op.startswith("w_addmany"):
        k = int(op[-1])
        out = []
        for vals in addmany_operands(k):
            out.append(_flat(*[var(v) for v in vals]))                                # all variables
            out.append(_flat(*[con(v) for v in vals]))                                # all constants: folds, no bit leaves
            out.append(_flat(*[con(v) if i else var(v) for i, v in enumerate(vals)]))  # one variable operand: constants count in k
            out.append(_flat(*[(v, 0xFFFFFFFE, 0) if i == k - 1 else con(v) for i, v in enumerate(vals)]))  # one variable BIT
        for _ in range(6):
            out.append(_flat(*[shapes[rng.randrange(len(shapes))] for _ in range(k)]))
        return out
    if op == "pext32":
        return [(v, m) for m in PEXT_MASKS for v in WORDS[:6] + WORDS[10:13]]
    if op == "popc32":
        return [(w,) for w in WORDS + PEXT_MASKS]
    if op == "sigma_var":
        return [(w, which) for w in WORDS for which in (0, 1)]
    if op == "sha_sched_word":
        out = []
        kinds = {"var": lambda: var(rng.getrandbits(32)), "const": lambda: con(rng.getrandbits(32)),
                 "mixed": lambda: (rng.getrandbits(32), rng.choice((0xFF000000, 0x00FFFFFF, 0xFFFF0000, 0x000000FF, 0x00FF0000)), 0)}
        for k15 in kinds:
            for k2 in kinds:
                for k16, k7 in (("var", "var"), ("const", "const"), ("const", "var"), ("mixed", "const")):
                    out.append(_flat(kinds[k16](), kinds[k15](), kinds[k7](), kinds[k2]()))
        out += [_flat(con(a), con(b), con(a ^ b), con(b)) for a in WORDS[:6] for b in (0, M32, 0x80000000)]  # all four constant: no bit leaves
        out += [_flat(var(M32), var(M32), var(M32), var(M32)), _flat(var(0), var(0), var(0), var(0))]
        return out
    if op == "sha_round_var":
        out = [tuple([w] * 8 + [w, S.SHA_K[0]]) for w in (0, M32)]
        out += [tuple([M32] * 9 + [M32])]  # the largest 35-bit sum
        out += [tuple(rng.getrandbits(32) for _ in range(9)) + (S.SHA_K[i],) for i in (0, 1, 63, 17, 40)]
        return out
    if op in ("sha_block_w", "sha_block_generic"):
        r32 = lambda: rng.getrandbits(32)
        vstate = lambda: [var(r32()) for _ in range(8)]
        cstate = [con(v) for v in S.SHA_H0]
        mixed = lambda: (r32(), rng.choice((0xFF000000, 0x00FFFFFF, 0xFFFF0000, 0x000000FF)), 0)
        first = lambda cm: (r32(), cm, 0)
        out = [
            vstate() + [var(r32()) for _ in range(16)],                                        # variable state, variable data
            vstate() + [con(r32()) for _ in range(16)],                                        # ... constant data (the second block of b1 .. b8)
            vstate() + [var(r32()), mixed(), mixed()] + [con(r32()) for _ in range(13)],       # ... mixed data (the last block of msg')
            [var(M32)] * 8 + [var(M32)] * 16,
            cstate + [first(0)] + [var(r32()) for _ in range(15)],                             # constant state, variable data[0]
            cstate + [first(0x0000FFFF)] + [con(r32()) for _ in range(15)],                    # msg_len 0: lib_str | 0 | DST
            cstate + [first(0x000000FF), mixed()] + [con(r32()) for _ in range(14)],           # msg_len 1
            cstate + [first(0), first(0xFFFF0000)] + [con(r32()) for _ in range(14)],          # msg_len 2
            cstate + [first(0), first(0x00FFFFFF)] + [con(r32()) for _ in range(14)],          # msg_len 3
            cstate + [con(r32()) for _ in range(16)],                                          # constant state, constant data: no bit may leave
            [con(r32())] * 4 + vstate()[:4] + [var(r32()) for _ in range(16)],                 # a mixed state: the fallback
            [mixed() for _ in range(8)] + [mixed() for _ in range(16)],
        ]
        return [_flat(*c) for c in out]
    if op == "hash_to_field_elem":
        P = S.P
        vals = [0, 1, (1 << 136) - 1, 1 << 136, ((1 << 376) - 1) << 136, S.P - 1, S.P, S.P + 1, (1 << 512) - 1, (1 << 512) // P * P, (1 << 511) // P * P,
                (1 << 512) // P * P - 1, (1 << 511) // P * P + 1, 0xFF << 136, 0xFFFF << 128, 1 << 143, 1 << 144, (1 << 512) - (1 << 136)]
        vals += [rng.getrandbits(512) for _ in range(12)]
        return [tuple((v >> (32 * (15 - i))) & M32 for i in range(16)) for v in vals]
    raise KeyError(op)


def msg_cases(op, msg_len, lanes=LANES):
    """the cases of an entry that takes a message, at one length"""
    msgs = messages(msg_len, lanes)
    if op == "b0_block":
        nblocks = (msg_len + 111 + 9 + 63) // 64
        return [((blk, c), msgs[(blk + c) % len(msgs)]) for blk in range(nblocks) for c in (0, 1)]
    return [((), m) for m in msgs]


B0_LENGTHS = [0, 1, 2, 3, 4, 8, 9, 10, 55, 56, 64, 72, 73, 74, 137, 8080, 8081]


def launches(op):
    """[(name, msg_len, cases)] for an entry without a message: every case in order, the same shuffled, and the item counts (a single item, a
    partial wave, a whole wave, a wave and one item, a wave and six)"""
    if S.OPS[op][2]:
        raise KeyError(op)
    cs = cases(op)
    sh = list(cs)
    random.Random(len(cs)).shuffle(sh)
    out = [("in order", 0, cs), ("shuffled", 0, sh)]
    for n in ITEM_COUNTS:
        out.append(("%d items" % n, 0, [sh[i % len(sh)] for i in range(n)]))
    return out


def xor_and_kind_pairs(op):
    """the set of (kind of a's bit, kind of b's bit) over every bit of every case of w_xor / w_and"""
    seen = set()
    for w, _ in cases(op):
        seen.update(zip(S.bit_kinds(w[0:3]), S.bit_kinds(w[3:6])))
    return seen
