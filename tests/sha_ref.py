"""Reference for the SHA-256 gadget and hash_to_field layer (csrc/sha.hpp), in two tiers, written without reading sha.hpp's masks.

MEANING: expand_message_xmd of RFC 9380 5.3.1 with hashlib and hash_to_field as int.from_bytes(64 bytes, "big") % p; the SHA-256 constants are
derived here from the primes (FIPS 180-4 4.2.2, 5.3.3), the Montgomery radix from pow. Nothing is taken from csrc/.

BITS: a restatement of what ark-r1cs-std 0.4 / ark-crypto-primitives 0.4 allocate. A Boolean is Constant, Is(var) or Not(var),
tracked per bit; xor / and allocate one witness exactly when both sides are variables, with arkworks' case tables; UInt32::addmany folds
all-constant operands and otherwise allocates bit_length(k (2^32 - 1)) result bits (constants count in k); Sha256Gadget::update_state and digest,
the bytewise UInt8 xor of b0 and b_(i-1), the two lib_str witness bytes first. The output is the allocation-order bit stream and the 64 output
words. LANES are the bits of Python integers: one integer per Boolean, bit i for lane i, so the circuit shape is walked once per message length
whatever the number of messages. A bit stream is only handed out after its digests have been held to the meaning tier (expand_gadget asserts
it)."""
import hashlib

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = pow(2, 384, P)
DST = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"  # the proof-of-possession ciphersuite of draft-irtf-cfrg-bls-signature
DST_PRIME = DST + bytes([len(DST)])
LEN_IN_BYTES = 256
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- meaning
def msg_prime(msg):
    """Z_pad(64) | msg | I2OSP(256, 2) | I2OSP(0, 1) | DST | I2OSP(43, 1)"""
    mp = bytes(64) + bytes(msg) + LEN_IN_BYTES.to_bytes(2, "big") + b"\x00" + DST_PRIME
    n = len(msg)
    assert len(mp) == n + 111 and mp[:64] == bytes(64) and mp[64:64 + n] == bytes(msg) and mp[64 + n:64 + n + 3] == b"\x01\x00\x00"
    assert mp[67 + n:110 + n] == DST and mp[110 + n] == 43 == len(DST)
    return mp


def expand_message_xmd(msg, len_in_bytes=LEN_IN_BYTES, dst=DST):
    ell = (len_in_bytes + 31) // 32
    assert ell <= 255 and len(dst) <= 255
    dst_prime = dst + bytes([len(dst)])
    mp = bytes(64) + bytes(msg) + len_in_bytes.to_bytes(2, "big") + b"\x00" + dst_prime
    if dst == DST and len_in_bytes == LEN_IN_BYTES:
        assert mp == msg_prime(msg)
    b0 = hashlib.sha256(mp).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(b)[:len_in_bytes]


def uniform_words(msg):
    u = expand_message_xmd(msg)
    return [int.from_bytes(u[4 * i:4 * i + 4], "big") for i in range(64)]


def hash_to_field(b64):
    assert len(b64) == 64
    return int.from_bytes(b64, "big") % P


def mont_limbs32(v):
    """the element v in Montgomery form, as 12 little-endian 32-bit limbs"""
    m = v * R % P
    return [(m >> (32 * i)) & M32 for i in range(12)]


def sha_padding(total):
    """the bytes FIPS 180-4 5.1.1 appends to a message of `total` bytes"""
    return b"\x80" + bytes((55 - total) % 64) + (8 * total).to_bytes(8, "big")


def _iroot(n, k):
    lo, hi = 0, 1 << (n.bit_length() // k + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** k <= n:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _primes(n):
    out, c = [], 2
    while len(out) < n:
        if all(c % q for q in out):
            out.append(c)
        c += 1
    return out


SHA_K = [_iroot(q << 96, 3) & M32 for q in _primes(64)]  # fractional parts of the cube roots
SHA_H0 = [_iroot(q << 64, 2) & M32 for q in _primes(8)]  # fractional parts of the square roots


def _check_constants():
    """the derived constants give hashlib's digest on one block, through a plain integer compression"""
    w = [int.from_bytes((b"abc" + sha_padding(3))[4 * i:4 * i + 4], "big") for i in range(16)]
    rot = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    for i in range(16, 64):
        s0 = rot(w[i - 15], 7) ^ rot(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rot(w[i - 2], 17) ^ rot(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    h = list(SHA_H0)
    for i in range(64):
        a, b, c, d, e, f, g, hh = h
        t0 = (hh + (rot(e, 6) ^ rot(e, 11) ^ rot(e, 25)) + ((e & f) ^ (~e & g & M32)) + SHA_K[i] + w[i]) & M32
        t1 = ((rot(a, 2) ^ rot(a, 13) ^ rot(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        h = [(t0 + t1) & M32, a, b, c, (d + t0) & M32, e, f, g]
    dig = b"".join(((x + y) & M32).to_bytes(4, "big") for x, y in zip(SHA_H0, h))
    assert dig == hashlib.sha256(b"abc").digest()


_check_constants()

# ---------------------------------------------------------------- bits
CONST, IS, NOT = 0, 1, 2
KIND_NAMES = ("const 0", "const 1", "Is 0", "Is 1", "Not 0", "Not 1")


class Gadget:
    """one constraint-system walk over `lanes` assignments at once. A Boolean is (kind, x): Constant with x = 0 or the all-lanes mask, Is / Not
    with x = the underlying variable's value in every lane. stream: the value of every allocated boolean witness, in allocation order."""

    def __init__(self, lanes=1):
        self.lanes = lanes
        self.M = (1 << lanes) - 1
        self.stream = []
        self.marks = []  # (stream position, label)
        self.label = ""
        self.carries = {}  # addmany operand count -> set of the values of the result above bit 31, over lanes

    # -- Boolean
    def const(self, bit):
        return (CONST, self.M if bit else 0)

    def witness(self, x):
        self.stream.append(x)
        return (IS, x)

    def value(self, b):
        return b[1] ^ self.M if b[0] == NOT else b[1]

    def not_(self, b):
        k, x = b
        if k == CONST:
            return (CONST, x ^ self.M)
        return (NOT, x) if k == IS else (IS, x)

    def xor(self, a, b):
        (ka, xa), (kb, xb) = a, b
        if ka == CONST:
            return self.not_(b) if xa else b
        if kb == CONST:
            return self.not_(a) if xb else a
        w = xa ^ xb  # AllocatedBool::xor of the two variables
        self.stream.append(w)
        return (IS, w) if ka == kb else (NOT, w)  # Is ^ Is = Not ^ Not = Is(w); Is ^ Not = Not(w)

    def and_(self, a, b):
        (ka, xa), (kb, xb) = a, b
        if ka == CONST:
            return b if xa else (CONST, 0)
        if kb == CONST:
            return a if xb else (CONST, 0)
        M = self.M
        if ka == IS and kb == IS:
            w = xa & xb           # AllocatedBool::and
        elif ka == IS:
            w = xa & (xb ^ M)     # and_not
        elif kb == IS:
            w = xb & (xa ^ M)     # and_not
        else:
            w = (xa | xb) ^ M     # nor
        self.stream.append(w)
        return (IS, w)

    # -- UInt32: 32 Booleans, little-endian
    def word_const(self, v):
        return [self.const((v >> i) & 1) for i in range(32)]

    def word_vars(self, per_lane):
        """an all-variable word that is NOT allocated here (the message, a state handed in): Is(var) with the lanes' values"""
        return [(IS, sum(((v >> i) & 1) << l for l, v in enumerate(per_lane))) for i in range(32)]

    def word_values(self, w):
        """-> the word's value in every lane"""
        vals = [self.value(b) for b in w]
        return [sum(((vals[i] >> l) & 1) << i for i in range(32)) for l in range(self.lanes)]

    @staticmethod
    def rotr(w, n):
        return w[n:] + w[:n]

    def shr(self, w, n):
        return w[n:] + [self.const(0)] * n

    def xor32(self, a, b):
        return [self.xor(x, y) for x, y in zip(a, b)]

    def and32(self, a, b):
        return [self.and_(x, y) for x, y in zip(a, b)]

    def not32(self, a):
        return [self.not_(x) for x in a]

    def addmany(self, ops):
        k = len(ops)
        assert k >= 2
        if all(b[0] == CONST for w in ops for b in w):
            total = sum(sum(1 << i for i in range(32) if w[i][1]) for w in ops)
            return self.word_const(total & M32)
        nbits = (k * M32).bit_length()
        acc = [self.value(b) for b in ops[0]] + [0] * (nbits - 32)
        for w in ops[1:]:
            c = 0
            for i in range(nbits):
                a = acc[i]
                b = self.value(w[i]) if i < 32 else 0
                t = a ^ b
                acc[i] = t ^ c
                c = (a & b) | (c & t)
            assert c == 0
        self.stream.extend(acc)
        seen = self.carries.setdefault(k, set())
        if len(seen) < k:
            for l in range(self.lanes):
                seen.add(sum(((acc[i] >> l) & 1) << (i - 32) for i in range(32, nbits)))
        return [(IS, x) for x in acc[:32]]

    # -- Sha256Gadget
    def mark(self, what):
        self.marks.append((len(self.stream), self.label + what))

    def sched_word(self, w16, w15, w7, w2):
        s0 = self.xor32(self.xor32(self.rotr(w15, 7), self.rotr(w15, 18)), self.shr(w15, 3))
        s1 = self.xor32(self.xor32(self.rotr(w2, 17), self.rotr(w2, 19)), self.shr(w2, 10))
        return self.addmany([w16, s0, w7, s1])

    def round(self, h, wi, k):
        ch = self.xor32(self.and32(h[4], h[5]), self.and32(self.not32(h[4]), h[6]))
        x1, x2, x3 = self.and32(h[0], h[1]), self.and32(h[0], h[2]), self.and32(h[1], h[2])
        ma = self.xor32(self.xor32(x1, x2), x3)
        s0 = self.xor32(self.xor32(self.rotr(h[0], 2), self.rotr(h[0], 13)), self.rotr(h[0], 22))
        s1 = self.xor32(self.xor32(self.rotr(h[4], 6), self.rotr(h[4], 11)), self.rotr(h[4], 25))
        t0 = self.addmany([h[7], s1, ch, self.word_const(k), wi])
        t1 = self.addmany([s0, ma])
        e = self.addmany([h[3], t0])
        a = self.addmany([t0, t1])
        return [a, h[0], h[1], h[2], e, h[4], h[5], h[6]]

    def update_state(self, state, data):
        w = list(data)
        for i in range(16, 64):
            self.mark("schedule word %d" % i)
            w.append(self.sched_word(w[i - 16], w[i - 15], w[i - 7], w[i - 2]))
        h = list(state)
        for i in range(64):
            self.mark("round %d" % i)
            h = self.round(h, w[i], SHA_K[i])
        self.mark("state sums")
        return [self.addmany([s, x]) for s, x in zip(state, h)]

    def digest(self, data, name=""):
        """data: UInt8s (8 Booleans each, little-endian) -> 32 UInt8s"""
        pad = [[self.const((byte >> j) & 1) for j in range(8)] for byte in sha_padding(len(data))]
        data = list(data) + pad
        assert len(data) % 64 == 0
        state = [self.word_const(v) for v in SHA_H0]
        for blk in range(len(data) // 64):
            self.label = "%s block %d, " % (name, blk)
            chunk = data[64 * blk:64 * blk + 64]
            words = [chunk[4 * i + 3] + chunk[4 * i + 2] + chunk[4 * i + 1] + chunk[4 * i] for i in range(16)]  # UInt32::from_bytes_be
            state = self.update_state(state, words)
        return [w[24 - 8 * j:32 - 8 * j] for w in state for j in range(4)]  # to_bytes_be

    def byte_const(self, v):
        return [self.const((v >> j) & 1) for j in range(8)]

    def byte_values(self, b):
        vals = [self.value(x) for x in b]
        return [sum(((vals[j] >> l) & 1) << j for j in range(8)) for l in range(self.lanes)]


def expand_gadget(msgs):
    """hasher.rs's expand_message_xmd gadget for equally long messages, one per lane -> (gadget, uniform words [lane][64]). The message bytes are
    variables allocated before this segment; the stream holds the segment's own witnesses. Every lane's b1 .. b8 are asserted against hashlib."""
    n = len(msgs[0])
    assert all(len(m) == n for m in msgs)
    g = Gadget(len(msgs))
    lib_str = [[g.witness(g.M if (byte >> j) & 1 else 0) for j in range(8)] for byte in LEN_IN_BYTES.to_bytes(2, "big")]
    msg = [[(IS, sum(((m[k] >> j) & 1) << l for l, m in enumerate(msgs))) for j in range(8)] for k in range(n)]
    dst_prime = [g.byte_const(v) for v in DST_PRIME]
    mp = [g.byte_const(0)] * 64 + msg + lib_str + [g.byte_const(0)] + dst_prime
    b0 = g.digest(mp, "b0")
    out, last = [], None
    for i in range(1, 9):
        if i == 1:
            head = b0
        else:
            g.label = "b%d, " % i
            g.mark("xor of b0 and b%d" % (i - 1))
            head = [[g.xor(x, y) for x, y in zip(p, q)] for p, q in zip(b0, last)]
        last = g.digest(head + [g.byte_const(i)] + dst_prime, "b%d" % i)
        out += last
    per_byte = [g.byte_values(b) for b in out]
    words = []
    for l, m in enumerate(msgs):
        u = bytes(per_byte[k][l] for k in range(256))
        assert u == expand_message_xmd(m), "the gadget walk disagrees with hashlib at lane %d, msg_len %d" % (l, n)
        words.append([int.from_bytes(u[4 * i:4 * i + 4], "big") for i in range(64)])
    return g, words


def stream_matrix(stream, lanes):
    """a lane-integer stream -> uint8 [lanes][bits]"""
    if not stream:
        return np.zeros((lanes, 0), dtype=np.uint8)
    nb = (lanes + 7) // 8
    raw = np.frombuffer(b"".join(x.to_bytes(nb, "little") for x in stream), dtype=np.uint8).reshape(len(stream), nb)
    return np.ascontiguousarray(np.unpackbits(raw, axis=1, bitorder="little")[:, :lanes].T)


def where_is(marks, pos):
    """the label of the last mark at or before stream position pos"""
    name = "lib_str"
    for p, label in marks:
        if p > pos:
            break
        name = label
    return name


# ---------------------------------------------------------------- the operation table of tests/devsha/ops.hpp
# name -> (operand words, result words, takes a message)
OPS = {
    "w_xor": (6, 3, 0), "w_and": (6, 3, 0), "w_not": (3, 3, 0), "w_rotr": (4, 3, 0), "w_shr": (4, 3, 0),
    "w_addmany2": (6, 3, 0), "w_addmany3": (9, 3, 0), "w_addmany4": (12, 3, 0), "w_addmany5": (15, 3, 0),
    "pext32": (2, 1, 0), "popc32": (1, 1, 0), "sigma_var": (2, 4, 0), "sha_sched_word": (12, 3, 0), "sha_round_var": (10, 16, 0),
    "sha_block_w": (72, 24, 0), "sha_block_generic": (72, 24, 0), "b0_block": (2, 32, 1), "expand_message_w": (0, 64, 1),
    "expand_message_values": (0, 64, 1), "hash_to_field_elem": (16, 12, 0),
}
OP_NAMES = list(OPS)


def from_triple(g, t):
    """(v, cm, nm) -> 32 Booleans of a one-lane gadget: a constant where cm, Not(var) where nm, Is(var) elsewhere; v holds the Boolean's VALUE"""
    v, cm, nm = t
    assert cm & nm == 0
    out = []
    for i in range(32):
        bit = (v >> i) & 1
        if (cm >> i) & 1:
            out.append(g.const(bit))
        elif (nm >> i) & 1:
            out.append((NOT, bit ^ 1))
        else:
            out.append((IS, bit))
    return out


def to_triple(g, w):
    v = sum(g.value(b) << i for i, b in enumerate(w))
    cm = sum(1 << i for i, b in enumerate(w) if b[0] == CONST)
    nm = sum(1 << i for i, b in enumerate(w) if b[0] == NOT)
    return [v, cm, nm]


def bit_kinds(t):
    """the kind of each bit of a triple, as an index into KIND_NAMES"""
    v, cm, nm = t
    return [(0 if (cm >> i) & 1 else (4 if (nm >> i) & 1 else 2)) + ((v >> i) & 1) for i in range(32)]


_EXPECT = {}


def expected(op, case):
    """case = (operand words tuple, message bytes) -> (result words, bit stream as a list of 0 / 1); cached"""
    key = (op, case)
    if key not in _EXPECT:
        _EXPECT[key] = _expected(op, case[0], case[1])
    return _EXPECT[key]


def _expected(op, w, msg):
    g = Gadget(1)
    t = lambda i: from_triple(g, w[3 * i:3 * i + 3])
    if op == "w_xor":
        out = to_triple(g, g.xor32(t(0), t(1)))
    elif op == "w_and":
        out = to_triple(g, g.and32(t(0), t(1)))
    elif op == "w_not":
        out = to_triple(g, g.not32(t(0)))
    elif op == "w_rotr":
        out = to_triple(g, g.rotr(t(0), w[3]))
    elif op == "w_shr":
        out = to_triple(g, g.shr(t(0), w[3]))
    elif op.startswith("w_addmany"):
        out = to_triple(g, g.addmany([t(i) for i in range(int(op[-1]))]))
    elif op == "pext32":
        picked = [(w[0] >> i) & 1 for i in range(32) if (w[1] >> i) & 1]
        out = [sum(b << k for k, b in enumerate(picked))]
    elif op == "popc32":
        out = [bin(w[0]).count("1")]
    elif op == "sigma_var":
        r1, r2, sh = (17, 19, 10) if w[1] else (7, 18, 3)
        out = []
        for _ in range(2):  # the fast path's bits, then the bits of the two generic xor it replaces: the same
            x = from_triple(g, (w[0], 0, 0))
            r = to_triple(g, g.xor32(g.xor32(g.rotr(x, r1), g.rotr(x, r2)), g.shr(x, sh)))
            out = [r[0]] + r if not out else out
    elif op == "sha_sched_word":
        out = to_triple(g, g.sched_word(t(0), t(1), t(2), t(3)))
    elif op == "sha_round_var":
        out = []
        for _ in range(2):  # sha_round_var, then sha_round_generic: the same bits
            h = g.round([from_triple(g, (x, 0, 0)) for x in w[:8]], from_triple(g, (w[8], 0, 0)), w[9])
            assert all(b[0] == IS for x in h for b in x)
            out += [to_triple(g, x)[0] for x in h]
    elif op in ("sha_block_w", "sha_block_generic"):
        st = g.update_state([t(i) for i in range(8)], [t(8 + i) for i in range(16)])
        out = [x for s in st for x in to_triple(g, s)]
    elif op == "b0_block":
        mp = msg_prime(msg)
        padded = mp + sha_padding(len(mp))
        var = set(range(64 + len(msg), 66 + len(msg))) | (set() if w[1] else set(range(64, 64 + len(msg))))
        blk = padded[64 * w[0]:64 * w[0] + 64]
        assert len(blk) == 64
        out = [int.from_bytes(blk[4 * i:4 * i + 4], "big") for i in range(16)]
        out += [sum(0xFF << (8 * (3 - b)) for b in range(4) if 64 * w[0] + 4 * i + b not in var) for i in range(16)]
    elif op == "expand_message_values":
        out = uniform_words(msg)
    elif op == "hash_to_field_elem":
        out = mont_limbs32(hash_to_field(b"".join(x.to_bytes(4, "big") for x in w)))
    else:
        raise KeyError(op)
    assert len(out) == OPS[op][1]
    return out, list(g.stream)
