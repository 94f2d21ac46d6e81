"""aggregate_verify instances that take the in-circuit key sum (mapped_aggregate, then pk != 0 and prepare_g1's to_affine: chain_mapped_aggregate
and chain_g1_post of csrc/chains.hpp, run by k_agg_keys / k_agg_sum / k_agg_sum_in / k_agg_sum_ks and k_keyset_alloc) to the group law's edges:
the identity as an operand, as a partial sum and as the result, a point with its negative, the same point twice. Shared by the host test
(test_agg_edges.py) and the device test (test_agg_edges_gpu.py).

K = 6 keys, a 32-byte message. Keys are minted from known secret keys (oracle.sk_to_pk) and the signature is oracle.sign(sum of the selected
secrets mod r, m), the identity (all zeros) when that sum is 0 mod r: the intended Boolean of a case with keys in the subgroup is known by
construction. O is the (0, 0) encoding of the identity, T the order-3 point (0, 2) of chain_edges.g1_operands().
synth.make_aggregate serves only the ordinary filler lanes: it asserts a signature that is not the identity.

What "known by construction" means here. The reference states `pk != 0` as a CONSTRAINT (constraints.rs:97-99, enforce_not_equal), not as a
term of its Boolean: the Boolean is the pairing equation e(-g, sig) e(sum, H(m)) = 1 alone. So for keys in the subgroup
  * the Boolean is true iff the signature is that of the selected secrets' sum on the untampered message, also when that sum is O and the
    signature the identity (e(-g, O) e(O, H(m)) = 1);
  * the vector satisfies the system iff sum != O; when sum = O exactly one row fails, the one that enforces pk != 0;
  * aggregate_verify's statement, a satisfied system with a true Boolean, is `sum != O and not tampered`: Case.expect.

A Witness key enters the sum as the end of its allocation chain, [h1] ([h1^-1 mod r] pk): pk itself for a subgroup key, O for T (3 | h1), 3G for
3G + T. An Input key enters as (x, y, 1), or (0, 1, 0) for O: only there T itself is summed. effective_key states both.

aggregate_reference restates the agg.count, agg.loop, verify.pk_not_zero and prepare.pk segments over Python integers: selects by plain
integers, the additions by curve_ref.proj_add (Renes-Costello-Batina, both z variable), the 33 result bits of each two-operand addmany, the
is_eq pairs [is_not_equal, multiplier] by field_ref.w_is_eq (the multiplier of an equal pair is 1, as AllocatedFp::is_neq allocates it), and
to_affine's inverse hint by the zero rule: the inverse of 0 is 0."""
import hashlib
from collections import namedtuple

import numpy as np

from tests import chain_edges as E
from tests import curve_ref as C
from tests import field_ref as F
from tests import synth
from tests.curve_ref import K1, R_ORDER

K, MSG_LEN, N = 6, 32, 70
EDGE_LANES = (0, 1, 31, 62, 63, 64, 69)
CHECK_LANES = sorted(set(EDGE_LANES) | {2, 30, 32, 61, 65, 68} | set(range(0, N, 8)))  # the edge lanes, their neighbours, every eighth ordinary lane
T3 = (0, 2)
SEGMENTS = ("agg.count", "agg.loop", "verify.pk_not_zero", "prepare.pk")
SEG_PK_ALLOC = 1942

# name: the case; letter: its item in the list a-i; pks [K, 12] / bitmap [K] uint8 / msg [32] uint8 / sig [24] uint64: the instance; points: the
# keys as affine points (None: O); secrets: per key the secret of its subgroup part; subgroup: every key is in the subgroup or O; sum_secret: sum
# of the selected secrets mod r. Known by construction where every key is in the subgroup (None otherwise: the oracle's stands): boolean, the
# gadget's Boolean = the pairing equation e(-g, sig) e(sum, H(m)) = 1, and expect = boolean and sum != O, what aggregate_verify states (below)
Case = namedtuple("Case", "name letter pks bitmap msg sig points secrets subgroup sum_secret tampered boolean expect")


def _secret(tag):
    return int.from_bytes(hashlib.sha256(b"agg_edges sk " + tag).digest(), "big") % R_ORDER or 1


S_P, S_Q = _secret(b"P"), _secret(b"Q")
S_FILL = [_secret(b"filler %d" % k) for k in range(K)]
IDENTITY_SIG = "identity"


def affine_of(xy):
    """[12] uint64 Montgomery limbs -> the affine point (None for the all-zero pair)"""
    x, y = F.dec(E.el(xy[:6])), F.dec(E.el(xy[6:]))
    return None if (x, y) == (0, 0) else (x, y)


def _mint(oracle, secret):
    """the key of a secret as [12] uint64, by the oracle's sk_to_pk; the secret 0 is O"""
    if secret % R_ORDER == 0:
        return np.zeros(12, dtype=np.uint64)
    st, xy, inf = oracle.g1_decompress(oracle.sk_to_pk(secret))
    assert st == 0 and not inf
    return xy


def _signature(oracle, secret, msg):
    if secret % R_ORDER == 0:
        return np.zeros(24, dtype=np.uint64)
    st, xy, inf = oracle.g2_decompress(oracle.sign(secret, msg))
    assert st == 0 and not inf
    return xy


def _case(oracle, name, slots, bitmap, sig=None, tamper=False):
    """slots: per key a secret (0: O), or (secret of the subgroup part, point outside the subgroup). sig: None = the signature of the selected
    secrets' sum, IDENTITY_SIG, or a secret to sign with."""
    assert len(slots) == len(bitmap) == K
    pks, points, secrets = [], [], []
    for s in slots:
        if isinstance(s, tuple):
            secrets.append(s[0]), pks.append(E.enc_g1(s[1])), points.append(s[1])
        else:
            secrets.append(s % R_ORDER), pks.append(_mint(oracle, s))
            points.append(affine_of(pks[-1]))
    subgroup = not any(isinstance(s, tuple) for s in slots)
    total = sum(s for s, b in zip(secrets, bitmap) if b) % R_ORDER
    m = hashlib.sha256(b"agg_edges msg " + name.encode()).digest()
    signed = 0 if sig == IDENTITY_SIG else (total if sig is None else sig % R_ORDER)
    sig_xy = _signature(oracle, signed, m)
    msg = np.frombuffer(m, dtype=np.uint8).copy()
    if tamper:
        assert signed  # e(-g, O) e(O, H(m')) = 1 for any m': tampering shows only under a signature that is not the identity
        msg[7] ^= 2
    boolean = (signed == total and not tamper) if subgroup else None
    expect = (boolean and total != 0) if subgroup else None
    return Case(name, name[0], np.stack(pks), np.array(bitmap, dtype=np.uint8), msg, sig_xy, points, secrets, subgroup, total, tamper, boolean, expect)


def cases(oracle):
    """[Case]: items a-i, 21 cases"""
    def make():
        f = S_FILL
        neg = lambda s: R_ORDER - s % R_ORDER
        t = (0, T3)
        s3 = (3, C.aff_add(K1, C.aff_mul(K1, 3, C.G1_GEN), T3))  # "subgroup + order 3" of chain_edges.g1_operands(): 3G + T
        d_first = ([S_P, neg(S_P), S_Q, f[3], f[4], f[5]], [1, 1, 1, 0, 0, 0])
        e_twice = ([S_P, S_P, f[2], f[3], f[4], f[5]], [1, 1, 0, 0, 0, 0])
        out = [
            _case(oracle, "a: empty selection, signature of key 0", f, [0] * K, sig=f[0]),
            _case(oracle, "a: empty selection, identity signature", f, [0] * K, sig=IDENTITY_SIG),
            _case(oracle, "b: one key, index 0", [S_P] + f[1:], [1, 0, 0, 0, 0, 0]),
            _case(oracle, "b: one key, index 3", f[:3] + [S_P] + f[4:], [0, 0, 0, 1, 0, 0]),
            _case(oracle, "b: one key, index K - 1", f[:5] + [S_P], [0, 0, 0, 0, 0, 1]),
            _case(oracle, "c: O selected at index 0", [0, f[1], S_Q, f[3], f[4], f[5]], [1, 0, 1, 0, 0, 0]),
            _case(oracle, "c: O selected at index 2", [S_P, f[1], 0, S_Q, f[4], f[5]], [1, 0, 1, 1, 0, 0]),
            _case(oracle, "c: O selected at index K - 1", [S_P, f[1], f[2], f[3], f[4], 0], [1, 0, 0, 0, 0, 1]),
            _case(oracle, "c: O not selected", [S_P, 0, S_Q, f[3], f[4], f[5]], [1, 0, 1, 0, 0, 0]),
            _case(oracle, "c: all keys O, all selected", [0] * K, [1] * K),
            _case(oracle, "d: P, -P at 0, 1, then Q", *d_first),
            _case(oracle, "d: P, -P at K - 2, K - 1 alone", f[:4] + [S_P, neg(S_P)], [0, 0, 0, 0, 1, 1]),
            _case(oracle, "e: P twice", *e_twice),
            _case(oracle, "e: P three times", [f[0], S_P, f[2], S_P, S_P, f[5]], [0, 1, 0, 1, 1, 0]),
            _case(oracle, "f: P, Q, then the key of s_P + s_Q", [S_P, S_Q, S_P + S_Q, f[3], f[4], f[5]], [1, 1, 1, 0, 0, 0]),
            _case(oracle, "g: P, Q, then the key of r - (s_P + s_Q)", [S_P, S_Q, neg(S_P + S_Q), f[3], f[4], f[5]], [1, 1, 1, 0, 0, 0]),
            _case(oracle, "h: T twice", [t, f[1], t, f[3], f[4], f[5]], [1, 0, 1, 0, 0, 0], sig=f[1]),
            _case(oracle, "h: T three times", [t, t, f[2], t, f[4], f[5]], [1, 1, 0, 1, 0, 0]),
            _case(oracle, "h: 3G + T between P and Q", [S_P, s3, S_Q, f[3], f[4], f[5]], [1, 1, 1, 0, 0, 0]),
            _case(oracle, "i: tampered, P, -P at 0, 1, then Q", *d_first, tamper=True),
            _case(oracle, "i: tampered, P twice", *e_twice, tamper=True),
        ]
        assert len(out) == 3 * len(EDGE_LANES) and len({c.name for c in out}) == len(out)
        return out
    return F._memo("agg_edges_cases", make)


def twin(oracle, c):
    """a case under the identity signature with the signature of filler 0 in its place: the same keys and bitmap, so the same key sum, and
    only what the key sum breaks is broken"""
    assert not c.sig.any() and c.sum_secret == 0
    return c._replace(name=c.name + " [twin]", sig=_signature(oracle, S_FILL[0], c.msg.tobytes()), boolean=False if c.subgroup else None)


def case(oracle, name):
    return {c.name: c for c in cases(oracle) + [wave_case(oracle)] + wave_tail(oracle)}[name]


D_SECOND = "d: P, -P at K - 2, K - 1 alone"
CASE_NAMES = ("a: empty selection, signature of key 0", "a: empty selection, identity signature", "b: one key, index 0", "b: one key, index 3", "b: one key, index K - 1",
              "c: O selected at index 0", "c: O selected at index 2", "c: O selected at index K - 1", "c: O not selected", "c: all keys O, all selected",
              "d: P, -P at 0, 1, then Q", D_SECOND, "e: P twice", "e: P three times", "f: P, Q, then the key of s_P + s_Q",
              "g: P, Q, then the key of r - (s_P + s_Q)", "h: T twice", "h: T three times", "h: 3G + T between P and Q", "i: tampered, P, -P at 0, 1, then Q",
              "i: tampered, P twice")
WAVE_NAME = "wave: O at 1, 2, 3, then P, -P alone"


def wave_case(oracle):
    """case d-second with the unselected keys 1, 2, 3 all O (lanes 0..63 of "wave")"""
    return F._memo("agg_edges_wave", lambda: _case(oracle, WAVE_NAME, [S_FILL[0], 0, 0, 0, S_P, R_ORDER - S_P], [0, 0, 0, 0, 1, 1]))


WAVE_TAIL_NAMES = ("wave tail: O at 1, 2, 3 beside an ordinary selection", "wave tail: the same, tampered")


def wave_tail(oracle):
    """lanes 64..69 of "wave": keys 1, 2, 3 are O here too, beside an ordinary selection (filler 0, P, Q), valid and tampered. k_agg_keys allocates
    key k of instance I in lane k N + I: with all 70 instances of a launch group holding O at 1, 2, 3, lanes 70..279 take the `inf` branch of
    chain_g1_alloc_only, the hardware waves 128..191 and 192..255 whole (all_identity_windows; key 2 alone, lanes 140..209, would fill none)."""
    def make():
        slots, bm = [S_FILL[0], 0, 0, 0, S_P, S_Q], [1, 0, 0, 0, 1, 1]
        return [_case(oracle, WAVE_TAIL_NAMES[0], slots, bm), _case(oracle, WAVE_TAIL_NAMES[1], slots, bm, tamper=True)]
    return F._memo("agg_edges_wave_tail", make)


def all_identity_windows(rows):
    """the 64-aligned windows [t, t + 64) of k_agg_keys' lanes t = k n + I over one launch group of n instances in which every key is O"""
    n = len(rows)
    is_o = [not rows[t % n][0][t // n].any() for t in range(K * n)]
    return [t for t in range(0, K * n - 63, 64) if all(is_o[t:t + 64])]


def ordinary(oracle):
    """four instances of synth.make_aggregate as (pks, bitmap, msg, sig): three valid ones and a tampered one"""
    def make():
        bitmaps = ([1, 0, 1, 1, 0, 1], [1, 1, 1, 1, 1, 1], [0, 1, 0, 0, 1, 0], [1, 1, 0, 1, 0, 0])
        out = [synth.make_aggregate(oracle, K, bm, start=10 * i, tamper=(i == 3)) for i, bm in enumerate(bitmaps)]
        assert [o[4] for o in out] == [True, True, True, False]
        return [o[:4] for o in out]
    return F._memo("agg_edges_ordinary", make)


BATCHES = ("wave", "mixed 0", "mixed 1", "mixed 2")


def batches(oracle):
    """{name: ([70] of (pks, bitmap, msg, sig), {lane: case name})}. "mixed r": case 7 r + j at edge lane j, so that the three batches put every
    case on a lane, between ordinary valid and tampered instances; only the edge lanes are named. "wave": lanes 0..63 are wave_case, lanes 64..69
    wave_tail's two cases in turn; all 70 lanes are named."""
    def make():
        cs, fill, out = cases(oracle), ordinary(oracle), {}
        for r in range(3):
            rows, at = [fill[i % 4] for i in range(N)], {}
            for j, lane in enumerate(EDGE_LANES):
                c = cs[7 * r + j]
                rows[lane], at[lane] = (c.pks, c.bitmap, c.msg, c.sig), c.name
            out["mixed %d" % r] = (rows, at)
        tail = wave_tail(oracle)
        lanes = [wave_case(oracle) if i < 64 else tail[i % 2] for i in range(N)]
        out["wave"] = ([(c.pks, c.bitmap, c.msg, c.sig) for c in lanes], {i: c.name for i, c in enumerate(lanes)})
        assert sorted(n for b in out if b != "wave" for n in out[b][1].values()) == sorted(CASE_NAMES)
        return out
    return F._memo("agg_edges_batches", make)


def check_lanes(name):
    """the lanes of a batch whose whole vectors are compared: every edge lane, its neighbours, every eighth ordinary lane"""
    return CHECK_LANES if name != "wave" else list(range(N))  # "wave": two distinct tail instances, every lane is cheap to compare


def stacked(rows):
    """[(pks, bitmap, msg, sig)] -> pks [n, K, 12], bitmap [n, K], msg [n, 32], sig [n, 24]"""
    return tuple(np.ascontiguousarray(np.stack([r[j] for r in rows])) for j in range(4))


# ---------------------------------------------------------------- the key set: every edge it can reach, by bitmaps alone
KEYSET_SECRETS = (S_P, R_ORDER - S_P, 0, S_Q, R_ORDER - (S_P + S_Q) % R_ORDER, (0, T3))  # P, -P, O, Q, the key of r - (s_P + s_Q), T
KEYSET_BITMAPS = (("a: empty selection", [0, 0, 0, 0, 0, 0]), ("c: O selected", [1, 0, 1, 1, 0, 0]), ("c: O alone", [0, 0, 1, 0, 0, 0]),
                  ("d: P, -P, then Q", [1, 1, 0, 1, 0, 0]), ("d: P, -P alone", [1, 1, 0, 0, 0, 0]), ("g: P, Q, then the key of r - (s_P + s_Q)", [1, 0, 0, 1, 1, 0]),
                  ("h: T with Q", [0, 0, 0, 1, 0, 1]), ("h: T alone", [0, 0, 0, 0, 0, 1]), ("b: P alone", [1, 0, 0, 0, 0, 0]), ("ordinary: P, Q", [1, 0, 0, 1, 0, 0]))


def keyset_cases(oracle):
    """[Case] over the one key set, and the tampered form of "d: P, -P, then Q\""""
    def make():
        out = [_case(oracle, "keyset " + name, list(KEYSET_SECRETS), bm) for name, bm in KEYSET_BITMAPS]
        out.append(_case(oracle, "keyset i: tampered, P, -P, then Q", list(KEYSET_SECRETS), [1, 1, 0, 1, 0, 0], tamper=True))
        assert all(np.array_equal(c.pks, out[0].pks) for c in out)
        return out
    return F._memo("agg_edges_keyset", make)


def keyset_batches(oracle):
    """{name: ([70] of (pks, bitmap, msg, sig), {lane: case name} for all 70 lanes)} over the one key set. "mixed": the eight edge bitmaps and the
    tampered case at the edge lanes and at lanes 2 and 30, "b: P alone", "ordinary: P, Q" and the tampered case elsewhere; "wave": lanes 0..63
    "d: P, -P alone", so the whole first wave inverts zero"""
    def make():
        cs = keyset_cases(oracle)
        by = {c.name: c for c in cs}
        row = lambda c: (c.pks, c.bitmap, c.msg, c.sig)
        fill = [by["keyset b: P alone"], by["keyset ordinary: P, Q"], by["keyset i: tampered, P, -P, then Q"]]
        at = {i: fill[i % 3].name for i in range(N)}
        edge = [c for c in cs if c.name not in (fill[0].name, fill[1].name)]
        lanes = EDGE_LANES + (2, 30)
        assert len(lanes) == len(edge)
        at.update({lane: c.name for lane, c in zip(lanes, edge)})
        wave = {i: "keyset d: P, -P alone" if i < 64 else fill[i % 3].name for i in range(N)}
        return {"mixed": ([row(by[at[i]]) for i in range(N)], at), "wave": ([row(by[wave[i]]) for i in range(N)], wave)}
    return F._memo("agg_edges_keyset_batches", make)


# ---------------------------------------------------------------- the meaning
_EFFECTIVE = {}


def effective_key(pt, keys_input):
    """the affine point a key contributes to the sum: the key itself as an Input, [h1] ([h1^-1 mod r] key) as a Witness"""
    if keys_input or pt is None:
        return pt
    if pt not in _EFFECTIVE:
        _EFFECTIVE[pt] = C.aff_mul(K1, E.H1, C.aff_mul(K1, E.H1_INV, pt))
    return _EFFECTIVE[pt]


def selected_sum(c, keys_input=False):
    """the affine sum of the selected keys by the chord-and-tangent law (None: the identity)"""
    acc = None
    for pt, b in zip(c.points, c.bitmap):
        if b:
            acc = C.aff_add(K1, acc, effective_key(pt, keys_input))
    return acc


# ---------------------------------------------------------------- the restatement
def key_of_alloc(seg):
    """the projective key at the end of one key's allocation segment (1 942 stored elements): the chain's last statement is an addition (h1 is
    odd) whose last six witnesses m0..m5 give X = m0 - m1, Y = m2 + m3, Z = m4 + m5"""
    assert E.H1 & 1 and len(seg) == SEG_PK_ALLOC
    m = [F.dec(v) for v in E.els(seg[-6:])]
    return (K1.sub(m[0], m[1]), K1.add(m[2], m[3]), K1.add(m[4], m[5]))


def key_of_input(pt):
    return (0, 1, 0) if pt is None else (pt[0], pt[1], 1)


def aggregate_reference(keys, bitmap):
    """({segment: stored elements}, count, the sum as a projective triple) for the K projective keys (canonical integers) the circuit holds"""
    loop, ret, count = [], None, 0
    for k, (key, bit) in enumerate(zip(keys, bitmap)):
        sel = tuple(key) if bit else (0, 1, 0)
        loop += [F.enc(v) for v in sel]
        ret = sel if k == 0 else C.proj_add(K1, loop, 0, ret, sel)  # zero + sel is sel: the accumulator starts as a constant
        total = count + (1 if bit else 0)
        loop += [F.w_bool((total >> i) & 1) for i in range(33)]  # addmany of two operands: 33 result bits, LSB first
        count = total & 0xFFFFFFFF
    x, y, z = ret
    x_eq, wx = F.w_is_eq(0, 0)  # pk.x 0 against 0 pk.z
    y_eq, wy = F.w_is_eq(0, z)  # pk.y 0 against 1 pk.z
    z_zero, wz = F.w_is_eq(0, z)  # pk.is_zero(); zero.is_zero() is a constant, so both_are_zero is this Boolean
    coords = x_eq and y_eq
    not_zero = wx + wy + [F.w_bool(coords)] + wz + [F.w_bool(not z_zero and not coords)]  # or(a, b) allocates and(!a, !b)
    infinity, prep = F.w_is_eq(0, z)
    zi = F.inv(z)  # 0 for 0
    prep = prep + [F.enc(zi)]
    nzx, nzy = K1.mul_w(prep, x, zi), K1.mul_w(prep, y, zi)
    prep += [F.enc(0 if infinity else nzx), F.enc(0 if infinity else nzy)]
    assert len(not_zero) == 8 and len(prep) == 7 and len(loop) == 36 * len(keys) + 12 * (len(keys) - 1)
    return {"agg.count": [0] * 32, "agg.loop": loop, "verify.pk_not_zero": not_zero, "prepare.pk": prep}, count, ret


def segments_of(marks, w):
    """{segment: stored elements} of the four segments, from a {name: start} mark table (the oracle's or the shim's) and a vector"""
    starts = sorted(set(marks.values()) | {len(w)})  # a segment ends where the next non-empty one starts (an Input argument's segment is empty)
    return {name: E.els(w[marks[name]:starts[starts.index(marks[name]) + 1]]) for name in SEGMENTS}


# ---------------------------------------------------------------- the constraint system of (32, n_keys = 6, agg_inputs = mask), for both tests
def rows_of(mats, r):
    """[columns of row r in A, in B, in C] of a matrices() dict"""
    return [mats[k][1][int(mats[k][0][r]):int(mats[k][0][r + 1])].tolist() for k in "ABC"]


def without_rows(mats, rows):
    out = dict(mats)
    out["n_constraints"] = mats["n_constraints"] - len(rows)
    keep = np.ones(mats["n_constraints"], dtype=bool)
    keep[list(rows)] = False
    for k in "ABC":
        rp, col, val = mats[k]
        n = np.diff(rp.astype(np.int64))
        entries = np.repeat(keep, n)
        out[k] = (np.concatenate([[0], np.cumsum(n[keep])]).astype(np.uint64), np.ascontiguousarray(col[entries]), np.ascontiguousarray(val[entries]))
    return out


_SYSTEMS = {}


def system(pkg, mask):
    """(the product's matrices, the row that enforces pk != 0, the layout), built once. The row is enforce_equal(pk.is_eq(zero), false):
    (1 - v) * 1 = 0 with v the last witness of verify.pk_not_zero (or(a, b) is not(and(!a, !b)))."""
    if mask not in _SYSTEMS:
        mats = pkg.matrices(MSG_LEN, n_keys=K, agg_inputs=mask)
        lay = pkg.layout_aggregate(MSG_LEN, K, mask)
        v = lay["n_instance_vars"] + lay["off_pk_not_zero"] + 7
        hits = [r for r in np.nonzero(np.diff(mats["A"][0].astype(np.int64)) == 2)[0].tolist() if rows_of(mats, r) == [[0, v], [0], []]]
        assert len(hits) == 1, hits
        _SYSTEMS[mask] = (mats, hits[0], lay)
    return _SYSTEMS[mask]
