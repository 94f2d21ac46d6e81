"""ctypes loader for tests/combine/libcombine.so — csrc/fr.hpp and the stages of blsw_combine_points_batch / blsw_lagrange_batch /
blsw_recover_points_batch (csrc/vcombine.hpp) compiled for the host (TEST HARNESS ONLY) — the Python reference of the three entries (integers mod r
and the affine group law of tests/curve_ref.py) and the vectors that the CPU and the GPU tests share."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

from tests import curve_ref as C
from tests.oracle_lib import eth_cases, unhex

HERE = os.path.dirname(os.path.abspath(__file__))
R = C.R_ORDER
X2 = C.X_ABS * C.X_ABS
ST_OK, ST_BAD_ENCODING, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_BAD_INDEX, ST_BAD_ID = 0, 1, 2, 3, 4, 6, 7
WIDTH = {1: 48, 2: 96}
KIND = {1: "g1", 2: "g2"}
FIELD = {1: C.K1, 2: C.K2}
GEN = {1: C.G1_GEN, 2: C.G2_GEN}
COMPRESS = {1: C.g1_compress, 2: C.g2_compress}
_lib = None
u8p, u32p, i32p, u64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint64))


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "combine"), "libcombine.so"])
        _lib = ctypes.CDLL(os.path.join(HERE, "combine", "libcombine.so"))
    return _lib


def words(x):
    return np.array([(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32)


def from_words(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def le32(x):
    return int(x).to_bytes(32, "little")


# ---------------------------------------------------------------- the host shim
def fr_op(op, a, b=0):
    """op: add sub mul sqr inv conv neg on canonical integers, through the device's Montgomery arithmetic"""
    out = np.zeros(8, dtype=np.uint32)
    code = ["add", "sub", "mul", "sqr", "inv", "conv", "neg"].index(op)
    assert load().cb_fr_op(code, words(a).ctypes.data_as(u32p), words(b).ctypes.data_as(u32p), out.ctypes.data_as(u32p)) == 0
    return from_words(out)


def fr_decode(data):
    """-> (accepted, the value read, the bytes written back from the words)"""
    w, back = np.zeros(8, dtype=np.uint32), (ctypes.c_uint8 * 32)()
    ok = load().cb_fr_decode((ctypes.c_uint8 * 32)(*data), w.ctypes.data_as(u32p), back)
    return bool(ok), from_words(w), bytes(back)


def fr_constants():
    r1, r2, inv = np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32), ctypes.c_uint32(0)
    load().cb_fr_constants(r1.ctypes.data_as(u32p), r2.ctypes.data_as(u32p), ctypes.byref(inv))
    return from_words(r1), from_words(r2), inv.value


def split(k):
    out = np.zeros(4, dtype=np.uint64)
    load().cb_split(words(k).ctypes.data_as(u32p), out.ctypes.data_as(u64p))
    return int(out[0]) | (int(out[1]) << 64), int(out[2]) | (int(out[3]) << 64)


def g1_mul(p48, k):
    out = (ctypes.c_uint8 * 48)()
    st = load().cb_g1_mul((ctypes.c_uint8 * 48)(*p48), words(k).ctypes.data_as(u32p), out)
    return st, bytes(out)


def _counts(counts):
    return None if counts is None else np.array([int(c) for c in counts], dtype=np.uint32)


def host_combine(group, points, scalars, counts=None):
    """uint8 [n, k, W], [n, k, 32] -> (out uint8 [n, W], status int32 [n], term_status int32 [n, k, 2]) by the host stages"""
    points, scalars = np.ascontiguousarray(points, dtype=np.uint8), np.ascontiguousarray(scalars, dtype=np.uint8)
    n, k = points.shape[:2]
    assert points.shape == (n, k, WIDTH[group]) and scalars.shape == (n, k, 32)
    cn = _counts(counts)
    out, st, tst = np.full((n, WIDTH[group]), 0xA5, np.uint8), np.full(n, -1, np.int32), np.full((n, k, 2), -1, np.int32)
    rc = load().cb_combine(ctypes.c_uint32(group), points.ctypes.data_as(u8p), scalars.ctypes.data_as(u8p), None if cn is None else cn.ctypes.data_as(u32p), ctypes.c_uint32(k),
                           ctypes.c_uint64(n), out.ctypes.data_as(u8p), st.ctypes.data_as(i32p), tst.ctypes.data_as(i32p))
    assert rc == 0
    return out, st, tst


def host_lagrange(ids, counts=None):
    ids = np.ascontiguousarray(ids, dtype=np.uint8)
    n, k = ids.shape[:2]
    assert ids.shape == (n, k, 32)
    cn = _counts(counts)
    coeff, st = np.full((n, k, 32), 0xA5, np.uint8), np.full(n, -1, np.int32)
    rc = load().cb_lagrange(ids.ctypes.data_as(u8p), None if cn is None else cn.ctypes.data_as(u32p), ctypes.c_uint32(k), ctypes.c_uint64(n), coeff.ctypes.data_as(u8p),
                            st.ctypes.data_as(i32p))
    assert rc == 0
    return coeff, st


def host_recover(group, points, ids, counts=None):
    points, ids = np.ascontiguousarray(points, dtype=np.uint8), np.ascontiguousarray(ids, dtype=np.uint8)
    n, k = points.shape[:2]
    assert points.shape == (n, k, WIDTH[group]) and ids.shape == (n, k, 32)
    cn = _counts(counts)
    out, st = np.full((n, WIDTH[group]), 0xA5, np.uint8), np.full(n, -1, np.int32)
    rc = load().cb_recover(ctypes.c_uint32(group), points.ctypes.data_as(u8p), ids.ctypes.data_as(u8p), None if cn is None else cn.ctypes.data_as(u32p), ctypes.c_uint32(k),
                           ctypes.c_uint64(n), out.ctypes.data_as(u8p), st.ctypes.data_as(i32p))
    assert rc == 0
    return out, st


# ---------------------------------------------------------------- the reference: integers and the affine law
@functools.lru_cache(maxsize=None)
def decode(group, data):
    """(status, affine point or None) of a compressed record, by tests/curve_ref.decode"""
    st, x, y = C.decode(KIND[group], data)
    return st, ((x, y) if st == ST_OK else None)


@functools.lru_cache(maxsize=None)
def mul(group, k, pt):
    return C.aff_mul(FIELD[group], k % R, pt)


def ref_lagrange(ids, count=None):
    """ids: integers below 2^256 (the row as the call carries it) -> (status, coefficients [k], zeros where the entry writes zeros)"""
    k = len(ids)
    count = k if count is None else count
    zeros = [0] * k
    if count > k:
        return ST_BAD_INDEX, zeros
    if count == 0:
        return ST_IDENTITY, zeros
    used = ids[:count]
    if any(v >= R for v in used):
        return ST_BAD_ENCODING, zeros
    if any(v == 0 for v in used) or len(set(used)) != count:
        return ST_BAD_ID, zeros
    out = []
    for j, xj in enumerate(used):
        num = den = 1
        for m, xm in enumerate(used):
            if m != j:
                num, den = num * xm % R, den * (xm - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return ST_OK, out + [0] * (k - count)


def ref_combine(group, points, scalars, count=None, lag=ST_OK):
    """points: compressed records, scalars: integers below 2^256 -> (status, out bytes) of one list"""
    k, zeros = len(points), bytes(WIDTH[group])
    count = k if count is None else count
    if count > k:
        return ST_BAD_INDEX, zeros
    if count == 0:
        return ST_IDENTITY, zeros
    if lag != ST_OK:
        return lag, zeros
    acc = None
    for b, s in zip(points[:count], scalars[:count]):
        st, pt = decode(group, bytes(b))
        if st not in (ST_OK, ST_IDENTITY):
            return st, zeros
        if s >= R:
            return ST_BAD_ENCODING, zeros
        if pt is not None:
            acc = C.aff_add(FIELD[group], acc, mul(group, s, pt))
    return ST_OK, COMPRESS[group](acc)


def ref_recover(group, points, ids, count=None):
    lag, coeff = ref_lagrange(ids, count)
    return ref_combine(group, points, coeff, count, lag)


def pack(rows, width):
    """a list of lists of byte strings -> uint8 [n, K, width], short lists padded with zero bytes"""
    K = max(1, max(len(r) for r in rows))
    out = np.zeros((len(rows), K, width), dtype=np.uint8)
    for i, r in enumerate(rows):
        for j, b in enumerate(r):
            assert len(b) == width
            out[i, j] = np.frombuffer(bytes(b), dtype=np.uint8)
    return out


# ---------------------------------------------------------------- shared vectors, built once and never changed
@functools.lru_cache(maxsize=None)
def pool(group):
    """six subgroup points as compressed records, with their negatives"""
    rng = random.Random(0xC0B1 + group)
    pts = [mul(group, rng.randrange(1, R), GEN[group]) for _ in range(6)]
    return tuple(COMPRESS[group](p) for p in pts), tuple(COMPRESS[group](C.aff_neg(FIELD[group], p)) for p in pts)


@functools.lru_cache(maxsize=None)
def bad_points(group):
    """decode status -> one record of the deserialization fixtures with that status (and the generated off-subgroup / off-curve ones)"""
    bad = {}
    for _, x in eth_cases("deserialization_G%d" % group):
        b = unhex(x["input"]["pubkey" if group == 1 else "signature"])
        if len(b) == WIDTH[group]:
            bad.setdefault(decode(group, b)[0], b)
    return bad


@functools.lru_cache(maxsize=None)
def fixture_points(group):
    return tuple(b for b in (unhex(x["input"]["pubkey" if group == 1 else "signature"]) for _, x in eth_cases("deserialization_G%d" % group)) if len(b) == WIDTH[group])


IDENTITY = {1: bytes([0xC0]) + bytes(47), 2: bytes([0xC0]) + bytes(95)}


@functools.lru_cache(maxsize=None)
def combine_vectors(group, k):
    """(names, points uint8 [n, k, W], scalars uint8 [n, k, 32], counts list [n], expected out uint8 [n, W], expected status [n]) — the cases of the
    combine stages at list length k, every expected value from ref_combine"""
    rng = random.Random(0x5CA1E + 16 * group + k)
    P, N = pool(group)
    W = WIDTH[group]
    bad = bad_points(group)
    garbage_pt, garbage_sc = bytes([0xFF]) * W, (1 << 256) - 1
    assert decode(group, garbage_pt)[0] == ST_BAD_ENCODING
    s = [rng.randrange(1, R) for _ in range(k)]
    rows = []  # (name, points, scalars, count)

    def row(name, pts, scs, count=k):
        assert len(pts) == k and len(scs) == k
        rows.append((name, list(pts), list(scs), count))

    base = [P[j % 6] for j in range(k)]
    row("random", base, s)
    row("edge scalars", base, [[1, R - 1, X2, X2 - 1, X2 + 1][j % 5] for j in range(k)])
    row("zero scalars at even terms", base, [0 if j % 2 == 0 else s[j] for j in range(k)])
    row("identity point first", [IDENTITY[group]] + base[1:], s)
    row("all scalars zero", base, [0] * k)
    row("all points the identity", [IDENTITY[group]] * k, s)
    row("count 0", base, s, 0)
    row("count k + 1", base, s, k + 1)
    row("count far beyond k", [garbage_pt] * k, [garbage_sc] * k, 0xFFFFFFFF)
    row("bad scalar r", base, s[:-1] + [R])
    row("bad scalar in a bad term: the point first", base[:-1] + [bad[ST_NOT_ON_CURVE]], s[:-1] + [R + 1])
    for st, b in sorted(bad.items()):
        row("fixture status %d last" % st, base[:-1] + [b], [1] * k)
    if k >= 2:
        row("s P + (r - s) P", [P[0], P[0]] + base[2:], [s[0], R - s[0]] + [0] * (k - 2))
        row("the same term twice", [P[1], P[1]] + base[2:], [s[1], s[1]] + s[2:])
        row("P and -P", [P[2], N[2]] + base[2:], [s[0], s[0]] + s[2:])
        row("count 1, garbage behind", [P[3]] + [garbage_pt] * (k - 1), [s[0]] + [garbage_sc] * (k - 1), 1)
        row("bad point in front of a bad scalar", [bad[ST_NOT_IN_SUBGROUP], P[0]] + base[2:], [s[0], R] + s[2:])
        row("bad scalar in front of a bad point", [P[0], bad[ST_NOT_IN_SUBGROUP]] + base[2:], [R, s[1]] + s[2:])
        row("bad point behind the count", base[:-1] + [bad[ST_NOT_ON_CURVE]], s, k - 1)
        row("bad scalar behind the count", base, s[:-1] + [garbage_sc], k - 1)
    for f, b in enumerate(fixture_points(group)):  # every deserialization fixture as a term with scalar 1, at a moving position
        j = f % k
        row("fixture %d at %d" % (f, j), base[:j] + [b] + base[j + 1:], [1] * k)
    exp = [ref_combine(group, pts, scs, count) for _, pts, scs, count in rows]
    return ([r[0] for r in rows], pack([r[1] for r in rows], W), pack([[le32(v) for v in r[2]] for r in rows], 32), [r[3] for r in rows],
            np.frombuffer(b"".join(e[1] for e in exp), np.uint8).reshape(len(rows), W).copy(), [e[0] for e in exp])


@functools.lru_cache(maxsize=None)
def lagrange_vectors(k):
    """(names, ids uint8 [n, k, 32], counts [n], expected coeff uint8 [n, k, 32], expected status [n])"""
    rng = random.Random(0x1A6 + k)
    rows = []

    def row(name, ids, count=k):
        assert len(ids) == k
        rows.append((name, list(ids), count))

    small, near, rnd = list(range(1, k + 1)), [R - 1 - j for j in range(k)], [rng.randrange(1, R) for _ in range(k)]
    row("1..k", small)
    row("near r - 1", near)
    row("random", rnd)
    row("mixed", [(small + near + rnd)[3 * j % (3 * k)] for j in range(k)])
    row("zero id first", [0] + rnd[1:])
    row("zero id last", rnd[:-1] + [0])
    row("id r", rnd[:-1] + [R])
    row("id 2^256 - 1 first", [(1 << 256) - 1] + rnd[1:])
    row("id r in front of a zero id" if k > 1 else "id r", ([R, 0] + rnd[2:])[:k])
    row("count 0", rnd, 0)
    row("count k + 1", rnd, k + 1)
    if k >= 2:
        row("zero id in front of an id r", [0, R] + rnd[2:])
        row("duplicate first and last", rnd[:-1] + [rnd[0]])
        row("duplicate adjacent at the front", [rnd[0], rnd[0]] + rnd[2:])
        row("duplicate adjacent at the end", rnd[:-2] + [rnd[-1], rnd[-1]])
        row("duplicate beyond the count", rnd[:-1] + [rnd[0]], k - 1)
        row("zero and id r beyond the count", rnd[:-2] + [0, R] if k > 2 else [rnd[0], R], k - 2 if k > 2 else 1)
        row("count 1", rnd, 1)
    if k >= 3:
        row("duplicate in the middle, apart", [rnd[0], rnd[1]] + rnd[2:-1] + [rnd[1]])
    exp = [ref_lagrange(ids, count) for _, ids, count in rows]
    return ([r[0] for r in rows], pack([[le32(v) for v in r[1]] for r in rows], 32), [r[2] for r in rows], pack([[le32(v) for v in e[1]] for e in exp], 32), [e[0] for e in exp])


@functools.lru_cache(maxsize=None)
def recover_vectors(group, k):
    """(names, points, ids, counts, expected out, expected status): the Lagrange rows at k over the pool's points, the term rules on top"""
    names, ids, counts, _, _ = lagrange_vectors(k)
    P, _ = pool(group)
    W = WIDTH[group]
    bad = bad_points(group)
    base = [P[(j + 1) % 6] for j in range(k)]
    id_rows = [[int.from_bytes(bytes(ids[i, j]), "little") for j in range(k)] for i in range(len(names))]
    rows = [(nm, base, r, c) for nm, r, c in zip(names, id_rows, counts)]
    rows.append(("bad point last", base[:-1] + [bad[ST_NOT_IN_SUBGROUP]], id_rows[2], k))
    rows.append(("identity point first", [IDENTITY[group]] + base[1:], id_rows[2], k))
    if k >= 2:
        rows.append(("duplicate id in front of a bad point", base[:-1] + [bad[ST_NOT_ON_CURVE]], id_rows[names.index("duplicate adjacent at the front")], k))
        rows.append(("bad point beyond the count", base[:-1] + [bytes([0xFF]) * W], id_rows[2], k - 1))
    exp = [ref_recover(group, pts, r, c) for _, pts, r, c in rows]
    return ([r[0] for r in rows], pack([r[1] for r in rows], W), pack([[le32(v) for v in r[2]] for r in rows], 32), [r[3] for r in rows],
            np.frombuffer(b"".join(e[1] for e in exp), np.uint8).reshape(len(rows), W).copy(), [e[0] for e in exp])


def shares(t, m, seed):
    """a seeded polynomial of degree t - 1 over Fr and its values at m seeded distinct non-zero ids -> (secret, ids, share secrets)"""
    rng = random.Random(seed)
    poly = [rng.randrange(1, R) for _ in range(t)]
    ids = []
    while len(ids) < m:
        v = rng.randrange(1, R)
        if v not in ids:
            ids.append(v)
    return poly[0], ids, [sum(c * pow(x, e, R) for e, c in enumerate(poly)) % R for x in ids]
