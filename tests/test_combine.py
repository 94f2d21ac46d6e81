"""Weighted point sums and threshold recovery (blsw_combine_points_batch, blsw_lagrange_batch, blsw_recover_points_batch) without a GPU: csrc/fr.hpp
and the stages of csrc/vcombine.hpp compiled for the host (tests/combine) against Python integers, the affine group law of tests/curve_ref.py and
the CPU oracle's signer; and the argument rules of the four entry points of libblsw.so, which precede any HIP call."""
import ctypes
import importlib
import itertools
import random

import numpy as np
import pytest

from tests import combine_lib as L
from tests import curve_ref as C
from tests.combine_lib import R, X2

ST_OK, ST_IDENTITY = L.ST_OK, L.ST_IDENTITY


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


# ---------------------------------------------------------------- Fr
def _fr_operands():
    r1, r2, inv32 = L.fr_constants()
    ones = [v for v in ((1 << 32 * n) - 1 for n in range(1, 8))] + [(1 << 254) - 1, ((1 << 32) - 1) << 192, R - ((1 << 32) - 1)]
    rng = random.Random(0xF2)
    vals = [0, 1, 2, R - 1, R - 2, (1 << 255) % R, r1, r2, inv32] + ones + [rng.randrange(R) for _ in range(12)]
    assert all(0 <= v < R for v in vals)
    return vals


def test_fr_constants_are_what_the_generator_prints():
    r1, r2, inv32 = L.fr_constants()
    assert r1 == (1 << 256) % R and r2 == pow(1 << 256, 2, R) and (R * inv32 + 1) % (1 << 32) == 0
    gen = importlib.import_module("tools.gen_fr_constants")
    assert open(gen.OUT).read() == gen.text(), "csrc/fr_constants.hpp is stale: run tools/gen_fr_constants.py"


def test_fr_operations_against_python_integers():
    vals = _fr_operands()
    for a in vals:
        assert L.fr_op("conv", a) == a
        assert L.fr_op("sqr", a) == a * a % R
        assert L.fr_op("neg", a) == -a % R
        inv = L.fr_op("inv", a)
        assert inv == (pow(a, -1, R) if a else 0) and inv * a % R == (1 if a else 0)
        for b in vals:
            assert L.fr_op("add", a, b) == (a + b) % R, (a, b)
            assert L.fr_op("sub", a, b) == (a - b) % R, (a, b)
            assert L.fr_op("mul", a, b) == a * b % R, (a, b)


def test_fr_byte_decode_accepts_zero_and_refuses_r():
    for v, ok in ((0, True), (1, True), (R - 1, True), (R, False), (R + 1, False), ((1 << 256) - 1, False), ((1 << 255), False), (R - (1 << 224), True)):
        got, value, back = L.fr_decode(L.le32(v))
        assert got == ok and value == v and back == L.le32(v), hex(v)


# ---------------------------------------------------------------- the digit split and the G1 ladder
EDGE_SCALARS = [0, 1, 2, 3, X2 - 1, X2, X2 + 1, 2 * X2, 2 * X2 + 1, R - 1, R - 2, (X2 - 1) * X2, (1 << 128) - 1, 1 << 128, 1 << 254]


def test_the_rule_the_ladder_rests_on():
    """[x^2] g1 == -(beta x, y) with beta the canonical value of K_G1_BETA (read from the generated header), and both digits fit 128 bits"""
    import os
    import re

    text = open(os.path.join(L.HERE, "..", "bls-verify-gadget_amd", "csrc", "constants.hpp")).read()
    m = re.search(r"K_G1_BETA\(\) \{\s*constexpr uint32_t k\[12\] = \{(.*?)\};", text, flags=re.S)
    mont = sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(m.group(1).split(",")))
    beta = mont * pow(1 << 384, -1, C.P) % C.P
    assert beta != 1 and pow(beta, 3, C.P) == 1
    gx, gy = C.G1_GEN
    assert C.aff_mul(C.K1, X2, C.G1_GEN) == (beta * gx % C.P, -gy % C.P)
    assert X2.bit_length() == 128 and (R // X2).bit_length() == 128 and R == X2 * X2 - X2 + 1


def test_digit_split():
    rng = random.Random(0xD161)
    for k in EDGE_SCALARS + [rng.randrange(R) for _ in range(64)]:
        k0, k1 = L.split(k)
        assert (k0, k1) == (k % X2, k // X2) and k0 + k1 * X2 == k and k0 < 1 << 128 and k1 < 1 << 128, hex(k)


def test_g1_ladder_against_the_affine_law():
    rng = random.Random(0x61AD)
    bases = [C.G1_GEN] + [C.aff_mul(C.K1, rng.randrange(1, R), C.G1_GEN) for _ in range(3)]
    for pt in bases:
        for k in [s for s in EDGE_SCALARS if s < R] + [rng.randrange(R) for _ in range(6)]:
            st, out = L.g1_mul(C.g1_compress(pt), k)
            assert st == 0 and out == C.g1_compress(C.aff_mul(C.K1, k, pt)), hex(k)


def test_g1_ladder_where_the_accumulator_meets_its_table():
    """Derived from the table {P, Q, P + Q}, Q = [x^2] P, not searched. Before the addition of step i the accumulator is 2 (a0 + a1 x^2) P with a0, a1
    the digits' prefixes, and the entry added is (b0 + b1 x^2) P with b the digits' bits. 2 (a0 + a1 x^2) = +-(b0 + b1 x^2) mod r = x^4 - x^2 + 1
    with digits below 2^128 and k0 < x^2 (k0 is a remainder) leaves, besides an accumulator that is the identity (k = 1, x^2, x^2 + 1: the first
    addition), exactly two scalars, both at the last step and both at the entry P + Q:
      k = r:              k0 = 1, k1 = x^2 - 1: the accumulator is -(P + Q), the sum is the identity (the opposite branch);
      k = x^4 + x^2 + 3:  k0 = 3, k1 = x^2 + 1: the accumulator is  +(P + Q), the doubling branch; the result is [2 x^2 + 2] P.
    +-P and +-Q are met by no scalar the split can produce: each needs k0 >= x^2 (x^2 is even, so 2 a0 + b0 - 1 = x^2 is the only way to cancel
    the odd term). Both scalars lie at or above r: below r an addition of the ladder never meets its operand, but the ladder must not depend on it."""
    for k, want in ((R, 0), (X2 * X2 + X2 + 3, 2 * X2 + 2)):
        k0, k1 = L.split(k)
        assert k0 + k1 * X2 == k and k1 < 1 << 128
        a0, a1 = k0 >> 1, k1 >> 1
        before, entry = 2 * (a0 + a1 * X2) % R, ((k0 & 1) + (k1 & 1) * X2) % R
        assert (k0 & 1, k1 & 1) == (1, 1) and before == (entry if want else R - entry)
        rng = random.Random(k & 0xFFFF)
        for pt in (C.G1_GEN, C.aff_mul(C.K1, rng.randrange(1, R), C.G1_GEN)):
            st, out = L.g1_mul(C.g1_compress(pt), k)
            assert st == 0 and out == C.g1_compress(C.aff_mul(C.K1, want, pt) if want else None)


# ---------------------------------------------------------------- the stages
@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("group", [1, 2])
def test_combine_stages(group, k):
    names, points, scalars, counts, want_out, want_st = L.combine_vectors(group, k)
    out, st, tst = L.host_combine(group, points, scalars, counts)
    assert st.tolist() == want_st, [(n, a, b) for n, a, b in zip(names, st.tolist(), want_st) if a != b]
    for i, name in enumerate(names):
        assert bytes(out[i]) == bytes(want_out[i]), name
        if want_st[i] != ST_OK:
            assert not out[i].any(), name
    # the cases that must come out as the infinity encoding with ST_OK, and the statuses the fixtures must show
    for name in ["all scalars zero", "all points the identity"] + (["s P + (r - s) P"] if k >= 2 else []) + (["P and -P"] if k == 2 else []):
        i = names.index(name)
        assert st[i] == ST_OK and bytes(out[i]) == L.IDENTITY[group], name
    assert {1, 2, 3, 6, ST_IDENTITY} <= set(want_st)
    if k >= 2:
        assert want_st[names.index("bad point in front of a bad scalar")] == L.ST_NOT_IN_SUBGROUP and want_st[names.index("bad scalar in front of a bad point")] == L.ST_BAD_ENCODING
        assert want_st[names.index("bad point behind the count")] == ST_OK and want_st[names.index("count 1, garbage behind")] == ST_OK
    assert want_st[names.index("bad scalar in a bad term: the point first")] == L.ST_NOT_ON_CURVE
    # every term's statuses, used or not
    for i in range(len(names)):
        for j in range(k):
            sc = int.from_bytes(bytes(scalars[i, j]), "little")
            assert tst[i, j].tolist() == [L.decode(group, bytes(points[i, j]))[0], L.ST_BAD_ENCODING if sc >= R else ST_OK], (names[i], j)
    # counts None is every term
    full = [i for i, c in enumerate(counts) if c == k]
    out2, st2, _ = L.host_combine(group, points[full], scalars[full], None)
    assert np.array_equal(out2, out[full]) and np.array_equal(st2, st[full])


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_lagrange_stages(k):
    names, ids, counts, want_coeff, want_st = L.lagrange_vectors(k)
    coeff, st = L.host_lagrange(ids, counts)
    assert st.tolist() == want_st, [(n, a, b) for n, a, b in zip(names, st.tolist(), want_st) if a != b]
    assert np.array_equal(coeff, want_coeff), [n for i, n in enumerate(names) if not np.array_equal(coeff[i], want_coeff[i])]
    assert {ST_OK, L.ST_BAD_ENCODING, L.ST_BAD_ID, ST_IDENTITY, L.ST_BAD_INDEX} == set(want_st)
    if k == 1:
        assert all(bytes(coeff[i, 0]) == L.le32(1) for i in range(len(names)) if want_st[i] == ST_OK)
    else:
        assert want_st[names.index("duplicate beyond the count")] == ST_OK and want_st[names.index("zero id in front of an id r")] == L.ST_BAD_ENCODING
    for i in range(len(names)):  # the coefficients interpolate at 0: sum lambda_j f(id_j) == f(0) for f of degree < count
        if want_st[i] == ST_OK:
            xs = [int.from_bytes(bytes(ids[i, j]), "little") for j in range(counts[i])]
            lam = [int.from_bytes(bytes(coeff[i, j]), "little") for j in range(counts[i])]
            for e in range(counts[i]):
                assert sum(l * pow(x, e, R) for l, x in zip(lam, xs)) % R == (1 if e == 0 else 0), (names[i], e)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("group", [1, 2])
def test_recover_stages(group, k):
    names, points, ids, counts, want_out, want_st = L.recover_vectors(group, k)
    out, st = L.host_recover(group, points, ids, counts)
    assert st.tolist() == want_st, [(n, a, b) for n, a, b in zip(names, st.tolist(), want_st) if a != b]
    assert np.array_equal(out, want_out), [n for i, n in enumerate(names) if not np.array_equal(out[i], want_out[i])]
    if k >= 2:
        assert want_st[names.index("duplicate id in front of a bad point")] == L.ST_BAD_ID


# ---------------------------------------------------------------- meaning: threshold signatures
@pytest.mark.parametrize("t", [1, 2, 3])
def test_recovery_of_a_threshold_signature_and_key(oracle, t):
    """shares of a seeded polynomial of degree t - 1 at t + 2 ids: every t-subset and the whole set recover oracle.sign(secret, msg) and
    oracle.sk_to_pk(secret) byte for byte; a (t - 1)-subset does not (the test's own check that it can fail)"""
    m, msg = t + 2, b"threshold message %d" % t
    secret, ids, sks = L.shares(t, m, 0x7E55 + t)
    sigs, pks = [oracle.sign(s, msg) for s in sks], [oracle.sk_to_pk(s) for s in sks]
    subsets = [list(c) for c in itertools.combinations(range(m), t)] + [list(range(m))]
    short = [list(c) for c in itertools.combinations(range(m), t - 1)] if t >= 2 else []
    rows = subsets + short
    counts = [len(r) for r in rows]
    id_rows = L.pack([[L.le32(ids[j]) for j in r] for r in rows], 32)
    assert id_rows.shape[1] == m
    for group, shares_, want in ((2, sigs, oracle.sign(secret, msg)), (1, pks, oracle.sk_to_pk(secret))):
        out, st = L.host_recover(group, L.pack([[shares_[j] for j in r] for r in rows], L.WIDTH[group]), id_rows, counts)
        assert not st.any()
        for i, r in enumerate(rows):
            assert (bytes(out[i]) == want) == (i < len(subsets)), (group, r)
        # the same through the coefficients: lagrange, then combine
        coeff, lst = L.host_lagrange(id_rows, counts)
        out2, st2, _ = L.host_combine(group, L.pack([[shares_[j] for j in r] for r in rows], L.WIDTH[group]), coeff, counts)
        assert not lst.any() and not st2.any() and np.array_equal(out2, out)
    assert oracle.verify_bytes(oracle.sk_to_pk(secret), msg, oracle.sign(secret, msg))


# ---------------------------------------------------------------- the entry points' argument rules (no HIP call is reached)
ERR_ARG, ERR_WORKSPACE = 1, 2


def test_argument_rules_without_a_gpu(pkg):
    lib = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    assert lib.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17 and H["defines"]["BLSW_ST_BAD_ID"] == pkg.ST_BAD_ID == L.ST_BAD_ID == 7
    assert {"blsw_combine_points_workspace_bytes", "blsw_combine_points_batch", "blsw_lagrange_batch", "blsw_recover_points_batch"} <= set(pkg.EXPORTED_SYMBOLS)
    # host buffers stand in for device memory: a refused call must leave them as they are, and a call that is not refused is never made here
    bufs = {name: np.full(256, 0x5A, dtype=np.uint8) for name in ("in", "sc", "counts", "out", "st", "tst", "ws")}
    ptr = {name: ctypes.c_void_p(b.ctypes.data) for name, b in bufs.items()}
    good = dict(group=2, k=2, n=1, ws_bytes=1 << 60, **ptr)
    b = ctypes.c_uint64(0)

    def size(group, n, k):
        assert lib.blsw_combine_points_workspace_bytes(group, n, k, ctypes.byref(b)) == 0
        return b.value

    def combine(**kw):
        a = dict(good, **kw)
        return lib.blsw_combine_points_batch(a["group"], a["in"], a["sc"], a["counts"], a["k"], a["n"], a["out"], a["st"], a["tst"], a["ws"], a["ws_bytes"], None)

    def recover(**kw):
        a = dict(good, **kw)
        return lib.blsw_recover_points_batch(a["group"], a["in"], a["sc"], a["counts"], a["k"], a["n"], a["out"], a["st"], a["ws"], a["ws_bytes"], None)

    def lagrange(**kw):
        a = dict(good, **kw)
        return lib.blsw_lagrange_batch(a["sc"], a["counts"], a["k"], a["n"], a["out"], a["st"], None)

    shapes = (dict(n=0), dict(k=0), dict(k=65536), dict(n=0x3FFFFFFF // 2 + 1), dict(n=0x40000000, k=1), dict(n=1 << 40, k=1), dict(n=(1 << 32) + 1, k=1))
    for kw in shapes + (dict(group=0), dict(group=3)) + tuple({name: None} for name in ("in", "sc", "out", "st", "ws")):
        assert combine(**kw) == ERR_ARG and recover(**kw) == ERR_ARG, kw
    for kw in shapes + tuple({name: None} for name in ("sc", "out", "st")):
        assert lagrange(**kw) == ERR_ARG, kw
    for group, n, k in ((0, 1, 2), (3, 1, 2), (2, 0, 2), (2, 1, 0), (2, 1, 65536), (1, 0x3FFFFFFF // 2 + 1, 2), (1, 0x40000000, 1)):
        assert lib.blsw_combine_points_workspace_bytes(group, n, k, ctypes.byref(b)) == ERR_ARG
    assert lib.blsw_combine_points_workspace_bytes(2, 1, 2, None) == ERR_ARG
    assert size(1, 0x3FFFFFFF, 1) > 0 and size(2, 0x3FFFFFFF // 65535, 65535) > 0  # the largest legal shapes
    for group in (1, 2):  # one byte less than the size is refused, by both entries that take a workspace
        need = size(group, 3, 5)
        assert combine(group=group, n=3, k=5, ws_bytes=need - 1) == ERR_WORKSPACE and recover(group=group, n=3, k=5, ws_bytes=need - 1) == ERR_WORKSPACE
        assert combine(group=group, n=3, k=5, ws_bytes=0) == ERR_WORKSPACE
    assert all((buf == 0x5A).all() for buf in bufs.values())
    # non-decreasing in n and in k; the terms' share as the header states it
    grid = (1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, 1024, 1025)
    for group in (1, 2):
        for fixed in (1, 5, 64):
            last_n = last_k = 0
            for v in grid:
                assert size(group, v, fixed) >= last_n and size(group, fixed, v) >= last_k, (group, fixed, v)
                last_n, last_k = size(group, v, fixed), size(group, fixed, v)
    per_term = {1: 276, 2: 4836}
    for group in (1, 2):
        assert size(group, 64, 16) - size(group, 64, 8) == 64 * 8 * per_term[group]
        assert size(group, 64, 8) >= 64 * 8 * per_term[group] + 64 * 4
