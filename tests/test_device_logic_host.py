"""Kernel logic without a GPU: the device headers (bls-verify-gadget_amd/csrc/*.hpp) compiled for the host and run on
one "lane" must reproduce the oracle's witness vector bit for bit. Also checks the segment table and the C-ABI exports."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

from tests import hostsim_lib, synth
from tests.oracle_lib import GOLDEN, eth_cases, unhex

LIT = json.load(open(os.path.join(GOLDEN, "literals.json")))
ORACLE_TO_ABI = {
    "msg": "off_msg", "pk_alloc": "off_pk_alloc", "sig_alloc": "off_sig_alloc", "verify.pk_not_zero": "off_pk_not_zero", "hash.expand": "off_expand",
    "hash.map0": "off_map0", "hash.map1": "off_map1", "hash.add": "off_add", "hash.clear_cofactor": "off_cofactor", "prepare.h": "off_prep_h",
    "prepare.pk": "off_prep_pk", "prepare.sig": "off_prep_sig", "miller": "off_miller", "final_exp": "off_final_exp", "is_one": "off_is_one",
}


# msg' of expand_message is 111 bytes longer than the message (sha.hpp: total = msg_len + 111), so its SHA-256 block count (msg_len + 183) / 64 changes
# at 8 / 9, 72 / 73, ...; the 0x80 byte opens a block of its own at msg_len = 17 (mod 64), and the two lib_str bytes straddle a block at 63 (mod 64)
BLOCK_BORDER_LENGTHS = [8, 9, 16, 17, 18, 62, 63, 64, 65, 72, 73]


@pytest.mark.parametrize("msg_len", [0, 3, 32, 55, 120] + BLOCK_BORDER_LENGTHS)
def test_layout_matches_oracle_trace(oracle, msg_len):
    marks, n_wit, n_cons = oracle.layout(msg_len)
    lay = hostsim_lib.layout(msg_len)
    assert lay["n_witness"] == n_wit
    for name, start in marks:
        if name in ORACLE_TO_ABI:
            assert lay[ORACLE_TO_ABI[name]] == start, name


def test_params_witness_layout_and_witness(oracle):
    """ParametersVar allocated with AllocationMode::Witness (constraints.rs:198-211): segment table against the oracle's trace, then the
    device chain code (k_g1's params lanes, team_miller_pv) on the host against the oracle's vector — a valid and a tampered instance."""
    marks, n_wit, n_cons = oracle.layout(32, params_mode=1)
    lay = hostsim_lib.layout(32, params_mode=1)
    names = dict(ORACLE_TO_ABI, **{"params_alloc": "off_params_alloc", "prepare.g1_neg": "off_prep_g1"})
    assert lay["n_witness"] == n_wit and lay["params_mode"] == 1
    for name, start in marks:
        if name in names:
            assert lay[names[name]] == start, name
    pk, msg, sig, expect = synth.make_batch(oracle, 16)
    for i in (3, 15):
        n, _, res, w = oracle.witness(pk[i], msg[i].tobytes(), sig[i], params_mode=1)
        r, out = hostsim_lib.witness(pk[i], msg[i].tobytes(), sig[i], params_mode=1)
        assert n == out.shape[0] and bool(r) == res == bool(expect[i])
        bad = np.nonzero((w != out).any(axis=1))[0]
        assert len(bad) == 0, "first mismatching witness index %d" % bad[0]
    # Constant parameters: all three fields are zero and the table is the reference circuit's
    assert hostsim_lib.layout(32)["params_mode"] == 0 and hostsim_lib.layout(32)["off_prep_g1"] == 0


def test_library_exports_and_layout():
    pkg = importlib.import_module("bls-verify-gadget_amd")
    L = pkg.lib()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "blsw.h")).read()
    for sym in pkg.EXPORTED_SYMBOLS:
        assert sym + "(" in header
        assert getattr(L, sym) is not None
    assert pkg.layout(32) == hostsim_lib.layout(32)
    assert pkg.engine_workspace_bytes(1024, 32, 1, 1) > 0 and pkg.engine_workspace_bytes(1024, 32, 4, 3) > pkg.engine_workspace_bytes(1024, 32, 1, 1)


def _check(oracle, pk, msg, sig):
    n, ncons, res, w = oracle.witness(pk, msg, sig)
    r, out = hostsim_lib.witness(pk, msg, sig)
    assert out.shape[0] == n
    bad = np.nonzero((w != out).any(axis=1))[0]
    assert len(bad) == 0, "first mismatching witness index %d" % bad[0]
    assert bool(r) == res
    return res


def test_reference_gadget_case(oracle):
    # constraints.rs:318-376
    g = LIT["gadget_verify"]
    _, pk, _ = oracle.g1_decompress(bytes.fromhex(g["pubkey"]))
    _, sig, _ = oracle.g2_decompress(bytes.fromhex(g["signature"]))
    got = [_check(oracle, pk, bytes.fromhex(m), sig) for m in g["messages"]]
    assert got == g["expected"]


def test_synthetic_and_edge_cases(oracle):
    pk, msg, sig, expect = synth.make_batch(oracle, 16)
    assert _check(oracle, pk[3], msg[3].tobytes(), sig[3]) is True
    assert _check(oracle, pk[15], msg[15].tobytes(), sig[15]) is False  # tampered
    # identity public key / identity signature (verify_infinity_pubkey_and_infinity_signature.json): values stay defined
    zero_pk = np.zeros(12, dtype=np.uint64)
    zero_sig = np.zeros(24, dtype=np.uint64)
    # (the gadget's output VALUE is not meaningful there: the circuit is unsatisfiable; only value parity is checked)
    _check(oracle, zero_pk, msg[0].tobytes(), zero_sig)
    _check(oracle, pk[0], msg[0].tobytes(), zero_sig)
    _check(oracle, zero_pk, msg[0].tobytes(), sig[0])


@pytest.mark.parametrize("msg", [b"", b"abc", b"x" * 119] + [bytes((7 * i + n) & 0xFF for i in range(n)) for n in BLOCK_BORDER_LENGTHS], ids=lambda m: "len%d" % len(m) if len(m) in BLOCK_BORDER_LENGTHS else None)  # (the three earlier cases keep their ids)
def test_other_message_lengths(oracle, msg):
    pk, _, sig, _ = synth.make_batch(oracle, 16)
    _check(oracle, pk[1], msg, sig[1])


def _hs_decode(kind, data):
    import ctypes

    H = hostsim_lib.load()
    n = 12 if kind == "g1" else 24
    out = np.zeros(n, dtype=np.uint64)
    buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
    fn = H.hostsim_g1_decode if kind == "g1" else H.hostsim_g2_decode
    st = fn(buf, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return st, out


@pytest.mark.parametrize("name,case", eth_cases("deserialization_G1"))
def test_decode_g1_device_logic(oracle, name, case):
    # tests/tests.rs:336-349; wrong lengths are rejected before the kernel (the ABI takes fixed 48-byte records)
    b = unhex(case["input"]["pubkey"])
    if len(b) != 48:
        assert case["output"] is False
        return
    st, xy = _hs_decode("g1", b)
    assert (st in (0, 4)) == case["output"]
    ost, oxy, oinf = oracle.g1_decompress(b)
    assert (ost == 0) == (st in (0, 4))
    if st == 0:
        assert np.array_equal(xy, oxy)


@pytest.mark.parametrize("name,case", eth_cases("deserialization_G2"))
def test_decode_g2_device_logic(oracle, name, case):
    b = unhex(case["input"]["signature"])
    if len(b) != 96:
        assert case["output"] is False
        return
    st, xy = _hs_decode("g2", b)
    assert (st in (0, 4)) == case["output"]
    ost, oxy, oinf = oracle.g2_decompress(b)
    assert (ost == 0) == (st in (0, 4))
    if st == 0:
        assert np.array_equal(xy, oxy)


def test_decode_all_verify_fixture_points(oracle):
    for name, case in eth_cases("verify"):
        for kind, key in (("g1", "pubkey"), ("g2", "signature")):
            b = unhex(case["input"][key])
            st, xy = _hs_decode(kind, b)
            ost, oxy, oinf = (oracle.g1_decompress if kind == "g1" else oracle.g2_decompress)(b)
            assert (ost == 0) == (st in (0, 4)), name
            if st == 0:
                assert np.array_equal(xy, oxy), name


def test_endomorphism_subgroup_tests_against_the_order_r_definition(oracle):
    """g1_in_subgroup / g2_in_subgroup (decode.hpp: phi(P) = -[x^2]P and psi(P) = [x]P, the tests ark-bls12-381 0.4 itself uses, eprint 2021/1130)
    against the oracle's [r]P == O: random encodings (about half decode to curve points, all of large order outside the subgroup), points of the
    COFACTOR torsion ([r]Q for random curve points Q: the false positives an endomorphism test could have), and their sums with subgroup points."""
    import random

    P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    rnd = random.Random(0xE2D0)

    ops1 = dict(add=lambda a, b: (a + b) % P, sub=lambda a, b: (a - b) % P, mul=lambda a, b: a * b % P, inv=lambda a: pow(a, -1, P), zero=0)
    ops2 = dict(add=lambda a, b: ((a[0] + b[0]) % P, (a[1] + b[1]) % P), sub=lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P),
                mul=lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P),
                inv=lambda a: (lambda n: (a[0] * n % P, -a[1] * n % P))(pow(a[0] * a[0] + a[1] * a[1], -1, P)), zero=(0, 0))

    def ec_add(o, A, B):
        if A is None:
            return B
        if B is None:
            return A
        (x1, y1), (x2, y2) = A, B
        if x1 == x2:
            if o["add"](y1, y2) == o["zero"]:
                return None
            lam = o["mul"](o["mul"](o["add"](o["add"](x1, x1), x1), x1), o["inv"](o["add"](y1, y1)))
        else:
            lam = o["mul"](o["sub"](y2, y1), o["inv"](o["sub"](x2, x1)))
        x3 = o["sub"](o["sub"](o["mul"](lam, lam), x1), x2)
        return (x3, o["sub"](o["mul"](lam, o["sub"](x1, x3)), y1))

    def ec_mul(o, k, A):
        acc = None
        for bit in bin(k)[2:]:
            acc = ec_add(o, acc, acc)
            if bit == "1":
                acc = ec_add(o, acc, A)
        return acc

    def lex_largest_fp(y):
        return y > (P - 1) // 2

    def enc1(pt):
        x, y = pt
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if lex_largest_fp(y) else 0)
        return bytes(b)

    def enc2(pt):
        (x0, x1), (y0, y1) = pt
        b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
        big = lex_largest_fp(y1) if y1 else lex_largest_fp(y0)
        b[0] |= 0x80 | (0x20 if big else 0)
        return bytes(b)

    def agree(kind, data):
        st, xy = _hs_decode(kind, data)
        ost, oxy, oinf = (oracle.g1_decompress if kind == "g1" else oracle.g2_decompress)(data)
        assert (st if st != 4 else 0) == ost, (kind, data.hex(), st, ost)
        return ost

    # random encodings
    seen = {0: 0, 1: 0, 2: 0, 3: 0}
    curve1, curve2 = [], []
    for kind, nbytes in (("g1", 48), ("g2", 96)):
        for _ in range(60):
            b = bytearray(rnd.randbytes(nbytes))
            b[0] = 0x80 | (b[0] & 0x20) | (b[0] & 0x0F)  # compressed, not infinity, x below 2^380 (< p)
            if kind == "g2":
                b[48] &= 0x0F
            ost = agree(kind, bytes(b))
            seen[ost] += 1
            if ost == 3:
                (curve1 if kind == "g1" else curve2).append(bytes(b))
    assert seen[3] >= 30 and seen[2] >= 30 and seen[0] == 0  # curve points outside the subgroup, and x values without a point
    # cofactor torsion: [r]Q, and a subgroup point plus a torsion point
    g1gen = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
             0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
    assert agree("g1", enc1(g1gen)) == 0 and agree("g1", enc1(ec_mul(ops1, 0xD201000000010000, g1gen))) == 0
    n_t = 0
    for data in curve1[:6]:
        x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
        y = pow((x * x * x + 4) % P, (P + 1) // 4, P)
        t = ec_mul(ops1, R, (x, y))
        if t is None:
            continue
        assert agree("g1", enc1(t)) == 3  # order divides the cofactor
        assert agree("g1", enc1(ec_add(ops1, t, g1gen))) == 3
        n_t += 1
    assert n_t >= 4
    n_t = 0
    for data in curve2[:4]:
        x1 = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:48], "big")
        x0 = int.from_bytes(data[48:], "big")
        # y^2 = x^3 + 4 (1 + i): square root in Fp2 by the norm method
        xx = ops2["mul"]((x0, x1), (x0, x1))
        rhs = ops2["add"](ops2["mul"](xx, (x0, x1)), (4, 4))
        nrm = (rhs[0] * rhs[0] + rhs[1] * rhs[1]) % P
        s_ = pow(nrm, (P + 1) // 4, P)
        if s_ * s_ % P != nrm:
            continue
        for sg in (s_, P - s_):
            half = (rhs[0] + sg) * pow(2, -1, P) % P
            a = pow(half, (P + 1) // 4, P)
            if a * a % P == half and a:
                y = (a, rhs[1] * pow(2 * a, -1, P) % P)
                break
        else:
            continue
        assert ops2["mul"](y, y) == rhs
        t = ec_mul(ops2, R, ((x0, x1), y))
        if t is None:
            continue
        assert agree("g2", enc2(t)) == 3
        n_t += 1
    assert n_t >= 2


def test_aggregate_verify_device_logic(oracle):
    # constraints.rs:378-521 shape with 6 keys: key1 + 5 x key2, bitmap first two (true) / all (false); bit-exact vs oracle
    pk1 = "a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a"
    pk2 = "b301803f8b5ac4a1133581fc676dfedc60d891dd5fa99028805e5ea5b08d3491af75d0707adab3b70c6a6a580217bf81"
    sig = "912c3615f69575407db9392eb21fee18fff797eeb2fbe1816366ca2a08ae574d8824dbfafb4c9eaa1cf61b63c6f9b69911f269b664c42947dd1b53ef1081926c1e82bb2a465f927124b08391a5249036146d6f3f1e17ff5f162f779746d830d1"
    msg = bytes.fromhex("56" * 32)
    _, p1, _ = oracle.g1_decompress(bytes.fromhex(pk1))
    _, p2, _ = oracle.g1_decompress(bytes.fromhex(pk2))
    _, s, _ = oracle.g2_decompress(bytes.fromhex(sig))
    K = 6
    pks = np.stack([p1] + [p2] * (K - 1))
    for bm, want, want_count in ((np.array([1, 1, 0, 0, 0, 0], dtype=np.uint8), True, 2), (np.ones(K, dtype=np.uint8), False, K),
                                 (np.array([0, 1, 0, 1, 0, 0], dtype=np.uint8), False, 2)):
        n, res, cnt, marks, w = oracle.witness_aggregate(pks, bm, msg, s)
        r, c, out, lay = hostsim_lib.witness_aggregate(pks, bm, msg, s)
        assert lay["n_witness"] == n and lay["off_keys"] == marks["agg.keys"] and lay["off_bitmap"] == marks["agg.bitmap"]
        assert lay["off_count"] == marks["agg.count"] and lay["off_agg"] == marks["agg.loop"] and lay["off_pk_not_zero"] == marks["verify.pk_not_zero"]
        bad = np.nonzero((w != out).any(axis=1))[0]
        assert len(bad) == 0, "first mismatching witness index %d" % bad[0]
        assert bool(r) == res == want and c == cnt == want_count


@pytest.mark.parametrize("name,case", eth_cases("sign"))
def test_sign_device_logic(oracle, name, case):
    """Signer ladders + point encoding (decode.hpp) against tests/test_cases/sign/*.json (tests.rs:203-237: big-endian
    privkey in the JSON; null output <=> sk == 0); H(msg) is supplied by the oracle, pk is checked against the oracle."""
    sk = int.from_bytes(unhex(case["input"]["privkey"]), "big")
    msg = unhex(case["input"]["message"])
    _, h_xy = oracle.hash_to_g2(msg)
    st, sig, pk = hostsim_lib.sign(sk.to_bytes(32, "little"), h_xy)
    if case["output"] is None:
        assert st == 5  # SIGN_INVALID_SECRET_KEY
        assert sig == bytes([0xC0]) + bytes(95) and pk == bytes([0xC0]) + bytes(47)
    else:
        assert st == 0
        assert sig == unhex(case["output"])
        assert pk == oracle.sk_to_pk(sk)


def test_sign_rejects_noncanonical_secret_key(oracle):
    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    _, h_xy = oracle.hash_to_g2(b"\0" * 32)
    assert hostsim_lib.sign(r.to_bytes(32, "little"), h_xy)[0] == 1  # SIGN_BAD_ENCODING
    assert hostsim_lib.sign((r - 1).to_bytes(32, "little"), h_xy)[0] == 0
    # bls.rs:602-614 literal key -> pk equals the oracle's (pinned through the aggregate literal in test_oracle_fixtures)
    sk_le = bytes.fromhex(LIT["sk_limbs"]["hex_le"])
    st, _, pk = hostsim_lib.sign(sk_le, h_xy)
    assert st == 0 and pk == oracle.sk_to_pk(int.from_bytes(sk_le, "little"))


def test_team_pairing_program(oracle):
    """team.hpp (six lanes per instance: op tables + lane routines + the Miller / final-exponentiation program) on the host,
    lanes run one after the other per phase: full witness vector bit-exact against the oracle, true / false / edge inputs."""
    lib = hostsim_lib.load()
    lib.hostsim_use_team(1)
    try:
        g = LIT["gadget_verify"]
        _, pk, _ = oracle.g1_decompress(bytes.fromhex(g["pubkey"]))
        _, sig, _ = oracle.g2_decompress(bytes.fromhex(g["signature"]))
        got = [_check(oracle, pk, bytes.fromhex(m), sig) for m in g["messages"][:2]]
        assert got == g["expected"][:2]
        _check(oracle, np.zeros(12, dtype=np.uint64), bytes.fromhex(g["messages"][0]), np.zeros(24, dtype=np.uint64))
    finally:
        lib.hostsim_use_team(0)


def test_team_tables_are_current(tmp_path):
    """team_tables.hpp is generated (tools/gen_team_tables.py expands the tower formulas into op tables): the committed
    header must be what the generator emits, and every op's witness count must be the single-lane code's."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "team_tables.hpp"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_team_tables.py"), str(out)], capture_output=True, text=True, check=True)
    assert out.read_text() == open(os.path.join(root, "bls-verify-gadget_amd", "csrc", "team_tables.hpp")).read()
    counts = {l.split(":")[0]: int(l.split(" witnesses")[0].split()[-1]) for l in r.stderr.strip().splitlines()}
    # fp12_mul_w 54, fp12_sqr_w 36, cyclotomic square 18, mul_by_014 30 (constant y) / 2 + 36 (variable y), inverse check 18+12+12
    # ... G2 projective double 3 * 2 + 8 * 3, addition 12 * 3
    # ELLGS / ELLGH: the value-only general mul_by_014 of the native pairing (blsw_verify_batch): no witnesses
    assert counts == {"MUL": 54, "SQR": 36, "CYC": 18, "ELLC": 30, "ELLV": 38, "ELLGS": 0, "ELLGH": 0, "G2DBL": 30, "G2ADD": 36, "INVCHK": 42}


def test_team_table_invariants():
    """Structural checks of the generated op tables (tools/gen_team_tables.py): at most six tasks per round, at most four
    rounds, every witness offset of an op used exactly once, product slots written once and read only in later rounds."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_team_tables", os.path.join(root, "tools", "gen_team_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for op in gen.build_ops():
        rounds = op.schedule()
        assert 1 <= len(rounds) <= 4 and all(1 <= len(r) <= 6 for r in rounds), op.name
        assert sorted(i for r in rounds for i in r) == list(range(len(op.tasks))), op.name
        covered = []
        written = {}
        for ri, r in enumerate(rounds):
            for i in r:
                t = op.tasks[i]
                covered += list(range(t["woff"], t["woff"] + gen.KIND_WITNESSES[t["kind"]]))
                for lc in (t["a"], t["b"]):
                    lc.lists()  # raises if a combination does not fit a descriptor
                    for slot in lc.d:
                        assert 0 <= slot < gen.N_SLOTS
                        if gen.P0 <= slot < gen.P0 + gen.N_P:
                            assert written[slot] < ri, "%s: product slot %d read in the round that writes it" % (op.name, slot)
                if t["dst"] != 0xFF:
                    assert t["dst"] not in written or t["dst"] == gen.XH1
                    written[t["dst"]] = ri
        assert sorted(covered) == list(range(op.woff)), op.name
        for o in op.out:
            o.lists()
            assert all(slot in written or slot < gen.P0 or slot >= gen.X0 for slot in o.d), op.name
        if op.name in ("G2DBL", "G2ADD"):
            # k_g2_alloc_team sizes its LDS file by these two tables: TS_P + 12 slots per team
            named = set(written) - {0xFF}
            for t in op.tasks:
                named |= set(t["a"].d) | set(t["b"].d)
            for o in op.out:
                named |= set(o.d)
            assert named and max(named) < gen.P0 + 12, "%s names slot %d: beyond the slot file of k_g2_alloc_team" % (op.name, max(named))


def test_value_only_hash_to_g2_device_logic(oracle):
    """vcurve.hpp (SSWU + isogeny without witnesses, psi-based cofactor clearing: two 64-bit ladders instead of the 636-bit
    h_eff ladder of the circuit) gives the point of hash_to_g2_with_cons (hasher.rs:727-740) — the reference's own equality,
    hasher.rs:1004-1026 — for the bls.rs:645 input, the reference's test strings and ragged lengths."""
    msgs = [b"", b"abc", b"abcdef0123456789", b"\x00" * 32, bytes(range(55)), bytes(range(56)), bytes(range(119)), bytes(range(120)), b"q" * 300]
    for m in msgs:
        _, want = oracle.hash_to_g2(m)
        got = hostsim_lib.hash_to_g2_values(m)
        assert np.array_equal(got, want), len(m)


def test_sign_random_scalars_device_logic(oracle):
    """vsign.hpp against the oracle's signer on scalars that exercise every digit pattern of the base-|x| decomposition
    (small, one-digit, digit borders, near r) and random ones: sig = sk * H(m) through the psi ladder, pk = sk * g1 through the
    fixed-base windows."""
    import random

    r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    z = 0xD201000000010000
    rng = random.Random(7)
    sks = [1, 2, 15, 16, z - 1, z, z + 1, z * z, z * z - 1, z ** 3, z ** 3 + z * z + z + 1, r - 1, r - 2, (1 << 254) + 1] + [rng.randrange(1, r) for _ in range(10)]
    msg = b"vsign"
    _, h_xy = oracle.hash_to_g2(msg)
    for sk in sks:
        st, sig, pk = hostsim_lib.sign(sk.to_bytes(32, "little"), h_xy)
        assert st == 0
        assert sig == oracle.sign(sk, msg), hex(sk)
        assert pk == oracle.sk_to_pk(sk), hex(sk)


def test_cofactor_chunks_in_parallel_device_logic(oracle):
    """cofactor_par.hpp: clear_cofactor2's three 255-bit chunks as independent programs (chunk order 2, 0, 1: the start points of
    chunks 1 and 2 are VALUES — Jacobian doublings and one inversion — not the end of the previous chunk) and the join that folds
    them: the whole witness vector stays bit-exact, for valid / tampered instances, identity inputs and another message length."""
    lib = hostsim_lib.load()
    lib.hostsim_cofactor_par(1)
    try:
        pk, msg, sig, _ = synth.make_batch(oracle, 16)
        assert _check(oracle, pk[3], msg[3].tobytes(), sig[3]) is True
        assert _check(oracle, pk[15], msg[15].tobytes(), sig[15]) is False
        _check(oracle, np.zeros(12, dtype=np.uint64), msg[0].tobytes(), np.zeros(24, dtype=np.uint64))
        _check(oracle, pk[1], b"x" * 119, sig[1])
    finally:
        lib.hostsim_cofactor_par(0)


def test_native_verify_values_device_logic(oracle):
    """vpairing.hpp (blsw_verify_batch): BLS::verify as values — projective line coefficients (no inversion per step: the lines differ from the
    circuit's affine ones by factors in Fp2, which the final exponentiation kills), a two-pair Miller loop on the six-lane team program with the
    general mul_by_014 op tables, team.hpp's final exponentiation with a null cursor. Verdicts against the reference's fixtures (all 29
    verify/*.json incl. tampered, infinity and non-subgroup inputs) and the oracle's native verify on synthetic valid / tampered instances."""
    n_true = 0
    for name, case in eth_cases("verify"):
        i = case["input"]
        pk, msg, sig = unhex(i["pubkey"]), unhex(i["message"]), unhex(i["signature"])
        if len(pk) != 48 or len(sig) != 96:
            continue
        r, st_pk, st_sig = hostsim_lib.verify_values(pk, sig, msg)
        assert bool(r) == case["output"] == oracle.verify_bytes(pk, msg, sig), name
        n_true += r
    assert n_true >= 9
    pk, msg, sig, expect = synth.make_batch(oracle, 32)
    for i in (0, 7, 15, 31):
        r, _, _ = hostsim_lib.verify_values(oracle.g1_compress(pk[i]), oracle.g2_compress(sig[i]), msg[i].tobytes())
        assert bool(r) == bool(expect[i]), i


def test_cofactor_values_first_device_logic(oracle):
    """cofactor_vf.hpp: the doubling chain and the addition chains of clear_cofactor2 as Jacobian VALUE programs (one inversion each, the
    other 1 / Z by the backward recurrence), every doubling's / addition's witnesses derived independently at its planned place (the
    parallel phases run in reverse lane order here) and the join: the whole witness vector stays bit-exact, for valid / tampered
    instances, identity inputs and another message length; and for chosen (Q0, Q1) incl. sum = identity, Q1 = identity, Q0 = Q1."""
    import ctypes

    lib = hostsim_lib.load()
    lib.hostsim_cofactor_par(2)
    try:
        pk, msg, sig, _ = synth.make_batch(oracle, 16)
        assert _check(oracle, pk[3], msg[3].tobytes(), sig[3]) is True
        assert _check(oracle, pk[15], msg[15].tobytes(), sig[15]) is False
        _check(oracle, np.zeros(12, dtype=np.uint64), msg[0].tobytes(), np.zeros(24, dtype=np.uint64))
        _check(oracle, pk[1], b"x" * 119, sig[1])
        p_mod = int("1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab", 16)
        _, a = oracle.hash_to_g2(b"cofactor-a")
        _, b = oracle.hash_to_g2(b"cofactor-b")

        def neg(xy):
            out = xy.copy()
            for k in (2, 3):
                v = int.from_bytes(xy[6 * k:6 * k + 6].tobytes(), "little")
                out[6 * k:6 * k + 6] = np.frombuffer(((p_mod - v) % p_mod).to_bytes(48, "little"), dtype=np.uint64)
            return out

        u64p = ctypes.POINTER(ctypes.c_uint64)
        zero = np.zeros(24, dtype=np.uint64)
        for q0, q1 in ((a, b), (a, neg(a)), (a, zero), (a, a), (zero, zero)):
            s1 = np.zeros((36 + 8979, 6), dtype=np.uint64)
            s2 = np.zeros((36 + 8979, 6), dtype=np.uint64)
            ok = lib.hostsim_cofactor_compare(np.ascontiguousarray(q0).ctypes.data_as(u64p), np.ascontiguousarray(q1).ctypes.data_as(u64p), s1.ctypes.data_as(u64p), s2.ctypes.data_as(u64p))
            assert ok == 1 and s1.any()
    finally:
        lib.hostsim_cofactor_par(0)


def test_prepare_values_first_device_logic(oracle):
    """prepare_vf.hpp: the 63 doublings + 5 additions of G2PreparedVar::from_group_var as one Jacobian value chain (one inversion, the other
    1 / Z by the backward recurrence) and every step's witnesses / line coefficients derived independently (steps in reverse order here): the
    whole witness vector — the pairing consumes the coefficients — stays bit-exact, incl. identity inputs, the N+1-pair circuit and the team program."""
    lib = hostsim_lib.load()
    lib.hostsim_prepare_vf(1)
    try:
        pk, msg, sig, _ = synth.make_batch(oracle, 16)
        assert _check(oracle, pk[3], msg[3].tobytes(), sig[3]) is True
        assert _check(oracle, pk[15], msg[15].tobytes(), sig[15]) is False
        _check(oracle, np.zeros(12, dtype=np.uint64), msg[0].tobytes(), np.zeros(24, dtype=np.uint64))
        lib.hostsim_use_team(1)
        _check(oracle, pk[1], b"x" * 3, sig[1])
    finally:
        lib.hostsim_use_team(0)
        lib.hostsim_prepare_vf(0)


def test_cofactor_chunks_when_the_sum_is_the_identity(oracle):
    """Q0 = -Q1 (not reachable by hashing): the circuit's affine chain then runs on (0, 0) with zero inverse hints. The chunked
    program must follow those values step by step (its Jacobian shortcut would compute a different, mathematically meaningful
    point), and must equal the serial chain on ordinary sums, Q1 = identity and Q0 = Q1 as well."""
    import ctypes

    lib = hostsim_lib.load()
    p_mod = int("1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab", 16)
    _, a = oracle.hash_to_g2(b"cofactor-a")
    _, b = oracle.hash_to_g2(b"cofactor-b")

    def neg(xy):  # (x, -y) on Montgomery limbs: p - y limbwise through python integers
        out = xy.copy()
        for k in (2, 3):
            v = int.from_bytes(xy[6 * k:6 * k + 6].tobytes(), "little")
            out[6 * k:6 * k + 6] = np.frombuffer(((p_mod - v) % p_mod).to_bytes(48, "little"), dtype=np.uint64)
        return out

    u64p = ctypes.POINTER(ctypes.c_uint64)
    zero = np.zeros(24, dtype=np.uint64)
    for q0, q1 in ((a, b), (a, neg(a)), (a, zero), (a, a), (zero, zero)):
        s1 = np.zeros((36 + 8979, 6), dtype=np.uint64)
        s2 = np.zeros((36 + 8979, 6), dtype=np.uint64)
        ok = lib.hostsim_cofactor_compare(np.ascontiguousarray(q0).ctypes.data_as(u64p), np.ascontiguousarray(q1).ctypes.data_as(u64p), s1.ctypes.data_as(u64p), s2.ctypes.data_as(u64p))
        assert ok == 1 and s1.any()
