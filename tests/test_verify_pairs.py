"""blsw_verify_pairs_batch (AggregateVerify as values) without a GPU: the stages of csrc/vpairs.hpp compiled for the host (tests/vpairs) against the
reference's fixtures, the CPU oracle and the construction of the instances — the four properties include/blsw.h states (Q1 one pair is BLS::verify,
Q2 order and unused pairs do not matter, Q3 equal messages give fast_aggregate_verify, Q4 the Boolean of the N+1-pair circuit), the status rules,
the chunk table — and the argument rules of the two entry points, which precede any HIP call."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import hostsim_lib, vpairs_lib
from tests.oracle_lib import eth_cases, unhex
from tests.vpairs_lib import IDENTITY48

ST_OK, ST_BAD_ENCODING, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_BAD_INDEX = 0, 1, 2, 3, 4, 6
IDENTITY96 = bytes([0xC0]) + bytes(95)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def c(pkg):
    return pkg.VERIFY_PAIRS_CHUNK


@pytest.fixture(scope="module")
def pool(oracle, c):
    """2 c + 2 secret keys with their public keys, distinct messages and single signatures, computed once and never changed"""
    m = 2 * c + 2
    sks = [0x2345671 + 7919 * j for j in range(m)]
    msgs = [bytes([0x60 + j, j]) * 16 for j in range(m)]
    return tuple(sks), tuple(oracle.sk_to_pk(s) for s in sks), tuple(msgs), tuple(oracle.sign(s, x) for s, x in zip(sks, msgs))


def _flip(msg):
    return bytes([msg[0] ^ 1]) + msg[1:]


def _circuit(oracle, pks, msgs, sig):
    """the Boolean of the N+1-pair circuit on decoded points (Q4)"""
    pks_xy = np.stack([oracle.g1_decompress(p)[1] for p in pks])
    st, sig_xy, inf = oracle.g2_decompress(sig)
    assert st == 0 and not inf
    return oracle.witness_multi(pks_xy, np.frombuffer(b"".join(msgs), np.uint8).reshape(len(msgs), -1), sig_xy, want_vector=False)[1]


@pytest.mark.parametrize("k_of", ["1", "2", "c", "c+1", "2c+1"])
def test_one_instance_through_the_host_stages(oracle, pool, c, k_of):
    """valid, a tampered message, a wrong key and a signature that misses one pair, each folded with chunk 1, c and 31 and held against the circuit"""
    K = {"1": 1, "2": 2, "c": c, "c+1": c + 1, "2c+1": 2 * c + 1}[k_of]
    _, pks, msgs, sigs = pool
    pks, msgs = list(pks[:K]), list(msgs[:K])
    sig = oracle.aggregate_g2(list(sigs[:K]))
    j = K - 1 if K <= c else c - 1  # the last pair of the first chunk, or of the list
    tampered = msgs[:j] + [_flip(msgs[j])] + msgs[j + 1:]
    wrong = pks[:j] + [pool[1][K]] + pks[j + 1:]
    short = oracle.aggregate_g2(list(sigs[:K - 1])) if K > 1 else IDENTITY96  # over K - 1 pairs; the sum of no signature is the identity
    cases = [("valid", pks, msgs, sig, True), ("tampered", pks, tampered, sig, False), ("wrong key", wrong, msgs, sig, False), ("short", pks, msgs, short, False)]
    res, st, kst, wr = vpairs_lib.instances(vpairs_lib.pack([p for _, p, _, _, _ in cases], 48), vpairs_lib.pack([m for _, _, m, _, _ in cases], 32),
                                            np.frombuffer(b"".join(s for _, _, _, s, _ in cases), np.uint8).reshape(4, 96), chunks=(1, c, 31))
    assert not kst.any() and not st[:3].any() and st[3].tolist() == [0, 0 if K > 1 else ST_IDENTITY]
    assert wr[:3].all() and wr[3].all() == (K > 1)
    for i, (name, p, m, s, expect) in enumerate(cases):
        assert res[:, i].tolist() == [int(expect)] * 3, (name, res[:, i])
        if s != IDENTITY96:
            assert _circuit(oracle, p, m, s) == expect, name


def test_q1_verify_fixtures_as_one_pair(oracle):
    rows = [(name, unhex(x["input"]["pubkey"]), unhex(x["input"]["message"]), unhex(x["input"]["signature"]), x["output"]) for name, x in eth_cases("verify")]
    assert len(rows) == 29 and all(len(r[1]) == 48 and len(r[2]) == 32 and len(r[3]) == 96 for r in rows)
    res, st, kst, _ = vpairs_lib.instances(vpairs_lib.pack([[r[1]] for r in rows], 48), vpairs_lib.pack([[r[2]] for r in rows], 32),
                                           np.frombuffer(b"".join(r[3] for r in rows), np.uint8).reshape(29, 96), chunks=(1, 8))
    for i, (name, pk, msg, sig, out) in enumerate(rows):
        v, st_pk, st_sig = hostsim_lib.verify_values(pk, sig, msg)
        assert res[:, i].tolist() == [v, v] and bool(v) == out == oracle.verify_bytes(pk, msg, sig), name
        assert st[i].tolist() == [st_pk, st_sig] and kst[i, 0] == st_pk, name
    assert res[0].sum() >= 9


def test_meaning_of_two_pairs(oracle, pool):
    """K = 2: the verdict is whether e_ref(-g1, sig) e_ref(pk_0, H(m_0)) e_ref(pk_1, H(m_1)) is one, by the independent pairing of tests/pairing_ref.py"""
    from tests import curve_ref as C
    from tests import field_ref as F
    from tests import pairing_ref as R

    assert R.prove()
    _, pks, msgs, sigs = pool
    sig = oracle.aggregate_g2(list(sigs[:2]))

    def point(kind, b):
        st, x, y = C.decode(kind, b)
        assert st == 0
        return (x, y)

    for m, expect in ((list(msgs[:2]), True), ([msgs[0], _flip(msgs[1])], False)):
        value = R.product([R.e_ref(R.NEG_G1, point("g2", sig))] + [R.e_ref(point("g1", p), point("g2", oracle.hash_to_g2(x)[0])) for p, x in zip(pks[:2], m)])
        assert (value == F.F12_ONE) == expect
        res, st, _ = vpairs_lib.instance(pks[:2], m, sig, chunks=(1, 8))
        assert res.tolist() == [int(expect)] * 2 and not st.any()


def test_q3_fast_aggregate_verify_fixtures(oracle):
    """the 11 fixtures with the message repeated for every key, padded to the longest list, one call with counts"""
    cases = eth_cases("fast_aggregate_verify")
    assert len(cases) == 11
    ins = [([unhex(p) for p in x["input"]["pubkeys"]], unhex(x["input"]["message"]), unhex(x["input"]["signature"]), x["output"]) for _, x in cases]
    assert all(len(m) == 32 and len(s) == 96 and IDENTITY48 not in p for p, m, s, _ in ins)
    counts = [len(p) for p, _, _, _ in ins]
    assert counts.count(0) == 2
    res, st, _, _ = vpairs_lib.instances(vpairs_lib.pack([p for p, _, _, _ in ins], 48), vpairs_lib.pack([[m] * len(p) for p, m, _, _ in ins], 32),
                                         np.frombuffer(b"".join(s for _, _, s, _ in ins), np.uint8).reshape(11, 96), counts=counts, chunks=(2, 8))
    for i, ((name, _), (p, m, s, out)) in enumerate(zip(cases, ins)):
        agg = oracle.aggregate_g1(p) if p else None
        assert res[:, i].tolist() == [int(out)] * 2 and out == bool(agg and oracle.verify_bytes(agg, m, s)), name
        if not p:
            assert "na_pubkeys" in name and st[i, 0] == ST_IDENTITY
    assert res[0].sum() == 3


def test_q2_order_and_unused_pairs(oracle, pool, c):
    _, pks, msgs, sigs = pool
    K, used = c + 3, c + 1
    sig = oracle.aggregate_g2(list(sigs[:used]))
    perm = np.random.default_rng(5).permutation(used).tolist()
    assert perm != sorted(perm)
    garbage = [bytes([0xFF]) * 48, bytes(48)]  # neither decodes
    rows_p = [list(pks[:used]) + list(pks[used:K]), [pks[j] for j in perm] + garbage, list(pks[:used]) + garbage]
    rows_m = [list(msgs[:used]) + list(msgs[used:K]), [msgs[j] for j in perm] + [b"\xEE" * 32] * 2, list(msgs[:used]) + [_flip(msgs[0])] * 2]
    sg = np.frombuffer(sig * 3, np.uint8).reshape(3, 96)
    res, st, kst, wr = vpairs_lib.instances(vpairs_lib.pack(rows_p, 48), vpairs_lib.pack(rows_m, 32), sg, counts=[used] * 3, chunks=(1, c, 31))
    assert (res == 1).all() and not st.any() and not kst[:, :used].any() and (kst[1:, used:] == ST_BAD_ENCODING).all()
    assert wr[:, :used].all() and not wr[:, used:K].any() and wr[:, K].all()  # an unused pair is not even walked
    # the same rows with every pair used: the valid keys behind the count now spoil the product, the garbage spoils the status
    res, st, _, _ = vpairs_lib.instances(vpairs_lib.pack(rows_p, 48), vpairs_lib.pack(rows_m, 32), sg, chunks=(c,))
    assert res.tolist() == [[0, 0, 0]] and st[:, 0].tolist() == [ST_OK, ST_BAD_ENCODING, ST_BAD_ENCODING]


def test_status_rules(oracle, pool, c):
    """key statuses from the G1 deserialization fixtures; the earliest bad USED pair wins, count 0 and a count beyond K come first"""
    from tests import curve_ref as C

    _, pks, msgs, sigs = pool
    bad = {}
    for name, x in eth_cases("deserialization_G1"):
        b = unhex(x["input"]["pubkey"])
        if len(b) == 48 and not (x["output"] and b != IDENTITY48):
            bad.setdefault(C.decode("g1", b)[0], b)
    assert sorted(bad) == [ST_BAD_ENCODING, ST_NOT_ON_CURVE, ST_NOT_IN_SUBGROUP, ST_IDENTITY]
    K = 4
    sig = oracle.aggregate_g2(list(sigs[:K]))
    good = list(pks[:K])
    rows, counts, want = [], [], []

    def row(keys, count, status):
        rows.append(keys)
        counts.append(count)
        want.append(status)

    for s, b in sorted(bad.items()):
        row([good[0], b, good[2], good[3]], K, s)          # a bad used pair
        row([good[0], good[1], b, good[3]], 2, ST_OK)      # behind the count: no influence
    row([good[0], bad[ST_IDENTITY], bad[ST_NOT_ON_CURVE], bad[ST_BAD_ENCODING]], K, ST_IDENTITY)  # the earliest wins
    row([good[0], good[1], bad[ST_NOT_IN_SUBGROUP], bad[ST_BAD_ENCODING]], 3, ST_NOT_IN_SUBGROUP)
    row([bad[ST_BAD_ENCODING]] * K, 0, ST_IDENTITY)         # an empty list, whatever it holds
    row(good, 0, ST_IDENTITY)
    row(good, K + 1, ST_BAD_INDEX)
    row([bad[ST_BAD_ENCODING]] * K, 0xFFFFFFFF, ST_BAD_INDEX)
    row(good, K, ST_OK)
    n = len(rows)
    res, st, kst, wr = vpairs_lib.instances(vpairs_lib.pack(rows, 48), vpairs_lib.pack([list(msgs[:K])] * n, 32), np.frombuffer(sig * n, np.uint8).reshape(n, 96), counts=counts,
                                            chunks=(2, c))
    assert st[:, 0].tolist() == want and not st[:, 1].any()
    assert kst.tolist() == [[C.decode("g1", k)[0] for k in keys] for keys in rows]
    assert res.tolist() == [[0] * (n - 1) + [1]] * 2  # the rows with a count of 2 carry a signature over four pairs
    assert not wr[[i for i in range(n) if want[i] != ST_OK]].any()  # an instance that cannot pass walks nothing
    # the rule alone, over a table: counts None = all K
    table = np.array([[0, 0, 0], [0, 3, 1], [4, 0, 2], [0, 0, 1]], dtype=np.int32)
    assert [vpairs_lib.status(None, i, 3, table) for i in range(4)] == [ST_OK, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_BAD_ENCODING]
    assert [vpairs_lib.status([2, 1, 0, 4], i, 3, table) for i in range(4)] == [ST_OK, ST_OK, ST_IDENTITY, ST_BAD_INDEX]
    assert [vpairs_lib.status([3, 3, 1, 2], i, 3, table) for i in range(4)] == [ST_OK, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_OK]


def test_chunk_table_covers_each_used_pair_once():
    for K in range(1, 2 * 31 + 2):
        for chunk in range(1, 32):
            cpi = vpairs_lib.chunks_per_instance(K, chunk)
            assert cpi == -(-K // chunk)
            for count in range(K + 1):
                seen = []
                for q in range(cpi):
                    first, cnt, mask, mask_off = vpairs_lib.chunk(chunk, count, q)
                    assert cnt <= chunk and mask_off == 0
                    assert mask == ((1 << cnt) - 1) | ((1 << cnt) if q == 0 else 0)  # the instance's own pair rides with chunk 0, behind its pairs
                    if cnt:
                        assert first == q * chunk
                    seen += list(range(first, first + cnt))
                assert seen == list(range(count)), (K, chunk, count)


def test_argument_rules_without_a_gpu(pkg):
    L = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17
    assert pkg.VERIFY_PAIRS_CHUNK == H["defines"]["BLSW_VPAIRS_CHUNK"] and 1 <= pkg.VERIFY_PAIRS_CHUNK <= 31
    assert {"blsw_verify_pairs_workspace_bytes", "blsw_verify_pairs_batch"} <= set(pkg.EXPORTED_SYMBOLS)
    ERR_ARG = 1
    p = ctypes.c_void_p(0x1000)  # never dereferenced: the calls fail before any device work
    good = dict(pks=p, msgs=p, msg_len=32, K=8, counts=p, sig=p, n=64, res=p, st=p, kst=p, ws=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.blsw_verify_pairs_batch(a["pks"], a["msgs"], a["msg_len"], a["K"], a["counts"], a["sig"], a["n"], a["res"], a["st"], a["kst"], a["ws"], 1 << 60, None)

    for kw in (dict(n=0), dict(K=0), dict(K=65536), dict(n=0x7FFFFFFF // 8 + 1), dict(n=0x80000000, K=1), dict(n=1 << 40, K=1), dict(msg_len=65536), dict(pks=None), dict(sig=None),
               dict(res=None), dict(st=None), dict(ws=None), dict(msgs=None), dict(counts=None, kst=None, n=0)):
        assert call(**kw) == ERR_ARG, kw
    b = ctypes.c_uint64(0)
    for n, msg_len, K in ((0, 32, 8), (64, 32, 0), (64, 32, 65536), (0x7FFFFFFF // 8 + 1, 32, 8), (0x80000000, 32, 1), (64, 65536, 8)):
        assert L.blsw_verify_pairs_workspace_bytes(n, msg_len, K, ctypes.byref(b)) == ERR_ARG
    assert L.blsw_verify_pairs_workspace_bytes(64, 32, 8, None) == ERR_ARG
    assert L.blsw_verify_pairs_workspace_bytes(0x7FFFFFFF // 8, 32, 8, ctypes.byref(b)) == 0  # the largest legal n * K at K = 8
    assert L.blsw_verify_pairs_workspace_bytes(0x7FFFFFFF, 0, 1, ctypes.byref(b)) == 0

    def size(n, msg_len, K):
        assert L.blsw_verify_pairs_workspace_bytes(n, msg_len, K, ctypes.byref(b)) == 0
        return b.value

    for axis in ("n", "K", "msg_len"):
        last = 0
        for v in (1, 2, 7, 8, 9, 63, 64, 65, 1000, 1024, 1025, 4096):
            shape = dict(n=5, K=3, msg_len=32)
            shape[axis] = v if axis != "msg_len" else v - 1
            assert size(**shape) >= last, (axis, v)
            last = size(**shape)
    # the dominant term: one set of lines per pair, 6 * 68 field elements of 48 bytes
    assert size(64, 32, 16) - size(64, 32, 8) >= 64 * 8 * 6 * 68 * 48
    v = ctypes.c_uint64(0)
    assert L.blsw_verify_workspace_bytes(64 * 8, 32, ctypes.byref(v)) == 0 and size(64, 32, 8) < v.value  # one set of lines per pair, where n K triples hold two
