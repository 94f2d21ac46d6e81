"""The SHA-256 gadget and hash_to_field layer (csrc/sha.hpp) through the host compilation (tests/hostsim: hostsim_sha_op, hostsim_hash_expand)
against the two-tier reference tests/sha_ref.py and the oracle's "hash.expand" segment, bit for bit, on every launch the device test
(test_sha_device_gpu.py) makes. The reference's meaning tier is held to hashlib and the RFC's vectors; its bit tier is only used after its digests
have been held to the meaning tier (sha_ref.expand_gadget asserts it on every lane). Without a GPU this validates the reference, the inputs and the
host compilation; the device test then holds the device compilations to the same expected values."""
import ctypes
from concurrent.futures import ThreadPoolExecutor
import json
import os

import numpy as np
import pytest

from tests import devsha_lib as D
from tests import hostsim_lib
from tests import sha_edges as X
from tests import sha_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NO_MSG_OPS = [op for op in S.OP_NAMES if not S.OPS[op][2]]
GROUP = 8  # lengths per case of the sweep
_SHORT = [n for n in X.STREAM_LENGTHS if n < 8000]
LENGTH_GROUPS = [_SHORT[i:i + GROUP] for i in range(0, len(_SHORT), GROUP)] + [[8080], [8081]]


def test_table_is_the_compiled_table():
    assert D.host_table() == [(n,) + S.OPS[n] for n in S.OP_NAMES]
    assert sorted(x for g in LENGTH_GROUPS for x in g) == sorted(X.STREAM_LENGTHS)


def test_meaning_tier():
    """expand_message_xmd against the RFC 9380 vectors of tests/golden/literals.json; the msg' layout (asserted inside msg_prime) and the SHA
    padding against hashlib's own at every length of the sweep; hash_to_field and the Montgomery form"""
    lit = json.load(open(os.path.join(GOLDEN, "literals.json")))
    assert len(lit["expand"]) >= 2
    for case in lit["expand"]:
        assert S.expand_message_xmd(bytes.fromhex(case["msg"]), case["len_in_bytes"], bytes.fromhex(case["dst"])).hex() == case["uniform_bytes"]
    for n in X.LENGTHS:
        mp = S.msg_prime(X.messages(n, 4)[3])
        padded = mp + S.sha_padding(len(mp))
        assert len(padded) % 64 == 0 and len(padded) // 64 == (n + 183) // 64 and int.from_bytes(padded[-8:], "big") == 8 * (n + 111)
        assert padded[len(mp)] == 0x80 and not any(padded[len(mp) + 1:-8])
    assert S.hash_to_field(bytes(63) + b"\x05") == 5 and S.hash_to_field(S.P.to_bytes(64, "big")) == 0
    assert S.mont_limbs32(1) == [(S.R >> (32 * i)) & 0xFFFFFFFF for i in range(12)] and S.R == (1 << 384) % S.P
    assert len(S.DST) == 43


def test_coverage_conditions():
    """what the lists must contain, asserted on the lists: every residue mod 64 and both sides of each block border among the lengths of the
    stream sweep; a length with a three-byte bit length in it and below it; every ordered pair of the six bit kinds in the operands of w_xor and of
    w_and; each carry value 0 .. k - 1 of each addmany; item counts on both sides of a wave"""
    assert {n % 64 for n in X.STREAM_LENGTHS} == set(range(64))
    blocks = lambda n: (n + 183) // 64
    for border in (9, 73, 137):
        assert border - 1 in X.STREAM_LENGTHS and border in X.STREAM_LENGTHS and blocks(border) == blocks(border - 1) + 1
    assert 8 * (8080 + 111) < 1 << 16 <= 8 * (8081 + 111) and {8080, 8081} <= set(X.STREAM_LENGTHS) and 65535 in X.LENGTHS
    for op in ("w_xor", "w_and"):
        assert X.xor_and_kind_pairs(op) == {(a, b) for a in range(6) for b in range(6)}
    for k in (2, 3, 4, 5):
        seen = set()
        for w, _ in X.cases("w_addmany%d" % k):
            if any(w[3 * i + 1] != 0xFFFFFFFF for i in range(k)):  # not folded
                seen.add(sum(w[3 * i] for i in range(k)) >> 32)
        assert seen == set(range(k)), (k, seen)
    assert {1, 63, 64, 65, 70} == set(X.ITEM_COUNTS) and X.LANES == 70
    bits136 = [w for w, _ in X.cases("hash_to_field_elem") if (w[11] >> 8) & 0xFF]  # bits 136 .. 143 of the 512-bit input
    assert len(bits136) >= 8


@pytest.mark.parametrize("op", NO_MSG_OPS)
def test_host_compilation_equals_reference(op):
    bad, items = [], 0
    for name, msg_len, cases in X.launches(op):
        bad += [(name,) + b for b in D.run_host(op, msg_len, cases)]
        items += len(cases)
    print("%s: %d launches, %d items, %d mismatches" % (op, len(X.launches(op)), items, len(bad)))
    assert not bad, bad[:10]
    if op == "sha_block_w":  # the constant-state, constant-data case: no bit may leave
        c = [c for c in X.cases(op) if all(c[0][3 * i + 1] == 0xFFFFFFFF for i in range(24))]
        assert c and all(S.expected(op, x)[1] == [] for x in c)


def test_fast_path_equals_generic_statement():
    """sha_block_w and sha_block_generic have the same cases and so the same expected bits: the header's "must emit the same bits", asserted"""
    assert X.cases("sha_block_w") is not X.cases("sha_block_generic")
    assert [c for c in X.cases("sha_block_w")] == [c for c in X.cases("sha_block_generic")]


@pytest.mark.parametrize("msg_len", X.B0_LENGTHS)
def test_b0_block_every_byte(msg_len):
    """b0_byte over every k of the padded msg', the message constant and not"""
    cases = X.msg_cases("b0_block", msg_len)
    assert len(cases) == 2 * ((msg_len + 183) // 64)
    bad = D.run_host("b0_block", msg_len, cases)
    assert not bad, bad[:10]


@pytest.mark.parametrize("msg_len", X.LENGTHS)
def test_expand_message_values(msg_len):
    lanes = 4 if msg_len > 10000 else X.LANES
    bad = D.run_host("expand_message_values", msg_len, X.msg_cases("expand_message_values", msg_len, lanes))
    assert not bad, bad[:10]


@pytest.mark.parametrize("lengths", LENGTH_GROUPS, ids=lambda g: "%d-%d" % (g[0], g[-1]))
def test_oracle_segment_equals_host_segment_equals_reference(oracle, lengths):
    """For every length and every message of the lists: the reference's bit stream (70 lanes per walk) == expand_message_w through the op table
    (streams, 64 words, bit and word counts) == hostsim_hash_expand's segment; and == the oracle's "hash.expand" segment for the all-0x00, all-0xFF,
    counter and first random message. The layout's sha_bits equals the reference's count. The first differing bit is named by digest, block and
    round."""
    H = hostsim_lib.load()
    H.hostsim_hash_expand.restype = ctypes.c_int64
    u8p = ctypes.POINTER(ctypes.c_uint8)
    for n in lengths:
        w = D.gadget_walk(n)
        nbits = w["bits"].shape[1]
        assert hostsim_lib.layout(n)["sha_bits"] == nbits, (n, nbits)
        cases = X.msg_cases("expand_message_w", n)
        bad = D.run_host("expand_message_w", n, cases)
        assert not bad, (n, bad[:5])
        with ThreadPoolExecutor(4) as pool:  # (the oracle's four walks beside each other: its state is per thread)
            from_oracle = list(pool.map(lambda lane: oracle.hash_expand(X.messages(n)[lane]), range(4)))
        for lane in (0, 1, 2, 3):
            msg = X.messages(n)[lane]
            seg, uni = np.zeros(nbits + 8, dtype=np.uint8), (ctypes.c_uint8 * 256)()
            buf = (ctypes.c_uint8 * max(1, n)).from_buffer_copy(msg if n else b"\0")
            assert H.hostsim_hash_expand(buf, n, seg.ctypes.data_as(u8p), ctypes.c_uint64(nbits + 8), uni) == nbits
            obits, ouni = from_oracle[lane]
            for name, got, gu in (("host", seg[:nbits], bytes(uni)), ("oracle", obits, ouni)):
                assert len(got) == nbits, (name, n, len(got), nbits)
                d = np.flatnonzero(got != w["bits"][lane])
                assert d.size == 0, "%s segment, msg_len %d, message %d: %d bits differ, the first is bit %d (%s)" % (name, n, lane, d.size, d[0], S.where_is(w["marks"], int(d[0])))
                assert gu == S.expand_message_xmd(msg), (name, n, lane)
        for k in (2, 4, 5):  # the carries a message can reach (no three-operand addmany is reachable from a message)
            assert 3 not in w["carries"] and len(w["carries"][k]) >= 2
