"""blsw_verify_groups_batch without a GPU: the stages of csrc/vgroups.hpp compiled for the host (tests/vgroups) on ONE group against the reference's
fixtures and the CPU oracle — the four properties include/blsw.h states (P1 any non-zero coefficients accept a valid group, P2 one bad instance
always rejects, P3 a group of one is BLS::verify, P4 predictable coefficients are not sound: the swap) and the two edge cases of the group sum
(doubling, identity) — and the argument rules of the two entry points, which precede any HIP call."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import hostsim_lib, vgroups_lib
from tests.oracle_lib import eth_cases, unhex
from tests.vgroups_lib import R_MOD

EDGE_SCALARS = [1, 2**64 - 1, 2**63, 3, 0xFFFFFFFF00000001]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def five(oracle):
    """five valid triples of distinct keys and messages, computed once and never changed"""
    msgs = [bytes([0x40 + i]) * 32 for i in range(5)]
    minted = [vgroups_lib.mint(oracle, 0x1234567 + 977 * i, m) for i, m in enumerate(msgs)]
    pks, sigs = [p for p, _ in minted], [s for _, s in minted]
    assert all(oracle.verify_bytes(p, m, s) for p, m, s in zip(pks, msgs, sigs))
    return tuple(pks), tuple(msgs), tuple(sigs)


def _flip(msg):
    return bytes([msg[0] ^ 1]) + msg[1:]


def test_p3_fixtures_as_groups_of_one(oracle):
    rows = [(name, unhex(c["input"]["pubkey"]), unhex(c["input"]["message"]), unhex(c["input"]["signature"]), c["output"]) for name, c in eth_cases("verify")]
    assert len(rows) == 29 and all(len(r[1]) == 48 and len(r[3]) == 96 for r in rows)
    n_true = 0
    for name, pk, msg, sig, out in rows:
        r, st = vgroups_lib.group([pk], [msg], [sig], [0x9E3779B97F4A7C15], 2)
        assert bool(r) == out == oracle.verify_bytes(pk, msg, sig), name
        _, st_pk, st_sig = hostsim_lib.verify_values(pk, sig, msg)
        assert st.tolist() == [[st_pk, st_sig]], name
        n_true += r
    assert n_true >= 9


@pytest.mark.parametrize("scalars", [EDGE_SCALARS, [1] * 5], ids=["edge", "ones"])
def test_p1_p2_chunks_of_two(five, scalars):
    """chunk = 2 over five instances: chunks (0, 1), (2, 3) and the short (4); the bad instance first, at a chunk's end, at a chunk's start, in the short chunk"""
    pks, msgs, sigs = five
    r, st = vgroups_lib.group(pks, msgs, sigs, scalars, 2)
    assert r == 1 and not st.any()
    for k in (0, 1, 2, 4):
        bad = list(msgs)
        bad[k] = _flip(bad[k])
        r, st = vgroups_lib.group(pks, bad, sigs, scalars, 2)
        assert r == 0 and not st.any(), k


def test_zero_scalar_fails_closed(five):
    pks, msgs, sigs = five
    scalars = list(EDGE_SCALARS)
    scalars[3] = 0
    r, st = vgroups_lib.group(pks, msgs, sigs, scalars, 2)
    assert r == 0 and not st.any()


def test_p4_swap_needs_unpredictable_scalars(oracle):
    """A = (pk, m1, sig2), B = (pk, m2, sig1): the exponent of the product is sk (r_A - r_B)(h1 - h2) — zero for equal coefficients"""
    sk, m1, m2 = 0x5EED5EED5EED, b"\x11" * 32, b"\x22" * 32
    pk, sig1 = vgroups_lib.mint(oracle, sk, m1)
    pk_b, sig2 = vgroups_lib.mint(oracle, sk, m2)
    assert pk == pk_b and not oracle.verify_bytes(pk, m1, sig2) and not oracle.verify_bytes(pk, m2, sig1)
    assert vgroups_lib.group([pk, pk], [m1, m2], [sig2, sig1], [5, 5], 2)[0] == 1  # the documented weakness of predictable coefficients
    assert vgroups_lib.group([pk, pk], [m1, m2], [sig2, sig1], [5, 7], 2)[0] == 0


def test_identity_sum_is_a_skipped_pair(oracle):
    """sk and r - sk on one message with equal coefficients: both valid, the signatures cancel, S_g is the identity and the group must pass"""
    sk, m = 0xC0FFEE, b"\x33" * 32
    pk_a, sig_a = vgroups_lib.mint(oracle, sk, m)
    pk_b, sig_b = vgroups_lib.mint(oracle, R_MOD - sk, m)
    assert oracle.verify_bytes(pk_a, m, sig_a) and oracle.verify_bytes(pk_b, m, sig_b) and sig_a != sig_b
    r, st = vgroups_lib.group([pk_a, pk_b], [m, m], [sig_a, sig_b], [7, 7], 2)
    assert r == 1 and not st.any()


def test_doubling_in_the_group_sum(oracle):
    pk, sig = vgroups_lib.mint(oracle, 0xABCDEF, b"\x44" * 32)
    r, st = vgroups_lib.group([pk, pk], [b"\x44" * 32] * 2, [sig, sig], [9, 9], 2)
    assert r == 1 and not st.any()


def test_argument_rules_without_a_gpu(pkg):
    L = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17
    assert pkg.VERIFY_GROUPS_CHUNK == H["defines"]["BLSW_VGROUP_CHUNK"]
    ERR_ARG = 1
    p = ctypes.c_void_p(0x1000)  # never dereferenced: the calls fail before any device work
    good = dict(pk=p, sig=p, msg=p, msg_len=32, n=64, scalars=p, group=8, res=p, st=p, ws=p)

    def call(**kw):
        a = dict(good, **kw)
        return L.blsw_verify_groups_batch(a["pk"], a["sig"], a["msg"], a["msg_len"], a["n"], a["scalars"], a["group"], a["res"], a["st"], a["ws"], 1 << 40, None)

    for kw in (dict(group=0), dict(group=65536), dict(n=0), dict(n=0x80000000), dict(msg_len=65536), dict(pk=None), dict(sig=None), dict(scalars=None), dict(res=None),
               dict(st=None), dict(ws=None), dict(msg=None)):
        assert call(**kw) == ERR_ARG, kw
    b = ctypes.c_uint64(0)
    for n, msg_len, group in ((0, 32, 8), (0x80000000, 32, 8), (64, 65536, 8), (64, 32, 0), (64, 32, 65536)):
        assert L.blsw_verify_groups_workspace_bytes(n, msg_len, group, ctypes.byref(b)) == ERR_ARG
    assert L.blsw_verify_groups_workspace_bytes(64, 32, 8, None) == ERR_ARG
    last = 0
    for n in (1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 65536):
        assert L.blsw_verify_groups_workspace_bytes(n, 32, 64, ctypes.byref(b)) == 0 and b.value >= last
        last = b.value
        if n >= 1024:  # one set of per-instance lines instead of two
            v = ctypes.c_uint64(0)
            assert L.blsw_verify_workspace_bytes(n, 32, ctypes.byref(v)) == 0 and b.value < v.value
    assert L.blsw_verify_groups_workspace_bytes(5, 0, 65535, ctypes.byref(b)) == 0  # a group beyond n is one group
