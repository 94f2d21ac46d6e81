"""The caller-chosen domain separation tag on the device (k_sha_values_dst and every *_dst entry of include/blsw.h), PopProve and PopVerify, against
the independent statement tests/dst_ref.py (hashlib's expand_message_xmd, the SSWU map, isogeny, group law and H_EFF of tests/curve_ref.py).
Every batch has n = 65 lanes: one full wave and one lane of the next, so the kernel's tail guard runs."""
import importlib
import os
import random
import subprocess

import numpy as np
import pytest

from tests import curve_ref as C
from tests import dst_ref as R
from tests.curve_ref import K1, K2, R_ORDER

pytestmark = pytest.mark.gpu
N = 65
ST_OK, ST_BAD_ENCODING, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_INVALID_SECRET_KEY = 0, 1, 3, 4, 5
TAG = b"QUUX-V01-CS02-with-BLS12381G2_XMD:SHA-256_SSWU_RO_"  # RFC 9380 J.10.1's suite tag: an application tag of 50 bytes
TAG_LAST = TAG[:-1] + bytes([TAG[-1] ^ 1])
IDENTITY48, IDENTITY96 = bytes([0xC0]) + bytes(47), bytes([0xC0]) + bytes(95)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg():
    assert R.pin()
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def tag_of(L, salt=0):
    special = [0x00, 0x80, 0xFF]
    return bytes(special[(k + salt) % 3] if k % 2 == 0 else (0x21 + 7 * k + salt) & 0xFF for k in range(L))


def messages(n, msg_len, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(msg_len)) for _ in range(n)]


def dev(torch, rows, width):
    """a list of byte strings of one length -> uint8 cuda tensor [n, width]"""
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy() if width else np.zeros((len(rows), 0), dtype=np.uint8)
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def secret_keys(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R_ORDER) for _ in range(n)]


def sk_tensor(torch, sks):
    return dev(torch, [int(s).to_bytes(32, "little") for s in sks], 32)


FIELD_CASES = [(L, (-(77 + L)) % 64 + d) for L in (1, 21, 22, 43, 85, 86, 149, 150, 213, 214, 255) for d in (0, 1)] + [(43, 0), (43, 32), (43, 48)]


@pytest.mark.parametrize("L,msg_len", FIELD_CASES)
def test_hash_to_field_batch(pkg, torch, L, msg_len):
    """blsw_hash_to_field_batch against dst_ref.hash_to_field on all 65 lanes: per tag length the two message lengths that put the end of b_0's
    padded input on a block boundary (77 + msg_len + L = 64 k) and one byte behind it (one block more); msg_len 0, 32, 48 at the 43-byte POP tag"""
    dst = R.DST_POP if L == 43 else tag_of(L, L)
    assert len(dst) == L and (msg_len in (0, 32, 48) or (77 + msg_len + L) % 64 in (0, 1))
    msgs = messages(N, msg_len, 1000 * L + msg_len)
    got = host(pkg.hash_to_field_batch(dev(torch, msgs, msg_len), dst=dst)).view(np.uint64)
    want = np.array([[R.mont_words(v) for v in R.hash_to_field(m, dst)] for m in msgs], dtype=np.uint64)
    assert got.shape == want.shape == (N, 4, 6)
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, (L, msg_len, bad[:8])


def test_hash_to_field_default_tag(pkg, torch):
    """dst=None is the library's tag"""
    m = dev(torch, messages(N, 32, 7), 32)
    assert torch.equal(pkg.hash_to_field_batch(m), pkg.hash_to_field_batch(m, dst=pkg.DST_DEFAULT))


@pytest.mark.parametrize("L", [1, 43, 255])
def test_hash_to_g2_batch(pkg, torch, L):
    """hash_to_g2_batch(dst=...) against dst_ref.hash_to_g2 on eight of the 65 messages (the first seven lanes and the lane behind the full wave)"""
    dst = R.DST_POP if L == 43 else tag_of(L, 3)
    msgs = messages(N, 37, 50 + L)
    got = host(pkg.hash_to_g2_batch(dev(torch, msgs, 37), dst=dst)).view(np.uint64)
    for i in list(range(7)) + [64]:
        assert [int(x) for x in got[i]] == R.g2_limbs(R.hash_to_g2(msgs[i], dst)), (L, i)


def test_hash_to_g2_default_tag_through_the_new_kernel(pkg, torch):
    """dst=DST_DEFAULT (the tag-taking kernel) equals dst=None (the fixed-tag kernel) bit for bit on the whole batch, at lengths on both sides of a
    block boundary of b_0"""
    for msg_len in (0, 7, 8, 32, 131):
        m = dev(torch, messages(N, msg_len, msg_len), msg_len)
        a, b = pkg.hash_to_g2_batch(m), pkg.hash_to_g2_batch(m, dst=pkg.DST_DEFAULT)
        assert torch.equal(a, b) and torch.equal(a, pkg.hash_to_g2_batch(m, dst=None)), msg_len


@pytest.fixture(scope="module")
def signed(pkg, torch):
    """65 (key, message) pairs signed under TAG and under the library's tag"""
    sks = secret_keys(N, 0xD57)
    msgs = messages(N, 32, 0xD58)
    sk, m = sk_tensor(torch, sks), dev(torch, msgs, 32)
    t, d = pkg.sign_batch(sk, m, dst=TAG), pkg.sign_batch(sk, m)
    assert not host(t["status"]).any() and not host(d["status"]).any() and torch.equal(t["pk48"], d["pk48"])
    return dict(sks=sks, msgs=msgs, sk=sk, msg=m, pk48=t["pk48"], sig_tag=t["sig96"], sig_default=d["sig96"])


def test_sign_and_verify_under_a_tag(pkg, torch, signed):
    """sign_batch(dst=t) is sk * H_t(m) of the reference on four instances; verify_batch(dst=t) accepts all 65, and rejects them under the library's
    tag and under a tag that differs in its last byte; signatures made under the library's tag are rejected under t"""
    sig = host(signed["sig_tag"])
    for i in (0, 1, 2, 64):
        assert sig[i].tobytes() == R.sign(signed["sks"][i], signed["msgs"][i], TAG), i
    pk, m = signed["pk48"], signed["msg"]
    ok, st = pkg.verify_batch(pk, m, signed["sig_tag"], want_status=True, dst=TAG)
    assert host(ok).tolist() == [1] * N and not host(st).any()
    assert host(pkg.verify_batch(pk, m, signed["sig_tag"])).tolist() == [0] * N
    assert host(pkg.verify_batch(pk, m, signed["sig_tag"], dst=None)).tolist() == [0] * N
    assert host(pkg.verify_batch(pk, m, signed["sig_tag"], dst=TAG_LAST)).tolist() == [0] * N
    assert host(pkg.verify_batch(pk, m, signed["sig_default"], dst=TAG)).tolist() == [0] * N
    assert host(pkg.verify_batch(pk, m, signed["sig_default"])).tolist() == [1] * N
    assert host(pkg.verify_batch(pk, m, signed["sig_default"], dst=pkg.DST_DEFAULT)).tolist() == [1] * N


def test_verify_groups_under_a_tag(pkg, torch, signed):
    """group 2: 33 groups, the last of one instance"""
    pk, m = signed["pk48"], signed["msg"]
    scalars = torch.arange(3, 3 + N, dtype=torch.int64, device="cuda")
    G = (N + 1) // 2
    assert host(pkg.verify_groups(pk, m, signed["sig_tag"], group=2, scalars=scalars, dst=TAG)).tolist() == [1] * G
    assert host(pkg.verify_groups(pk, m, signed["sig_tag"], group=2, scalars=scalars)).tolist() == [0] * G
    assert host(pkg.verify_groups(pk, m, signed["sig_default"], group=2, scalars=scalars, dst=TAG)).tolist() == [0] * G
    plain = pkg.verify_groups(pk, m, signed["sig_default"], group=2, scalars=scalars)
    assert host(plain).tolist() == [1] * G and torch.equal(plain, pkg.verify_groups(pk, m, signed["sig_default"], group=2, scalars=scalars, dst=None))
    assert host(pkg.verify_batch_grouped(pk, m, signed["sig_tag"], group=2, scalars=scalars, dst=TAG)).tolist() == [1] * N
    assert host(pkg.verify_batch_grouped(pk, m, signed["sig_tag"], group=2, scalars=scalars)).tolist() == [0] * N


def test_verify_pairs_under_a_tag(pkg, torch):
    """K = 2: one aggregate signature over two (key, message) pairs per instance"""
    sks = secret_keys(2 * N, 0xA66)
    msgs = messages(2 * N, 20, 0xA67)
    sk, m = sk_tensor(torch, sks), dev(torch, msgs, 20)
    sigs = {}
    for name, dst in (("tag", TAG), ("default", None)):
        s = pkg.sign_batch(sk, m, dst=dst)
        agg, st = pkg.aggregate_signatures(s["sig96"].reshape(N, 2, 96).contiguous())
        assert not host(st).any()
        sigs[name] = agg
        pks = s["pk48"].reshape(N, 2, 48).contiguous()
    m2 = m.reshape(N, 2, 20).contiguous()
    assert host(pkg.verify_pairs(pks, m2, sigs["tag"], dst=TAG)).tolist() == [1] * N
    assert host(pkg.verify_pairs(pks, m2, sigs["tag"])).tolist() == [0] * N
    assert host(pkg.verify_pairs(pks, m2, sigs["default"], dst=TAG)).tolist() == [0] * N
    plain = pkg.verify_pairs(pks, m2, sigs["default"])
    assert host(plain).tolist() == [1] * N and torch.equal(plain, pkg.verify_pairs(pks, m2, sigs["default"], dst=None))


@pytest.fixture(scope="module")
def committee(pkg, torch):
    """three keys, 65 instances each selecting a non-empty subset, one message and the aggregate signature of the selected keys per instance, under
    TAG and under the library's tag (an unselected key's share is the infinity encoding: a valid summand of Signature::aggregate)"""
    sks = secret_keys(3, 0xC03)
    msgs = messages(N, 32, 0xC04)
    subsets = [[(s >> k) & 1 for k in range(3)] for s in (1 + i % 7 for i in range(N))]
    sk = sk_tensor(torch, sks * N)
    m3 = dev(torch, [msgs[i] for i in range(N) for _ in range(3)], 32)
    sel = torch.from_numpy(np.array(subsets, dtype=bool)).cuda()
    out = dict(bitmap=torch.from_numpy(np.array(subsets, dtype=np.uint8)).cuda(), msg=dev(torch, msgs, 32), lists=[[k for k in range(3) if b[k]] for b in subsets])
    inf = dev(torch, [IDENTITY96], 96)[0]
    for name, dst in (("tag", TAG), ("default", None)):
        s = pkg.sign_batch(sk, m3, dst=dst)
        shares = s["sig96"].reshape(N, 3, 96).clone()
        shares[~sel] = inf
        out[name], st = pkg.aggregate_signatures(shares.contiguous())
        assert not host(st).any()
        out["pks48"] = s["pk48"][:3].contiguous()
    return out


def test_committee_verify_under_a_tag(pkg, torch, committee):
    c = committee
    assert host(pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["tag"], dst=TAG)).tolist() == [1] * N
    assert host(pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["tag"])).tolist() == [0] * N
    assert host(pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["default"], dst=TAG)).tolist() == [0] * N
    plain = pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["default"])
    assert host(plain).tolist() == [1] * N and torch.equal(plain, pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["default"], dst=None))
    scalars = torch.arange(5, 5 + N, dtype=torch.int64, device="cuda")
    assert host(pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["tag"], group=4, scalars=scalars, dst=TAG)).tolist() == [1] * ((N + 3) // 4)
    assert host(pkg.committee_verify(c["pks48"], c["bitmap"], c["msg"], c["tag"], group=4, scalars=scalars)).tolist() == [0] * ((N + 3) // 4)
    assert host(pkg.committee_verify_grouped(c["pks48"], c["bitmap"], c["msg"], c["tag"], group=4, scalars=scalars, dst=TAG)).tolist() == [1] * N


def test_registry_verify_under_a_tag(pkg, torch, committee):
    """the committee's three keys in a registry, the selections as index lists"""
    c = committee
    reg = pkg.KeyRegistry(3)
    reg.append(c["pks48"])
    flat = [k for l in c["lists"] for k in l]
    off = np.zeros(N + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(l) for l in c["lists"]])
    idx, off = torch.from_numpy(np.array(flat, dtype=np.int32)).cuda(), torch.from_numpy(off).cuda()
    assert host(pkg.registry_verify(reg, idx, off, c["msg"], c["tag"], dst=TAG)).tolist() == [1] * N
    assert host(pkg.registry_verify(reg, idx, off, c["msg"], c["tag"])).tolist() == [0] * N
    assert host(pkg.registry_verify(reg, idx, off, c["msg"], c["default"], dst=TAG)).tolist() == [0] * N
    plain = pkg.registry_verify(reg, idx, off, c["msg"], c["default"])
    assert host(plain).tolist() == [1] * N and torch.equal(plain, pkg.registry_verify(reg, idx, off, c["msg"], c["default"], dst=None))
    scalars = torch.arange(9, 9 + N, dtype=torch.int64, device="cuda")
    assert host(pkg.registry_verify(reg, idx, off, c["msg"], c["tag"], group=4, scalars=scalars, dst=TAG)).tolist() == [1] * ((N + 3) // 4)
    assert host(pkg.registry_verify_grouped(reg, idx, off, c["msg"], c["tag"], group=4, scalars=scalars, dst=TAG)).tolist() == [1] * N
    reg.close()


@pytest.fixture(scope="module")
def proved(pkg, torch):
    """65 keys, of which key 1 is 0 and key 2 is r: the two secret keys blsw_sign_batch refuses"""
    sks = secret_keys(N, 0x909)
    sks[1], sks[2] = 0, R_ORDER
    sk = sk_tensor(torch, sks)
    p = pkg.pop_prove(sk)
    return dict(sks=sks, sk=sk, **p)


def test_pop_prove(pkg, torch, proved):
    """the keys are sign_batch's, the proofs sk * H_pop(pk48) of the reference, the statuses sign_batch's"""
    p = proved
    s = pkg.sign_batch(p["sk"], dev(torch, messages(N, 8, 1), 8))
    assert torch.equal(p["pk48"], s["pk48"]) and torch.equal(p["status"], s["status"])
    want = [ST_OK] * N
    want[1], want[2] = ST_INVALID_SECRET_KEY, ST_BAD_ENCODING
    assert host(p["status"]).tolist() == want
    pk, proof = host(p["pk48"]), host(p["proof96"])
    for i in (0, 3, 64):
        assert pk[i].tobytes() == R.public_key(p["sks"][i])
        assert proof[i].tobytes() == R.sign(p["sks"][i], pk[i].tobytes(), R.DST_POP), i
    for i in (1, 2):
        assert pk[i].tobytes() == IDENTITY48 and proof[i].tobytes() == IDENTITY96


def test_pop_verify(pkg, torch, proved):
    p = proved
    ok, st = pkg.pop_verify(p["pk48"], p["proof96"], want_status=True)
    want = [1] * N
    want[1] = want[2] = 0  # the identity key and the identity proof of a refused secret key
    assert host(ok).tolist() == want
    want_st = [[ST_OK, ST_OK]] * N
    want_st[1] = want_st[2] = [ST_IDENTITY, ST_IDENTITY]
    assert host(st).tolist() == want_st
    # PopVerify IS Verify over the key bytes under the POP tag
    assert torch.equal(ok, pkg.verify_batch(p["pk48"], p["pk48"], p["proof96"], dst=pkg.DST_POP))
    # domain separation: a signature over the key bytes under the library's tag is no proof
    s = pkg.sign_batch(p["sk"], p["pk48"])
    assert host(pkg.verify_batch(p["pk48"], p["pk48"], s["sig96"])).tolist() == want
    ok2, st2 = pkg.pop_verify(p["pk48"], s["sig96"], want_status=True)
    assert host(ok2).tolist() == [0] * N and host(st2).tolist() == want_st
    # another key's proof
    assert host(pkg.pop_verify(p["pk48"], torch.roll(p["proof96"], 1, 0).contiguous())).tolist() == [0] * N


def test_pop_verify_refuses_bad_keys_and_proofs(pkg, torch, proved):
    """an identity key, an identity proof, keys of order 3 and 11 (on the curve, off the subgroup) and a key plus a point of order 3, each in a full
    batch next to good pairs"""
    from tests import chain_edges as E

    p = proved
    g1 = {name: pt for name, pt, _ in E.g1_operands()}
    off = [C.g1_compress((0, 2)), C.g1_compress(g1["order 11"]), C.g1_compress(g1["subgroup + order 3"])]
    assert all(C.decode("g1", b)[0] == C.DEC_NOT_IN_SUBGROUP for b in off)
    pk, proof = host(p["pk48"]).copy(), host(p["proof96"]).copy()
    pk[5] = np.frombuffer(IDENTITY48, dtype=np.uint8)
    proof[6] = np.frombuffer(IDENTITY96, dtype=np.uint8)
    for k, b in enumerate(off):
        pk[7 + k] = np.frombuffer(b, dtype=np.uint8)
    ok, st = pkg.pop_verify(torch.from_numpy(pk).cuda(), torch.from_numpy(proof).cuda(), want_status=True)
    ok, st = host(ok).tolist(), host(st).tolist()
    want = [1] * N
    for i in (1, 2, 5, 6, 7, 8, 9):
        want[i] = 0
    assert ok == want
    assert st[5] == [ST_IDENTITY, ST_OK] and st[6] == [ST_OK, ST_IDENTITY] and st[7] == st[8] == st[9] == [ST_NOT_IN_SUBGROUP, ST_OK] and st[0] == st[64] == [ST_OK, ST_OK]


def test_cpp_caller(pkg, torch):
    """BLS::pop_prove -> BLS::pop_verify and a tagged BLS::sign -> BLS::verify through include/blsw.hpp"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "dst"), "cpp_caller"])
    sks = secret_keys(3, 0xCAFE)
    r = subprocess.run([os.path.join(HERE, "dst", "cpp_caller")] + ["%064x" % s for s in sks], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    p = pkg.pop_prove(sk_tensor(torch, sks))
    for i in range(3):
        assert lines[i].split() == [host(p["pk48"])[i].tobytes().hex(), host(p["proof96"])[i].tobytes().hex(), "0", "1"]
    assert lines[3] == "swapped 0 0 0" and lines[4] == "tagged 1 0 1"
