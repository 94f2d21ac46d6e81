"""blsw_verify_pairs_batch (AggregateVerify as values) on the MI355X. The instances are built from secret keys (sign_batch + aggregate_signatures), so
every tamper has a known verdict; the yardsticks are verify_batch (Q1), fast_aggregate_verify_batch (Q3), the N+1-pair circuit (Q4), the reference's
fixtures and the rules of include/blsw.h. Shapes are the smallest that cross every boundary: n = 11 instances of up to K = 2 c + 1 pairs (c =
VERIFY_PAIRS_CHUNK: 187 pair lanes in three waves, 33 teams in a ragged fourth wave), n = 70 at K = 1 (the ragged second wave). No test times anything."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.oracle_lib import eth_cases, unhex

pytestmark = pytest.mark.gpu
ST_OK, ST_BAD_ENCODING, ST_NOT_IN_SUBGROUP, ST_IDENTITY, ST_BAD_INDEX = 0, 1, 3, 4, 6
IDENTITY48, IDENTITY96 = bytes([0xC0]) + bytes(47), bytes([0xC0]) + bytes(95)
N = 11
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def c(pkg):
    return pkg.VERIFY_PAIRS_CHUNK


def _t(dev, xs, w):
    import torch

    return torch.from_numpy(np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(len(xs), w).copy()).to(dev)


@pytest.fixture(scope="module")
def pool(pkg, dev, c):
    """N instances of 2 c + 1 pairs of distinct keys and messages, signed once by sign_batch and never changed: dict of cuda tensors pks [N, K, 48],
    msgs [N, K, 32], sigs [N, K, 96] (the single signatures) and pk_xy [N, K, 12]"""
    import torch

    K = 2 * c + 1
    m = N * K
    sk = np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(m)), dtype=np.uint8).reshape(m, 32).copy()
    msg = np.random.default_rng(0xA66).integers(0, 256, size=(m, 32), dtype=np.uint8)
    msg_t = torch.from_numpy(msg).to(dev)
    r = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg_t)
    assert int(r["status"].abs().sum().item()) == 0
    return {"K": K, "pks": r["pk48"].reshape(N, K, 48), "msgs": msg_t.reshape(N, K, 32), "sigs": r["sig96"].reshape(N, K, 96), "pk_xy": r["pk_xy"].reshape(N, K, 12)}


def _aggregate(pkg, dev, sigs, counts):
    """the aggregate of each instance's first counts[i] single signatures (the identity where the count is 0): [n, 96]"""
    import torch

    s = sigs.clone()
    ident = torch.from_numpy(np.frombuffer(IDENTITY96, np.uint8).copy()).to(dev)
    for i, cnt in enumerate(counts):
        s[i, cnt:] = ident  # a well-formed identity is a valid summand
    agg, st = pkg.aggregate_signatures(s.contiguous())
    assert not st.cpu().numpy().any()
    return agg


def _take(pool, K):
    return pool["pks"][:, :K].contiguous(), pool["msgs"][:, :K].contiguous()


@pytest.mark.parametrize("k_of", ["1", "2", "c-1", "c", "c+1", "2c+1"])
def test_all_valid(pkg, dev, pool, c, k_of):
    K = {"1": 1, "2": 2, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+1": 2 * c + 1}[k_of]
    pks, msgs = _take(pool, K)
    res, st, kst = pkg.verify_pairs(pks, msgs, _aggregate(pkg, dev, pool["sigs"][:, :K], [K] * N), want_status=True, want_key_status=True)
    assert res.tolist() == [1] * N and not st.cpu().numpy().any() and not kst.cpu().numpy().any() and kst.shape == (N, K)


def test_q1_one_pair_is_verify_batch(pkg, dev, pool):
    """n = 70 at K = 1 against verify_batch: verdicts and statuses, with tampered messages, swapped signatures, an identity key and an undecodable key"""
    import torch

    n = 70
    pk = pool["pks"].reshape(-1, 48)[:n].clone()
    msg = pool["msgs"].reshape(-1, 32)[:n].clone()
    sig = pool["sigs"].reshape(-1, 96)[:n].clone()
    msg[5, 0] ^= 1
    msg[64, 31] ^= 0x80
    sig[[9, 10]] = sig[[10, 9]]
    pk[20] = torch.from_numpy(np.frombuffer(IDENTITY48, np.uint8).copy()).to(dev)
    pk[69] = 0xFF
    sig[33] = torch.from_numpy(np.frombuffer(IDENTITY96, np.uint8).copy()).to(dev)
    ref, ref_st = pkg.verify_batch(pk, msg, sig, want_status=True)
    res, st = pkg.verify_pairs(pk.reshape(n, 1, 48), msg.reshape(n, 1, 32), sig, want_status=True)
    assert torch.equal(res, ref) and torch.equal(st, ref_st)
    assert sorted(np.flatnonzero(res.cpu().numpy() == 0).tolist()) == [5, 9, 10, 20, 33, 64, 69]
    assert st[20].tolist() == [ST_IDENTITY, ST_OK] and st[69].tolist() == [ST_BAD_ENCODING, ST_OK] and st[33].tolist() == [ST_OK, ST_IDENTITY]


def test_q1_verify_fixtures_in_one_call(pkg, dev):
    import torch

    rows = [(unhex(x["input"]["pubkey"]), unhex(x["input"]["message"]), unhex(x["input"]["signature"]), x["output"]) for _, x in eth_cases("verify")]
    assert len(rows) == 29
    pk, msg, sig = _t(dev, [r[0] for r in rows], 48), _t(dev, [r[1] for r in rows], 32), _t(dev, [r[2] for r in rows], 96)
    ref, ref_st = pkg.verify_batch(pk, msg, sig, want_status=True)
    res, st = pkg.verify_pairs(pk.reshape(29, 1, 48), msg.reshape(29, 1, 32), sig, want_status=True)
    assert torch.equal(res, ref) and torch.equal(st, ref_st) and res.tolist() == [int(r[3]) for r in rows]


def test_one_tamper_fails_one_instance(pkg, dev, pool, c):
    """K = 2 c + 1: a tampered message in the first pair of instance 0, in the last pair of the first chunk of a middle instance and in the last pair
    of the last instance; then with the signatures of two other instances swapped"""
    K = pool["K"]
    pks, msgs = _take(pool, K)
    sig = _aggregate(pkg, dev, pool["sigs"], [K] * N)
    msgs = msgs.clone()
    for i, j in ((0, 0), (5, c - 1), (N - 1, K - 1)):
        msgs[i, j, 7] ^= 4
    res, st = pkg.verify_pairs(pks, msgs, sig, want_status=True)
    assert np.flatnonzero(res.cpu().numpy() == 0).tolist() == [0, 5, N - 1] and not st.cpu().numpy().any()
    sig = sig.clone()
    sig[[2, 7]] = sig[[7, 2]]
    res, st = pkg.verify_pairs(pks, msgs, sig, want_status=True)
    assert np.flatnonzero(res.cpu().numpy() == 0).tolist() == [0, 2, 5, 7, N - 1] and not st.cpu().numpy().any()


def test_counts(pkg, dev, pool, c):
    import torch

    K = pool["K"]
    counts = [0, 1, c, c + 1, K, K + 1, c - 1, 2, 2 * c, K, 0xFFFFFFFF]
    used = [cnt if cnt <= K else 0 for cnt in counts]
    want_st = [ST_IDENTITY if cnt == 0 else (ST_BAD_INDEX if cnt > K else ST_OK) for cnt in counts]
    pks, msgs = _take(pool, K)
    cn = torch.from_numpy(np.array(counts, dtype=np.uint32).view(np.int32)).to(dev)
    sig = _aggregate(pkg, dev, pool["sigs"], [u if u else K for u in used])  # a count that is refused meets a signature over all K pairs
    res, st = pkg.verify_pairs(pks, msgs, sig, counts=cn, want_status=True)
    assert st[:, 0].tolist() == want_st and not st[:, 1].cpu().numpy().any()
    assert res.tolist() == [int(s == ST_OK) for s in want_st]
    # a signature over all K pairs passes only where all K are used
    full = _aggregate(pkg, dev, pool["sigs"], [K] * N)
    res_full, st_full = pkg.verify_pairs(pks, msgs, full, counts=cn, want_status=True)
    assert res_full.tolist() == [int(cnt == K) for cnt in counts] and torch.equal(st_full, st)
    # Q2: garbage behind the count changes neither verdict nor status
    pks_g, msgs_g = pks.clone(), msgs.clone()
    for i, u in enumerate(used):
        if counts[i] <= K:
            pks_g[i, u:] = 0xFF
            msgs_g[i, u:] = 0xEE
    res_g, st_g, kst = pkg.verify_pairs(pks_g, msgs_g, sig, counts=cn, want_status=True, want_key_status=True)
    assert torch.equal(res_g, res) and torch.equal(st_g, st)
    kst = kst.cpu().numpy()
    for i, u in enumerate(used):
        if counts[i] <= K:
            assert not kst[i, :u].any() and (kst[i, u:] == ST_BAD_ENCODING).all(), i
    # and so does a permutation of the used pairs
    perm = torch.from_numpy(np.random.default_rng(3).permutation(c + 1)).to(dev)
    pks_p, msgs_p = pks.clone(), msgs.clone()
    pks_p[3, :c + 1], msgs_p[3, :c + 1] = pks[3, perm], msgs[3, perm]
    assert torch.equal(pkg.verify_pairs(pks_p, msgs_p, sig, counts=cn), res)


def test_statuses_on_the_device(pkg, dev, pool, c):
    import torch

    K = pool["K"]
    not_in_g1 = [unhex(x["input"]["pubkey"]) for name, x in eth_cases("deserialization_G1") if "not_in_G1" in name]
    assert len(not_in_g1) == 1 and len(not_in_g1[0]) == 48
    pks, msgs = _take(pool, K)
    pks = pks.clone()
    put = {(1, 0): (IDENTITY48, ST_IDENTITY), (4, c): (not_in_g1[0], ST_NOT_IN_SUBGROUP), (8, K - 1): (bytes(48), ST_BAD_ENCODING), (8, 3): (IDENTITY48, ST_IDENTITY)}
    for (i, j), (b, _) in put.items():
        pks[i, j] = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev)
    res, st, kst = pkg.verify_pairs(pks, msgs, _aggregate(pkg, dev, pool["sigs"], [K] * N), want_status=True, want_key_status=True)
    want_k = np.zeros((N, K), np.int32)
    for (i, j), (_, s) in put.items():
        want_k[i, j] = s
    want = np.zeros((N, 2), np.int32)
    want[1, 0], want[4, 0], want[8, 0] = ST_IDENTITY, ST_NOT_IN_SUBGROUP, ST_IDENTITY  # the earliest bad pair of instance 8 is the identity at 3
    assert np.array_equal(kst.cpu().numpy(), want_k) and np.array_equal(st.cpu().numpy(), want)
    assert res.tolist() == [int(i not in (1, 4, 8)) for i in range(N)]


def test_q3_fast_aggregate_verify_fixtures(pkg, dev):
    """the 11 fixtures, the message repeated for every key, padded to the longest list: one call with counts against one fast_aggregate_verify_batch per list"""
    import torch

    cases = eth_cases("fast_aggregate_verify")
    assert len(cases) == 11
    ins = [([unhex(p) for p in x["input"]["pubkeys"]], unhex(x["input"]["message"]), unhex(x["input"]["signature"]), x["output"]) for _, x in cases]
    K = max(len(p) for p, _, _, _ in ins)
    pks, msgs = np.zeros((11, K, 48), np.uint8), np.zeros((11, K, 32), np.uint8)
    ref = []
    for i, (p, m, s, out) in enumerate(ins):
        for j, b in enumerate(p):
            pks[i, j], msgs[i, j] = np.frombuffer(b, np.uint8), np.frombuffer(m, np.uint8)
        ref.append(int(pkg.fast_aggregate_verify_batch(_t(dev, p, 48).reshape(1, len(p), 48), _t(dev, [m], 32), _t(dev, [s], 96))[0].item()) if p else 0)
    counts = torch.tensor([len(p) for p, _, _, _ in ins], dtype=torch.int32, device=dev)
    res, st = pkg.verify_pairs(torch.from_numpy(pks).to(dev), torch.from_numpy(msgs).to(dev), _t(dev, [s for _, _, s, _ in ins], 96), counts=counts, want_status=True)
    assert res.tolist() == ref == [int(out) for _, _, _, out in ins] and sum(ref) == 3
    for i, (p, _, _, _) in enumerate(ins):
        if not p:
            assert st[i, 0].item() == ST_IDENTITY


def test_q4_against_the_circuit(pkg, dev, pool):
    """n = 3, K = 2: the Boolean of the N+1-pair circuit on the decoded points; instance 1 carries a tampered message"""
    import torch

    pks, msgs = pool["pks"][:3, :2].contiguous(), pool["msgs"][:3, :2].contiguous().clone()
    msgs[1, 1, 0] ^= 1
    sig = _aggregate(pkg, dev, pool["sigs"][:3, :2], [2] * 3)
    _, sig_xy, dst = pkg.decode_batch(pks[:, 0].contiguous(), sig)
    assert not dst.cpu().numpy().any()
    circ, _ = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pool["pk_xy"][:3, :2].contiguous()), msgs, pkg.SignatureVar.new_witness(sig_xy), want_witness=False)
    res = pkg.verify_pairs(pks, msgs, sig)
    assert torch.equal(res, circ) and res.tolist() == [1, 0, 1]


def test_workspace_one_byte_short(pkg, dev, pool, c):
    import torch

    K = c + 1
    pks, msgs = _take(pool, K)
    sig = _aggregate(pkg, dev, pool["sigs"][:, :K], [K] * N)
    wb = ctypes.c_uint64(0)
    assert pkg.lib().blsw_verify_pairs_workspace_bytes(N, 32, K, ctypes.byref(wb)) == 0
    ws = torch.full((wb.value,), 0xA5, dtype=torch.uint8, device=dev)
    res = torch.full((N,), -7, dtype=torch.int32, device=dev)
    st = torch.full((N, 2), -7, dtype=torch.int32, device=dev)
    call = lambda size: pkg.lib().blsw_verify_pairs_batch(pks.data_ptr(), msgs.data_ptr(), 32, K, None, sig.data_ptr(), N, res.data_ptr(), st.data_ptr(), None, ws.data_ptr(), size,
                                                          torch.cuda.current_stream(dev).cuda_stream)
    assert call(wb.value - 1) == 2  # BLSW_ERR_WORKSPACE, nothing written
    torch.cuda.synchronize(dev)
    assert bool((ws == 0xA5).all().item()) and bool((res == -7).all().item()) and bool((st == -7).all().item())
    assert call(wb.value) == 0
    torch.cuda.synchronize(dev)
    assert res.tolist() == [1] * N and not st.cpu().numpy().any()


def _ragged(pkg, dev, pool, c):
    """a ragged case: counts, tensors padded to the longest, signatures over the used pairs, one instance tampered -> (pks, msgs, sig, counts list, expect)"""
    K = c + 2
    counts = [K, 1, 0, c, 3, c + 1]
    n = len(counts)
    pks, msgs = pool["pks"][:n, :K].contiguous(), pool["msgs"][:n, :K].contiguous().clone()
    msgs[4, 2, 5] ^= 2
    sig = _aggregate(pkg, dev, pool["sigs"][:n, :K], [u if u else 1 for u in counts])
    return pks, msgs, sig, counts, [1, 1, 0, 1, 0, 1]


def test_two_streams_with_their_own_workspaces(pkg, dev, pool, c, tmp_path):
    """two calls in flight on two non-default streams, in a child process (tests/verify_pairs_stream_worker.py says why): the verdicts of the serial calls"""
    import torch

    K = pool["K"]
    pks_a, msgs_a = _take(pool, K)
    msgs_a = msgs_a.clone()
    msgs_a[6, c, 0] ^= 1
    sig_a = _aggregate(pkg, dev, pool["sigs"], [K] * N)
    pks_b, msgs_b, sig_b, counts, expect_b = _ragged(pkg, dev, pool, c)
    counts_b = torch.tensor(counts, dtype=torch.int32, device=dev)
    a, a_st = pkg.verify_pairs(pks_a, msgs_a, sig_a, want_status=True)
    b, b_st = pkg.verify_pairs(pks_b, msgs_b, sig_b, counts=counts_b, want_status=True)
    assert a.tolist() == [int(i != 6) for i in range(N)] and b.tolist() == expect_b
    f = tmp_path / "batch.npz"
    np.savez(f, pks_a=pks_a.cpu().numpy(), msgs_a=msgs_a.cpu().numpy(), sig_a=sig_a.cpu().numpy(), pks_b=pks_b.cpu().numpy(), msgs_b=msgs_b.cpu().numpy(), sig_b=sig_b.cpu().numpy(),
             counts_b=counts_b.cpu().numpy())
    out = subprocess.check_output([sys.executable, "-m", "tests.verify_pairs_stream_worker", str(f)], cwd=os.path.dirname(HERE), text=True, timeout=120)
    got = json.loads(out.strip().split("\n")[-1])
    assert (got["a"], got["a_status"], got["b"], got["b_status"]) == (a.tolist(), a_st.tolist(), b.tolist(), b_st.tolist())


def test_cpp_host_mirror(pkg, dev, pool, c, tmp_path):
    """BLS::aggregate_verify (include/blsw.hpp) from a C++ host (tests/vpairs/cpp_caller) on a ragged case equals the Python call"""
    import torch

    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "vpairs"), "cpp_caller"])
    pks, msgs, sig, counts, expect = _ragged(pkg, dev, pool, c)
    pks = pks.clone()
    pks[5, 1] = torch.from_numpy(np.frombuffer(IDENTITY48, np.uint8).copy()).to(dev)  # an identity key among the used pairs of the last instance
    res, st, kst = pkg.verify_pairs(pks, msgs, sig, counts=torch.tensor(counts, dtype=torch.int32, device=dev), want_status=True, want_key_status=True)
    assert res.tolist() == expect[:5] + [0] and st[5].tolist() == [ST_IDENTITY, ST_OK]
    hexs = lambda t: [bytes(r).hex() for r in t.cpu().numpy()]
    lines = []
    for i, cnt in enumerate(counts):
        lines.append("%s %s %s" % (",".join(hexs(pks[i, :cnt])) or "-", ",".join(hexs(msgs[i, :cnt])) or "-", hexs(sig[i:i + 1])[0]))
    f = tmp_path / "pairs.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([os.path.join(HERE, "vpairs", "cpp_caller"), str(f)], text=True, timeout=120).split("\n")
    res, st, kst = res.cpu().numpy(), st.cpu().numpy(), kst.cpu().numpy()
    for i in range(len(counts)):
        assert [int(v) for v in out[i].split()] == [res[i], st[i, 0], st[i, 1]], i
    got_k = np.array([int(v) for v in out[len(counts)].split()[1:]]).reshape(len(counts), -1)
    for i, cnt in enumerate(counts):  # behind the count the C++ side pads with zero bytes, which do not decode
        assert got_k[i, :cnt].tolist() == kst[i, :cnt].tolist() and (got_k[i, cnt:] == ST_BAD_ENCODING).all(), i
