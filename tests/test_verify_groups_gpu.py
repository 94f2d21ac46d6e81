"""blsw_verify_groups_batch on the MI355X: groups of (pk, msg, sig) triples verified with caller-chosen coefficients. Shapes are the smallest that cross
every boundary — wave (64 lanes, 10 teams), chunk (VERIFY_GROUPS_CHUNK pairs per team) and group — and the properties are those of include/blsw.h
(P1 - P4) plus fail-closed coefficients, the two edge cases of the group sum, and verify_batch_grouped == verify_batch. No test times anything."""
import importlib

import numpy as np
import pytest

from tests.oracle_lib import eth_cases, unhex

pytestmark = pytest.mark.gpu
SEED = 0x5EED
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _t(dev, xs, w):
    import torch

    return torch.from_numpy(np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(len(xs), w).copy()).to(dev)


def _scalars(dev, values):
    import torch

    return torch.from_numpy(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64)).to(dev)


def _seeded(dev, n, seed=7):
    r = np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64) * 2 + 1  # odd, so distinct from zero; the top bit set in half of them
    return _scalars(dev, r)


def _sign(pkg, dev, sks, msgs):
    """sign_batch over secret keys (ints) and messages (bytes of one length) -> (pk48, msg, sig96) cuda tensors"""
    import torch

    sk = np.frombuffer(b"".join(int(s).to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(len(sks), 32).copy()
    msg = _t(dev, msgs, len(msgs[0]))
    r = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg)
    assert int(r["status"].abs().sum().item()) == 0
    return r["pk48"], msg, r["sig96"]


def _workload(pkg, dev, n):
    """the bench's batch as compressed bytes, nothing tampered: 16 keys, msg_i = SHA-256(seed || "m" || i)"""
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    sks = workload.secret_keys(SEED, 16)
    msgs = workload.messages(SEED, 0, n)
    return _sign(pkg, dev, [sks[i % 16] for i in range(n)], [m.tobytes() for m in msgs])


@pytest.fixture(scope="module")
def batch70(pkg, dev):
    return _workload(pkg, dev, 70)


@pytest.fixture(scope="module")
def batch1024(pkg, dev):
    return _workload(pkg, dev, 1024)


def _tampered(msg, idx):
    m = msg.clone()
    m[idx, 31] ^= 1
    return m


def _fixture_rows():
    rows = [(name, unhex(c["input"]["pubkey"]), unhex(c["input"]["message"]), unhex(c["input"]["signature"]), c["output"]) for name, c in eth_cases("verify")]
    assert len(rows) == 29 and all(len(r[1]) == 48 and len(r[3]) == 96 and len(r[2]) == 32 for r in rows)
    return rows


def test_p3_fixtures_in_one_call_of_groups_of_one(pkg, dev):
    rows = _fixture_rows()
    pk, msg, sig = _t(dev, [r[1] for r in rows], 48), _t(dev, [r[2] for r in rows], 32), _t(dev, [r[3] for r in rows], 96)
    res, st = pkg.verify_groups(pk, msg, sig, group=1, scalars=_scalars(dev, [0x9E3779B97F4A7C15] * 29), want_status=True)
    got = res.cpu().numpy().astype(bool).tolist()
    assert got == [r[4] for r in rows], [r[0] for r, g in zip(rows, got) if g != r[4]]
    _, st_ref = pkg.verify_batch(pk, msg, sig, want_status=True)
    assert np.array_equal(st.cpu().numpy(), st_ref.cpu().numpy())


def _group_sizes(c):
    return sorted({g for g in (1, 2, c - 1, c, c + 1, 2 * c + 1, 64, 70, 71) if g > 0})


def test_p1_valid_batch_passes_for_every_group_size(pkg, dev, batch70):
    """n = 70: two waves of the lane kernels, a ragged last wave of teams"""
    pk, msg, sig = batch70
    sc = _seeded(dev, 70)
    for group in _group_sizes(pkg.VERIFY_GROUPS_CHUNK):
        res = pkg.verify_groups(pk, msg, sig, group=group, scalars=sc).cpu().numpy()
        assert res.shape == ((70 + group - 1) // group,) and (res == 1).all(), (group, res.tolist())


def _p2_shape(c, n=70):
    """a group size with a middle group and a short tail group, and the three instances to tamper: the first of group 0, the last of the first chunk of
    a middle group, the last of the tail group"""
    group = next(g for g in (2 * c + 1, c + 1, c + 2) if n % g and (n + g - 1) // g >= 3)
    n_groups = (n + group - 1) // group
    mid = n_groups // 2
    assert 0 < mid < n_groups - 1 and min(c, group) - 1 < group
    return group, n_groups, [0, mid * group + min(c, group) - 1, n - 1], [0, mid, n_groups - 1]


@pytest.mark.parametrize("which", ["seeded", "ones", "max"])
def test_p2_one_bad_instance_fails_exactly_its_group(pkg, dev, batch70, which):
    pk, msg, sig = batch70
    group, n_groups, idx, bad_groups = _p2_shape(pkg.VERIFY_GROUPS_CHUNK)
    sc = {"seeded": _seeded(dev, 70), "ones": _scalars(dev, [1] * 70), "max": _scalars(dev, [2**64 - 1] * 70)}[which]
    res, st = pkg.verify_groups(pk, _tampered(msg, idx), sig, group=group, scalars=sc, want_status=True)
    expect = np.ones(n_groups, dtype=np.int32)
    expect[bad_groups] = 0
    assert np.array_equal(res.cpu().numpy(), expect) and not st.cpu().numpy().any()


def test_zero_scalar_fails_its_group_only(pkg, dev, batch70):
    pk, msg, sig = batch70
    group = pkg.VERIFY_GROUPS_CHUNK + 1
    sc = _seeded(dev, 70)
    sc[group + 1] = 0
    res = pkg.verify_groups(pk, msg, sig, group=group, scalars=sc).cpu().numpy()
    expect = np.ones((70 + group - 1) // group, dtype=np.int32)
    expect[1] = 0
    assert np.array_equal(res, expect)


def test_swap_identity_sum_doubling_and_a_single_instance(pkg, dev, oracle):
    import torch

    # the swap (P4): A = (pk, m1, sig2), B = (pk, m2, sig1)
    sk, m1, m2 = 0x5EED5EED5EED, b"\x11" * 32, b"\x22" * 32
    pk, msg, sig = _sign(pkg, dev, [sk, sk], [m1, m2])
    swapped = sig.flip(0).contiguous()
    pkb, sgb = bytes(pk[0].cpu().numpy()), [bytes(s.cpu().numpy()) for s in sig]
    assert not oracle.verify_bytes(pkb, m1, sgb[1]) and not oracle.verify_bytes(pkb, m2, sgb[0]) and oracle.verify_bytes(pkb, m1, sgb[0])
    assert pkg.verify_groups(pk, msg, swapped, group=2, scalars=_scalars(dev, [5, 5])).tolist() == [1]  # the documented weakness of predictable coefficients
    assert pkg.verify_groups(pk, msg, swapped, group=2, scalars=_scalars(dev, [5, 7])).tolist() == [0]
    assert pkg.verify_batch(pk, msg, swapped).tolist() == [0, 0]
    # identity sum: sk and r - sk on one message with equal coefficients — both valid, S_g = 0, a skipped pair and a group that passes
    m = b"\x33" * 32
    pk, msg, sig = _sign(pkg, dev, [0xC0FFEE, R_MOD - 0xC0FFEE], [m, m])
    assert pkg.verify_batch(pk, msg, sig).tolist() == [1, 1] and not torch.equal(sig[0], sig[1])
    assert pkg.verify_groups(pk, msg, sig, group=2, scalars=_scalars(dev, [7, 7])).tolist() == [1]
    # doubling in the sum: the same triple twice with the same coefficient
    pk, msg, sig = _sign(pkg, dev, [0xABCDEF, 0xABCDEF], [b"\x44" * 32] * 2)
    assert pkg.verify_groups(pk, msg, sig, group=2, scalars=_scalars(dev, [9, 9])).tolist() == [1]
    # n = 1 in a group of 64, host-drawn coefficients
    res, st = pkg.verify_groups(pk[:1], msg[:1], sig[:1], want_status=True)
    assert res.tolist() == [1] and st.tolist() == [[0, 0]]
    assert pkg.verify_groups(pk[:1], _tampered(msg[:1], [0]), sig[:1]).tolist() == [0]


def test_grouped_equals_verify_batch_on_the_fixtures(pkg, dev):
    rows = _fixture_rows()
    pk, msg, sig = _t(dev, [r[1] for r in rows], 48), _t(dev, [r[2] for r in rows], 32), _t(dev, [r[3] for r in rows], 96)
    ref, st_ref = pkg.verify_batch(pk, msg, sig, want_status=True)
    got, st = pkg.verify_batch_grouped(pk, msg, sig, group=8, scalars=_seeded(dev, 29), want_status=True)
    assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(st.cpu().numpy(), st_ref.cpu().numpy())
    assert got.cpu().numpy().astype(bool).tolist() == [r[4] for r in rows]


@pytest.mark.parametrize("tamper,group", [(True, 8), (True, 64), (False, 64)], ids=["half-fall-back", "all-fall-back", "none-falls-back"])
def test_grouped_equals_verify_batch_on_the_workload(pkg, dev, batch1024, tamper, group):
    pk, msg, sig = batch1024
    expect = np.ones(1024, dtype=bool)
    if tamper:
        bad = np.arange(15, 1024, 16)
        msg = _tampered(msg, bad)
        expect[bad] = False
    gres = pkg.verify_groups(pk, msg, sig, group=group, scalars=_seeded(dev, 1024)).cpu().numpy().astype(bool)
    assert np.array_equal(gres, expect.reshape(-1, group).all(axis=1))
    got = pkg.verify_batch_grouped(pk, msg, sig, group=group, scalars=_seeded(dev, 1024)).cpu().numpy().astype(bool)
    assert np.array_equal(got, pkg.verify_batch(pk, msg, sig).cpu().numpy().astype(bool)) and np.array_equal(got, expect)


def test_two_calls_on_a_side_stream_agree(pkg, dev, batch70):
    import torch

    pk, msg, sig = batch70
    group, n_groups, idx, bad_groups = _p2_shape(pkg.VERIFY_GROUPS_CHUNK)
    msg = _tampered(msg, idx)
    sc = _seeded(dev, 70)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        a, st_a = pkg.verify_groups(pk, msg, sig, group=group, scalars=sc, want_status=True)
        b, st_b = pkg.verify_groups(pk, msg, sig, group=group, scalars=sc, want_status=True)
    s.synchronize()
    expect = np.ones(n_groups, dtype=np.int32)
    expect[bad_groups] = 0
    assert np.array_equal(a.cpu().numpy(), expect) and torch.equal(a, b) and torch.equal(st_a, st_b)
