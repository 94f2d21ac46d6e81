"""blsw_verify_groups_shared_batch and blsw_registry_verify_shared_batch on the MI355X: grouped verification over a message table, one pair per run of
equal adjacent indices. n = 70 as in test_verify_groups_gpu.py, so the last group is short; keys and signatures come from sign_batch. The yardstick is
always the plain grouped entry on msg[msg_index] with the same scalars (S1 of include/blsw.h), plus the run counts restated in Python (S3) and direct
expectations where a case states them. No test times anything."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 70
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
ST_BAD_INDEX = 6
GROUPS = (1, 7, 8, 9, 17, 64, 200)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _i32(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _i64(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def _seeded(dev, n, seed=7):
    return _i64(dev, np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64) * 2 + 1)


def _sk(i):
    return 0x2000003 + 6151 * i


def _table(dev, n_msgs, msg_len, seed=3):
    import torch

    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(n_msgs, msg_len), dtype=np.uint8)).to(dev)


def _sign(pkg, dev, sks, msg, dst=None):
    """sign_batch over secret keys (ints) and a cuda tensor of messages -> (pk48, sig96)"""
    import torch

    sk = np.frombuffer(b"".join(int(s % R_MOD).to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(len(sks), 32).copy()
    r = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg, dst=dst)
    assert int(r["status"].abs().sum().item()) == 0
    return r["pk48"].contiguous(), r["sig96"].contiguous()


def _rows(dev, index):
    import torch

    return torch.from_numpy(np.asarray(index, dtype=np.int64)).to(dev)


def _runs(index, group):
    """S3: the runs per group, restated"""
    n = len(index)
    return [sum(1 for i in range(lo, min(n, lo + group)) if i == lo or index[i] != index[i - 1]) for lo in range(0, n, group)]


def _run_lengths_pattern():
    """runs of lengths 1, 2, 8 and 9: seven single instances first, so that the run of two straddles instance 8 and, in a group of 64, the run of nine
    sits in slots beyond the first chunk of eight; rows are reused (mod 5), so equal indices also occur apart"""
    lengths = [1] * 7 + [2, 9, 8, 1, 2, 8, 9, 1, 1, 2, 8, 9, 1, 2]
    index = [k % 5 for k, ln in enumerate(lengths) for _ in range(ln)]
    assert len(index) >= N
    return index[:N]


PATTERNS = {
    "all-equal": ([0] * N, 1),
    "identity": (list(range(N)), N),
    "identity-unused-rows": (list(range(N)), N + 5),
    "run-lengths": (_run_lengths_pattern(), 5),
    "a-b-a": ([(0, 1, 0, 0, 2)[i % 5] for i in range(N)], 3),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_s1_equals_the_plain_entry_across_shapes(pkg, dev, pattern):
    """every group size against the plain entry on gathered messages: verdicts and statuses equal, run counts as stated. Two instances carry another
    index than was signed, so some groups fail (not with empty messages, which are all one message)"""
    index, n_msgs = PATTERNS[pattern]
    sc = _seeded(dev, N)
    for msg_len, dst in ((32, None), (65, pkg.DST_POP), (0, None)):
        table = _table(dev, n_msgs, msg_len)
        pk, sig = _sign(pkg, dev, [_sk(i % 16) for i in range(N)], table[_rows(dev, index)].contiguous(), dst=dst)
        used = list(index)
        if n_msgs > 1:
            used[8] = (used[8] + 1) % n_msgs
            used[N - 1] = (used[N - 1] + 1) % n_msgs
        gathered = table[_rows(dev, used)].contiguous()
        some_fail = False
        for group in GROUPS:
            ref, st_ref = pkg.verify_groups(pk, gathered, sig, group=group, scalars=sc, want_status=True, dst=dst)
            res, st, runs = pkg.verify_groups(pk, table, sig, group=group, scalars=sc, want_status=True, dst=dst, msg_index=_i32(dev, used), want_runs=True)
            assert np.array_equal(res.cpu().numpy(), ref.cpu().numpy()), (msg_len, group, res.tolist(), ref.tolist())
            assert np.array_equal(st.cpu().numpy(), st_ref.cpu().numpy()) and not st.cpu().numpy().any()
            assert runs.tolist() == _runs(used, group), (msg_len, group)
            if msg_len and n_msgs > 1:
                expect = np.ones(N, bool)
                expect[[8, N - 1]] = False
                assert res.cpu().numpy().astype(bool).tolist() == [bool(expect[lo:lo + group].all()) for lo in range(0, N, group)]
                some_fail = True
            else:
                assert (res.cpu().numpy() == 1).all()
        assert some_fail == bool(msg_len and n_msgs > 1)


@pytest.fixture(scope="module")
def shared70(pkg, dev):
    """70 valid triples over a table of 9 rows, eight instances per row: groups of 8 are one run each"""
    table = _table(dev, 9, 32, seed=5)
    index = [i // 8 for i in range(N)]
    pk, sig = _sign(pkg, dev, [_sk(i % 16) for i in range(N)], table[_rows(dev, index)].contiguous())
    return pk, sig, table, index


def test_a_run_never_crosses_a_group(pkg, dev, shared70):
    pk, sig, table, _ = shared70
    index = [0] * 16  # two adjacent groups of 8 over ONE index
    pk16, sig16 = _sign(pkg, dev, [_sk(i) for i in range(16)], table[_rows(dev, index)].contiguous())
    sig16[3] = sig16[4]  # one tampered instance in the first group
    res, runs = pkg.verify_groups(pk16, table, sig16, group=8, scalars=_seeded(dev, 16), msg_index=_i32(dev, index), want_runs=True)
    assert res.tolist() == [0, 1] and runs.tolist() == [1, 1] == _runs(index, 8)


@pytest.mark.parametrize("which", ["seeded", "ones", "max"])
def test_p2_one_tampered_index_inside_a_run_fails_exactly_its_group(pkg, dev, shared70, which):
    pk, sig, table, index = shared70
    sc = {"seeded": _seeded(dev, N), "ones": _i64(dev, [1] * N), "max": _i64(dev, [2**64 - 1] * N)}[which]
    used = list(index)
    used[3 * 8 + 5] = 0  # inside the run of group 3
    res, st, runs = pkg.verify_groups(pk, table, sig, group=8, scalars=sc, want_status=True, msg_index=_i32(dev, used), want_runs=True)
    expect = np.ones(9, np.int32)
    expect[3] = 0
    assert np.array_equal(res.cpu().numpy(), expect) and not st.cpu().numpy().any() and runs.tolist() == _runs(used, 8)
    assert np.array_equal(pkg.verify_groups(pk, table[_rows(dev, used)].contiguous(), sig, group=8, scalars=sc).cpu().numpy(), expect)


def test_zero_scalar_and_undecodable_signature_inside_a_run(pkg, dev, shared70):
    pk, sig, table, index = shared70
    idx = _i32(dev, index)
    gathered = table[_rows(dev, index)].contiguous()
    sc = _seeded(dev, N)
    sc[2 * 8 + 4] = 0
    expect = np.ones(9, np.int32)
    expect[2] = 0
    res, st = pkg.verify_groups(pk, table, sig, group=8, scalars=sc, want_status=True, msg_index=idx)
    assert np.array_equal(res.cpu().numpy(), expect) and not st.cpu().numpy().any()
    bad = sig.clone()
    bad[5 * 8 + 1] = 0  # no compression flag: a signature that does not decode
    sc = _seeded(dev, N)
    ref, st_ref = pkg.verify_groups(pk, gathered, bad, group=8, scalars=sc, want_status=True)
    res, st = pkg.verify_groups(pk, table, bad, group=8, scalars=sc, want_status=True, msg_index=idx)
    expect = np.ones(9, np.int32)
    expect[5] = 0
    assert np.array_equal(res.cpu().numpy(), expect) and np.array_equal(ref.cpu().numpy(), expect)
    assert np.array_equal(st.cpu().numpy(), st_ref.cpu().numpy()) and st[5 * 8 + 1, 1].item() != 0 and int((st != 0).sum().item()) == 1


def test_bad_message_index(pkg, dev, shared70):
    pk, sig, table, index = shared70
    sc = _seeded(dev, N)
    ref, st_ref = pkg.verify_groups(pk, table, sig, group=8, scalars=sc, want_status=True, msg_index=_i32(dev, index))
    assert (ref.cpu().numpy() == 1).all()
    used = np.array(index, dtype=np.uint32)
    used[1 * 8 + 2] = table.shape[0]  # == n_msgs
    used[6 * 8 + 7] = 0xFFFFFFFF
    res, st, runs = pkg.verify_groups(pk, table, sig, group=8, scalars=sc, want_status=True, msg_index=_i32(dev, used), want_runs=True)
    expect = np.ones(9, np.int32)
    expect[[1, 6]] = 0
    st_expect = st_ref.cpu().numpy().copy()
    st_expect[[1 * 8 + 2, 6 * 8 + 7], 0] = ST_BAD_INDEX
    assert np.array_equal(res.cpu().numpy(), expect) and np.array_equal(st.cpu().numpy(), st_expect) and runs.tolist() == _runs(used.tolist(), 8)


def test_the_additions_branches(pkg, dev):
    table = _table(dev, 2, 32, seed=9)
    # doubling: the same (key, scalar) twice in one run
    sks, index = [0xABCDEF, 0xABCDEF, 0x123457], [0, 0, 0]
    pk, sig = _sign(pkg, dev, sks, table[_rows(dev, index)].contiguous())
    sc = _i64(dev, [9, 9, 5])
    res, runs = pkg.verify_groups(pk, table, sig, group=3, scalars=sc, msg_index=_i32(dev, index), want_runs=True)
    assert res.tolist() == [1] == pkg.verify_groups(pk, table[_rows(dev, index)].contiguous(), sig, group=3, scalars=sc).tolist() and runs.tolist() == [1]
    # sk and r - sk with equal scalars in one run, both valid: R and S_g are both the identity, a group with no pair passes
    sks = [0xC0FFEE, R_MOD - 0xC0FFEE, 0x123457]
    pk, sig = _sign(pkg, dev, sks, table[_rows(dev, index)].contiguous())
    assert pkg.verify_batch(pk, table[_rows(dev, index)].contiguous(), sig).tolist() == [1, 1, 1]
    two = _i32(dev, [0, 0])
    assert pkg.verify_groups(pk[:2].contiguous(), table, sig[:2].contiguous(), group=2, scalars=_i64(dev, [7, 7]), msg_index=two).tolist() == [1]
    # the cancelling pair with a third instance: valid passes, tampered (another index than was signed) fails
    sc = _i64(dev, [7, 7, 5])
    assert pkg.verify_groups(pk, table, sig, group=3, scalars=sc, msg_index=_i32(dev, [0, 0, 0])).tolist() == [1]
    res, runs = pkg.verify_groups(pk, table, sig, group=3, scalars=sc, msg_index=_i32(dev, [0, 0, 1]), want_runs=True)
    assert res.tolist() == [0] and runs.tolist() == [2]


def test_s2_a_permutation_within_groups_keeps_the_verdicts(pkg, dev, shared70):
    import torch

    pk, sig, table, _ = shared70
    index = _run_lengths_pattern()
    pk, sig = _sign(pkg, dev, [_sk(i % 16) for i in range(N)], table[_rows(dev, index)].contiguous())
    used = list(index)
    used[20] = (used[20] + 1) % 5
    sc = _seeded(dev, N)
    group = 17
    rng = np.random.default_rng(23)
    perm = np.concatenate([lo + rng.permutation(min(N, lo + group) - lo) for lo in range(0, N, group)])
    pt = torch.from_numpy(perm).to(dev)
    a, runs_a = pkg.verify_groups(pk, table, sig, group=group, scalars=sc, msg_index=_i32(dev, used), want_runs=True)
    b, runs_b = pkg.verify_groups(pk[pt].contiguous(), table, sig[pt].contiguous(), group=group, scalars=sc[pt].contiguous(), msg_index=_i32(dev, np.array(used)[perm]), want_runs=True)
    assert a.tolist() == b.tolist() == [1, 0, 1, 1, 1]
    assert runs_a.tolist() == _runs(used, group) and runs_b.tolist() == _runs(np.array(used)[perm].tolist(), group) and runs_a.tolist() != runs_b.tolist()


@pytest.fixture(scope="module")
def registry300(pkg, dev):
    import torch

    sks = [_sk(100 + i) for i in range(300)]
    sk = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(300, 32).copy()
    r = pkg.sign_batch(torch.from_numpy(sk).to(dev), torch.zeros((300, 32), dtype=torch.uint8, device=dev))
    reg = pkg.KeyRegistry(300, device=dev)
    assert reg.append(r["pk48"].contiguous()) == 300
    yield reg, sks
    reg.close()


def _csr(lists):
    return np.concatenate(lists + [[]]).astype(np.uint32), np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)


def test_registry_form_equals_the_plain_registry_entry(pkg, dev, registry300):
    reg, sks = registry300
    rng = np.random.default_rng(31)
    lists = [rng.integers(0, 300, size=1 + i % 40).tolist() for i in range(N)]
    set_sks = [sum(sks[k] for k in lst) % R_MOD for lst in lists]
    assert all(set_sks)
    sc = _seeded(dev, N)
    for pattern in ("all-equal", "identity-unused-rows", "run-lengths", "a-b-a"):
        index, n_msgs = PATTERNS[pattern]
        table = _table(dev, n_msgs, 32, seed=13)
        _, sig = _sign(pkg, dev, set_sks, table[_rows(dev, index)].contiguous())
        used, spoiled = np.array(index, dtype=np.uint32), [list(x) for x in lists]
        if n_msgs > 1:
            used[40] = (used[40] + 1) % n_msgs  # another row than was signed
        used[12] = n_msgs  # a bad message index ...
        spoiled[55][0] = 300  # ... and a bad registry index in another set: each reported by its own rule
        idx, off = _csr(spoiled)
        ti, to = _i32(dev, idx), _i64(dev, off)
        in_range = used.copy()
        in_range[12] = index[12]
        gathered = table[_rows(dev, in_range)].contiguous()
        for group in (8, 9, 64):
            ref, st_ref, agg_ref = pkg.registry_verify(reg, ti, to, gathered, sig, group=group, scalars=sc, want_status=True, want_aggregate=True)
            res, st, agg, runs = pkg.registry_verify(reg, ti, to, table, sig, group=group, scalars=sc, want_status=True, want_aggregate=True, msg_index=_i32(dev, used), want_runs=True)
            assert np.array_equal(agg.cpu().numpy(), agg_ref.cpu().numpy())
            st_expect = st_ref.cpu().numpy().copy()
            assert st_expect[55, 0] == ST_BAD_INDEX and st_expect[12, 0] == 0 and int((st_expect != 0).sum()) == 1
            st_expect[12, 0] = ST_BAD_INDEX
            assert np.array_equal(st.cpu().numpy(), st_expect)
            expect = ref.cpu().numpy().copy()
            assert expect[55 // group] == 0
            expect[12 // group] = 0
            assert np.array_equal(res.cpu().numpy(), expect) and runs.tolist() == _runs(used.tolist(), group), (pattern, group)
            ok = np.ones(N, bool)
            ok[[12, 55] + ([40] if n_msgs > 1 else [])] = False
            assert res.cpu().numpy().astype(bool).tolist() == [bool(ok[lo:lo + group].all()) for lo in range(0, N, group)]


def test_python_wrappers(pkg, dev, shared70, registry300):
    import torch

    pk, sig, table, index = shared70
    idx = _i32(dev, index)
    gathered = table[_rows(dev, index)].contiguous()
    bad = sig.clone()
    bad[37] = sig[36]
    sc = _seeded(dev, N)
    # verify_batch_grouped: the per-instance verdicts of the plain call
    ref, st_ref = pkg.verify_batch(pk, gathered, bad, want_status=True)
    got, st, runs = pkg.verify_batch_grouped(pk, table, bad, group=8, scalars=sc, want_status=True, msg_index=idx, want_runs=True)
    expect = np.ones(N, np.int32)
    expect[37] = 0
    assert np.array_equal(got.cpu().numpy(), expect) and np.array_equal(ref.cpu().numpy(), expect) and torch.equal(st, st_ref) and runs.tolist() == _runs(index, 8)
    assert torch.equal(got, pkg.verify_batch_grouped(pk, gathered, bad, group=8, scalars=sc))
    # msg_index=None is the call it was: the same tensors as a second call
    a, st_a = pkg.verify_groups(pk, gathered, bad, group=8, scalars=sc, want_status=True)
    b, st_b = pkg.verify_groups(pk, gathered, bad, group=8, scalars=sc, want_status=True, msg_index=None)
    assert torch.equal(a, b) and torch.equal(st_a, st_b) and a.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    with pytest.raises(ValueError):
        pkg.verify_groups(pk, gathered, bad, group=8, scalars=sc, want_runs=True)
    # registry_verify_grouped and registry_verify(group=0) over the table
    reg, sks = registry300
    rng = np.random.default_rng(37)
    lists = [rng.integers(0, 300, size=1 + i % 5).tolist() for i in range(N)]
    _, rsig = _sign(pkg, dev, [sum(sks[k] for k in lst) % R_MOD for lst in lists], gathered)
    rsig[37] = rsig[36]
    ridx, roff = _csr(lists)
    ti, to = _i32(dev, ridx), _i64(dev, roff)
    ref, st_ref = pkg.registry_verify(reg, ti, to, gathered, rsig, want_status=True)
    assert np.array_equal(ref.cpu().numpy(), expect)
    got, st = pkg.registry_verify_grouped(reg, ti, to, table, rsig, group=8, scalars=sc, want_status=True, msg_index=idx)
    assert torch.equal(got, ref) and torch.equal(st, st_ref)
    got, st = pkg.registry_verify(reg, ti, to, table, rsig, want_status=True, msg_index=idx)
    assert torch.equal(got, ref) and torch.equal(st, st_ref)
    assert torch.equal(pkg.registry_verify_grouped(reg, ti, to, gathered, rsig, group=8, scalars=sc), ref)
    # two calls on a side stream agree
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        a, st_a, runs_a = pkg.verify_groups(pk, table, bad, group=8, scalars=sc, want_status=True, msg_index=idx, want_runs=True)
        b, st_b, runs_b = pkg.verify_groups(pk, table, bad, group=8, scalars=sc, want_status=True, msg_index=idx, want_runs=True)
    s.synchronize()
    assert torch.equal(a, b) and torch.equal(st_a, st_b) and torch.equal(runs_a, runs_b) and a.tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
