"""blsw_registry_* on the MI355X: keys decoded once into a resident registry, n index lists summed with REGISTRY_LANES lanes each, the sums through
the two value verifiers. The yardsticks are the parent's composition on the gathered keys (aggregate_points + fast_aggregate_verify_batch, one call
per list length), the committee form on the same selection, the CPU oracle and the construction of the batch. The shape is the smallest with several
waves of the sum, partial waves and lanes that walk nothing: capacity 200, size 131, n = 70 sets, 32-byte messages, list lengths cycling through
0 .. 2 L + 1. The argument rules that need a live handle are here too (tests/test_registry_ref.py has the others). No test times anything."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import committee_lib, registry_lib
from tests.committee_lib import IDENTITY48, R_MOD
from tests.oracle_lib import eth_cases, unhex
from tests.registry_lib import ST_BAD_INDEX, ST_IDENTITY, ST_OK, csr

pytestmark = pytest.mark.gpu
CAPACITY, SIZE, N = 200, 131, 70


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


def _i32(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _i64(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def _seeded(dev, n, seed=7):
    return _i64(dev, np.random.default_rng(seed).integers(1, 2**63, size=n, dtype=np.uint64) * 2 + 1)


def _sk(i):
    return 0x1000003 + 7919 * i


_KEYS = {}


def _keys(pkg, dev):
    """131 keys minted once by sign_batch -> (secret keys, pk48 cuda [131, 48])"""
    import torch

    if not _KEYS:
        sks = [_sk(i) for i in range(SIZE)]
        sk = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(SIZE, 32).copy()
        r = pkg.sign_batch(torch.from_numpy(sk).to(dev), torch.zeros((SIZE, 32), dtype=torch.uint8, device=dev))
        assert int(r["status"].abs().sum().item()) == 0
        _KEYS["sks"], _KEYS["pk48"] = sks, r["pk48"].contiguous()
    return _KEYS["sks"], _KEYS["pk48"]


@pytest.fixture(scope="module")
def registry(pkg, dev):
    """capacity 200, the 131 keys appended in two parts; shared and never appended to again"""
    _, pk48 = _keys(pkg, dev)
    reg = pkg.KeyRegistry(CAPACITY, device=dev)
    assert reg.size == 0 and reg.append(pk48[:64].contiguous()) == 64 and reg.append(pk48[64:].contiguous()) == SIZE
    assert reg.size == SIZE and reg.key_status().shape == (SIZE,) and not reg.key_status().cpu().numpy().any()
    yield reg
    reg.close()


def test_a_registry_on_the_unindexed_device_takes_indexed_tensors(pkg, dev, oracle):
    """KeyRegistry(device="cuda") is the current device with its index: tensors on cuda:0 are its tensors"""
    sks, pk48 = _keys(pkg, dev)
    reg = pkg.KeyRegistry(4, device="cuda")
    assert reg.device == pk48.device and reg.append(pk48[:3].contiguous()) == 3
    m = b"\x19" * 32
    res = _verify(pkg, dev, reg, [[2, 0]], _t(dev, [m], 32), _t(dev, [oracle.sign((sks[2] + sks[0]) % R_MOD, m)], 96))
    assert res.tolist() == [1]
    reg.close()


_BATCHES = {}


def _batch(pkg, dev, oracle, seed, empty=True, spoil=True):
    """(lists, msg, sig96 as cuda tensors, expected verdicts): set i has i % (2 L + 2) entries (from 1 on without `empty`) drawn with repetition and
    is signed by the sum of the keys it names; with `spoil` about one in eight then gets a tampered message and one in eight another last index than
    was signed. Made once per shape and shared: callers change copies"""
    key = (seed, empty, spoil)
    if key not in _BATCHES:
        L = pkg.REGISTRY_LANES
        sks, _ = _keys(pkg, dev)
        rng = np.random.default_rng(seed)
        lists = [rng.integers(0, SIZE, size=(i % (2 * L + 2) if empty else 1 + i % (2 * L + 1))).tolist() for i in range(N)]
        msgs = [bytes([i & 0xFF, 0x52, seed & 0xFF, 0x47]) * 8 for i in range(N)]
        sigs, expect = [], []
        for lst, m in zip(lists, msgs):
            sk = sum(sks[k] for k in lst) % R_MOD
            sigs.append(oracle.sign(sk if sk else 1, m))  # an empty list is false whatever the signature
            expect.append(bool(lst))
        for i in range(N):
            if spoil and i % 8 == 5:
                msgs[i] = bytes([msgs[i][0] ^ 1]) + msgs[i][1:]
                expect[i] = False
            if spoil and i % 8 == 6 and lists[i]:
                lists[i][-1] = (lists[i][-1] + 1) % SIZE
                expect[i] = False
        _BATCHES[key] = (lists, _t(dev, msgs, 32), _t(dev, sigs, 96), np.array(expect))
    return _BATCHES[key]


def _parent(pkg, dev, pks48, lists, msg, sig):
    """the parent's way: gather the named keys, aggregate_points + fast_aggregate_verify_batch, one call per list length -> (agg48 [n, 48], verdicts [n])"""
    import torch

    counts = np.array([len(x) for x in lists])
    agg = np.zeros((len(lists), 48), np.uint8)
    res = np.zeros(len(lists), bool)
    for k in sorted(set(counts.tolist())):
        idx = np.flatnonzero(counts == k)
        if k == 0:
            agg[idx] = np.frombuffer(IDENTITY48, np.uint8)
            continue
        sel = torch.from_numpy(np.array([lists[i] for i in idx], dtype=np.int64)).to(dev)
        gathered = pks48[sel].contiguous()  # [m, k, 48]
        a, st = pkg.aggregate_points(1, gathered)
        assert not st.cpu().numpy().any()
        ti = torch.from_numpy(idx).to(dev)
        agg[idx] = a.cpu().numpy()
        res[idx] = pkg.fast_aggregate_verify_batch(gathered, msg[ti].contiguous(), sig[ti].contiguous()).cpu().numpy().astype(bool)
    return agg, res


def _verify(pkg, dev, reg, lists, msg, sig, **kw):
    idx, off = csr(lists)
    return pkg.registry_verify(reg, _i32(dev, idx), _i64(dev, off), msg, sig, **kw)


def test_seventy_sets_equal_the_parents_composition(pkg, dev, oracle, registry):
    _, pk48 = _keys(pkg, dev)
    lists, msg, sig, expect = _batch(pkg, dev, oracle, 11)
    L = pkg.REGISTRY_LANES
    assert sorted({len(x) for x in lists}) == list(range(min(N, 2 * L + 2)))
    res, st, agg = _verify(pkg, dev, registry, lists, msg, sig, want_status=True, want_aggregate=True)
    res, st, agg = res.cpu().numpy().astype(bool), st.cpu().numpy(), agg.cpu().numpy()
    p_agg, p_res = _parent(pkg, dev, pk48, lists, msg, sig)
    assert np.array_equal(agg, p_agg), np.flatnonzero((agg != p_agg).any(axis=1)).tolist()
    assert np.array_equal(st[:, 0], np.where(np.array([len(x) for x in lists]) == 0, ST_IDENTITY, ST_OK)) and not st[:, 1].any()
    assert np.array_equal(res, p_res), np.flatnonzero(res != p_res).tolist()
    assert np.array_equal(res, expect), np.flatnonzero(res != expect).tolist()
    assert 0 < res.sum() < N
    for i in (1, 33, 69):  # and the oracle's aggregate, for a few
        assert bytes(agg[i]) == (oracle.aggregate_g1([bytes(pk48[k].cpu().numpy()) for k in lists[i]]) if lists[i] else IDENTITY48)


def test_lists_taken_from_bitmaps_equal_the_committee_form(pkg, dev, oracle, registry):
    import torch

    K = 65
    sks, pk48 = _keys(pkg, dev)
    rng = np.random.default_rng(65)
    rows = [np.zeros(K, np.uint8), np.ones(K, np.uint8)]
    while len(rows) < N:
        row = np.zeros(K, np.uint8)
        row[rng.choice(K, size=(1, K // 10, K // 2, K - 1)[len(rows) % 4], replace=False)] = 1
        rows.append(row)
    bitmap = np.stack(rows)
    msgs = [bytes([i, 0x65]) * 16 for i in range(N)]
    sigs = [oracle.sign(sum(s for s, b in zip(sks, row) if b) % R_MOD or 1, m) for row, m in zip(bitmap, msgs)]
    msg, sig = _t(dev, msgs, 32), _t(dev, sigs, 96)
    c_res, (c_st, c_kst), c_agg = pkg.committee_verify(pk48[:K].contiguous(), torch.from_numpy(bitmap).to(dev), msg, sig, want_status=True, want_aggregate=True)
    lists = [np.flatnonzero(r).tolist() for r in rows]
    res, st, agg = _verify(pkg, dev, registry, lists, msg, sig, want_status=True, want_aggregate=True)
    assert torch.equal(res, c_res) and torch.equal(st, c_st) and torch.equal(agg, c_agg)
    assert res.tolist() == [0] + [1] * (N - 1) and not c_kst.cpu().numpy().any()


def test_edges_and_bad_entries_on_the_device(pkg, dev, oracle):
    """tests/registry_lib.edge_lists in ONE call, good sets between the cases: the group law's edges, every failing key status, bad indices"""
    pks, sks, names = registry_lib.edge_registry(oracle)
    reg = pkg.KeyRegistry(len(pks) + 8, device=dev)
    reg.append(_t(dev, pks, 48))
    kst_exp = []
    for p in pks:
        ost, _, oinf = oracle.g1_decompress(p)
        kst_exp.append(ST_IDENTITY if (ost == 0 and oinf) else ost)
    assert reg.key_status().tolist() == kst_exp
    cases = registry_lib.edge_lists(pkg.REGISTRY_LANES, names, reg.size, reg.capacity)
    lists, labels = [], []
    for j, (name, lst, _) in enumerate(cases):
        lists += [[j % registry_lib.BASE_KEYS, (j + 3) % registry_lib.BASE_KEYS], lst]
        labels += [None, name]
    lists.append([5])
    labels.append(None)
    m = b"\x77" * 32
    sigs = [oracle.sign(registry_lib.list_sk(sks, lst, reg.size) or 1, m) for lst in lists]
    res, st, agg = _verify(pkg, dev, reg, lists, _t(dev, [m] * len(lists), 32), _t(dev, sigs, 96), want_status=True, want_aggregate=True)
    res, st, agg = res.cpu().numpy(), st.cpu().numpy(), agg.cpu().numpy()
    seen = {}
    for i, (lst, label) in enumerate(zip(lists, labels)):
        est, eagg = registry_lib.expected(oracle, pks, kst_exp, reg.size, lst)
        assert (st[i].tolist(), bytes(agg[i])) == ([est, 0], eagg), (i, label)
        assert bool(res[i]) == (est == ST_OK and oracle.verify_bytes(eagg, m, sigs[i])), (i, label)
        if label is None:
            assert res[i] == 1, i  # the neighbours are unaffected
        else:
            seen[label.split(":")[0]] = (est, bool(res[i]))
    for (name, _, want) in cases:
        if want is not None:
            assert seen[name.split(":")[0]][0] == want, name
    assert seen["the same index at positions 0 and L, then Q in the lane"] == (ST_OK, True) and seen["the same index at positions 0 and 1, nothing else"] == (ST_OK, True)
    assert seen["a key, its negation and Q in one lane"] == (ST_OK, True) and seen["a key and its negation in two lanes"] == (ST_IDENTITY, False)
    assert seen["an identity key among others"] == (ST_OK, True) and seen["one index 3 L times"] == (ST_OK, True)
    for name in ("index == size", "index == 0xffffffff", "an index >= size below the capacity", "a bad index then a bad key"):
        assert seen[name] == (ST_BAD_INDEX, False), name
    reg.close()


def test_bad_offsets_fail_their_own_set_only(pkg, dev, oracle, registry):
    sks, _ = _keys(pkg, dev)
    m = 2 * pkg.REGISTRY_LANES + 1
    good = list(range(m))
    idx = np.array(good * 3, dtype=np.uint32)
    off = np.array([0, m, m - 1, 2 * m - 1, 3 * m + 1, 2**63], dtype=np.uint64)  # good | descending | good | beyond n_indices | beyond, and huge
    lists = [good, None, idx[m - 1:2 * m - 1].tolist(), None, None]
    msg = _t(dev, [bytes([0x30 + i]) * 32 for i in range(5)], 32)
    sigs = [oracle.sign(sum(sks[k] for k in lst) % R_MOD if lst else 1, bytes([0x30 + i]) * 32) for i, lst in enumerate(lists)]
    res, st, agg = pkg.registry_verify(registry, _i32(dev, idx), _i64(dev, off), msg, _t(dev, sigs, 96), want_status=True, want_aggregate=True)
    assert res.tolist() == [1, 0, 1, 0, 0] and st.tolist() == [[0, 0], [ST_BAD_INDEX, 0], [0, 0], [ST_BAD_INDEX, 0], [ST_BAD_INDEX, 0]]
    assert not agg[[1, 3, 4]].cpu().numpy().any() and agg[[0, 2]].cpu().numpy().any(axis=1).all()
    # no index array at all: every list must be empty, and one that is not has bad offsets
    import torch

    none = torch.zeros(0, dtype=torch.int32, device=dev)
    res, st = pkg.registry_verify(registry, none, _i64(dev, [0, 0, 1]), msg[:2].contiguous(), _t(dev, sigs[:2], 96), want_status=True)
    assert res.tolist() == [0, 0] and st[:, 0].tolist() == [ST_IDENTITY, ST_BAD_INDEX]


def test_no_stale_row_counts_between_two_appends(pkg, dev, oracle, registry):
    """the buffer of a fresh handle holds every record of an earlier life (the shared registry's bytes, copied in): a verify between the two appends
    still answers BAD_INDEX for an index of the second part, and the true verdict after the second append"""
    sks, pk48 = _keys(pkg, dev)
    reg = pkg.KeyRegistry(CAPACITY, device=dev)
    reg.buffer.copy_(registry.buffer)
    assert reg.append(pk48[:64].contiguous()) == 64
    lists = [[3, 63], [3, 64], [100, 5, 130]]
    msgs = [bytes([0x21 + i]) * 32 for i in range(3)]
    msg, sig = _t(dev, msgs, 32), _t(dev, [oracle.sign(sum(sks[k] for k in lst) % R_MOD, m) for lst, m in zip(lists, msgs)], 96)
    res, st = _verify(pkg, dev, reg, lists, msg, sig, want_status=True)
    assert res.tolist() == [1, 0, 0] and st[:, 0].tolist() == [ST_OK, ST_BAD_INDEX, ST_BAD_INDEX]
    assert reg.append(pk48[64:].contiguous()) == SIZE
    res, st = _verify(pkg, dev, reg, lists, msg, sig, want_status=True)
    assert res.tolist() == [1, 1, 1] and not st.cpu().numpy().any()
    reg.close()


@pytest.fixture(scope="module")
def valid70(pkg, dev, oracle):
    """n = 70, every set valid, no empty list"""
    return _batch(pkg, dev, oracle, 900, empty=False, spoil=False)[:3]


def _tampered(msg, idx):
    m = msg.clone()
    m[idx, 31] ^= 1
    return m


@pytest.mark.parametrize("group", [1, 8, 64])
def test_grouped_p1_p2_zero_coefficient_and_a_bad_index(pkg, dev, registry, valid70, group):
    lists, msg, sig = valid70
    idx, off = csr(lists)
    ti, to = _i32(dev, idx), _i64(dev, off)
    n_groups = (N + group - 1) // group
    ones = np.ones(n_groups, np.int32)
    for sc in (_seeded(dev, N), _i64(dev, [2**64 - 1] * N)):  # P1
        res, st = pkg.registry_verify(registry, ti, to, msg, sig, group=group, scalars=sc, want_status=True)
        assert np.array_equal(res.cpu().numpy(), ones) and not st.cpu().numpy().any()
    sc = _seeded(dev, N)
    for bad in (0, 37, 69):  # P2: exactly one tampered set fails its group only
        expect = ones.copy()
        expect[bad // group] = 0
        assert np.array_equal(pkg.registry_verify(registry, ti, to, _tampered(msg, [bad]), sig, group=group, scalars=sc).cpu().numpy(), expect), bad
    zero = sc.clone()
    zero[66] = 0
    expect = ones.copy()
    expect[66 // group] = 0
    assert np.array_equal(pkg.registry_verify(registry, ti, to, msg, sig, group=group, scalars=zero).cpu().numpy(), expect)
    spoiled = idx.copy()
    spoiled[int(off[9])] = SIZE  # index == size: BAD_INDEX, excluded, fails its own group only
    expect = ones.copy()
    expect[9 // group] = 0
    res, st = pkg.registry_verify(registry, _i32(dev, spoiled), to, msg, sig, group=group, scalars=sc, want_status=True)
    assert np.array_equal(res.cpu().numpy(), expect) and st[9].tolist() == [ST_BAD_INDEX, 0] and int(st.cpu().numpy().sum()) == ST_BAD_INDEX


def test_grouped_p3_and_the_per_set_form_through_groups(pkg, dev, oracle, registry, valid70):
    lists, msg, sig, expect = _batch(pkg, dev, oracle, 11)
    per = _verify(pkg, dev, registry, lists, msg, sig).cpu().numpy()
    assert np.array_equal(per.astype(bool), expect)
    assert np.array_equal(_verify(pkg, dev, registry, lists, msg, sig, group=1, scalars=_seeded(dev, N)).cpu().numpy(), per)  # P3
    assert np.array_equal(_verify(pkg, dev, registry, lists, msg, sig, group=1).cpu().numpy(), per)  # host-drawn coefficients
    # registry_verify_grouped: three bad sets in two groups of eight, one of them by a bad index
    lists, msg, sig = valid70
    idx, off = csr(lists)
    idx[int(off[41])] = 0xFFFFFFFF
    ti, to, bad = _i32(dev, idx), _i64(dev, off), _tampered(msg, [3, 40])
    ref, st_ref = pkg.registry_verify(registry, ti, to, bad, sig, want_status=True)
    got, st = pkg.registry_verify_grouped(registry, ti, to, bad, sig, group=8, scalars=_seeded(dev, N), want_status=True)
    want = np.ones(N, np.int32)
    want[[3, 40, 41]] = 0
    assert np.array_equal(ref.cpu().numpy(), want) and np.array_equal(got.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), st_ref.cpu().numpy())
    idx, off = csr(lists)
    assert np.array_equal(pkg.registry_verify_grouped(registry, _i32(dev, idx), _i64(dev, off), msg, sig).cpu().numpy(), np.ones(N, np.int32))
    # a set with bad offsets in a failing group stays false
    off2 = off.copy()
    off2[N] = len(idx) + 1
    got = pkg.registry_verify_grouped(registry, _i32(dev, idx), _i64(dev, off2), msg, sig, group=8, scalars=_seeded(dev, N)).cpu().numpy()
    want = np.ones(N, np.int32)
    want[N - 1] = 0
    assert np.array_equal(got, want)


def test_fast_aggregate_verify_fixtures(pkg, dev):
    """the 11 fast_aggregate_verify fixtures: the registry holds the fixture's keys and the list names all of them; the fixture with no key is the
    empty list over a registry of one unrelated key (a registry of size 0 is refused)"""
    cases = eth_cases("fast_aggregate_verify")
    assert len(cases) == 11
    done = 0
    for name, c in cases:
        i = c["input"]
        pks, m, sig = [unhex(p) for p in i["pubkeys"]], unhex(i["message"]), unhex(i["signature"])
        assert len(sig) == 96 and len(m) == 32 and all(len(p) == 48 for p in pks)
        reg = pkg.KeyRegistry(max(1, len(pks)), device=dev)
        if not pks:
            with pytest.raises(pkg.BlswError):
                _verify(pkg, dev, reg, [[]], _t(dev, [m], 32), _t(dev, [sig], 96))
            reg.append(_keys(pkg, dev)[1][:1].contiguous())
        else:
            reg.append(_t(dev, pks, 48))
        res, st = _verify(pkg, dev, reg, [list(range(len(pks)))], _t(dev, [m], 32), _t(dev, [sig], 96), want_status=True)
        got = bool(res[0].item())
        assert got == c["output"], name
        assert pks or st[0, 0].item() == ST_IDENTITY
        done += got
        reg.close()
    assert done >= 3


def test_cpp_host_mirror(pkg, dev, oracle, registry, tmp_path):
    """BLS::KeyRegistry, BLS::fast_aggregate_verify_indexed and its _grouped form (include/blsw.hpp) from a C++ host (tests/registry/cpp_caller) equal
    the Python calls"""
    import os
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "registry"), "cpp_caller"])
    _, pk48 = _keys(pkg, dev)
    lists, msg, sig, expect = _batch(pkg, dev, oracle, 11)
    lists = [list(x) for x in lists]
    lists[20][0] = SIZE  # a bad index too
    res, st, agg = _verify(pkg, dev, registry, lists, msg, sig, want_status=True, want_aggregate=True)
    groups = _verify(pkg, dev, registry, lists, msg, sig, group=8, scalars=_seeded(dev, N)).cpu().numpy()  # the C++ side draws its own coefficients: P1 / P2 make the verdicts equal
    expect = expect.copy()
    expect[20] = False
    assert np.array_equal(res.cpu().numpy().astype(bool), expect) and np.array_equal(groups.astype(bool), [expect[g:g + 8].all() for g in range(0, N, 8)])
    hexs = lambda t: [bytes(r).hex() for r in t.cpu().numpy()]
    f = tmp_path / "registry.txt"
    f.write_text(" ".join(hexs(pk48)) + "\n" + "".join("%s %s %s\n" % (",".join(str(k) for k in lst) or "-", m, s) for lst, m, s in zip(lists, hexs(msg), hexs(sig))))
    out = subprocess.check_output([os.path.join(here, "registry", "cpp_caller"), str(f), "8", str(CAPACITY)], text=True, timeout=120).split("\n")
    res, st, agg = res.cpu().numpy(), st.cpu().numpy(), hexs(agg)
    for i in range(N):
        v, via, s0, s1, a = out[i].split()
        assert (int(v), int(via), int(s0), int(s1), a) == (res[i], res[i], st[i, 0], st[i, 1], agg[i]), i
    assert st[20, 0] == ST_BAD_INDEX
    assert out[N].split() == ["groups"] + [str(g) for g in groups] and out[N + 1].split() == ["keys"] + ["0"] * SIZE


def test_two_calls_on_a_side_stream_agree(pkg, dev, oracle, registry, tmp_path):
    """the appends and the call on a non-default stream, twice per mode, in a child process (tests/registry_stream_worker.py says why a process of
    its own): the two calls agree, and they give what this process gets on the default stream"""
    import json
    import os
    import subprocess
    import sys

    _, pk48 = _keys(pkg, dev)
    lists, msg, sig, expect = _batch(pkg, dev, oracle, 11)
    idx, off = csr(lists)
    sc = _seeded(dev, N)
    f = tmp_path / "batch.npz"
    np.savez(f, pks48=pk48.cpu().numpy(), indices=idx.view(np.int32), offsets=off.view(np.int64), msg=msg.cpu().numpy(), sig=sig.cpu().numpy(), scalars=sc.cpu().numpy(), group=8,
             capacity=CAPACITY, cut=64)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output([sys.executable, "-m", "tests.registry_stream_worker", str(f)], cwd=root, text=True, timeout=120)
    got = json.loads(out.strip().split("\n")[-1])
    res, st, agg = _verify(pkg, dev, registry, lists, msg, sig, want_status=True, want_aggregate=True)
    groups = _verify(pkg, dev, registry, lists, msg, sig, group=8, scalars=sc)
    assert got["same"] and got["size"] == SIZE and np.array_equal(np.array(got["verdicts"], bool), expect)
    assert (got["verdicts"], got["status"], got["key_status"]) == (res.tolist(), st.tolist(), registry.key_status().tolist())
    assert got["aggregate"] == [bytes(r).hex() for r in agg.cpu().numpy()]
    assert got["groups"] == groups.tolist() == [int(expect[g:g + 8].all()) for g in range(0, N, 8)]


@pytest.mark.parametrize("group", [0, 8])
def test_outputs_and_the_registry_stay_between_their_sentinels(pkg, dev, oracle, registry, group):
    """the C entry points with the registry's buffer and every output carved out of sentinel-filled buffers, guards on both sides of each: nothing
    but the appended rows and the outputs changes, the outputs are the wrapper's; then the rules that need a live handle"""
    import torch

    L = pkg.lib()
    _, pk48 = _keys(pkg, dev)
    lists, msg, sig, _ = _batch(pkg, dev, oracle, 11)
    idx, off = csr(lists)
    ti, to = _i32(dev, idx), _i64(dev, off)
    sc = _seeded(dev, N) if group else None
    n_res = (N + group - 1) // group if group else N
    GUARD, S32, S8 = 64, 0x5A5A5A5A, 0xA5
    rb = ctypes.c_uint64(0)
    assert L.blsw_registry_bytes(CAPACITY, ctypes.byref(rb)) == 0
    buf = torch.full((256 + rb.value + 256,), S8, dtype=torch.uint8, device=dev)  # the allocator's blocks are 512-byte aligned: + 256 stays aligned
    h = ctypes.c_void_p()
    assert L.blsw_registry_create(ctypes.byref(h), CAPACITY, 0, buf.data_ptr() + 256, rb.value) == 0 and h.value
    stream = torch.cuda.current_stream(dev).cuda_stream
    sizes = [n_res, 2 * N]  # result, status (int32 words)
    offs, o = [], GUARD
    for w in sizes:
        offs.append(o)
        o += w + GUARD
    words = torch.full((o,), S32, dtype=torch.int32, device=dev)
    agg = torch.full((GUARD + N * 48 + GUARD,), S8, dtype=torch.uint8, device=dev)
    wb = ctypes.c_uint64(0)
    assert L.blsw_registry_verify_workspace_bytes(N, 32, group, ctypes.byref(wb)) == 0
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    ptr = lambda k: words.data_ptr() + 4 * offs[k]

    NOT_GIVEN = object()  # None is a value here: a NULL pointer

    def call(r=h, indices=ti.data_ptr(), n_indices=len(idx), offsets=to.data_ptr(), workspace=ws, scalars=NOT_GIVEN, grp=group, sig96=sig.data_ptr(), m=msg.data_ptr(), msg_len=32,
             n=N, result=NOT_GIVEN, status=NOT_GIVEN, ws_ptr=NOT_GIVEN):
        scalars = (sc.data_ptr() if group else None) if scalars is NOT_GIVEN else scalars
        result, status = ptr(0) if result is NOT_GIVEN else result, ptr(1) if status is NOT_GIVEN else status
        ws_ptr = workspace.data_ptr() if ws_ptr is NOT_GIVEN else ws_ptr
        return L.blsw_registry_verify_batch(r, indices, n_indices, offsets, sig96, m, msg_len, n, scalars, grp, result, status, agg.data_ptr() + GUARD, ws_ptr, workspace.numel(),
                                            stream)

    n32 = ctypes.c_uint32(9)
    assert call() == 1 and L.blsw_registry_size(h, ctypes.byref(n32)) == 0 and n32.value == 0  # a registry of size 0
    assert L.blsw_registry_append(h, pk48.data_ptr(), 64, stream) == 0 and L.blsw_registry_append(h, pk48[64:].data_ptr(), SIZE - 64, stream) == 0
    # append's rules: nothing is launched and the size stays
    for args in ((h, None, 4), (h, pk48.data_ptr(), 0), (h, pk48.data_ptr(), CAPACITY - SIZE + 1), (h, pk48.data_ptr(), 0xFFFFFFFF)):
        assert L.blsw_registry_append(*args, stream) == 1, args[2]
    assert L.blsw_registry_size(h, ctypes.byref(n32)) == 0 and n32.value == SIZE and L.blsw_registry_size(h, None) == 1 and L.blsw_registry_key_status(h, None) == 1
    # the call's rules, before anything is written
    p = ti.data_ptr()
    assert call(indices=None) == 1 and call(n_indices=(1 << 40) + 1) == 1 and call(offsets=None) == 1 and call(r=None) == 1
    assert call(scalars=None if group else p, grp=group) == 1 and call(grp=65536, scalars=p) == 1
    # ... the committee entry's own bounds and NULLs, each alone with a live handle and everything else valid
    for kw in (dict(n=0), dict(n=0x80000000), dict(msg_len=65536), dict(sig96=None), dict(result=None), dict(status=None), dict(ws_ptr=None), dict(m=None)):
        assert call(**kw) == 1, kw
    small = torch.full((wb.value - 1,), S8, dtype=torch.uint8, device=dev)
    assert call(workspace=small) == 2
    torch.cuda.synchronize(dev)
    assert bool((small == S8).all().item()) and bool((words == S32).all().item()) and bool((agg == S8).all().item())
    assert call() == 0
    torch.cuda.synchronize(dev)
    ref = pkg.registry_verify(registry, ti, to, msg, sig, group=group, scalars=sc, want_status=True, want_aggregate=True)
    w, a = words.cpu().numpy(), agg.cpu().numpy()
    keep = np.ones(len(w), bool)
    for at, size, r in zip(offs, sizes, [ref[0], ref[1].flatten()]):
        assert np.array_equal(w[at:at + size], r.cpu().numpy()), at
        keep[at:at + size] = False
    assert (w[keep] == S32).all() and keep.sum() == GUARD * (len(sizes) + 1)
    assert (a[:GUARD] == S8).all() and (a[-GUARD:] == S8).all() and np.array_equal(a[GUARD:-GUARD].reshape(N, 48), ref[2].cpu().numpy())
    # the registry's buffer: the guards, and every row and status entry at or beyond the size, are as they were; the rows below are the shared registry's
    b = buf.cpu().numpy()
    sp = ctypes.c_void_p()
    assert L.blsw_registry_key_status(h, ctypes.byref(sp)) == 0
    st_off = sp.value - buf.data_ptr()
    assert (b[:256] == S8).all() and (b[256 + rb.value:] == S8).all() and 256 + 128 * CAPACITY <= st_off and st_off + 4 * CAPACITY <= 256 + rb.value
    assert (b[256 + 128 * SIZE:st_off] == S8).all() and (b[st_off + 4 * SIZE:] == S8).all()
    assert np.array_equal(b[256:256 + 128 * SIZE], registry.buffer[:128 * SIZE].cpu().numpy()) and not b[st_off:st_off + 4 * SIZE].any()
    assert L.blsw_registry_destroy(h) == 0
