"""blsw_registry_* without a GPU: the stages of csrc/registry.hpp compiled for the host (tests/registry) — the decode into records, the lane walks
over index lists for L lanes, the tree and the affine / status / compression step — against the CPU oracle's PublicKey::aggregate of the gathered
keys, byte for byte, for every L; permuted lists; the committee form on the same selection; the group law's edges inside a lane and inside the
tree; bad entries and bad offsets; appending in parts; and the argument rules of the entry points that precede any HIP call. A handle cannot be made
without a device (blsw_registry_create answers BLSW_ERR_NO_DEVICE, as blsw_keyset_create does), so the rules that need a live handle — append's
capacity rule, the call's size == 0, n_indices and BLSW_ERR_WORKSPACE — are exercised in tests/test_registry_gpu.py."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import committee_lib, registry_lib
from tests.registry_lib import ST_BAD_INDEX, ST_IDENTITY, ST_OK, HostRegistry, csr, list_lengths

LANES = [1, 2, 4, 8, 16, 32, 64]
N_KEYS, CAPACITY = 130, 200


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def _sk(i):
    return 0x1000003 + 7919 * i


@pytest.fixture(scope="module")
def registry(oracle):
    """130 keys minted by the oracle (the committee tests' progression: partial sums of two lanes can coincide) in a registry of capacity 200,
    appended at once; computed once and never changed"""
    pks = tuple(oracle.sk_to_pk(_sk(i)) for i in range(N_KEYS))
    reg = HostRegistry(CAPACITY).append(list(pks))
    assert reg.size == N_KEYS and not reg.key_status().any()
    for k in (0, 1, 64, 129):  # the records hold the oracle's affine coordinates
        ost, oxy, oinf = oracle.g1_decompress(pks[k])
        assert ost == 0 and not oinf and np.array_equal(reg.xy(k), oxy)
    reg.records.setflags(write=False)
    reg.status.setflags(write=False)
    return pks, reg


def _check(oracle, pks, reg, lists, L):
    """every output of the sum stage against the oracle, for one L; returns the outputs"""
    idx, off = csr(lists)
    pk_xy, status, agg = registry_lib.sums(reg, idx, off, L)
    kst = reg.key_status()
    for i, lst in enumerate(lists):
        est, eagg = registry_lib.expected(oracle, pks, kst, reg.size, lst)
        assert (int(status[i]), agg[i]) == (est, eagg), (L, i, len(lst))
        if est == ST_OK:
            ost, oxy, oinf = oracle.g1_decompress(eagg)
            assert ost == 0 and not oinf and np.array_equal(pk_xy[i], oxy), (L, i)
        else:
            assert not pk_xy[i].any()
    return pk_xy, status, agg


def _random_lists(L, seed):
    """one list per length in 0, 1, L - 1, L, L + 1, 2 L + 1, 3 L: indices drawn with repetition"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, N_KEYS, size=m).tolist() for m in list_lengths(L)]


@pytest.mark.parametrize("L", LANES)
def test_sum_equals_the_oracles_aggregate_and_ignores_the_order(oracle, registry, L):
    pks, reg = registry
    lists = _random_lists(L, 4000 + L)
    pk_xy, status, agg = _check(oracle, pks, reg, lists, L)
    assert status.tolist() == [ST_IDENTITY] + [ST_OK] * (len(lists) - 1)
    permuted = [lst[::-1][1:] + lst[::-1][:1] for lst in lists]  # reversed, then rotated by one: every entry of a longer list changes its lane
    assert permuted[-1] != lists[-1] and sorted(permuted[-1]) == sorted(lists[-1])
    idx, off = csr(permuted)
    got = registry_lib.sums(reg, idx, off, L)
    assert np.array_equal(got[0], pk_xy) and np.array_equal(got[1], status) and got[2] == agg


def test_every_L_gives_identical_outputs(registry):
    """the output is affine: neither L nor the order of the tree shows in it"""
    _, reg = registry
    idx, off = csr(_random_lists(16, 99) + _random_lists(5, 98))
    ref = registry_lib.sums(reg, idx, off, 1)
    for L in LANES[1:]:
        got = registry_lib.sums(reg, idx, off, L)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == ref[2], L


@pytest.mark.parametrize("L", LANES)
def test_ascending_indices_of_a_bitmap_row_equal_the_committee_form(registry, L):
    pks, reg = registry
    K = 65
    rng = np.random.default_rng(700 + L)
    rows = [np.zeros(K, np.uint8), np.ones(K, np.uint8)] + [(rng.random(K) < d).astype(np.uint8) for d in (0.5, 0.9, 0.1)]
    bitmap = np.stack(rows)
    c_xy, c_st, c_count, c_agg = committee_lib.sums(committee_lib.decode(pks[:K]), bitmap, L)
    lists = [np.flatnonzero(r).tolist() for r in rows]
    idx, off = csr(lists)
    r_xy, r_st, r_agg = registry_lib.sums(reg, idx, off, L)
    assert np.array_equal(r_xy, c_xy) and np.array_equal(r_st, c_st) and r_agg == c_agg and c_count.tolist() == [len(x) for x in lists]


@pytest.fixture(scope="module")
def edges(oracle):
    pks, sks, names = registry_lib.edge_registry(oracle)
    reg = HostRegistry(len(pks) + 8).append(pks)
    kst = reg.key_status().tolist()
    for k, p in enumerate(pks):  # the append's statuses are the oracle's
        ost, _, oinf = oracle.g1_decompress(p)
        assert kst[k] == (ST_IDENTITY if (ost == 0 and oinf) else ost), k
    assert [kst[names["bad%d" % s]] for s in (1, 2, 3)] == [1, 2, 3] and kst[names["torsion"]] == 3 and kst[names["identity"]] == ST_IDENTITY
    return pks, names, reg


@pytest.mark.parametrize("L", LANES)
def test_group_law_edges_and_bad_entries(oracle, edges, L):
    pks, names, reg = edges
    cases = registry_lib.edge_lists(L, names, reg.size, reg.capacity)
    lists = [c[1] for c in cases]
    _, status, agg = _check(oracle, pks, reg, lists, L)  # all in one call: a set's neighbours are unaffected
    seen = {}
    for (name, lst, want), st, a in zip(cases, status, agg):
        if want is not None:
            assert int(st) == want, (L, name)
        seen[name.split(":")[0]] = (int(st), a)
    P, Q = pks[names["P"]], pks[names["Q"]]
    two_p = oracle.aggregate_g1([P, P])
    # what the cases were set up to meet, stated directly
    fillers = [pks[k % registry_lib.BASE_KEYS] for k in range(2 * L + 1)]
    rest = [f for p, f in enumerate(fillers) if p not in (0, L, 2 * L)]
    assert seen["the same index at positions 0 and L, then Q in the lane"] == (ST_OK, oracle.aggregate_g1([two_p, Q] + rest))
    assert seen["the same index at positions 0 and 1, nothing else"] == (ST_OK, two_p)
    assert seen["a key, its negation and Q in one lane"] == (ST_OK, oracle.aggregate_g1([Q] + rest))
    assert seen["a key and its negation in two lanes"] == (ST_IDENTITY, committee_lib.IDENTITY48)
    assert seen["an identity key among others"] == (ST_OK, oracle.aggregate_g1([pks[0], pks[1]]))
    assert seen["an identity key alone"] == (ST_IDENTITY, committee_lib.IDENTITY48)
    assert seen["one index 3 L times"][0] == ST_OK
    for name in ("index == size", "index == 0xffffffff", "an index >= size below the capacity", "a bad index then a bad key"):
        assert seen[name] == (ST_BAD_INDEX, bytes(48)), name


@pytest.mark.parametrize("L", LANES)
def test_bad_offsets_fail_their_own_set_only(oracle, registry, L):
    pks, reg = registry
    good = list(range(2 * L + 1))
    est, eagg = registry_lib.expected(oracle, pks, reg.key_status(), reg.size, good)
    idx = np.array(good + good, dtype=np.uint32)
    m = len(good)
    for name, off in (("descending offsets", [0, m, m - 1, 2 * m - 1]), ("an offset beyond n_indices", [0, m, 2 * m + 1, 2 * m + 1]),
                      ("both offsets beyond n_indices", [0, m, 2 * m + 5, 2 * m + 9]), ("an offset of 2^63", [0, m, 2**63, 2**63 + m])):
        # the sets around the bad one: the first is `good`; the third has bad offsets too in all but the first case, where it is [m - 1, 2 m - 1)
        pk_xy, status, agg = registry_lib.sums(reg, idx, np.array(off, dtype=np.uint64), L)
        assert (int(status[0]), agg[0]) == (est, eagg) and est == ST_OK, name
        assert (int(status[1]), agg[1]) == (ST_BAD_INDEX, bytes(48)) and not pk_xy[1].any(), name
        if name == "descending offsets":
            lst = idx[m - 1:2 * m - 1].tolist()
            assert (int(status[2]), agg[2]) == registry_lib.expected(oracle, pks, reg.key_status(), reg.size, lst), name
        else:
            assert (int(status[2]), agg[2]) == (ST_BAD_INDEX, bytes(48)), name
    # n_indices smaller than the array: an offset the array could serve is still beyond the list
    _, status, _ = registry_lib.sums(reg, idx, np.array([0, m, 2 * m], dtype=np.uint64), L, n_indices=2 * m - 1)
    assert status.tolist() == [ST_OK, ST_BAD_INDEX]


def test_appending_in_two_parts_equals_appending_at_once(oracle, registry):
    pks, whole = registry
    for cut in (1, 64, 129):
        parts = HostRegistry(CAPACITY).append(list(pks[:cut]))
        assert parts.size == cut
        # between the appends: an index of the second part is beyond the size, whatever its row holds
        _, status, _ = registry_lib.sums(parts, np.array([0, cut], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint64), 4)
        assert status.tolist() == [ST_OK, ST_BAD_INDEX]
        parts.append(list(pks[cut:]))
        n = N_KEYS * registry_lib.RECORD_BYTES
        assert parts.size == N_KEYS and np.array_equal(parts.records[:n], whole.records[:n]) and np.array_equal(parts.key_status(), whole.key_status())
    # a call made with the size of an earlier moment reads no row at or beyond it, though the rows are there by now
    _, status, _ = registry_lib.sums(whole, np.array([63, 64], dtype=np.uint32), np.array([0, 1, 2], dtype=np.uint64), 4, size=64)
    assert status.tolist() == [ST_OK, ST_BAD_INDEX]


def test_verdict_end_to_end_on_the_host(oracle, registry):
    """three sets over the registry, one with a repeated index: the shim's sums through the oracle's verify"""
    pks, reg = registry
    lists = [[5, 9, 100], [7, 7, 8], [129]]
    msgs = [bytes([0x40 + i]) * 32 for i in range(3)]
    sigs = [oracle.sign(sum(_sk(k) for k in lst) % committee_lib.R_MOD, m) for lst, m in zip(lists, msgs)]
    idx, off = csr(lists)
    _, status, agg = registry_lib.sums(reg, idx, off, 4)
    assert not status.any() and [oracle.verify_bytes(a, m, s) for a, m, s in zip(agg, msgs, sigs)] == [True] * 3
    idx[4] = 8  # [7, 8, 8]: another multiset than was signed
    _, status, agg = registry_lib.sums(reg, idx, off, 4)
    assert not status.any() and [oracle.verify_bytes(a, m, s) for a, m, s in zip(agg, msgs, sigs)] == [True, False, True]


def test_argument_rules_without_a_gpu(pkg):
    L = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    lanes = H["defines"]["BLSW_REGISTRY_LANES"]
    assert pkg.REGISTRY_LANES == lanes and 1 <= lanes <= 64 and lanes & (lanes - 1) == 0
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17  # new symbols only
    assert pkg.ST_BAD_INDEX == H["defines"]["BLSW_ST_BAD_INDEX"] == ST_BAD_INDEX == 6
    for name in ("blsw_registry_bytes", "blsw_registry_create", "blsw_registry_append", "blsw_registry_size", "blsw_registry_key_status", "blsw_registry_destroy",
                 "blsw_registry_verify_workspace_bytes", "blsw_registry_verify_batch"):
        assert name in pkg.EXPORTED_SYMBOLS and getattr(L, name).argtypes
    for name in ("KeyRegistry", "registry_verify", "registry_verify_grouped"):
        assert callable(getattr(pkg, name))
    ERR_ARG = 1
    p = ctypes.c_void_p(0x1000)  # 256-byte aligned, never dereferenced: the calls fail before any device work
    b = ctypes.c_uint64(0)
    # blsw_registry_bytes: capacity 1 .. 2^24; records of 128 bytes and the status array
    assert L.blsw_registry_bytes(0, ctypes.byref(b)) == ERR_ARG and L.blsw_registry_bytes((1 << 24) + 1, ctypes.byref(b)) == ERR_ARG
    assert L.blsw_registry_bytes(16, None) == ERR_ARG
    last = 0
    for cap in (1, 2, 63, 64, 65, 200, 1 << 20, 1 << 24):
        assert L.blsw_registry_bytes(cap, ctypes.byref(b)) == 0 and b.value >= cap * 132 and b.value >= last and b.value % 256 == 0
        last = b.value
    assert L.blsw_registry_bytes(1 << 20, ctypes.byref(b)) == 0 and b.value < 256 << 20  # a 2^20-key table fits the 256 MiB Infinity Cache
    # blsw_registry_create
    assert L.blsw_registry_bytes(200, ctypes.byref(b)) == 0
    h = ctypes.c_void_p()
    for args in ((None, 200, -1, p, b.value), (ctypes.byref(h), 0, -1, p, b.value), (ctypes.byref(h), (1 << 24) + 1, -1, p, 1 << 40), (ctypes.byref(h), 200, -1, None, b.value),
                 (ctypes.byref(h), 200, -1, p, b.value - 1), (ctypes.byref(h), 200, -1, ctypes.c_void_p(0x1080), b.value)):
        assert L.blsw_registry_create(*args) == ERR_ARG and not h.value, args
    rc = L.blsw_registry_create(ctypes.byref(h), 200, -1, p, b.value)  # valid arguments: no device here, or a handle on a GPU box
    assert rc != ERR_ARG and (rc == 0) == bool(h.value)
    if h.value:
        assert L.blsw_registry_destroy(h) == 0
    # the entry points that take a handle refuse a NULL one
    n32, sp = ctypes.c_uint32(7), ctypes.c_void_p()
    assert L.blsw_registry_append(None, p, 4, None) == ERR_ARG
    assert L.blsw_registry_size(None, ctypes.byref(n32)) == ERR_ARG and n32.value == 7
    assert L.blsw_registry_key_status(None, ctypes.byref(sp)) == ERR_ARG and not sp.value
    assert L.blsw_registry_destroy(None) == ERR_ARG
    assert L.blsw_registry_verify_batch(None, p, 64, p, p, p, 32, 8, None, 0, p, p, p, p, 1 << 40, None) == ERR_ARG
    # blsw_registry_verify_workspace_bytes: the committee entry's bounds, without n_keys
    for n, msg_len, group in ((0, 32, 0), (0x80000000, 32, 0), (64, 65536, 0), (64, 32, 65536), (0, 32, 8)):
        assert L.blsw_registry_verify_workspace_bytes(n, msg_len, group, ctypes.byref(b)) == ERR_ARG
    assert L.blsw_registry_verify_workspace_bytes(64, 32, 0, None) == ERR_ARG
    assert L.blsw_registry_verify_workspace_bytes(64, 0, 65535, ctypes.byref(b)) == 0  # a group beyond n is one group


def test_workspace_is_the_verifiers_without_a_table(pkg):
    L = pkg.lib()
    b, v, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    for group in (0, 1, 64):
        last = 0
        for n in (1, 2, 63, 64, 65, 1000, 1024, 1025, 8192, 65536):
            assert L.blsw_registry_verify_workspace_bytes(n, 32, group, ctypes.byref(b)) == 0 and b.value >= last
            last = b.value
            if group == 0:
                assert L.blsw_verify_workspace_bytes(n, 32, ctypes.byref(v)) == 0
            else:
                assert L.blsw_verify_groups_workspace_bytes(n, 32, group, ctypes.byref(v)) == 0
            assert b.value == v.value  # the chosen verifier's offsets and the hash's carve, nothing else
            assert L.blsw_committee_verify_workspace_bytes(n, 32, 512, group, ctypes.byref(c)) == 0 and c.value == b.value + 2 * 512 * 48
