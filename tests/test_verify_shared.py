"""blsw_verify_groups_shared_batch / blsw_registry_verify_shared_batch without a GPU: the run rule of csrc/vshared.hpp against a restatement in
Python, exhaustively over short index arrays; the shared stages composed on the host (tests/vshared) against the plain stages on materialised
messages; and the argument and workspace rules of the four entry points, which precede any HIP call.

What "the same GT value" means here: the plain and the shared form multiply different Miller functions — prod_i f(P_i, H) against f(sum_i P_i, H) —
which differ by a factor the final exponentiation removes. So the products of the partials BEFORE the final exponentiation are compared bit for bit
where every run is one instance (there the two forms walk the same lines), and everywhere their quotient is checked to go to one under the final
exponentiation: the same element of GT."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

from tests import vgroups_lib, vshared_lib
from tests.vshared_lib import SENTINEL

ST_BAD_INDEX = 6


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def _rule_py(index, group, chunk, n_msgs):
    """the statement of include/blsw.h, written the slow way"""
    n = len(index)
    n_groups = (n + group - 1) // group
    cpg = (min(group, n) + chunk - 1) // chunk
    leader = [i % group == 0 or index[i] != index[i - 1] for i in range(n)]
    slot_leader, slot_len, runs = [SENTINEL] * n, [SENTINEL] * n, []
    for g in range(n_groups):
        lo, hi = g * group, min(n, (g + 1) * group)
        heads = [i for i in range(lo, hi) if leader[i]]
        for k, i in enumerate(heads):
            slot_leader[lo + k] = i
            slot_len[lo + k] = (heads[k + 1] if k + 1 < len(heads) else hi) - i
        runs.append(len(heads))
    first, count, walks = [], [], []
    for g in range(n_groups):
        for q in range(cpg):
            c = max(0, min(runs[g], (q + 1) * chunk) - q * chunk)
            first.append(g * group + (q * chunk if c else 0))
            count.append(c)
            walks.append(True)  # every team walks: vshared.hpp, vs_chunk_walks
    return dict(leader=leader, slot_leader=slot_leader, slot_len=slot_len, runs=runs, bad=[i >= n_msgs for i in index], chunk_first=first, chunk_count=count, chunk_walks=walks)


def _same(got, want, ctx):
    for k, v in want.items():
        assert got[k].astype(np.int64).tolist() == [int(x) for x in v], (k, ctx)


def test_run_rule_exhaustive():
    """every index array of length <= 7 over {0, 1, 2}, group 1 .. 4, chunk 1 .. 3, in tiles of a whole wave and of two lanes (so that runs cross tiles)"""
    for n in range(1, 8):
        for index in itertools.product((0, 1, 2), repeat=n):
            for group in (1, 2, 3, 4):
                for chunk in (1, 2, 3):
                    want = _rule_py(index, group, chunk, 2)
                    for tile in (64, 2):
                        _same(vshared_lib.rule(index, group, chunk, tile=tile, n_msgs=2), want, (index, group, chunk, tile))


def test_run_rule_long_groups_cross_tiles():
    """groups longer than a tile: runs that span one, two and many tiles, a leader in a tile's first and last lane, a group that ends on a tile's edge"""
    rng = np.random.default_rng(11)
    for group, n in ((200, 470), (128, 128), (65, 131), (64, 129)):
        for p in (0.0, 0.02, 0.5, 1.0):
            index = np.cumsum(rng.random(n) < p).astype(np.uint32)
            for chunk in (8, 31):
                _same(vshared_lib.rule(index, group, chunk, n_msgs=3), _rule_py(index.tolist(), group, chunk, 3), (group, n, p, chunk))
    for index in ([5] * 63 + [6] * 66 + [5], [1] + [2] * 127 + [3], [0xFFFFFFFF] * 64 + [0xFFFFFFFE] * 64):
        _same(vshared_lib.rule(index, 200, 8, n_msgs=3), _rule_py(index, 200, 8, 3), index[:2])


@pytest.fixture(scope="module")
def nine(oracle):
    """a table of three rows and, per row, nine valid signatures by nine keys: computed once and never changed"""
    table = [bytes([0x50 + r]) * 32 for r in range(3)]
    minted = [[vgroups_lib.mint(oracle, 0x2345678 + 991 * k, m) for k in range(9)] for m in table]
    return tuple(table), tuple(minted[0][k][0] for k in range(9)), tuple(tuple(minted[r][k][1] for k in range(9)) for r in range(3))


SCALARS = [1, 2**64 - 1, 2**63, 3, 0xFFFFFFFF00000001, 5, 7, 11, 13]


def _check(out, want_res, want_runs):
    assert out["res_shared"].tolist() == out["res_plain"].tolist() == want_res
    assert out["runs"].tolist() == want_runs and out["same_gt"].tolist() == [1] * len(want_res)
    assert np.array_equal(out["st_shared"], out["st_plain"]) and not out["st_shared"].any()


@pytest.mark.parametrize("chunk", [8, 2])
def test_host_stages_equal_the_plain_stages(nine, chunk):
    table, pks, sigs = nine
    # group 0: one run of 9 (one run per group; its instances cross the plain form's chunk edge); group 1: nine runs, slots 0 .. 8 (one run per
    # instance: slot 8 lies in the second chunk of eight)
    index = [1] * 9 + [0, 1, 2, 0, 1, 2, 0, 1, 2]
    out = vshared_lib.groups(pks + pks, [sigs[r][k] for k, r in enumerate(index[:9])] + [sigs[r][k] for k, r in enumerate(index[9:])], table, index, SCALARS + SCALARS, 9, chunk)
    _check(out, [1, 1], [1, 9])
    assert not np.array_equal(out["f_shared"][0], out["f_plain"][0])  # other Miller functions, the same element of GT
    assert np.array_equal(out["f_shared"][1], out["f_plain"][1])  # one run per instance: the same lines, bit for bit
    # A B A and A A B B B in groups of five, one signature of the second group over another row than its index names
    index = [0, 1, 0, 0, 2, 2, 2, 1, 1, 1]
    signed = list(index)
    signed[8] = 0
    out = vshared_lib.groups(pks + pks[:1], [sigs[r][k % 9] for k, r in enumerate(signed)], table, index, SCALARS + [17], 5, chunk, tile=2)
    _check(out, [1, 0], [4, 2])


def test_host_stages_bad_index_doubling_and_cancellation(oracle, nine):
    table, pks, sigs = nine
    # an index at n_msgs and one at 2^32 - 1: ST_BAD_INDEX in front, their groups 0, no row read; the third group passes
    index = [0, 3, 1, 0xFFFFFFFF, 2, 2]
    out = vshared_lib.groups(pks[:6], [sigs[min(r, 2)][k] for k, r in enumerate(index)], table, index, SCALARS[:6], 2, 8)
    assert out["res_shared"].tolist() == [0, 0, 1] and out["runs"].tolist() == [2, 2, 1]
    assert out["st_shared"].tolist() == [[0, 0], [ST_BAD_INDEX, 0], [0, 0], [ST_BAD_INDEX, 0], [0, 0], [0, 0]] and not out["st_plain"].any()
    # the same (key, scalar) twice in a run: the doubling branch of the merge
    out = vshared_lib.groups([pks[0], pks[0], pks[1]], [sigs[0][0], sigs[0][0], sigs[0][1]], table, [0, 0, 0], [9, 9, 5], 3, 8)
    _check(out, [1], [1])
    # sk and r - sk with equal scalars in one run: R and S_g are both the identity, a group with no pair passes; a tampered third fails it
    sk, m = 0xC0FFEE, table[0]
    pk_a, sig_a = vgroups_lib.mint(oracle, sk, m)
    pk_b, sig_b = vgroups_lib.mint(oracle, vgroups_lib.R_MOD - sk, m)
    _check(vshared_lib.groups([pk_a, pk_b], [sig_a, sig_b], table, [0, 0], [7, 7], 2, 8), [1], [1])
    _check(vshared_lib.groups([pk_a, pk_b, pks[2]], [sig_a, sig_b, sigs[0][2]], table, [0, 0, 0], [7, 7, 5], 3, 8), [1], [1])
    _check(vshared_lib.groups([pk_a, pk_b, pks[2]], [sig_a, sig_b, sigs[0][2]], table, [0, 0, 1], [7, 7, 5], 3, 8), [0], [2])


def test_argument_rules_without_a_gpu(pkg):
    L = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17 and pkg.ST_BAD_INDEX == ST_BAD_INDEX
    ERR_ARG = 1
    p = ctypes.c_void_p(0x1000)  # never dereferenced: the calls fail before any device work
    empty = pkg.blsw_dst_t()  # a tag of length 0
    good = dict(r=p, ind=p, n_ind=10, off=p, pk=p, sig=p, msgs=p, msg_len=32, n_msgs=4, idx=p, n=64, scalars=p, group=8, dst=None, res=p, runs=p, st=p, agg=p, ws=p)

    def plain(**kw):
        a = dict(good, **kw)
        return L.blsw_verify_groups_shared_batch(a["pk"], a["sig"], a["msgs"], a["msg_len"], a["n_msgs"], a["idx"], a["n"], a["scalars"], a["group"], a["dst"], a["res"], a["runs"],
                                                 a["st"], a["ws"], 1 << 40, None)

    def registry(**kw):
        a = dict(good, **kw)
        return L.blsw_registry_verify_shared_batch(a["r"], a["ind"], a["n_ind"], a["off"], a["sig"], a["msgs"], a["msg_len"], a["n_msgs"], a["idx"], a["n"], a["scalars"], a["group"],
                                                   a["dst"], a["res"], a["runs"], a["st"], a["agg"], a["ws"], 1 << 40, None)

    shared = (dict(group=0), dict(group=65536), dict(n=0), dict(n=0x80000000), dict(msg_len=65536), dict(sig=None), dict(scalars=None), dict(res=None), dict(st=None), dict(ws=None),
              dict(msgs=None), dict(n_msgs=0), dict(n_msgs=0x80000000), dict(idx=None), dict(dst=ctypes.byref(empty)))
    for kw in shared + (dict(pk=None),):
        assert plain(**kw) == ERR_ARG, kw
    for kw in shared + (dict(r=None), dict(off=None), dict(ind=None), dict(n_ind=(1 << 40) + 1)):
        assert registry(**kw) == ERR_ARG, kw
    b = ctypes.c_uint64(0)
    for size in (L.blsw_verify_groups_shared_workspace_bytes, L.blsw_registry_verify_shared_workspace_bytes):
        for n, n_msgs, msg_len, group in ((0, 4, 32, 8), (0x80000000, 4, 32, 8), (64, 0, 32, 8), (64, 0x80000000, 32, 8), (64, 4, 65536, 8), (64, 4, 32, 0), (64, 4, 32, 65536)):
            assert size(n, n_msgs, msg_len, group, ctypes.byref(b)) == ERR_ARG
        assert size(64, 4, 32, 8, None) == ERR_ARG
        assert size(5, 1, 0, 65535, ctypes.byref(b)) == 0  # a group beyond n is one group


def test_workspace_size_rules(pkg):
    """non-decreasing in n, n_msgs and msg_len; in `group` it follows the plain layout (whose per-group rows shrink as groups grow) plus arrays that do
    not grow with it; the hash's carve is over the table, so a call over few messages needs a fraction of the plain entry's workspace"""
    L = pkg.lib()
    b = ctypes.c_uint64(0)

    def size(n, n_msgs, msg_len, group, fn=L.blsw_verify_groups_shared_workspace_bytes):
        assert fn(n, n_msgs, msg_len, group, ctypes.byref(b)) == 0
        return b.value

    ns = (1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 65536)
    for group in (1, 8, 64, 200):
        for fixed in (1, 64, 65536):
            sizes = [size(n, fixed, 32, group) for n in ns]
            assert sizes == sorted(sizes), ("n", group, fixed)
            sizes = [size(fixed, m, 32, group) for m in ns]
            assert sizes == sorted(sizes), ("n_msgs", group, fixed)
        sizes = [size(1000, 100, msg_len, group) for msg_len in (0, 1, 31, 32, 33, 55, 56, 64, 65, 1000, 65535)]
        assert sizes == sorted(sizes), ("msg_len", group)
    plain = ctypes.c_uint64(0)
    for n, group in ((1024, 64), (65536, 64), (65536, 8), (70, 9)):
        assert L.blsw_verify_groups_workspace_bytes(n, 32, group, ctypes.byref(plain)) == 0
        assert size(n, 1, 32, group) < size(n, n // 8 + 1, 32, group) < size(n, n, 32, group)
        assert size(n, 1, 32, group) == size(n, 1, 32, group, L.blsw_registry_verify_shared_workspace_bytes)
        if n >= 1024:
            assert 4 * size(n, max(1, n // 64), 32, group) < plain.value  # no hash workspace per instance
        smaller = [size(n, 16, 32, g) for g in (1, 2, 8, 64, 65535)]  # as the plain layout: never larger for larger groups
        assert smaller == sorted(smaller, reverse=True)
