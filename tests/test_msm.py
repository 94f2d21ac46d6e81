"""blsw_msm_points_batch without a GPU: the stages of csrc/vmsm.hpp run on the host (tests/msm, lanes one after the other, the scatter's order a
parameter) against combine_lib.ref_combine — Python integers and the affine group law —, the stand-alone sanitizer program over the index
arithmetic, and the entry's argument rules on libblsw.so."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests import combine_lib as L
from tests import msm_lib as M

ERR_ARG, ERR_WORKSPACE = 1, 2


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def _check(names, out, st, want_out, want_st):
    assert st.tolist() == list(want_st), [(n, a, b) for n, a, b in zip(names, st.tolist(), want_st) if a != b]
    assert np.array_equal(out, want_out), [n for i, n in enumerate(names) if not np.array_equal(out[i], want_out[i])]


def test_shape_functions_and_digits():
    assert M.shape("segment", 0) == 32 and M.shape("segment", 0, "libmsm_seg4.so") == 4
    for c in range(1, 17):
        W = M.shape("windows", c)
        assert W == -(-255 // c) and M.shape("segments", c) == -(-(1 << c) // 32)
        for x in (0, 1, L.R - 1, (1 << 255) - 1, 0x0123456789ABCDEF << 100, (1 << c) - 1, 1 << c):
            got = [M.digit(x, w, c) for w in range(W)]
            assert got == [(x >> (c * w)) & ((1 << c) - 1) for w in range(W)], (c, hex(x))
            assert sum(d << (c * w) for w, d in enumerate(got)) == x
    assert [c for c in M.WINDOWS if 255 % c] == [2, 7, 8, 13, 16]  # a narrower top window
    last = 0
    for k in list(range(1, 300)) + [1 << e for e in range(9, 25)] + [(1 << e) - 1 for e in range(9, 25)]:
        c = M.shape("default_window", k)
        assert 1 <= c <= 16
        if k & (k - 1) == 0:
            assert c >= last
            last = c


@pytest.mark.parametrize("c", M.WINDOWS)
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("group", [1, 2])
def test_host_stages_on_the_combine_vectors(group, k, c):
    """every row of combine_vectors — bad terms, identity points, counts, failing lists — gives ref_combine's bytes and status. At 13 and 16 bits a
    list's buckets are 2^13 .. 2^16 points per window, so the rows go through the shim a few lists at a time."""
    names, points, scalars, counts, want_out, want_st = L.combine_vectors(group, k)
    step = len(names) if c <= 8 else 4 if c == 13 else 1
    for lo in range(0, len(names), step):
        sl = slice(lo, lo + step)
        out, st = M.host_msm(group, points[sl], scalars[sl], counts[sl], c)
        _check(names[sl], out, st, want_out[sl], want_st[sl])


@pytest.mark.parametrize("c", M.WINDOWS)
@pytest.mark.parametrize("group", [1, 2])
def test_bucket_edges_in_every_scatter_order(group, c):
    """the edge lists (msm_lib.edge_vectors) with the scatter's lanes forward, reversed and in a seeded random order: ref_combine's bytes each time. Up
    to 8 bits also with 4 buckets per segment, so that edge digits fall on the first and last bucket of a segment and into a partial last one."""
    for name, segment in (("libmsm.so", 32),) + ((("libmsm_seg4.so", 4),) if c <= 8 else ()):
        names, points, scalars, counts, want_out, want_st = M.edge_vectors(group, c, 130 if c <= 8 else 20, segment)
        assert {L.ST_OK, L.ST_BAD_ENCODING} == set(want_st) and bytes(want_out[3]) == L.IDENTITY[group]
        step = 3 if c <= 8 else 1
        for lo in range(0, len(names), step):
            sl = slice(lo, lo + step)
            for order in (None, "reversed", 0x5EED):
                out, st = M.host_msm(group, points[sl], scalars[sl], counts[sl], c, order, name)
                _check(names[sl], out, st, want_out[sl], want_st[sl])


@pytest.mark.parametrize("group", [1, 2])
def test_ragged_counts_across_three_lists(group):
    """counts 0, 1, k and k + 1 over n = 3 lists: a list's sorted indices and buckets start where the list in front of it ends"""
    k = 5
    names, points, scalars, _, _, _ = L.combine_vectors(group, k)
    rows = [names.index("random"), names.index("edge scalars"), names.index("the same term twice")]
    for counts in ((0, 1, k), (k + 1, k, 1), (k, k, k)):
        want = [L.ref_combine(group, list(points[r]), [int.from_bytes(bytes(x), "little") for x in scalars[r]], cnt) for r, cnt in zip(rows, counts)]
        for c in (0, 1, 3, 7):
            out, st = M.host_msm(group, points[rows], scalars[rows], counts, c, "reversed")
            assert st.tolist() == [w[0] for w in want] and [bytes(o) for o in out] == [w[1] for w in want], (counts, c)


def test_sanitizer_program():
    """tests/msm/edges_main: the same stages, stand-alone under the address and undefined-behaviour sanitizers, every array at its exact length"""
    here = os.path.join(L.HERE, "msm")
    subprocess.check_call(["make", "-s", "-C", here, "edges_main"])
    p = subprocess.run([os.path.join(here, "edges_main")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("0 failures") and "FAILED" not in p.stdout, p.stdout[-4000:]


def test_argument_rules_without_a_gpu(pkg):
    lib = pkg.lib()
    H = importlib.import_module("tools.gen_bindings").parse_header()
    assert lib.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] == 17
    assert {"blsw_msm_workspace_bytes", "blsw_msm_points_batch"} <= set(pkg.EXPORTED_SYMBOLS)
    bufs = {name: np.full(256, 0x5A, dtype=np.uint8) for name in ("in", "sc", "counts", "out", "st", "ws")}
    ptr = {name: ctypes.c_void_p(b.ctypes.data) for name, b in bufs.items()}
    good = dict(group=2, k=2, n=1, c=0, ws_bytes=1 << 62, **ptr)
    b = ctypes.c_uint64(0)

    def size(group, n, k, c=0):
        assert lib.blsw_msm_workspace_bytes(group, n, k, c, ctypes.byref(b)) == 0
        return b.value

    def msm(**kw):
        a = dict(good, **kw)
        return lib.blsw_msm_points_batch(a["group"], a["in"], a["sc"], a["counts"], a["k"], a["n"], a["c"], a["out"], a["st"], a["ws"], a["ws_bytes"], None)

    shapes = (dict(n=0), dict(k=0), dict(k=(1 << 24) + 1), dict(n=0x3FFFFFFF // 2 + 1), dict(n=0x40000000, k=1), dict(n=1 << 40, k=1), dict(n=(1 << 32) + 1, k=1),
              dict(c=17), dict(c=0xFFFFFFFF), dict(group=0), dict(group=3))
    for kw in shapes + tuple({name: None} for name in ("in", "sc", "out", "st", "ws")):
        assert msm(**kw) == ERR_ARG, kw
        if not set(kw) & set(ptr):
            a = dict(good, **kw)
            assert lib.blsw_msm_workspace_bytes(a["group"], a["n"], a["k"], a["c"], ctypes.byref(b)) == ERR_ARG, kw
    assert lib.blsw_msm_workspace_bytes(2, 1, 2, 0, None) == ERR_ARG
    # 65 536 terms: accepted here, refused by the combine entry
    assert size(1, 1, 65536) > 0 and size(2, 1, 1 << 24) > 0 and size(1, 0x3FFFFFFF, 1, 16) > 0
    assert lib.blsw_combine_points_workspace_bytes(1, 1, 65536, ctypes.byref(b)) == ERR_ARG
    for group in (1, 2):
        for c in (0, 1, 16):
            need = size(group, 3, 5, c)
            assert msm(group=group, n=3, k=5, c=c, ws_bytes=need - 1) == ERR_WORKSPACE and msm(group=group, n=3, k=5, c=c, ws_bytes=0) == ERR_WORKSPACE
    assert all((buf == 0x5A).all() for buf in bufs.values())
    # non-decreasing in n and in k at a fixed window_bits, 0 (the library's choice moves with k) included
    grid = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 1023, 1024, 1025, 4095, 4096, 32767, 32768, 65535, 65536, 65537, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, 1 << 20)
    for group in (1, 2):
        for c in (0, 1, 3, 7, 13, 16):
            for fixed in (1, 5, 64):
                last_n = last_k = 0
                for v in grid:
                    assert size(group, v, fixed, c) >= last_n and size(group, fixed, v, c) >= last_k, (group, c, fixed, v)
                    last_n, last_k = size(group, v, fixed, c), size(group, fixed, v, c)
    # the parts as the header states them, c = 12: W = 22, B = 4096
    per_term, jac = {1: 100 + 4 * 22, 2: 196 + 4 * 22}, {1: 144, 2: 288}
    for group in (1, 2):
        assert size(group, 1, 2048, 12) - size(group, 1, 1024, 12) == 1024 * per_term[group]
        assert size(group, 32, 1024, 12) - size(group, 16, 1024, 12) == 16 * (1024 * per_term[group] + 8 * 22 * 4096 + 22 * (4096 + 128 + 1) * jac[group])


def test_registry_argument_rules_without_a_gpu(pkg):
    """every BLSW_ERR_ARG case of blsw_registry_msm_batch that needs no handle, and the size function. A handle exists only with a device
    (blsw_registry_create asks for one), so the rules behind a non-NULL handle run in tests/test_msm_gpu.py."""
    lib = pkg.lib()
    assert {"blsw_registry_msm_workspace_bytes", "blsw_registry_msm_batch"} <= set(pkg.EXPORTED_SYMBOLS)
    b = ctypes.c_uint64(0)

    def size(n, n_indices, c):
        assert lib.blsw_registry_msm_workspace_bytes(n, n_indices, c, ctypes.byref(b)) == 0
        return b.value

    for n, n_indices, c in ((0, 5, 0), (0x80000000, 5, 0), (1, (1 << 40) + 1, 0), (1, 5, 17), (1, 5, 0xFFFFFFFF)):
        assert lib.blsw_registry_msm_workspace_bytes(n, n_indices, c, ctypes.byref(b)) == ERR_ARG, (n, n_indices, c)
    assert lib.blsw_registry_msm_workspace_bytes(1, 5, 0, None) == ERR_ARG
    assert size(1, 0, 0) > 0 and size(0x7FFFFFFF, 0, 1) > 0 and size(1, 1 << 40, 16) > 0
    buf = np.full(256, 0x5A, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.blsw_registry_msm_batch(None, p, 4, p, p, 1, 0, p, p, p, 1 << 62, None) == ERR_ARG  # no handle
    assert (buf == 0x5A).all()
    grid = (0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1000, 4096, 32767, 32768, 65536, (1 << 19) - 1, 1 << 19, 1 << 20)
    for c in (0, 1, 3, 7, 13, 16):
        for fixed in (1, 5, 64):
            last = 0
            for v in grid:  # non-decreasing in n_indices at every window_bits, 0 included
                assert size(fixed, v, c) >= last, (c, fixed, v)
                last = size(fixed, v, c)
            if c:
                last = 0
                for v in grid[1:]:  # and in n at 1 .. 16 (at 0 more lists over the same indices are shorter lists: the header says so)
                    assert size(v, 4096, c) >= last, (c, v)
                    last = size(v, 4096, c)
