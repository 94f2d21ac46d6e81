"""The compact checker of shared-keys steps (ABI 16: blsw_compact_layout_keyset, blsw_r1cs_head_rows, blsw_r1cs_check_keyset, blsw_r1cs_check_compact_keyset /
_evaluate_compact_keyset), host side: the header, the ctypes mirror, the layout of a shared-keys step's buffer, the head rows of the library's and of
synthetic matrices against a plain numpy scan, and every argument rule that is checked before any HIP call. Runs without a GPU."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import r1cs_synth as S

gen = importlib.import_module("tools.gen_bindings")
H = gen.parse_header()
ERR_ARG = 1
SEG = 1942        # witnesses of one key's allocation
HEAD_ROWS = 1939  # constraints of one key's allocation: the rows that read that key's block alone
NEW = ["blsw_compact_layout_keyset", "blsw_r1cs_head_rows", "blsw_r1cs_handle_head_rows", "blsw_r1cs_check_keyset", "blsw_r1cs_check_compact_keyset",
       "blsw_r1cs_evaluate_compact_keyset"]
_MATS = {}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def mats(pkg, n_keys, mask):
    if (n_keys, mask) not in _MATS:
        _MATS[n_keys, mask] = pkg.matrices(32, n_keys=n_keys, agg_inputs=mask)
    return _MATS[n_keys, mask]


def head_rows(pkg, sys, head_len, rows=True):
    """blsw_r1cs_head_rows -> (rc, rows); the output starts at a sentinel"""
    info, m = pkg._matrices_struct(sys)
    out = ctypes.c_uint64(777)
    rc = pkg.lib().blsw_r1cs_head_rows(ctypes.byref(info), ctypes.byref(m), head_len, ctypes.byref(out) if rows else None)
    return rc, out.value


def scan(sys, head_len):
    """the reference: the number of leading rows whose every column is 0 or in [n_instance_vars, n_instance_vars + head_len), from the CSR with numpy"""
    ni, nc = sys["n_instance_vars"], sys["n_constraints"]
    ok = np.ones(nc, dtype=bool)
    for name in "ABC":
        rp, col, _ = sys[name]
        bad = (col != 0) & ((col < ni) | (col >= ni + head_len))
        row_of = np.repeat(np.arange(nc), np.diff(rp.astype(np.int64)))
        ok[row_of[bad]] = False
    return nc if ok.all() else int(np.argmin(ok))


def test_symbols(pkg):
    L = pkg.lib()
    assert L.blsw_version() == H["defines"]["BLSW_ABI_VERSION"] >= 16
    assert H["defines"]["BLSW_R1CS_HEAD_CHECK"] == 0 and H["defines"]["BLSW_R1CS_HEAD_SKIP"] == 1
    params = {name: p for name, _, p in H["functions"]}
    for name in NEW:
        assert name in params and name in pkg.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == len(params[name]), name
    # the struct a shared-keys step's buffer is described by is the one of ABI 14
    assert [f for _, f in H["structs"]["blsw_compact_layout_t"]] == [n for n, _ in pkg.blsw_compact_layout_t._fields_]
    assert ctypes.sizeof(pkg.blsw_compact_layout_t) == 4 * 8 + 10 * 4


@pytest.mark.parametrize("mask", [0, 2, 14])
def test_layout_is_the_keys_input_layout(pkg, mask):
    lay, head_len = pkg.compact_layout_keyset(128, 32, n_keys=5, shared_keys=1, agg_inputs=mask)
    assert head_len == 5 * SEG
    ref = pkg.compact_layout(128, 32, n_keys=5, agg_inputs=mask | 1)
    for name, _ in pkg.blsw_compact_layout_t._fields_:
        assert getattr(lay, name) == getattr(ref, name), name
    assert lay.n_witness + head_len == pkg.layout_aggregate(32, 5, mask)["n_witness"]
    assert lay.n == 128 and lay.total % 256 == 0


def test_layout_refusals(pkg):
    L = pkg.lib()
    c, h = pkg.blsw_compact_layout_t(), ctypes.c_uint32(7)
    c.n = 7

    def layout(n=128, rows=ctypes.byref(c), head=ctypes.byref(h), opt=True, **kw):
        o = pkg.engine_options(**kw)
        return L.blsw_compact_layout_keyset(n, 32, ctypes.byref(o) if opt else None, rows, head)

    assert layout(n_keys=5) == ERR_ARG  # without shared_keys: that is blsw_compact_layout's
    assert layout(n_keys=5, shared_keys=1, agg_inputs=1) == ERR_ARG and layout(n_keys=5, shared_keys=1, agg_inputs=15) == ERR_ARG  # BLSW_AGG_KEYS_INPUT
    assert layout(n=100, n_keys=5, shared_keys=1) == ERR_ARG and layout(n=32, n_keys=5, shared_keys=1) == ERR_ARG and layout(n=0, n_keys=5, shared_keys=1) == ERR_ARG
    assert layout(rows=None, n_keys=5, shared_keys=1) == ERR_ARG and layout(head=None, n_keys=5, shared_keys=1) == ERR_ARG
    assert layout(opt=False, n_keys=5, shared_keys=1) == ERR_ARG
    assert layout(shared_keys=1) == ERR_ARG and layout(n_keys=5, shared_keys=2) == ERR_ARG  # what the engine refuses
    assert (c.n, h.value) == (7, 7)  # nothing written on refusal
    assert layout(n_keys=5, shared_keys=1) == 0 and (c.n, h.value) == (128, 5 * SEG)
    with pytest.raises(pkg.BlswError):
        pkg.compact_layout_keyset(128, 32, n_keys=5)


@pytest.mark.parametrize("n_keys,mask", [(1, 0), (2, 0), (5, 0), (5, 14)])
def test_head_rows_of_the_aggregate_circuit(pkg, n_keys, mask):
    """1 939 rows per key read that key's 1 942 allocation witnesses alone, whatever else is a public input"""
    P = mats(pkg, n_keys, mask)
    assert P["n_instance_vars"] == {0: 1, 14: 13}[mask]
    assert head_rows(pkg, P, n_keys * SEG) == (0, HEAD_ROWS * n_keys)
    assert pkg.r1cs_head_rows(P, n_keys * SEG) == HEAD_ROWS * n_keys
    assert head_rows(pkg, P, 0) == (0, 0)
    if n_keys == 5:  # a head of fewer keys covers those keys' rows; one element short of a key's block does not cover its last rows
        assert head_rows(pkg, P, 2 * SEG) == (0, 2 * HEAD_ROWS)
        rc, rows = head_rows(pkg, P, 2 * SEG - 1)
        assert rc == 0 and rows == scan(P, 2 * SEG - 1) and HEAD_ROWS <= rows < 2 * HEAD_ROWS


def test_head_rows_equal_a_numpy_scan(pkg):
    """the single-key matrices with head_len 1942, and the aggregate circuit at a head that ends inside a key's block and one past all keys"""
    P = pkg.matrices(32)
    assert head_rows(pkg, P, SEG) == (0, scan(P, SEG))
    P = mats(pkg, 2, 0)
    for head_len in (1000, SEG + 7, 2 * SEG + 40, P["n_witness"]):
        assert head_rows(pkg, P, head_len) == (0, scan(P, head_len)), head_len
    assert scan(P, P["n_witness"]) == P["n_constraints"] and scan(P, 2 * SEG) == 2 * HEAD_ROWS


def small_system(rows, ni, n_witness):
    """rows: [A, B, C] entry lists of (column, coefficient) -> a matrices()-shaped dict without slacks"""
    return S.system_from_rows([(None, [list(a), list(b), list(c)], None) for a, b, c in rows], ni, n_witness=n_witness)


def test_head_rows_edges_on_synthetic_systems(pkg):
    ni, nw = 3, 10
    w = lambda k: ni + k  # the column of witness k
    head = [[(0, 5), (w(0), 2)], [(w(1), 3)], [(w(2), 7)]]
    # a first row that reads an instance column: no head covers it
    sys = small_system([[[(1, 2)], [(w(0), 1)], [(w(1), 1)]], head], ni, nw)
    for head_len in (0, 3, nw):
        assert head_rows(pkg, sys, head_len) == (0, 0) == (0, scan(sys, head_len))
    # a row with an empty A (and an all-empty row) stays head-only; an instance column in a later row ends the head rows for every head_len
    sys = small_system([head, [[], [(w(1), 3)], [(w(0), 1)]], [[], [], []], [[(w(3), 1)], [(2, 1)], []], head], ni, nw)
    assert head_rows(pkg, sys, 3) == (0, 3) and head_rows(pkg, sys, nw) == (0, 3) and scan(sys, nw) == 3
    assert head_rows(pkg, sys, 2) == (0, 0) and head_rows(pkg, sys, 0) == (0, 0)
    # head_len one short of a row's largest column stops before that row
    sys = small_system([head, [[(w(0), 1)], [(w(5), 1)], [(w(1), 1)]], head, [[(w(9), 1)], [], []]], ni, nw)
    assert head_rows(pkg, sys, 5) == (0, 1) == (0, scan(sys, 5))
    assert head_rows(pkg, sys, 6) == (0, 3) == (0, scan(sys, 6))
    assert head_rows(pkg, sys, 9) == (0, 3) == (0, scan(sys, 9))
    # head_len = n_witness gives all rows
    assert head_rows(pkg, sys, nw) == (0, 4) == (0, scan(sys, nw))
    # the big synthetic system of the device tests: every head_len the scan agrees on
    big = S.make_system(n_instance_vars=1)
    for head_len in (0, 1, S.N_POOL, S.N_POOL + S.N_PM1, big["n_witness"] - 1, big["n_witness"]):
        assert head_rows(pkg, big, head_len) == (0, scan(big, head_len)), head_len


def test_head_rows_refusals(pkg):
    sys = small_system([[[(0, 5)], [(1, 3)], [(2, 7)]]], 1, 4)
    assert head_rows(pkg, sys, 4) == (0, 1)
    assert head_rows(pkg, sys, 5) == (ERR_ARG, 777) and head_rows(pkg, sys, 1 << 40) == (ERR_ARG, 777)
    assert head_rows(pkg, sys, 1, rows=False)[0] == ERR_ARG
    L = pkg.lib()
    info, m = pkg._matrices_struct(sys)
    out = ctypes.c_uint64(777)
    assert L.blsw_r1cs_head_rows(None, ctypes.byref(m), 1, ctypes.byref(out)) == ERR_ARG
    assert L.blsw_r1cs_head_rows(ctypes.byref(info), None, 1, ctypes.byref(out)) == ERR_ARG
    # a CSR blsw_r1cs_create refuses (a column beyond z)
    bad = dict(sys)
    bad["A"] = (sys["A"][0], np.array([9], dtype=np.uint32), sys["A"][2])
    assert head_rows(pkg, bad, 1) == (ERR_ARG, 777)
    assert L.blsw_r1cs_handle_head_rows(None, 1, ctypes.byref(out)) == ERR_ARG and out.value == 777
    with pytest.raises(pkg.BlswError):
        pkg.r1cs_head_rows(sys, 5)


def test_entry_points_refuse_null_handles(pkg):
    """a NULL handle or a NULL set: BLSW_ERR_ARG on the host, nothing is dereferenced (the other pointers are never read)"""
    L = pkg.lib()
    p = ctypes.c_void_p(0x10000)
    lay, _ = pkg.compact_layout_keyset(64, 32, n_keys=5, shared_keys=1)
    c = ctypes.byref(lay)
    assert L.blsw_r1cs_check_keyset(None, p, p, p, None) == ERR_ARG and L.blsw_r1cs_check_keyset(p, None, p, p, None) == ERR_ARG
    for mode in (0, 1):
        assert L.blsw_r1cs_check_compact_keyset(None, c, p, p, mode, None, 0, p, p, None) == ERR_ARG
        assert L.blsw_r1cs_check_compact_keyset(p, c, p, None, mode, None, 0, p, p, None) == ERR_ARG
    assert L.blsw_r1cs_evaluate_compact_keyset(None, c, p, p, None, 0, 0, 4, p, p, p, None) == ERR_ARG
    assert L.blsw_r1cs_evaluate_compact_keyset(p, c, p, None, None, 0, 0, 4, p, p, p, None) == ERR_ARG
