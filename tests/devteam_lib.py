"""ctypes loader for tests/devteam/libdevteam.so (TEST HARNESS ONLY): the team operation table of tests/devteam/ops.hpp on the device, and the
launch-and-compare steps the host test (through hostsim_team_op) and the device test share. Expected values are formed once per distinct item:
the single-lane host form's result and witness stream, held to the big-integer reference tests/team_ref.py wherever that states a value or a
stream, and to the group law for the G2 entries."""
import ctypes
import os
import subprocess

import numpy as np

from tests import field_ref as F
from tests import hostsim_lib
from tests import team_ref as T

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devteam")
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
PAD = 3  # witness slots behind an entry's stream: they keep the sentinel
FORMS = {"single": 0, "exec": 1, "exec_hot": 2}
NO_CURSOR = 0xFFFFFFFF

_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevteam.so"))
    return _lib


def host_table():
    """[(name, witnesses, tail, dual)] of the compiled table, by entry index. witnesses: the stream's length, from the op tables' counts; tail: how
    many of them go through the second cursor, which the team's own cursor does not pass"""
    L = hostsim_lib.load()
    L.hostsim_team_op_name.restype = ctypes.c_char_p
    return [(L.hostsim_team_op_name(i).decode(), L.hostsim_team_op_n_wit(i), L.hostsim_team_op_tail(i), L.hostsim_team_op_dual(i)) for i in range(L.hostsim_team_op_count())]


_counts = {}


def counts(op):
    """(witnesses, tail) of entry `op`"""
    if not _counts:
        for name, n_wit, tail, _ in host_table():
            _counts[name] = (n_wit, tail)
    return _counts[op]


def _pack(blocks):
    """[n] blocks of twelve stored integers -> uint64 [n, 12, 6]"""
    raw = b"".join(x.to_bytes(48, "little") for blk in blocks for x in blk)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(blocks), 12, 6).copy()


def _ints(arr):
    """uint64 [k, 6] -> [k] integers"""
    return [int.from_bytes(arr[i].tobytes(), "little") for i in range(arr.shape[0])]


def run_host(form, op, items):
    """entry `op` over `items` through hostsim_team_op -> (out uint64 [n, 12, 6], wit [n, wcap, 6], npos uint32 [n]), the sentinel where nothing is written"""
    n = len(items)
    n_wit, _ = counts(op)
    wcap = n_wit + PAD
    A, B, C = (_pack([it[k] for it in items]) for k in range(3))
    out = np.full((n, 12, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(n, NO_CURSOR, dtype=np.uint32)
    fn = hostsim_lib.load().hostsim_team_op
    fn.restype = ctypes.c_int
    rc = fn(FORMS[form], T.OP_NAMES.index(op), ctypes.c_uint64(n), A.ctypes.data_as(u64p), B.ctypes.data_as(u64p), C.ctypes.data_as(u64p), out.ctypes.data_as(u64p),
            wit.ctypes.data_as(u64p), ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "host %s %s: %d items returned %d" % (form, op, n, rc)
    return out, wit, npos


def run_device(form, op, items):
    """entry `op` over `items` on the device -> (out uint64 [lanes, 2, 6], wit [n, wcap, 6], npos uint32 [lanes]), lanes = 64 per wave of ten items"""
    n = len(items)
    n_wit, _ = counts(op)
    wcap = n_wit + PAD
    lanes = 64 * ((n + T.TEAMS - 1) // T.TEAMS)
    A, B, C = (_pack([it[k] for it in items]) for k in range(3))
    out = np.full((lanes, 2, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(lanes, NO_CURSOR, dtype=np.uint32)
    fn = load().devteam_run
    fn.restype = ctypes.c_int
    rc = fn(T.OP_NAMES.index(op), int(form == "exec_hot"), ctypes.c_uint64(n), A.ctypes.data_as(u64p), B.ctypes.data_as(u64p), C.ctypes.data_as(u64p),
            out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p), ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "device %s %s: the launch over %d items returned %d" % (form, op, n, rc)
    return out, wit, npos


_expected = {}


def expected(op, items):
    """[(result elements [12], stream)] per item. Formed once per distinct item from the single-lane host form; on the way that form is held to the
    reference: its values (every entry but the G2 ones, which are held to the group law), its stream where the reference states one, its cursor
    to the table's count. A disagreement is an AssertionError naming the item: there is no expected value to compare anything else with."""
    memo = _expected.setdefault(op, {})
    new = list(dict.fromkeys(it for it in items if it not in memo))
    if new:
        n_wit, _ = counts(op)
        out, wit, npos = run_host("single", op, new)
        assert (npos == n_wit).all(), "%s: the single-lane form's cursor is not the table's count %d: %s" % (op, n_wit, sorted(set(npos.tolist())))
        assert (wit[:, n_wit:] == np.uint64(F.SENTINEL)).all(), "%s: the single-lane form writes behind its stream" % op
        for i, it in enumerate(new):
            res, w = _ints(out[i]), _ints(wit[i, :n_wit])
            ref_res, ref_w = T.reference(op, *it)
            if op in T.G2_OPS:
                assert T.g2_law_holds(op, it[0], it[1], res), "%s: the single-lane result is not the group law's, item %s" % (op, _hex_item(it))
            else:
                assert res == ref_res, "%s: the single-lane value is not the reference's, item %s" % (op, _hex_item(it))
            assert ref_w is None or w == ref_w, "%s: the single-lane stream is not the reference's, item %s" % (op, _hex_item(it))
            memo[it] = (res, w)
    return [memo[it] for it in items]


def _elements(rows, width):
    """[n] lists of stored integers (equal lengths <= width) -> uint64 [n, width, 6], the sentinel behind each list"""
    out = np.full((len(rows), width, 6), F.SENTINEL, dtype=np.uint64)
    k = len(rows[0])
    if k:
        raw = b"".join(x.to_bytes(48, "little") for r in rows for x in r)
        out[:, :k] = np.frombuffer(raw, dtype=np.uint64).reshape(len(rows), k, 6)
    return out


def _hex(blk):
    blk = list(blk)
    while len(blk) > 1 and blk[-1] == 0:
        blk.pop()
    return "[" + ", ".join(hex(x) for x in blk) + "]"


def _hex_item(it):
    return " ".join(_hex(b) for b in it)


def _first_bad_witness(wit, want, n_wit):
    k = int(np.flatnonzero((wit != want).any(axis=1))[0])
    return "witness %d%s" % (k, " (behind the stream)" if k >= n_wit else "")


def check_host(form, op, items):
    """the team form through the looped host team, bit for bit against expected(): the six coefficients, the stream, the sentinel behind it, the
    team's cursor -> mismatches [(form, op, item, operands, what)]"""
    n_wit, tail = counts(op)
    exp = expected(op, items)
    out, wit, npos = run_host(form, op, items)
    want_out = _elements([r for r, _ in exp], 12)
    want_wit = _elements([w for _, w in exp], n_wit + PAD)
    bad_out = (out != want_out).any(axis=(1, 2))
    bad_pos = npos != n_wit - tail
    bad_wit = (wit != want_wit).any(axis=(1, 2))
    bad = []
    for i in np.flatnonzero(bad_out | bad_pos | bad_wit)[:10].tolist():
        what = []
        if bad_out[i]:
            what.append("result, coefficients %s" % np.flatnonzero((out[i] != want_out[i]).any(axis=1).reshape(6, 2).any(axis=1)).tolist())
        if bad_pos[i]:
            what.append("cursor %d" % npos[i])
        if bad_wit[i]:
            what.append(_first_bad_witness(wit[i], want_wit[i], n_wit))
        bad.append((form, op, i, _hex_item(items[i]), "; ".join(what)))
    return bad


def check_device(form, op, items):
    """one launch on the device, bit for bit against expected(): lane j of item i's team holds coefficient j of the result (a verdict: the same
    flag on all six) and the team's cursor; every other lane of the grid (lanes 60..63 of a wave, the idle teams of the last wave) keeps the
    sentinel in its result slot and its cursor slot; the stream, and the sentinel behind it -> mismatches"""
    n = len(items)
    n_wit, tail = counts(op)
    exp = expected(op, items)
    out, wit, npos = run_device(form, op, items)
    lanes = out.shape[0]
    item = np.arange(n)
    lane0 = (item // T.TEAMS) * 64 + (item % T.TEAMS) * 6
    owned = (lane0[:, None] + np.arange(6)[None, :]).reshape(-1)  # lane of (item, j)
    want_out = np.full((lanes, 2, 6), F.SENTINEL, dtype=np.uint64)
    want_out[owned] = _elements([r for r, _ in exp], 12).reshape(n * 6, 2, 6)
    want_pos = np.full(lanes, NO_CURSOR, dtype=np.uint32)
    want_pos[owned] = n_wit - tail
    want_wit = _elements([w for _, w in exp], n_wit + PAD)
    bad_lane = (out != want_out).any(axis=(1, 2)) | (npos != want_pos)
    bad_wit = (wit != want_wit).any(axis=(1, 2))
    lane_item = np.full(lanes, -1, dtype=np.int64)
    lane_item[owned] = np.repeat(item, 6)
    bad = []
    for ln in np.flatnonzero(bad_lane)[:10].tolist():
        i = int(lane_item[ln])
        what = "lane %d (wave %d, team %d, j %d): %s%s" % (ln, ln // 64, (ln % 64) // 6, (ln % 64) % 6, "result " if (out[ln] != want_out[ln]).any() else "",
                                                          "cursor %d" % npos[ln] if npos[ln] != want_pos[ln] else "")
        bad.append((form, op, i, _hex_item(items[i]) if i >= 0 else "idle lane", what))
    for i in np.flatnonzero(bad_wit)[:10].tolist():
        bad.append((form, op, i, _hex_item(items[i]), _first_bad_witness(wit[i], want_wit[i], n_wit)))
    return bad
