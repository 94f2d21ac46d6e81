"""ctypes loader for tests/devfield/libdevfield.so (TEST HARNESS ONLY): the operation table of tests/devfield/ops.hpp compiled three times for the
device, and the launch-and-compare step the host test (through hostsim_field_op_batch) and the device test share."""
import ctypes
import os
import subprocess

import numpy as np

from tests import field_ref as F
from tests import hostsim_lib

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfield")
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
BUILDS = {"outline": "", "inl": "_inl", "quad": "_q"}  # build -> suffix of its entries (csrc/kcommon.hpp: BLSW_K)
PAD = 3  # witness slots behind an operation's stream: they keep the sentinel

_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-j3", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevfield.so"))
    return _lib


def lanes_per_item(build):
    fn = getattr(load(), "devfield_lpi" + BUILDS[build])
    fn.restype = ctypes.c_uint32
    return fn()


def device_runner(build):
    fn = getattr(load(), "devfield_run" + BUILDS[build])
    fn.restype = ctypes.c_int
    return fn


def host_runner():
    fn = hostsim_lib.load().hostsim_field_op_batch
    fn.restype = ctypes.c_int
    return fn


def host_table():
    """[(name, result elements, witnesses)] of the compiled table, by operation index"""
    L = hostsim_lib.load()
    L.hostsim_field_op_name.restype = ctypes.c_char_p
    return [(L.hostsim_field_op_name(i).decode(), L.hostsim_field_op_n_out(i), L.hostsim_field_op_n_wit(i)) for i in range(L.hostsim_field_op_count())]


def _pack(blocks):
    """[n] blocks of twelve stored integers -> uint64 [n, 12, 6]"""
    raw = b"".join(x.to_bytes(48, "little") for blk in blocks for x in blk)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(blocks), 12, 6).copy()


def _elements(rows, width):
    """[n] lists of stored integers (equal lengths <= width) -> uint64 [n, width, 6], the sentinel behind each list"""
    out = np.full((len(rows), width, 6), F.SENTINEL, dtype=np.uint64)
    k = len(rows[0])
    if k:
        raw = b"".join(x.to_bytes(48, "little") for r in rows for x in r)
        out[:, :k] = np.frombuffer(raw, dtype=np.uint64).reshape(len(rows), k, 6)
    return out


def host_stream(op, a, b):
    """the host compilation's witness stream of one item (the expected stream of the Fp6 / Fp12 operations)"""
    n_out, n_wit = F.OPS[op]
    A, B = _pack([a]), _pack([b])
    out = np.zeros((12, 6), dtype=np.uint64)
    wit = np.zeros((max(1, n_wit), 6), dtype=np.uint64)
    pos = hostsim_lib.load().hostsim_field_op(F.OP_NAMES.index(op), A.ctypes.data_as(u64p), B.ctypes.data_as(u64p), out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p))
    assert pos == n_wit, (op, pos)
    return [int.from_bytes(wit[i].tobytes(), "little") for i in range(n_wit)]


def _hex(blk):
    blk = list(blk)
    while len(blk) > 1 and blk[-1] == 0:
        blk.pop()
    return "[" + ", ".join(hex(x) for x in blk) + "]"


def run_launch(build, op, items, runner, lpi):
    """One launch of operation `op` over `items` [(a, b)] by `runner` (devfield_run* or hostsim_field_op_batch, lpi lanes per item), compared bit for
    bit with field_ref.expected: every lane's result elements (so the lanes of a quad agree), every lane's cursor, the witness stream, and the
    sentinel in every result slot and witness slot the operation does not own. -> mismatches [(build, op, item, operands, what)]"""
    n = len(items)
    n_out, n_wit = F.OPS[op]
    wcap = n_wit + PAD
    exp = F.expected(op, items, host_stream)
    A, B = _pack([a for a, _ in items]), _pack([b for _, b in items])
    out = np.full((n * lpi, 12, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(n * lpi, 0xFFFFFFFF, dtype=np.uint32)
    rc = runner(F.OP_NAMES.index(op), ctypes.c_uint64(n), A.ctypes.data_as(u64p), B.ctypes.data_as(u64p), out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p),
                ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "%s %s: the launch over %d items returned %d" % (build, op, n, rc)
    want_out = _elements([r for r, _ in exp], 12)
    want_wit = _elements([w for _, w in exp], wcap)
    bad_out = (out.reshape(n, lpi, 12, 6) != want_out[:, None]).any(axis=(1, 2, 3))
    bad_pos = (npos.reshape(n, lpi) != n_wit).any(axis=1)
    bad_wit = (wit != want_wit).any(axis=(1, 2))
    bad = []
    for i in np.flatnonzero(bad_out | bad_pos | bad_wit)[:10].tolist():
        what = []
        if bad_out[i]:
            lanes = out.reshape(n, lpi, 12, 6)[i]
            what.append("result" if (lanes == lanes[0]).all() else "result, lanes differ")
        if bad_pos[i]:
            what.append("cursor %s" % npos.reshape(n, lpi)[i].tolist())
        if bad_wit[i]:
            k = int(np.flatnonzero((wit[i] != want_wit[i]).any(axis=1))[0])
            what.append("witness %d%s" % (k, " (behind the stream)" if k >= n_wit else ""))
        bad.append((build, op, i, _hex(items[i][0]) + " " + _hex(items[i][1]), "; ".join(what)))
    return bad
