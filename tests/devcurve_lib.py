"""ctypes loader for tests/devcurve/libdevcurve.so (TEST HARNESS ONLY): the operation table of tests/devcurve/ops.hpp compiled three times for the
device, and the launch-and-compare step the host test (through hostsim_curve_op_batch) and the device test share."""
import ctypes
import os
import subprocess

import numpy as np

from tests import curve_ref as C
from tests import field_ref as F
from tests import hostsim_lib
from tests.devfield_lib import BUILDS, PAD, _elements, _hex, _pack, u32p, u64p

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devcurve")

_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-j3", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevcurve.so"))
    return _lib


def lanes_per_item(build):
    fn = getattr(load(), "devcurve_lpi" + BUILDS[build])
    fn.restype = ctypes.c_uint32
    return fn()


def device_runner(build):
    fn = getattr(load(), "devcurve_run" + BUILDS[build])
    fn.restype = ctypes.c_int
    return fn


def host_runner():
    fn = hostsim_lib.load().hostsim_curve_op_batch
    fn.restype = ctypes.c_int
    return fn


def host_table():
    """[(name, result elements, witnesses, in the quad build)] of the compiled table, by operation index"""
    L = hostsim_lib.load()
    L.hostsim_curve_op_name.restype = ctypes.c_char_p
    return [(L.hostsim_curve_op_name(i).decode(), L.hostsim_curve_op_n_out(i), L.hostsim_curve_op_n_wit(i), L.hostsim_curve_op_quad(i)) for i in range(L.hostsim_curve_op_count())]


def in_build(build, op):
    return build != "quad" or bool(C.OPS[op][2])


def run_launch(build, op, items, runner, lpi):
    """One launch of operation `op` over `items` [(a, b)] by `runner` (devcurve_run* or hostsim_curve_op_batch, lpi lanes per item), compared bit for
    bit with curve_ref.expected: every lane's result elements (so the lanes of a quad agree), every lane's cursor, the witness stream, and the
    sentinel in every result slot and witness slot the operation does not own. -> mismatches [(build, op, item, operands, what)]"""
    n = len(items)
    n_out, n_wit, _ = C.OPS[op]
    wcap = n_wit + PAD
    exp = C.expected(op, items)
    A, B = _pack([a for a, _ in items]), _pack([b for _, b in items])
    out = np.full((n * lpi, 12, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(n * lpi, 0xFFFFFFFF, dtype=np.uint32)
    rc = runner(C.OP_NAMES.index(op), ctypes.c_uint64(n), A.ctypes.data_as(u64p), B.ctypes.data_as(u64p), out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p),
                ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "%s %s: the launch over %d items returned %d" % (build, op, n, rc)
    want_out = _elements([r for r, _, _ in exp], 12)
    want_wit = _elements([w for _, w, _ in exp], wcap)
    bad_out = (out.reshape(n, lpi, 12, 6) != want_out[:, None]).any(axis=(1, 2, 3))
    bad_pos = (npos.reshape(n, lpi) != n_wit).any(axis=1)
    bad_wit = (wit != want_wit).any(axis=(1, 2))
    bad = []
    for i in np.flatnonzero(bad_out | bad_pos | bad_wit)[:10].tolist():
        what = []
        if bad_out[i]:
            lanes = out.reshape(n, lpi, 12, 6)[i]
            k = int(np.flatnonzero((lanes != want_out[i][None]).any(axis=(0, 2)))[0])
            what.append("result %d%s%s" % (k, " (behind the results)" if k >= n_out else "", "" if (lanes == lanes[0]).all() else ", lanes differ"))
        if bad_pos[i]:
            what.append("cursor %s" % npos.reshape(n, lpi)[i].tolist())
        if bad_wit[i]:
            k = int(np.flatnonzero((wit[i] != want_wit[i]).any(axis=1))[0])
            what.append("witness %d%s" % (k, " (behind the stream)" if k >= n_wit else ""))
        bad.append((build, op, i, exp[i][2], _hex(items[i][0]) + " " + _hex(items[i][1]), "; ".join(what)))
    return bad
