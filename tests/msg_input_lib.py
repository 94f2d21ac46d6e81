"""ctypes loaders for tests/msg_input (TEST HARNESS ONLY): libmsgshim.so, the message-input circuit (UInt8::new_input_vec) composed from the
oracle's headers, and libmsgemit.so, the product's message emitter compiled for the host."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "msg_input")
u64p = ctypes.POINTER(ctypes.c_uint64)
CHUNK = 47  # message bytes per public input
SEG_CHUNK = 761  # witnesses per chunk (to_bits_le)

_libs = {}


def _load(name):
    if name not in _libs:
        subprocess.check_call(["make", "-s", "-C", HERE])
        L = ctypes.CDLL(os.path.join(HERE, name))
        for f in ("msh_witness", "msh_layout", "msh_matrices"):
            if hasattr(L, f):
                getattr(L, f).restype = ctypes.c_uint64
        if hasattr(L, "msh_check"):
            L.msh_check.restype = ctypes.c_int64
        if hasattr(L, "msgemit_segment"):
            L.msgemit_segment.restype = ctypes.c_uint32
        _libs[name] = L
    return _libs[name]


def shim():
    return _load("libmsgshim.so")


def emit():
    return _load("libmsgemit.so")


def chunks(msg_len):
    return (msg_len + CHUNK - 1) // CHUNK


def _buf(msg):
    b = bytes(msg)
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def _u64(a, n):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    assert a.size == n
    return a


def witness(pk_xy, msg, sig_xy, pk_input=0, sig_input=0):
    """-> (result, witness [n_witness, 6] uint64, instance [n_instance_vars, 6] uint64, n_constraints)"""
    pk, sig = _u64(pk_xy, 12), _u64(sig_xy, 24)
    nc, ni, res = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    args = lambda w, cap, inst: (pk.ctypes.data_as(u64p), _buf(msg), ctypes.c_size_t(len(msg)), sig.ctypes.data_as(u64p), int(pk_input), int(sig_input), w,
                                 ctypes.c_uint64(cap), inst, ctypes.byref(ni), ctypes.byref(nc), ctypes.byref(res))
    n = shim().msh_witness(*args(None, 0, None))
    w = np.zeros((n, 6), dtype=np.uint64)
    inst = np.zeros((ni.value, 6), dtype=np.uint64)
    shim().msh_witness(*args(w.ctypes.data_as(u64p), n, inst.ctypes.data_as(u64p)))
    return bool(res.value), w, inst, nc.value


def layout(msg_len, pk_input=0, sig_input=0):
    """-> (marks {name: witness index}, n_witness, n_constraints, n_instance_vars)"""
    starts = (ctypes.c_uint64 * 64)()
    names = ctypes.create_string_buffer(4096)
    nw, nc, ni = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    k = shim().msh_layout(ctypes.c_size_t(msg_len), int(pk_input), int(sig_input), starts, ctypes.c_uint64(64), names, ctypes.c_size_t(4096), ctypes.byref(nw),
                          ctypes.byref(nc), ctypes.byref(ni))
    nm = names.value.decode().split("\n")[:k]
    return {nm[i]: starts[i] for i in range(k)}, nw.value, nc.value, ni.value


def matrices(msg_len, pk_input=0, sig_input=0):
    """-> (n_constraints, n_witness, n_instance_vars, [(row_ptr, col, val)] * 3)"""
    nnz = (ctypes.c_uint64 * 3)()
    nw, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
    a = (ctypes.c_size_t(msg_len), int(pk_input), int(sig_input), nnz, ctypes.byref(nw), ctypes.byref(ni))
    nc = shim().msh_matrices(*a, None, None, None)
    rp = [np.zeros(nc + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(nnz[m], dtype=np.uint32) for m in range(3)]
    val = [np.zeros((nnz[m], 6), dtype=np.uint64) for m in range(3)]
    RP = (u64p * 3)(*[r.ctypes.data_as(u64p) for r in rp])
    CO = (ctypes.POINTER(ctypes.c_uint32) * 3)(*[c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for c in col])
    VA = (u64p * 3)(*[v.ctypes.data_as(u64p) for v in val])
    shim().msh_matrices(*a, RP, CO, VA)
    return nc, nw.value, ni.value, [(rp[m], col[m], val[m]) for m in range(3)]


def check(pk_xy, msg, sig_xy, pk_input=0, sig_input=0, instance=None, witness=None):
    """first unsatisfied constraint of z = [instance | witness] (None: the shim's own), -1 when satisfied"""
    pk, sig = _u64(pk_xy, 12), _u64(sig_xy, 24)
    ip = np.ascontiguousarray(instance, dtype=np.uint64) if instance is not None else None
    wp = np.ascontiguousarray(witness, dtype=np.uint64) if witness is not None else None
    return shim().msh_check(pk.ctypes.data_as(u64p), _buf(msg), ctypes.c_size_t(len(msg)), sig.ctypes.data_as(u64p), int(pk_input), int(sig_input),
                            ip.ctypes.data_as(u64p) if ip is not None else None, wp.ctypes.data_as(u64p) if wp is not None else None,
                            ctypes.c_uint64(wp.shape[0] if wp is not None else 0))


def emit_segment(msg):
    """the product's emitter on the host -> (segment [c * 761, 6] uint64, inputs [c, 6] uint64)"""
    c = chunks(len(msg))
    seg = np.zeros((max(1, c * SEG_CHUNK), 6), dtype=np.uint64)
    inp = np.zeros((max(1, c), 6), dtype=np.uint64)
    got = emit().msgemit_segment(_buf(msg), len(msg), seg.ctypes.data_as(u64p), inp.ctypes.data_as(u64p))
    assert got == c
    return seg[: c * SEG_CHUNK], inp[:c]
