"""ctypes loaders for tests/multi_inputs (TEST HARNESS ONLY): libmultishim.so, the N+1-pair product with Input arguments composed from the oracle's
headers, and libmultiemit.so, the product's instance-index rules and Input branches (csrc/multi_input.hpp) compiled for the host. Both are built on
demand."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_inputs")
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)
KEYS, MSG, SIG = 1, 4, 8  # bits of the mask (include/blsw.h: BLSW_MULTI_*_INPUT)
MASKS = (0, 1, 4, 5, 8, 9, 12, 13)  # all eight
CHUNK = 47  # message bytes per public input
SEG_PK_ALLOC, SEG_SIG_ALLOC, SEG_MSG_CHUNK = 1942, 12413, 761
# shim mark -> field of blsw_layout_t (a mark that repeats per pair: its first occurrence)
MARKS = (("msg", "off_msg"), ("pk_alloc", "off_pk_alloc"), ("sig_alloc", "off_sig_alloc"), ("verify.pk_not_zero", "off_pk_not_zero"), ("hash.expand", "off_expand"),
         ("hash.map0", "off_map0"), ("hash.map1", "off_map1"), ("hash.add", "off_add"), ("hash.clear_cofactor", "off_cofactor"), ("prepare.h", "off_prep_h"),
         ("prepare.pk", "off_prep_pk"), ("prepare.sig", "off_prep_sig"), ("miller", "off_miller"), ("final_exp", "off_final_exp"), ("is_one", "off_is_one"))

_libs = {}


def _load(name):
    if name not in _libs:
        subprocess.check_call(["make", "-s", "-C", HERE, name])
        L = ctypes.CDLL(os.path.join(HERE, name))
        for f in ("mush_witness", "mush_layout", "mush_matrices"):
            if hasattr(L, f):
                getattr(L, f).restype = ctypes.c_uint64
        if hasattr(L, "mush_check"):
            L.mush_check.restype = ctypes.c_int64
        if hasattr(L, "multiemit_index"):
            L.multiemit_index.restype = ctypes.c_uint32
        _libs[name] = L
    return _libs[name]


def shim():
    return _load("libmultishim.so")


def emit():
    return _load("libmultiemit.so")


def chunks(msg_len):
    return (msg_len + CHUNK - 1) // CHUNK


def n_instance_vars(K, msg_len, mask):
    return 1 + (K * chunks(msg_len) if mask & MSG else 0) + (3 * K if mask & KEYS else 0) + (6 if mask & SIG else 0)


def _inputs(pks_xy, msgs, sig_xy):
    pks = np.ascontiguousarray(pks_xy, dtype=np.uint64).reshape(-1, 12)
    m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(pks.shape[0], -1)
    sig = np.ascontiguousarray(sig_xy, dtype=np.uint64).reshape(-1)
    assert sig.size == 24
    mp = m.ctypes.data_as(u8p) if m.shape[1] else (ctypes.c_uint8 * 1)()
    return pks, m, mp, sig


def witness(pks_xy, msgs, sig_xy, mask):
    """pks_xy [K, 12], msgs [K, msg_len] -> (result, witness [n_witness, 6] uint64, instance [n_instance_vars, 6] uint64, n_constraints)"""
    pks, m, mp, sig = _inputs(pks_xy, msgs, sig_xy)
    K, msg_len = m.shape
    nc, ni, res = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0)
    n = n_witness_of(K, msg_len, mask)
    w = np.zeros((n, 6), dtype=np.uint64)
    inst = np.zeros((n_instance_vars(K, msg_len, mask), 6), dtype=np.uint64)
    got = shim().mush_witness(pks.ctypes.data_as(u64p), ctypes.c_size_t(K), mp, ctypes.c_size_t(msg_len), sig.ctypes.data_as(u64p), int(mask), w.ctypes.data_as(u64p),
                              ctypes.c_uint64(n), inst.ctypes.data_as(u64p), ctypes.byref(ni), ctypes.byref(nc), ctypes.byref(res))
    assert got == n and ni.value == inst.shape[0]
    return bool(res.value), w, inst, nc.value


_NW = {}


def n_witness_of(K, msg_len, mask):
    if (K, msg_len, mask) not in _NW:
        _NW[(K, msg_len, mask)] = layout(K, msg_len, mask)[1]
    return _NW[(K, msg_len, mask)]


def layout(K, msg_len, mask):
    """-> (marks [(name, witness index)] in synthesis order, n_witness, n_constraints, n_instance_vars)"""
    cap = 16 + 8 * K
    starts = (ctypes.c_uint64 * cap)()
    names = ctypes.create_string_buffer(64 * cap)
    nw, nc, ni = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    k = shim().mush_layout(ctypes.c_size_t(K), ctypes.c_size_t(msg_len), int(mask), starts, ctypes.c_uint64(cap), names, ctypes.c_size_t(64 * cap), ctypes.byref(nw),
                           ctypes.byref(nc), ctypes.byref(ni))
    assert k <= cap
    nm = names.value.decode().split("\n")[:k]
    return [(nm[i], starts[i]) for i in range(k)], nw.value, nc.value, ni.value


def first_marks(marks):
    d = {}
    for name, start in marks:
        d.setdefault(name, start)
    return d


def matrices(K, msg_len, mask):
    """-> (n_constraints, n_witness, n_instance_vars, [(row_ptr, col, val)] * 3)"""
    nnz = (ctypes.c_uint64 * 3)()
    nw, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
    a = (ctypes.c_size_t(K), ctypes.c_size_t(msg_len), int(mask), nnz, ctypes.byref(nw), ctypes.byref(ni))
    nc = shim().mush_matrices(*a, None, None, None)
    rp = [np.zeros(nc + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(nnz[m], dtype=np.uint32) for m in range(3)]
    val = [np.zeros((nnz[m], 6), dtype=np.uint64) for m in range(3)]
    RP = (u64p * 3)(*[r.ctypes.data_as(u64p) for r in rp])
    CO = (ctypes.POINTER(ctypes.c_uint32) * 3)(*[c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for c in col])
    VA = (u64p * 3)(*[v.ctypes.data_as(u64p) for v in val])
    shim().mush_matrices(*a, RP, CO, VA)
    return nc, nw.value, ni.value, [(rp[m], col[m], val[m]) for m in range(3)]


def check(pks_xy, msgs, sig_xy, mask, instance=None, witness=None):
    """first unsatisfied constraint of z = [instance | witness] (None: the shim's own), -1 when satisfied"""
    pks, m, mp, sig = _inputs(pks_xy, msgs, sig_xy)
    ip = np.ascontiguousarray(instance, dtype=np.uint64) if instance is not None else None
    wp = np.ascontiguousarray(witness, dtype=np.uint64) if witness is not None else None
    return shim().mush_check(pks.ctypes.data_as(u64p), ctypes.c_size_t(m.shape[0]), mp, ctypes.c_size_t(m.shape[1]), sig.ctypes.data_as(u64p), int(mask),
                             ip.ctypes.data_as(u64p) if ip is not None else None, wp.ctypes.data_as(u64p) if wp is not None else None,
                             ctypes.c_uint64(wp.shape[0] if wp is not None else 0))


def emit_layout(pkg, msg_len, K, mask):
    L = pkg.blsw_layout_t()
    emit().multiemit_layout(msg_len, K, int(mask), ctypes.byref(L))
    return {n: getattr(L, n) for n in pkg._LAYOUT_FIELDS}


def emit_index(msg_len, K, mask, which, j, t):
    return emit().multiemit_index(msg_len, K, int(mask), which, j, t)


def emit_instance(pks_xy, msgs, mask, n_witness):
    """the product's pair-lane logic on the host -> (witness [n_witness, 6] with the message / pk_not_zero / prep_pk segments of the Input arguments
    filled and zeros elsewhere, instance [n_instance_vars, 6] with the signature's elements left zero)"""
    pks, m, mp, _ = _inputs(pks_xy, msgs, np.zeros(24, dtype=np.uint64))
    K, msg_len = m.shape
    w = np.zeros((n_witness, 6), dtype=np.uint64)
    inst = np.zeros((n_instance_vars(K, msg_len, mask), 6), dtype=np.uint64)
    emit().multiemit_instance(pks.ctypes.data_as(u64p), mp, K, msg_len, int(mask), w.ctypes.data_as(u64p), inst.ctypes.data_as(u64p))
    return w, inst


def segments(lay):
    """[name, begin, end] of every segment of a product layout dict, in vector order (the per-pair segments as one run over all pairs)"""
    order = ["off_msg", "off_pk_alloc", "off_sig_alloc", "off_pk_not_zero", "off_expand", "off_prep_h", "off_prep_pk", "off_prep_sig", "off_miller", "off_final_exp", "off_is_one"]
    ends = [lay[k] for k in order[1:]] + [lay["n_witness"]]
    return [[k[4:], int(lay[k]), int(e)] for k, e in zip(order, ends)]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_inputs_digests.json")
GOLDEN_K, GOLDEN_MSG_LEN, GOLDEN_START = 2, 50, 11


def golden_case(oracle):
    """the fixed case of tests/golden/multi_inputs_digests.json: K = 2, msg_len 50, valid -> (pks, msgs, sig, expect)"""
    from tests import synth

    return synth.make_multi(oracle, GOLDEN_K, msg_len=GOLDEN_MSG_LEN, start=GOLDEN_START)


def digests(w, inst, lay):
    """sha256 of a vector, its segments and its instance as the golden file records them"""
    b = np.ascontiguousarray(w).view(np.uint8).reshape(w.shape[0], 48)
    return {"sha256_all": hashlib.sha256(b.tobytes()).hexdigest(), "sha256_instance": hashlib.sha256(np.ascontiguousarray(inst).tobytes()).hexdigest(),
            "sha256_segments": {name: hashlib.sha256(b[lo:hi].tobytes()).hexdigest() for name, lo, hi in segments(lay)}}
