"""ctypes loaders for tests/agg_inputs (TEST HARNESS ONLY): libaggshim.so, the aggregate_verify circuit with Input arguments composed from the
oracle's headers, and libaggemit.so, the product's key source and instance element function compiled for the host."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agg_inputs")
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)
KEYS, BITMAP, MSG, SIG = 1, 2, 4, 8  # bits of the mask (include/blsw.h: BLSW_AGG_*_INPUT)
CHUNK = 47  # message bytes per public input
# shim mark -> field of blsw_layout_t
MARKS = (("agg.keys", "off_keys"), ("agg.bitmap", "off_bitmap"), ("msg", "off_msg"), ("sig_alloc", "off_sig_alloc"), ("agg.count", "off_count"), ("agg.loop", "off_agg"),
         ("verify.pk_not_zero", "off_pk_not_zero"), ("hash.expand", "off_expand"), ("hash.map0", "off_map0"), ("hash.map1", "off_map1"), ("hash.add", "off_add"),
         ("hash.clear_cofactor", "off_cofactor"), ("prepare.h", "off_prep_h"), ("prepare.pk", "off_prep_pk"), ("prepare.sig", "off_prep_sig"), ("miller", "off_miller"),
         ("final_exp", "off_final_exp"), ("is_one", "off_is_one"))

_libs = {}


def _load(name):
    if name not in _libs:
        subprocess.check_call(["make", "-s", "-C", HERE])
        L = ctypes.CDLL(os.path.join(HERE, name))
        for f in ("agsh_witness", "agsh_layout", "agsh_matrices"):
            if hasattr(L, f):
                getattr(L, f).restype = ctypes.c_uint64
        if hasattr(L, "agsh_check"):
            L.agsh_check.restype = ctypes.c_int64
        if hasattr(L, "aggemit_instance"):
            L.aggemit_instance.restype = ctypes.c_uint32
        _libs[name] = L
    return _libs[name]


def shim():
    return _load("libaggshim.so")


def emit():
    return _load("libaggemit.so")


def chunks(msg_len):
    return (msg_len + CHUNK - 1) // CHUNK


def n_instance_vars(K, msg_len, mask):
    return 1 + (3 * K if mask & KEYS else 0) + (K if mask & BITMAP else 0) + (chunks(msg_len) if mask & MSG else 0) + (6 if mask & SIG else 0)


def _buf(msg):
    b = bytes(msg)
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def _inputs(pks_xy, bitmap, sig_xy):
    pks = np.ascontiguousarray(pks_xy, dtype=np.uint64).reshape(-1, 12)
    bm = np.ascontiguousarray(bitmap, dtype=np.uint8).reshape(-1)
    sig = np.ascontiguousarray(sig_xy, dtype=np.uint64).reshape(-1)
    assert pks.shape[0] == bm.size and sig.size == 24
    return pks, bm, sig


def witness(pks_xy, bitmap, msg, sig_xy, mask):
    """-> (result, count, witness [n_witness, 6] uint64, instance [n_instance_vars, 6] uint64, n_constraints)"""
    pks, bm, sig = _inputs(pks_xy, bitmap, sig_xy)
    nc, ni, res, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint32(0)
    args = lambda w, cap, inst: (pks.ctypes.data_as(u64p), bm.ctypes.data_as(u8p), ctypes.c_size_t(bm.size), _buf(msg), ctypes.c_size_t(len(msg)),
                                 sig.ctypes.data_as(u64p), int(mask), w, ctypes.c_uint64(cap), inst, ctypes.byref(ni), ctypes.byref(nc), ctypes.byref(res), ctypes.byref(cnt))
    n = n_witness_of(bm.size, len(msg), mask)
    w = np.zeros((n, 6), dtype=np.uint64)
    inst = np.zeros((n_instance_vars(bm.size, len(msg), mask), 6), dtype=np.uint64)
    got = shim().agsh_witness(*args(w.ctypes.data_as(u64p), n, inst.ctypes.data_as(u64p)))
    assert got == n and ni.value == inst.shape[0]
    return bool(res.value), int(cnt.value), w, inst, nc.value


_NW = {}


def n_witness_of(K, msg_len, mask):
    if (K, msg_len, mask) not in _NW:
        _NW[(K, msg_len, mask)] = layout(K, msg_len, mask)[1]
    return _NW[(K, msg_len, mask)]


def layout(K, msg_len, mask):
    """-> (marks {name: witness index}, n_witness, n_constraints, n_instance_vars)"""
    starts = (ctypes.c_uint64 * 64)()
    names = ctypes.create_string_buffer(4096)
    nw, nc, ni = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    k = shim().agsh_layout(ctypes.c_size_t(K), ctypes.c_size_t(msg_len), int(mask), starts, ctypes.c_uint64(64), names, ctypes.c_size_t(4096), ctypes.byref(nw),
                           ctypes.byref(nc), ctypes.byref(ni))
    nm = names.value.decode().split("\n")[:k]
    return {nm[i]: starts[i] for i in range(k)}, nw.value, nc.value, ni.value


def matrices(K, msg_len, mask):
    """-> (n_constraints, n_witness, n_instance_vars, [(row_ptr, col, val)] * 3)"""
    nnz = (ctypes.c_uint64 * 3)()
    nw, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
    a = (ctypes.c_size_t(K), ctypes.c_size_t(msg_len), int(mask), nnz, ctypes.byref(nw), ctypes.byref(ni))
    nc = shim().agsh_matrices(*a, None, None, None)
    rp = [np.zeros(nc + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(nnz[m], dtype=np.uint32) for m in range(3)]
    val = [np.zeros((nnz[m], 6), dtype=np.uint64) for m in range(3)]
    RP = (u64p * 3)(*[r.ctypes.data_as(u64p) for r in rp])
    CO = (ctypes.POINTER(ctypes.c_uint32) * 3)(*[c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) for c in col])
    VA = (u64p * 3)(*[v.ctypes.data_as(u64p) for v in val])
    shim().agsh_matrices(*a, RP, CO, VA)
    return nc, nw.value, ni.value, [(rp[m], col[m], val[m]) for m in range(3)]


def check(pks_xy, bitmap, msg, sig_xy, mask, instance=None, witness=None):
    """first unsatisfied constraint of z = [instance | witness] (None: the shim's own), -1 when satisfied"""
    pks, bm, sig = _inputs(pks_xy, bitmap, sig_xy)
    ip = np.ascontiguousarray(instance, dtype=np.uint64) if instance is not None else None
    wp = np.ascontiguousarray(witness, dtype=np.uint64) if witness is not None else None
    return shim().agsh_check(pks.ctypes.data_as(u64p), bm.ctypes.data_as(u8p), ctypes.c_size_t(bm.size), _buf(msg), ctypes.c_size_t(len(msg)), sig.ctypes.data_as(u64p),
                             int(mask), ip.ctypes.data_as(u64p) if ip is not None else None, wp.ctypes.data_as(u64p) if wp is not None else None,
                             ctypes.c_uint64(wp.shape[0] if wp is not None else 0))


def emit_instance(pks_xy, bitmap, msg_len, mask, n_witness):
    """the product's device logic on the host (Input keys) -> (count, witness [n_witness, 6] with the bitmap / count / agg / pk_not_zero / prep_pk
    segments filled and zeros elsewhere, head of instance_assignment [1 + 3 K (+ K), 6])"""
    pks = np.ascontiguousarray(pks_xy, dtype=np.uint64).reshape(-1, 12)
    bm = np.ascontiguousarray(bitmap, dtype=np.uint8).reshape(-1)
    K = bm.size
    w = np.zeros((n_witness, 6), dtype=np.uint64)
    inst = np.zeros((1 + 4 * K, 6), dtype=np.uint64)
    head = ctypes.c_uint32(0)
    cnt = emit().aggemit_instance(pks.ctypes.data_as(u64p), bm.ctypes.data_as(u8p), K, msg_len, int(mask), w.ctypes.data_as(u64p), inst.ctypes.data_as(u64p), ctypes.byref(head))
    return int(cnt), w, inst[: head.value]


def reference_case(oracle):
    """constraints.rs:378-441: 512 keys (key 1, then 511 x key 2), message 0x56 * 32 and the signature of the fast_aggregate_verify fixture; the reference
    selects the first two keys (true, count 2). -> (pks [512, 12], msg bytes, sig [24])"""
    pk1 = "a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a"
    pk2 = "b301803f8b5ac4a1133581fc676dfedc60d891dd5fa99028805e5ea5b08d3491af75d0707adab3b70c6a6a580217bf81"
    sig = "912c3615f69575407db9392eb21fee18fff797eeb2fbe1816366ca2a08ae574d8824dbfafb4c9eaa1cf61b63c6f9b69911f269b664c42947dd1b53ef1081926c1e82bb2a465f927124b08391a5249036146d6f3f1e17ff5f162f779746d830d1"
    _, p1, _ = oracle.g1_decompress(bytes.fromhex(pk1))
    _, p2, _ = oracle.g1_decompress(bytes.fromhex(pk2))
    _, s, _ = oracle.g2_decompress(bytes.fromhex(sig))
    return np.stack([p1] + [p2] * 511), bytes.fromhex("56" * 32), s, (pk1, pk2, sig)


def segments(lay):
    """[name, begin, end] of every segment of a layout dict, in vector order"""
    order = ["off_keys", "off_bitmap", "off_msg", "off_sig_alloc", "off_count", "off_agg", "off_pk_not_zero", "off_expand", "off_map0", "off_map1", "off_add",
             "off_cofactor", "off_prep_h", "off_prep_pk", "off_prep_sig", "off_miller", "off_final_exp", "off_is_one"]
    ends = [lay[k] for k in order[1:]] + [lay["n_witness"]]
    return [[k[4:], int(lay[k]), int(e)] for k, e in zip(order, ends)]
