"""ctypes loader for tests/vshared/libvshared.so: the run rule and the stages of blsw_verify_groups_shared_batch (csrc/vshared.hpp) compiled for the
host (TEST HARNESS ONLY), next to the plain stages on materialised messages."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xFFFFFFFF
_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "vshared"), "libvshared.so"])
        _lib = ctypes.CDLL(os.path.join(HERE, "vshared", "libvshared.so"))
        _lib.vshared_rule.restype = ctypes.c_int32
        _lib.vshared_rule.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 8
        _lib.vshared_groups.restype = ctypes.c_int64
        _lib.vshared_groups.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 8
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rule(index, group, chunk, tile=64, n_msgs=3):
    """the rule of vshared.hpp over an index array -> dict of what the scan and the chunking store; slots beyond a group's runs keep SENTINEL"""
    idx = np.array(index, dtype=np.uint32)
    n = len(idx)
    n_groups = (n + group - 1) // group
    cpg = (min(group, n) + chunk - 1) // chunk
    out = dict(leader=np.zeros(n, np.uint8), slot_leader=np.full(n, SENTINEL, np.uint32), slot_len=np.full(n, SENTINEL, np.uint32), runs=np.zeros(n_groups, np.uint32),
               bad=np.zeros(n, np.uint8), chunk_first=np.zeros(n_groups * cpg, np.uint64), chunk_count=np.zeros(n_groups * cpg, np.uint32), chunk_walks=np.zeros(n_groups * cpg, np.uint8))
    rc = load().vshared_rule(n, group, chunk, tile, _p(idx), n_msgs, *[_p(out[k]) for k in ("leader", "slot_leader", "slot_len", "runs", "bad", "chunk_first", "chunk_count", "chunk_walks")])
    assert rc == cpg, rc
    return out


def groups(pks, sigs, table, msg_index, scalars, group, chunk, tile=64):
    """n triples over a message table (bytes each, rows of one length) -> dict: res_shared, res_plain, runs [G], f_shared, f_plain [G, 72] (the products
    of the partials before the final exponentiation), same_gt [G], st_shared, st_plain [n, 2]"""
    n, n_msgs, msg_len = len(pks), len(table), len(table[0])
    assert len(sigs) == len(msg_index) == len(scalars) == n and all(len(r) == msg_len for r in table)
    pk = np.frombuffer(b"".join(bytes(p).ljust(48, b"\0")[:48] for p in pks), dtype=np.uint8).copy()
    sg = np.frombuffer(b"".join(bytes(s).ljust(96, b"\0")[:96] for s in sigs), dtype=np.uint8).copy()
    ms = np.frombuffer(b"".join(table) or b"\0", dtype=np.uint8).copy()
    idx = np.array(msg_index, dtype=np.uint32)
    sc = np.array([int(r) for r in scalars], dtype=np.uint64)
    n_groups = (n + group - 1) // group
    out = dict(st_shared=np.zeros((n, 2), np.int32), st_plain=np.zeros((n, 2), np.int32), res_shared=np.zeros(n_groups, np.int32), res_plain=np.zeros(n_groups, np.int32),
               runs=np.zeros(n_groups, np.uint32), f_shared=np.zeros((n_groups, 72), np.uint64), f_plain=np.zeros((n_groups, 72), np.uint64), same_gt=np.zeros(n_groups, np.int32))
    rc = load().vshared_groups(_p(pk), _p(sg), _p(ms), msg_len, n_msgs, _p(idx), _p(sc), n, group, chunk, tile,
                               *[_p(out[k]) for k in ("st_shared", "st_plain", "res_shared", "res_plain", "runs", "f_shared", "f_plain", "same_gt")])
    assert rc == n_groups, rc
    return out
