"""ctypes loader for tests/vpairs/libvpairs.so: the stages of blsw_verify_pairs_batch (csrc/vpairs.hpp) compiled for the host (TEST HARNESS ONLY),
and the minting of aggregate signatures over distinct messages on the CPU."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
IDENTITY48 = bytes([0xC0]) + bytes(47)
_lib = None
u8p, u32p, i32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "vpairs"), "libvpairs.so"])
        _lib = ctypes.CDLL(os.path.join(HERE, "vpairs", "libvpairs.so"))
        _lib.vpairs_status.argtypes = [u32p, ctypes.c_uint64, ctypes.c_uint32, i32p]
        _lib.vpairs_chunk.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p]
    return _lib


def pack(rows, width):
    """a list of lists of byte strings -> uint8 [n, K, width], short lists padded with zero bytes"""
    K = max(1, max(len(r) for r in rows))
    out = np.zeros((len(rows), K, width), dtype=np.uint8)
    for i, r in enumerate(rows):
        for j, b in enumerate(r):
            assert len(b) == width
            out[i, j] = np.frombuffer(bytes(b), dtype=np.uint8)
    return out


def instances(pks, msgs, sigs, counts=None, chunks=(8,)):
    """the host stages over n instances: pks uint8 [n, K, 48], msgs uint8 [n, K, msg_len], sigs uint8 [n, 96], counts a list [n] or None, chunks the
    values of `chunk` to fold with -> (verdicts int32 [len(chunks), n], status [n, 2], key_status [n, K], written uint8 [n, K + 1])"""
    pks, msgs, sigs = (np.ascontiguousarray(a, dtype=np.uint8) for a in (pks, msgs, sigs))
    n, K, msg_len = pks.shape[0], pks.shape[1], msgs.shape[2]
    assert pks.shape == (n, K, 48) and msgs.shape == (n, K, msg_len) and sigs.shape == (n, 96)
    ms = msgs if msg_len else np.zeros(1, np.uint8)
    cn = None if counts is None else np.array([int(c) for c in counts], dtype=np.uint32)
    ch = np.array(chunks, dtype=np.uint32)
    res = np.full((len(ch), n), -1, dtype=np.int32)
    st = np.full((n, 2), -1, dtype=np.int32)
    kst = np.full((n, K), -1, dtype=np.int32)
    wr = np.zeros((n, K + 1), dtype=np.uint8)
    rc = load().vpairs_instances(pks.ctypes.data_as(u8p), ms.ctypes.data_as(u8p), ctypes.c_uint32(msg_len), ctypes.c_uint32(K), None if cn is None else cn.ctypes.data_as(u32p),
                                 sigs.ctypes.data_as(u8p), ctypes.c_uint64(n), ch.ctypes.data_as(u32p), ctypes.c_uint32(len(ch)), res.ctypes.data_as(i32p), st.ctypes.data_as(i32p),
                                 kst.ctypes.data_as(i32p), wr.ctypes.data_as(u8p))
    assert rc == 0
    return res, st, kst, wr


def instance(pks, msgs, sig, count=None, chunks=(8,)):
    """one instance from lists of byte strings -> (verdicts [len(chunks)], status [2], key_status [K])"""
    res, st, kst, _ = instances(pack([pks], 48), pack([msgs], len(msgs[0])), np.frombuffer(bytes(sig), np.uint8).reshape(1, 96), None if count is None else [count], chunks)
    return res[:, 0], st[0], kst[0]


def status(counts, i, K, key_status):
    """vp_instance_status: counts a list or None, key_status int32 [n, K]"""
    cn = None if counts is None else np.array(counts, dtype=np.uint32)
    ks = np.ascontiguousarray(key_status, dtype=np.int32)
    return load().vpairs_status(None if cn is None else cn.ctypes.data_as(u32p), i, K, ks.ctypes.data_as(i32p))


def chunk(chunk_, count, q):
    """vp_chunk and vp_chunk_mask: (first, count, mask of a folding instance, mask of one that does not fold)"""
    out = (ctypes.c_uint32 * 4)()
    load().vpairs_chunk(chunk_, count, q, out)
    return tuple(out)


def chunks_per_instance(K, chunk_):
    return load().vpairs_chunks_per_instance(K, chunk_)


def mint(oracle, sks, msgs):
    """(pk48 list, the aggregate signature of sk_j on msgs[j]) by the oracle's signer and its G2 sum"""
    pks = [oracle.sk_to_pk(sk) for sk in sks]
    sig = oracle.aggregate_g2([oracle.sign(sk, m) for sk, m in zip(sks, msgs)])
    assert sig is not None
    return pks, sig
