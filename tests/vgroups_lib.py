"""ctypes loader for tests/vgroups/libvgroups.so: the stages of blsw_verify_groups_batch (csrc/vgroups.hpp) compiled for the host (TEST HARNESS
ONLY), and the minting of valid triples on the CPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import hostsim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "vgroups")])
        _lib = ctypes.CDLL(os.path.join(HERE, "vgroups", "libvgroups.so"))
    return _lib


def group(pks, msgs, sigs, scalars, chunk):
    """one group of triples (bytes each, messages of one length) with its coefficients -> (verdict, statuses [m, 2])"""
    m, msg_len = len(pks), len(msgs[0])
    assert len(msgs) == len(sigs) == len(scalars) == m and all(len(x) == msg_len for x in msgs)
    pk = np.frombuffer(b"".join(bytes(p).ljust(48, b"\0")[:48] for p in pks), dtype=np.uint8).copy()
    sg = np.frombuffer(b"".join(bytes(s).ljust(96, b"\0")[:96] for s in sigs), dtype=np.uint8).copy()
    ms = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
    sc = np.array([int(r) for r in scalars], dtype=np.uint64)
    st = np.zeros((m, 2), dtype=np.int32)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    r = load().vgroups_group(pk.ctypes.data_as(u8p), sg.ctypes.data_as(u8p), ms.ctypes.data_as(u8p), msg_len, sc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), m, chunk,
                             st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return r, st


def mint(oracle, sk, msg):
    """(pk48, sig96) of secret key sk on msg, by the device signer's logic on the host over the oracle's hash"""
    _, h_xy = oracle.hash_to_g2(msg)
    st, sig, pk = hostsim_lib.sign((sk % R_MOD).to_bytes(32, "little"), h_xy)
    assert st == 0
    return pk, sig
