"""ctypes loader for tests/registry/libregistry.so: the stages of blsw_registry_append / blsw_registry_verify_batch (csrc/registry.hpp) compiled for the
host (TEST HARNESS ONLY) — the decode into 128-byte records, and the lane walks over index lists, tree and finish of every set for a given number of
lanes L — and the cases the two test files share."""
import ctypes
import os
import subprocess

import numpy as np

from tests.committee_lib import IDENTITY48, R_MOD, TORSION48, EDGE_SK_P, EDGE_SK_Q, bad_encodings, negated

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
ST_OK, ST_IDENTITY, ST_BAD_INDEX = 0, 4, 6
RECORD_BYTES = 128


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "registry"), "libregistry.so"])
        _lib = ctypes.CDLL(os.path.join(HERE, "registry", "libregistry.so"))
        _lib.registry_sum.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]
        _lib.registry_append.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    return _lib


class HostRegistry:
    """the handle's state on the host: `capacity` records (128-byte aligned, filled with 0xEE: a row that was never appended holds no zeros),
    the status array and the size"""

    def __init__(self, capacity):
        self.capacity, self.size = capacity, 0
        raw = np.full(capacity * RECORD_BYTES + RECORD_BYTES, 0xEE, dtype=np.uint8)
        skip = (-raw.ctypes.data) % RECORD_BYTES
        self.records = raw[skip:skip + capacity * RECORD_BYTES]
        self._raw = raw
        self.status = np.full(capacity, 0x5A5A5A5A, dtype=np.int32)

    def append(self, pks):
        assert all(len(p) == 48 for p in pks) and self.size + len(pks) <= self.capacity
        if pks:
            raw = np.frombuffer(b"".join(pks), dtype=np.uint8).copy()
            load().registry_append(raw.ctypes.data, self.size, len(pks), self.records.ctypes.data, self.status.ctypes.data)
            self.size += len(pks)
        return self

    def key_status(self):
        return self.status[:self.size].copy()

    def xy(self, k):
        """the affine coordinates of key k as the oracle prints them: uint64 [12]"""
        return self.records[k * RECORD_BYTES:k * RECORD_BYTES + 96].view(np.uint64).copy()


def csr(lists):
    """lists of indices -> (indices uint32 [n_indices], offsets uint64 [n + 1])"""
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    flat = [int(k) for x in lists for k in x]
    return np.array(flat, dtype=np.uint32), off


def sums(reg, indices, offsets, L, size=None, n_indices=None):
    """-> (pk_xy uint64 [n, 12], status int32 [n], agg48 [bytes] * n); size / n_indices default to the registry's size and len(indices)"""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    pk_xy = np.zeros((n, 24), dtype=np.uint32)
    status = np.full(n, -1, dtype=np.int32)
    agg = np.full((n, 48), 0x5A, dtype=np.uint8)
    rc = load().registry_sum(reg.records.ctypes.data, reg.size if size is None else size, indices.ctypes.data if len(indices) else None,
                             len(indices) if n_indices is None else n_indices, offsets.ctypes.data, n, L, pk_xy.ctypes.data, status.ctypes.data, agg.ctypes.data)
    assert rc == 0
    return pk_xy.view(np.uint64), status, [a.tobytes() for a in agg]


def expected(oracle, pks, key_status, size, lst):
    """what the header promises for one list with good offsets, from the oracle alone: (status, agg48)"""
    for k in lst:
        if k >= size:
            return ST_BAD_INDEX, bytes(48)
        if key_status[k] not in (ST_OK, ST_IDENTITY):
            return int(key_status[k]), bytes(48)
    agg = oracle.aggregate_g1([pks[k] for k in lst]) if len(lst) else IDENTITY48
    assert agg is not None
    return (ST_IDENTITY if agg == IDENTITY48 else ST_OK), agg


def list_lengths(L):
    return sorted({k for k in (0, 1, L - 1, L, L + 1, 2 * L + 1, 3 * L) if k >= 0})


def _sk(i):
    return 0x1000003 + 7919 * i


BASE_KEYS = 20  # ordinary keys in front of the special ones of edge_registry


def edge_registry(oracle):
    """One registry for every group-law and bad-key edge: BASE_KEYS ordinary keys, then P, -P, Q, the identity, one key per failing decode status and
    the order-3 point -> (pks, sks, names): sks[k] is key k's secret key (None when it has none), names maps a word to its index"""
    pks = [oracle.sk_to_pk(_sk(300 + k)) for k in range(BASE_KEYS)]
    sks = [_sk(300 + k) for k in range(BASE_KEYS)]
    names = {}

    def add(name, pk, sk):
        names[name] = len(pks)
        pks.append(pk)
        sks.append(sk)

    P, Q = oracle.sk_to_pk(EDGE_SK_P), oracle.sk_to_pk(EDGE_SK_Q)
    add("P", P, EDGE_SK_P)
    add("-P", negated(P), R_MOD - EDGE_SK_P)
    add("Q", Q, EDGE_SK_Q)
    add("identity", IDENTITY48, 0)
    for st, b in sorted(bad_encodings(oracle).items()):
        add("bad%d" % st, b, None)
    add("torsion", TORSION48, None)
    return pks, sks, names


def edge_lists(L, names, size, capacity):
    """The index lists of the group-law edges and the bad entries for L lanes over edge_registry -> [(name, list, expected status or None)]. A status
    of None: the list is good, the oracle's aggregate decides between OK and IDENTITY. Fillers are the ordinary keys 0, 1, 2, ..."""
    P, NP, Q, I = names["P"], names["-P"], names["Q"], names["identity"]
    fill = lambda n, start=0: [(start + k) % BASE_KEYS for k in range(n)]

    def at(n, puts):  # a list of n fillers with the given positions replaced
        lst = fill(n)
        for p, k in puts.items():
            lst[p] = k
        return lst

    out = [("the same index at positions 0 and L, then Q in the lane: the lane doubles", at(2 * L + 1, {0: P, L: P, 2 * L: Q}), None),
           ("the same index at positions 0 and 1, nothing else: the tree doubles (L >= 2)", [P, P], None),
           ("a key, its negation and Q in one lane: the accumulator passes through the identity", at(2 * L + 1, {0: P, L: NP, 2 * L: Q}), None),
           ("a key and its negation in two lanes: the tree adds opposite points", [P, NP], ST_IDENTITY),
           ("an identity key among others", [0, I, 1], None),
           ("an identity key alone", [I], ST_IDENTITY),
           ("one index 3 L times", [Q] * (3 * L), None)]
    for st in (1, 2, 3):
        out.append(("a key of status %d in the middle" % st, at(2 * L + 1, {L: names["bad%d" % st]}), st))
    out.append(("the order-3 point", [0, names["torsion"]], 3))
    out.append(("index == size", at(L + 1, {L: size}), ST_BAD_INDEX))
    out.append(("index == 0xffffffff", [0xFFFFFFFF] + fill(L), ST_BAD_INDEX))
    out.append(("an index >= size below the capacity", at(2 * L + 1, {2 * L: capacity - 1}), ST_BAD_INDEX))
    out.append(("a bad key then a bad index: the earlier position wins", at(2 * L + 1, {1: names["bad2"], 2 * L: size}), 2))
    out.append(("a bad index then a bad key", at(2 * L + 1, {1: size + 1, 2 * L: names["bad2"]}), ST_BAD_INDEX))
    out.append(("two bad keys, the earlier position wins", at(2 * L + 1, {0: names["bad1"], 2 * L: names["bad2"]}), 1))
    out.append(("two bad keys the other way round", at(2 * L + 1, {0: names["bad2"], 2 * L: names["bad1"]}), 2))
    return out


def list_sk(sks, lst, size):
    """the sum of the secret keys a list names, mod r; None when an entry has none"""
    chosen = [sks[k] if k < size else None for k in lst]
    return None if any(s is None for s in chosen) else sum(chosen) % R_MOD
