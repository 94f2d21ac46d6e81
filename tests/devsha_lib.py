"""ctypes loaders and the launch-and-compare steps for the SHA gadget operation table (tests/devsha/ops.hpp; TEST HARNESS ONLY): the host
compilation through tests/hostsim (hostsim_sha_op_batch) and the device compilations through tests/devsha/libdevsha.so, against tests/sha_ref.py.
Every array an entry writes into starts as a position-dependent sentinel and is compared WHOLE; on the device the bit words leave through the
sink's 64-byte runs into a guarded buffer of k_sha's tile addressing (tests/stream_ref.py: word_index), of which only the words of a partial last
run behind a lane's stream are excepted (never read, not defined)."""
import ctypes
import os
import subprocess

import numpy as np

from tests import hostsim_lib
from tests import sha_edges as X
from tests import sha_ref as S
from tests import stream_ref as SR

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devsha")
IN_MAX, OUT_MAX = 72, 64
GUARD = 1 << 16  # u32 words (256 KiB) in front of and behind the tiles
BUILDS = {"grouped": "devsha_run", "inl": "devsha_run_inl"}  # the compilations of csrc/k_sha.hip: k_sha (register policy W2) and k_sha_inl

u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)
u64p = ctypes.POINTER(ctypes.c_uint64)
_dev = None


def load_device():
    global _dev
    if _dev is None:
        import torch  # noqa: F401  BEFORE the library: it brings the process's HIP runtime (a harness library loaded first gives the process two)

        subprocess.check_call(["make", "-s", "-j2", "-C", HERE])
        _dev = ctypes.CDLL(os.path.join(HERE, "libdevsha.so"))
        for name in BUILDS.values():
            getattr(_dev, name).restype = ctypes.c_int
    return _dev


def host_table():
    """[(name, operand words, result words, takes a message)] of the compiled table"""
    H = hostsim_lib.load()
    H.hostsim_sha_op_name.restype = ctypes.c_char_p
    return [(H.hostsim_sha_op_name(i).decode(), H.hostsim_sha_op_n_in(i), H.hostsim_sha_op_n_out(i), H.hostsim_sha_op_msg(i)) for i in range(H.hostsim_sha_op_count())]


def sentinel(n, salt=0):
    return ((np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) + np.uint64(0x7F4A7C15)).astype(np.uint32)


def pack_bits(bits):
    """0 / 1 array -> u32 words, bit b of the stream = bit b & 31 of word b / 32, the last word's upper bits zero"""
    bits = np.asarray(bits, dtype=np.uint8)
    full = np.zeros((len(bits) + 31) // 32 * 32, dtype=np.uint8)
    full[:len(bits)] = bits
    return np.packbits(full, bitorder="little").view(np.uint32)


_WALKS = {}


def gadget_walk(msg_len):
    """the reference's walk of the whole expansion at one length over the sha_edges.LANES messages, once per process ->
    dict(bits uint8 [lanes][n], words [lanes][64], marks, carries, index: message -> lane)"""
    if msg_len not in _WALKS:
        msgs = X.messages(msg_len)
        g, words = S.expand_gadget(msgs)
        _WALKS[msg_len] = dict(bits=S.stream_matrix(g.stream, len(msgs)), words=words, marks=g.marks, carries=g.carries, index={m: l for l, m in enumerate(msgs)})
    return _WALKS[msg_len]


def expect_launch(op, msg_len, cases):
    """-> (result words per item, bit arrays per item)"""
    if op == "expand_message_w":
        w = gadget_walk(msg_len)
        lanes = [w["index"][m] for _, m in cases]
        return [w["words"][l] for l in lanes], [w["bits"][l] for l in lanes]
    outs, streams = [], []
    for c in cases:
        o, b = S.expected(op, c)
        outs.append(o)
        streams.append(np.array(b, dtype=np.uint8))
    return outs, streams


def _arrays(op, msg_len, cases):
    n = len(cases)
    n_in = S.OPS[op][0]
    ins = sentinel(n * IN_MAX, 3).reshape(n, IN_MAX)
    for i, (w, _) in enumerate(cases):
        assert len(w) == n_in
        ins[i, :n_in] = np.array(w, dtype=np.uint64).astype(np.uint32) if n_in else 0
    msg = np.zeros(max(1, n * msg_len), dtype=np.uint8)
    if msg_len:
        msg[:] = np.frombuffer(b"".join(m for _, m in cases), dtype=np.uint8)
        assert all(len(m) == msg_len for _, m in cases)
    out = sentinel(n * OUT_MAX, 5).reshape(n, OUT_MAX)
    return ins, msg, out


def _check_out(op, outs, got, bad):
    want = sentinel(got.size, 5).reshape(got.shape)
    for i, o in enumerate(outs):
        want[i, :len(o)] = np.array(o, dtype=np.uint64).astype(np.uint32)
    for i in np.flatnonzero((got != want).any(axis=1))[:4]:
        j = int(np.flatnonzero(got[i] != want[i])[0])
        bad.append(("item %d result word %d%s" % (i, j, " (not the entry's: a stray store)" if j >= S.OPS[op][1] else ""), hex(int(got[i, j])), hex(int(want[i, j]))))


def _first_bit(op, msg_len, got_words, want_bits):
    """the first differing bit of a stream, by name where the reference has marks for it"""
    got = np.unpackbits(np.asarray(got_words, dtype=np.uint32).view(np.uint8), bitorder="little")
    n = min(len(got), len(want_bits))
    d = np.flatnonzero(got[:n] != want_bits[:n])
    pos = int(d[0]) if d.size else n
    where = S.where_is(gadget_walk(msg_len)["marks"], pos) if op == "expand_message_w" else ""
    return "bit %d%s" % (pos, " (" + where + ")" if where else "")


def run_host(op, msg_len, cases):
    """one launch through hostsim_sha_op_batch -> list of mismatches"""
    H = hostsim_lib.load()
    n = len(cases)
    outs, streams = expect_launch(op, msg_len, cases)
    ins, msg, out = _arrays(op, msg_len, cases)
    cap = max(len(b) for b in streams) // 32 + 4
    words = sentinel(n * cap, 7).reshape(n, cap)
    nwords = sentinel(n, 9)
    nbits = np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = H.hostsim_sha_op_batch(S.OP_NAMES.index(op), ctypes.c_uint64(n), ins.ctypes.data_as(u32p), msg.ctypes.data_as(u8p), ctypes.c_uint32(msg_len), out.ctypes.data_as(u32p),
                                words.ctypes.data_as(u32p), ctypes.c_uint64(cap), nwords.ctypes.data_as(u32p), nbits.ctypes.data_as(u64p))
    bad = []
    if rc:
        return [("hostsim_sha_op_batch returned %d (-2: an item's stream is longer than the reference's by more than three words)" % rc,)]
    _check_out(op, outs, out, bad)
    want = sentinel(n * cap, 7).reshape(n, cap)
    for i, b in enumerate(streams):
        w = pack_bits(b)
        want[i, :len(w)] = w
        if int(nbits[i]) != len(b) or int(nwords[i]) != len(w):
            bad.append(("item %d" % i, "%d bits in %d words" % (nbits[i], nwords[i]), "%d bits in %d words" % (len(b), len(w))))
    for i in np.flatnonzero((words != want).any(axis=1))[:4]:
        bad.append(("item %d stream" % i, _first_bit(op, msg_len, words[i, :(len(streams[i]) + 31) // 32], streams[i])))
    return bad


def run_device(build, op, msg_len, cases):
    """one launch of a device compilation -> list of mismatches"""
    L = load_device()
    n = len(cases)
    outs, streams = expect_launch(op, msg_len, cases)
    ins, msg, out = _arrays(op, msg_len, cases)
    lane_words = [pack_bits(b) for b in streams]
    sha_words = SR.align_up(max(len(w) for w in lane_words), SR.CHUNK_WORDS) + SR.CHUNK_WORDS  # one run more than any stream needs: the sentinel behind it
    tiles = (n + 63) // 64
    total = 2 * GUARD + tiles * sha_words * 64
    bits = sentinel(total, 11)
    want = bits.copy()
    compared = np.ones(total, dtype=bool)
    for l, w in enumerate(lane_words):
        idx = np.arange(SR.align_up(len(w), SR.CHUNK_WORDS), dtype=np.int64)
        at = GUARD + (l >> 6) * sha_words * 64 + (idx // 16) * 1024 + (l & 63) * 16 + idx % 16
        assert len(w) == 0 or at[0] == GUARD + SR.word_index(l, 0, sha_words) and at[len(w) - 1] == GUARD + SR.word_index(l, len(w) - 1, sha_words)
        want[at[:len(w)]] = w
        compared[at[len(w):]] = False
    nwords = sentinel(n, 9)
    rc = getattr(L, BUILDS[build])(S.OP_NAMES.index(op), ctypes.c_uint64(n), ins.ctypes.data_as(u32p), msg.ctypes.data_as(u8p), ctypes.c_uint32(msg_len), out.ctypes.data_as(u32p),
                                   bits.ctypes.data_as(u32p), ctypes.c_uint64(total), ctypes.c_uint64(GUARD), ctypes.c_uint64(sha_words), nwords.ctypes.data_as(u32p))
    assert rc == 0, "%s returned %d for %s, msg_len %d, %d items" % (BUILDS[build], rc, op, msg_len, n)
    bad = []
    _check_out(op, outs, out, bad)
    for l, w in enumerate(lane_words):
        if int(nwords[l]) != len(w):
            bad.append(("item %d" % l, "%d words" % nwords[l], "%d words" % len(w)))
    d = np.flatnonzero((bits != want) & compared)
    if d.size:
        i = int(d[0]) - GUARD
        if 0 <= i < tiles * sha_words * 64:
            lane, word = (i // (sha_words * 64)) * 64 + i % 1024 // 16, (i % (sha_words * 64)) // 1024 * 16 + i % 16
            what = "item %d word %d" % (lane, word)
            if lane < n and word < len(lane_words[lane]):
                at = GUARD + np.array([SR.word_index(lane, k, sha_words) for k in range(len(lane_words[lane]))], dtype=np.int64)
                what += ", " + _first_bit(op, msg_len, bits[at], streams[lane])
            else:
                what += " (a SENTINEL word: a stray store)"
        else:
            what = "word %d of the guard (a stray store)" % i
        bad.append(("%d words differ, the first: %s" % (d.size, what), hex(int(bits[d[0]])), hex(int(want[d[0]]))))
    return bad
