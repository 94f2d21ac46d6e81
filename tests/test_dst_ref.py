"""The tag-taking expansion of csrc/sha.hpp through its host compilation (tests/dst: the host construction of k_sha_values_dst's kernel argument,
and the function the lanes run on that argument) against the independent statement tests/dst_ref.py — hashlib's expand_message_xmd and integers
mod p — at every tag length, and the tag constructors of include/blsw.h. No GPU: the device test (test_dst_gpu.py) holds the kernel to the same
statement."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests import dst_ref as R
from tests import hostsim_lib
from tests import sha_ref as S

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dst")
u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def shim():
    subprocess.check_call(["make", "-s", "-C", HERE])
    L = ctypes.CDLL(os.path.join(HERE, "libdst.so"))
    L.dst_arg_words.restype = ctypes.c_uint32
    return L


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def tag_of(L, salt=0):
    """L bytes that include 0x00, 0x80 and 0xff wherever the length allows, and differ from tag to tag"""
    special = [0x00, 0x80, 0xFF]
    return bytes(special[(k + salt) % 3] if k % 2 == 0 else (0x21 + 7 * k + salt) & 0xFF for k in range(L))


def message(n, salt=0):
    return bytes((0xA7 * k + 0x3D + salt) & 0xFF for k in range(n))


def run_batch(shim, dst, msgs, want_u=True):
    """messages of one length through dst_batch -> (uniform words [n][64], u [n][4][12] Montgomery limbs)"""
    n, msg_len = len(msgs), len(msgs[0])
    flat = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()  # never empty
    d = np.frombuffer(dst + b"\0", dtype=np.uint8).copy()
    uw = np.zeros((n, 64), dtype=np.uint32)
    u = np.zeros((n, 4, 12), dtype=np.uint32)
    rc = shim.dst_batch(d.ctypes.data_as(u8p), ctypes.c_uint32(len(dst)), flat.ctypes.data_as(u8p), ctypes.c_uint32(msg_len), ctypes.c_uint64(n), uw.ctypes.data_as(u32p),
                        u.ctypes.data_as(u32p) if want_u else None)
    assert rc == 0
    return uw, u


def expect_words(msg, dst):
    b = S.expand_message_xmd(msg, 256, dst)
    return [int.from_bytes(b[4 * i:4 * i + 4], "big") for i in range(64)]


def limbs_to_int(l):
    return sum(int(x) << (32 * i) for i, x in enumerate(l))


def test_reference_is_pinned():
    assert R.pin()
    assert R.hash_to_field(b"abc", R.DST_DEFAULT) == [S.hash_to_field(S.expand_message_xmd(b"abc")[64 * j:64 * j + 64]) for j in range(4)]


def test_reference_equals_the_oracle_at_the_library_tag(oracle):
    """dst_ref.hash_to_g2 under the library's tag is oracle.hash_to_g2 on the reference's five test_hash_to_curve messages (hasher.rs:1006-1012)"""
    import json

    lit = json.load(open(os.path.join(R.GOLDEN, "literals.json")))
    for s in lit["hash_strings"]:
        m = s.encode("utf-8")
        c, aff = oracle.hash_to_g2(m)
        pt = R.hash_to_g2(m, R.DST_DEFAULT)
        assert R.C.g2_compress(pt) == c and R.g2_limbs(pt) == [int(x) for x in aff], s


def test_every_tag_length_and_message_length(shim):
    """L in 1 .. 255 crossed with msg_len in 0 .. 130: the uniform bytes are hashlib's, the field elements the integers mod p (in Montgomery form)"""
    bad = []
    for L in range(1, 256):
        dst = tag_of(L, L)
        for msg_len in range(0, 131):
            msgs = [message(msg_len, L + msg_len)]
            uw, u = run_batch(shim, dst, msgs)
            want = expect_words(msgs[0], dst)
            if [int(x) for x in uw[0]] != want:
                bad.append((L, msg_len, "words"))
                continue
            e = R.hash_to_field(msgs[0], dst)
            if [limbs_to_int(u[0, j]) for j in range(4)] != [v * S.R % S.P for v in e]:
                bad.append((L, msg_len, "field"))
    assert not bad, bad[:10]


def boundary_lengths(L, limit=8081):
    """msg_len <= limit at which 77 + msg_len + L is 64 k - 1, 64 k or 64 k + 1: b_0's padded end one byte below, on and above a block boundary"""
    out = []
    k = (77 + L) // 64
    while True:
        base = 64 * k - 77 - L
        if base - 1 > limit:
            return out
        out += [m for m in (base - 1, base, base + 1) if 0 <= m <= limit]
        k += 1


def test_block_boundaries_up_to_8081(shim):
    """every boundary length up to 8081 at the tag lengths where b_i gains a block (and the library's 43), three lanes of different messages each"""
    bad, count = [], 0
    for L in (1, 21, 22, 43, 85, 86, 149, 150, 213, 214, 255):
        dst = tag_of(L, 1)
        lens = boundary_lengths(L)
        assert lens[-1] >= 8081 - 64 and len(lens) >= 3 * 120
        for msg_len in lens:
            msgs = [message(msg_len, s) for s in range(3)]
            uw, _ = run_batch(shim, dst, msgs, want_u=False)
            count += 1
            for i, m in enumerate(msgs):
                if [int(x) for x in uw[i]] != expect_words(m, dst):
                    bad.append((L, msg_len, i))
    assert not bad and count > 4000, (count, bad[:10])


def test_library_tag_equals_the_fixed_tag_expansion(shim):
    """at the library's tag the new function's words equal expand_message_values', bit for bit, through tests/hostsim's compilation of it"""
    H = hostsim_lib.load()
    op = S.OP_NAMES.index("expand_message_values")
    for msg_len in list(range(0, 131)) + [255, 256, 1000, 8081]:
        msgs = [message(msg_len, s) for s in range(4)]
        uw, _ = run_batch(shim, S.DST, msgs, want_u=False)
        n = len(msgs)
        ins = np.zeros((n, 72), dtype=np.uint32)
        flat = np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()
        out = np.zeros((n, 64), dtype=np.uint32)
        words, nwords, nbits = np.zeros((n, 8), dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        rc = H.hostsim_sha_op_batch(op, ctypes.c_uint64(n), ins.ctypes.data_as(u32p), flat.ctypes.data_as(u8p), ctypes.c_uint32(msg_len), out.ctypes.data_as(u32p),
                                    words.ctypes.data_as(u32p), ctypes.c_uint64(8), nwords.ctypes.data_as(u32p), nbits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        assert rc == 0 and np.array_equal(out, uw), msg_len


def test_kernel_argument(shim):
    """the argument the device gets: its block counts are the issue's formulas, everything behind the used words is zero, a lane that consumes the
    exported words gives the batch's result, and the tag lengths the library refuses are refused here too"""
    nw = shim.dst_arg_words()
    for L, msg_len in ((1, 0), (21, 5), (22, 5), (43, 32), (43, 48), (85, 7), (86, 7), (149, 1), (150, 1), (213, 130), (214, 130), (255, 8081)):
        dst = tag_of(L, 2)
        d = np.frombuffer(dst, dtype=np.uint8).copy()
        arg = np.full(nw, 0xDEADBEEF, dtype=np.uint32)
        assert shim.dst_arg(d.ctypes.data_as(u8p), ctypes.c_uint32(L), ctypes.c_uint32(msg_len), arg.ctypes.data_as(u32p)) == 0
        b0_blocks, msg_words, msg_rem, bi_blocks = (int(x) for x in arg[8:12])
        assert b0_blocks + 1 == -(-(77 + msg_len + L) // 64) and bi_blocks == -(-(43 + L) // 64) and (msg_words, msg_rem) == divmod(msg_len, 4)
        assert bi_blocks == 1 + (L > 21) + (L > 85) + (L > 149) + (L > 213)
        suffix, tail = arg[12:12 + 84], arg[12 + 84:]
        assert len(tail) == 72 and nw == 12 + 84 + 72
        assert b0_blocks * 16 - msg_words <= 84 and not suffix[b0_blocks * 16 - msg_words:].any() and not tail[bi_blocks * 16 - 8:].any()
        msg = np.frombuffer(message(msg_len, 9) + b"\0", dtype=np.uint8).copy()
        uw, u = np.zeros(64, dtype=np.uint32), np.zeros(48, dtype=np.uint32)
        shim.dst_lane(arg.ctypes.data_as(u32p), msg.ctypes.data_as(u8p), uw.ctypes.data_as(u32p), u.ctypes.data_as(u32p))
        assert [int(x) for x in uw] == expect_words(message(msg_len, 9), dst)
    one = np.ones(300, dtype=np.uint8)
    arg = np.zeros(nw, dtype=np.uint32)
    for L in (0, 256, 300):
        assert shim.dst_arg(one.ctypes.data_as(u8p), ctypes.c_uint32(L), ctypes.c_uint32(32), arg.ctypes.data_as(u32p)) == -1


def test_tag_constructors(pkg):
    """blsw_dst_set refuses 0 and 256 bytes and NULL; blsw_dst_default and blsw_dst_pop give the two tags of the POP ciphersuite; the ABI number and
    the options struct are what they were"""
    L = pkg.lib()
    t = pkg.blsw_dst_t()
    buf = bytes(range(1, 256)) + b"\x07"
    assert ctypes.sizeof(pkg.blsw_dst_t) == 256
    assert L.blsw_dst_set(ctypes.byref(t), buf, 0) == 1 and L.blsw_dst_set(ctypes.byref(t), buf, 256) == 1
    assert L.blsw_dst_set(None, buf, 4) == 1 and L.blsw_dst_set(ctypes.byref(t), None, 4) == 1
    assert L.blsw_dst_set(ctypes.byref(t), buf, 255) == 0 and t.len == 255 and bytes(t.bytes) == buf[:255]
    assert L.blsw_dst_set(ctypes.byref(t), buf, 1) == 0 and t.len == 1 and bytes(t.bytes) == b"\x01" + bytes(254)
    assert L.blsw_dst_pop(ctypes.byref(t)) == 0 and bytes(t.bytes)[:t.len] == b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_" == pkg.DST_POP == R.DST_POP and t.len == 43
    assert L.blsw_dst_default(ctypes.byref(t)) == 0 and bytes(t.bytes)[:t.len] == S.DST == pkg.DST_DEFAULT
    assert L.blsw_version() == 17
    with pytest.raises(pkg.BlswError):
        pkg._dst_struct(b"")
    with pytest.raises(pkg.BlswError):
        pkg._dst_struct(bytes(256))
    # argument rules that precede any HIP call: a tag of length 0 is refused by every entry that takes one
    t0 = pkg.blsw_dst_t()
    ws = ctypes.c_void_p(0x1000)  # never dereferenced
    assert L.blsw_hash_to_field_batch(ws, 32, 4, ctypes.byref(t0), ws, None) == 1
    assert L.blsw_hash_to_g2_batch_dst(ws, 32, 4, ws, ws, 1 << 30, ctypes.byref(t0), None) == 1
    assert L.blsw_verify_batch_dst(ws, ws, ws, 32, 4, ws, ws, ws, 1 << 30, ctypes.byref(t0), None) == 1
    assert L.blsw_hash_to_field_batch(ws, 32, 0, None, ws, None) == 1 and L.blsw_hash_to_field_batch(ws, 32, 4, None, None, None) == 1
    assert L.blsw_pop_prove_batch(ws, 0, ws, ws, ws, ws, 1 << 30, None) == 1 and L.blsw_pop_prove_batch(ws, 4, ws, None, ws, ws, 1 << 30, None) == 1
    assert L.blsw_pop_verify_batch(ws, ws, 0, ws, ws, ws, 1 << 30, None) == 1

