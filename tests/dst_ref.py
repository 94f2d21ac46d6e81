"""Independent statement of hash_to_field and hash_to_g2 under ANY domain separation tag (the *_dst entries of include/blsw.h), from parts the
suite already proves: tests/sha_ref.expand_message_xmd (RFC 9380 5.3.1 with hashlib) and tests/curve_ref's SSWU map, 3-isogeny, affine group law
and H_EFF (tests/test_curve_ref.py). Nothing here reads csrc/.

pin() holds it to the reference before a test uses it: at the library's tag hash_to_g2 reproduces the oracle's frozen outputs on the reference's
five test_hash_to_curve messages (hasher.rs:1006-1012; tests/golden/oracle_hash_strings.json), and expand_message_xmd reproduces the reference's
expand literals, which carry tags of their own (hasher.rs:819-886; the "expand" cases of tests/golden/literals.json)."""
import json
import os

from tests import curve_ref as C
from tests import field_ref as F
from tests import sha_ref as S
from tests.curve_ref import K1, K2

P = S.P
DST_DEFAULT = S.DST
DST_POP = b"BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hash_to_field(msg, dst):
    """-> [u0.c0, u0.c1, u1.c0, u1.c1] as canonical integers (RFC 9380 5.2: count 2, m 2, L 64)"""
    u = S.expand_message_xmd(bytes(msg), 256, bytes(dst))
    return [int.from_bytes(u[64 * j:64 * j + 64], "big") % P for j in range(4)]


def mont_words(v):
    """a canonical integer as the six u64 Montgomery words the library stores"""
    m = v * S.R % P
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def hash_to_g2(msg, dst):
    """-> affine point ((x.c0, x.c1), (y.c0, y.c1)) of canonical integers, or None for the identity"""
    e = hash_to_field(msg, dst)
    q0, q1 = C.iso_map(C.sswu((e[0], e[1]))[0]), C.iso_map(C.sswu((e[2], e[3]))[0])
    return C.aff_mul(K2, C.H_EFF, C.aff_add(K2, q0, q1))


def g2_limbs(pt):
    """an affine G2 point as the 24 u64 words blsw_hash_to_g2_batch writes (x.c0, x.c1, y.c0, y.c1, Montgomery)"""
    return [w for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) for w in mont_words(c)]


def sign(sk, msg, dst):
    """sk * H(msg) compressed"""
    return C.g2_compress(C.aff_mul(K2, sk, hash_to_g2(msg, dst)))


def public_key(sk):
    return C.g1_compress(C.aff_mul(K1, sk, C.G1_GEN))


_pinned = []


def pin():
    if _pinned:
        return True
    assert C.prove_isogeny()
    lit = json.load(open(os.path.join(GOLDEN, "literals.json")))
    frozen = json.load(open(os.path.join(GOLDEN, "oracle_hash_strings.json")))["compressed"]
    assert len(lit["hash_strings"]) == len(frozen) == 5
    for s, want in zip(lit["hash_strings"], frozen):
        assert C.g2_compress(hash_to_g2(s.encode("utf-8"), DST_DEFAULT)).hex() == want, s
    tags = set()
    for case in lit["expand"]:
        dst = bytes.fromhex(case["dst"])
        tags.add(dst)
        assert S.expand_message_xmd(bytes.fromhex(case["msg"]), case["len_in_bytes"], dst).hex() == case["uniform_bytes"]
    assert tags and DST_DEFAULT not in tags  # tags of their own
    _pinned.append(True)
    return True


assert F.P == P
