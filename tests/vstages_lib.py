"""The shipped value kernels on chosen points (TEST HARNESS ONLY): launch_verify_groups and launch_verify_values of csrc/k_vgroups.hip and
csrc/k_team.hip, compiled unchanged into tests/devpair/libdevvalues.so, against the same stages on the host (tests/vgroups/shim.cpp:
vgroups_stages, vgroups_value_lines). Inputs are written directly, the hash and decode stages are not run: affine pk_xy and sig_xy in Montgomery
form, ws.h as homogeneous projective G2 points with Z != 1, status, scalars. Every output array starts as the sentinel and is compared whole.
What a stage's output MEANS is stated here with the affine group law of tests/curve_ref.py and the pairing of tests/pairing_ref.py."""
import ctypes
import os
import random
import subprocess

import numpy as np

from tests import curve_ref as C
from tests import field_ref as F
from tests import pairing_edges as E
from tests import vgroups_lib
from tests.curve_ref import K1, K2, R_ORDER
from tests.field_edges import ONE, P
from tests.field_ref import enc

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devpair")
u64p = ctypes.POINTER(ctypes.c_uint64)
i32p = ctypes.POINTER(ctypes.c_int32)
ROWS = 408
SHAPES = ((1, 64, 8), (11, 1, 8), (23, 5, 2), (23, 5, 1), (23, 7, 3), (33, 32, 31), (70, 17, 8))  # (n, group, chunk)
VALUE_COUNTS = (1, 10, 11, 21)
VG_FLAG_OK, VG_FLAG_SUM = 1, 2
ST_BAD = 2  # any decode status but 0
S64 = np.uint64(F.SENTINEL)
S32 = np.int32(-0x5A5A5A5B)

_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevvalues.so"))
    return _lib


def _limbs(vals):
    """[k] integers -> uint64 [k, 6]"""
    return np.frombuffer(b"".join(int(v).to_bytes(48, "little") for v in vals), dtype=np.uint64).reshape(len(vals), 6).copy()


def _int(row):
    return int.from_bytes(np.ascontiguousarray(row).tobytes(), "little")


def homogeneous(q, z):
    """(x z, y z, z) of the affine G2 point q"""
    return (F.f2_mul(q[0], z), F.f2_mul(q[1], z), z)


def pool():
    """[(sk, h)]: key sk g1, hashed message h g2, signature sk h g2"""
    rng = random.Random(0x6E0)
    return [(1, 1), (R_ORDER - 1, 3), (rng.randrange(2, R_ORDER), 2), (2, rng.randrange(2, R_ORDER)), (3, R_ORDER - 1)]


def chunks_of(m, chunk, cpg):
    """[(first position, count)] of the cpg chunks of a group of m instances"""
    return [(min(q * chunk, m) if q * chunk < m else 0, max(0, min(chunk, m - q * chunk))) for q in range(cpg)]


class Batch:
    """the inputs of one launch of n instances, as points and as the kernels' arrays"""

    def __init__(self, pks, hs, sigs, status, scalars, group, chunk, seed=1):
        n = len(pks)
        rng = random.Random(0x2A + seed)
        self.n, self.group, self.chunk = n, group, chunk
        self.pks, self.hs, self.sigs, self.status, self.scalars = pks, hs, sigs, status, scalars
        self.G = (n + group - 1) // group
        self.cpg = (min(group, n) + chunk - 1) // chunk
        self.zs = [(rng.randrange(P), rng.randrange(1, P)) for _ in range(n)]  # Z != 1 (and no element of Fp)
        self.pk_xy = _limbs([enc(c) for p in pks for c in p]).reshape(n, 12)
        self.sig_xy = _limbs([v for s in sigs for v in E.st_g2(s)]).reshape(n, 24)
        hom = [homogeneous(h, z) for h, z in zip(hs, self.zs)]
        self.h = np.ascontiguousarray(_limbs([v for t in hom for c in t for v in F.e2(c)]).reshape(n, 6, 6).transpose(1, 0, 2))  # [6][n]
        self.st = np.array(status, dtype=np.int32).reshape(n, 2)
        self.sc = np.array(scalars, dtype=np.uint64)

    def included(self, i):
        return self.status[i] == (0, 0) and self.scalars[i] != 0

    def members(self, g):
        return range(g * self.group, min(self.n, (g + 1) * self.group))


def groups_batch(n, group, chunk):
    """instances from the pool in rotation, valid unless a pattern says otherwise; group g follows pattern g % 5:
      0  all included; scalars 1, 2^63, 2^64 - 1 at its first positions
      1  exclusions: a status that is not OK at the first position of the first chunk and at the first position of the last chunk, a zero scalar at
         the last position of the first chunk and at the last position of the group
      2  every instance excluded, by status and by zero scalar in turn
      3  S_g the identity by two VALID signatures that cancel (keys sk and r - sk on one message, one scalar), the others excluded: a group of
         exactly two passes (vgroups.hpp), with its own pair skipped and, where the chunk is smaller than the group, with empty chunks
      4  a signature of another key at the last position (the product is not 1), an excluded instance at the first if there are three"""
    rng = random.Random(0x5EED + n * 1000 + group * 10 + chunk)
    pl = pool()
    pks, hs, sigs, status, scalars, dl = [], [], [], [], [], []
    for i in range(n):
        sk, h = pl[i % len(pl)]
        dl.append([sk, h, sk * h % R_ORDER])  # discrete logarithms of (pk, H, sig)
        pks.append(E.g1(sk))
        hs.append(E.g2(h))
        sigs.append(E.g2(sk * h))
        status.append((0, 0))
        scalars.append(rng.randrange(1, 1 << 64))
    G = (n + group - 1) // group
    for g in range(G):
        lo = g * group
        m = min(n, lo + group) - lo
        pat = g % 5
        if pat == 0:
            for k, r in enumerate((1, 1 << 63, (1 << 64) - 1)[:m]):
                scalars[lo + k] = r
        elif pat == 1:
            last_first = ((m - 1) // chunk) * chunk
            for pos, kind in ((0, "pk"), (min(chunk, m) - 1, "zero"), (last_first, "sig"), (m - 1, "zero")):
                if kind == "zero" and status[lo + pos] == (0, 0):
                    scalars[lo + pos] = 0
                elif kind != "zero" and scalars[lo + pos] != 0:
                    status[lo + pos] = (ST_BAD, 0) if kind == "pk" else (0, ST_BAD)
        elif pat == 2:
            for k in range(m):
                if k % 2:
                    scalars[lo + k] = 0
                else:
                    status[lo + k] = (ST_BAD, ST_BAD)
        elif pat == 3 and m >= 2:
            pks[lo + 1], hs[lo + 1], sigs[lo + 1] = C.aff_neg(K1, pks[lo]), hs[lo], C.aff_neg(K2, sigs[lo])  # the key r - sk on the same message
            dl[lo + 1] = [-dl[lo][0] % R_ORDER, dl[lo][1], -dl[lo][2] % R_ORDER]
            scalars[lo + 1] = scalars[lo]
            for k in range(2, m):
                scalars[lo + k] = 0
        elif pat == 4:
            sigs[lo + m - 1] = E.g2(7 * (g + 2))
            dl[lo + m - 1][2] = 7 * (g + 2)
            if m >= 3:
                status[lo] = (0, ST_BAD)
    b = Batch(pks, hs, sigs, status, scalars, group, chunk)
    b.dlogs = dl
    return b


def want_results(b):
    """the verdict of every group by bilinearity on the discrete logarithms the batch was built from: the product is 1 iff the sum of r_i sk_i h_i
    equals the sum of r_i log(sig_i) over the included instances; ANDed with 'every instance included'"""
    out = []
    for g in range(b.G):
        inc = [i for i in b.members(g) if b.included(i)]
        lhs = sum(b.scalars[i] * b.dlogs[i][0] * b.dlogs[i][1] for i in inc) % R_ORDER
        rhs = sum(b.scalars[i] * b.dlogs[i][2] for i in inc) % R_ORDER
        out.append(int(lhs == rhs and len(inc) == len(b.members(g))))
    return out


def meaning_batch():
    """n = 7 in groups of 3, chunks of 2 (the last group of one has an empty second chunk), on the operands on which pairing_ref.prove() has
    evaluated the reference already: pk = g1, scalars in {1, 2, 3}, H in {g2, 2 g2, 3 g2, -g2}, and S_g one of 7 g2, 7 g2, 5 g2.
    group 0: valid (the product is 1); group 1: one wrong signature and one excluded instance (a generic product); group 2: a generic product"""
    g1 = E.g1(1)
    hs = [E.g2(2), E.g2(-1), E.g2(3), E.g2(3), E.g2(2), E.g2(5), E.g2(1)]
    sigs = [E.g2(2), E.g2(-1), E.g2(3), E.g2(3), E.g2(-1), E.g2(11), E.g2(5)]
    scalars = [2, 3, 2, 3, 2, 9, 1]
    status = [(0, 0)] * 5 + [(ST_BAD, 0)] + [(0, 0)]
    return Batch([g1] * 7, hs, sigs, status, scalars, 3, 2, seed=2)


# ---------------------------------------------------------------- runs
def _group_arrays(b):
    n, G = b.n, b.G
    return dict(p_scaled=np.full((3, n, 6), S64), s_scaled=np.full((6, n, 6), S64), sum_xy=np.full((4, G, 6), S64), gflag=np.full(G, S32), lines_h=np.full((ROWS, n, 6), S64),
                lines_g=np.full((ROWS, G, 6), S64), partials=np.full((G * b.cpg, 12, 6), S64), result=np.full(G, S32))


ARRAYS = ("p_scaled", "s_scaled", "sum_xy", "gflag", "lines_h", "lines_g", "partials", "result")


def _call_groups(fn, b):
    a = _group_arrays(b)
    ptr = lambda x: x.ctypes.data_as(i32p if x.dtype == np.int32 else u64p)
    rc = fn(ctypes.c_uint64(b.n), ctypes.c_uint32(b.group), ctypes.c_uint32(b.chunk), ptr(b.pk_xy), ptr(b.sig_xy), ptr(b.h), ptr(b.st), ptr(b.sc), *[ptr(a[k]) for k in ARRAYS])
    return rc, a


def groups_host(b):
    fn = vgroups_lib.load().vgroups_stages
    fn.restype = ctypes.c_int64
    rc, a = _call_groups(fn, b)
    assert rc == b.G, rc
    return a


def groups_device(b):
    fn = load().devvalues_groups
    fn.restype = ctypes.c_int
    rc, a = _call_groups(fn, b)
    assert rc == 0, "launch_verify_groups over %d instances returned %d" % (b.n, rc)
    return a


def values_host(b):
    ls, lh = np.full((ROWS, b.n, 6), S64), np.full((ROWS, b.n, 6), S64)
    vgroups_lib.load().vgroups_value_lines(ctypes.c_uint64(b.n), b.pk_xy.ctypes.data_as(u64p), b.sig_xy.ctypes.data_as(u64p), b.h.ctypes.data_as(u64p), ls.ctypes.data_as(u64p),
                                           lh.ctypes.data_as(u64p))
    return ls, lh


def values_device(b):
    ls, lh, res = np.full((ROWS, b.n, 6), S64), np.full((ROWS, b.n, 6), S64), np.full(b.n, S32)
    fn = load().devvalues_values
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_uint64(b.n), b.pk_xy.ctypes.data_as(u64p), b.sig_xy.ctypes.data_as(u64p), b.h.ctypes.data_as(u64p), b.st.ctypes.data_as(i32p), ls.ctypes.data_as(u64p),
            lh.ctypes.data_as(u64p), res.ctypes.data_as(i32p))
    assert rc == 0, "launch_verify_values over %d instances returned %d" % (b.n, rc)
    return ls, lh, res


# ---------------------------------------------------------------- what the arrays must be
def group_sum(b, g):
    """S_g = sum of r_i sig_i over the included instances of group g, by the affine group law (None: the identity)"""
    acc = None
    for i in b.members(g):
        if b.included(i):
            acc = C.aff_add(K2, acc, C.aff_mul(K2, b.scalars[i], b.sigs[i]))
    return acc


def check_group_arrays(b, a):
    """the stage outputs against the group law and the rules of vgroups.hpp -> mismatches. p_scaled: r_i pk_i (Jacobian; Z = 0 when excluded); sum_xy:
    S_g affine, zeros for the identity; gflag; the rows of a skipped pair keep the sentinel and those of a folded pair are written; the partial of
    a chunk without a folded pair is exactly one; result is 0 wherever a flag is missing"""
    bad = []
    n, G, cpg = b.n, b.G, b.cpg
    one12 = _limbs([ONE] + [0] * 11)
    for i in range(n):
        jac = tuple(F.dec(_int(a["p_scaled"][k, i])) for k in range(3))
        want = C.aff_mul(K1, b.scalars[i], b.pks[i]) if b.included(i) else None
        if C.jac_affine(K1, jac) != want:
            bad.append("p_scaled[%d]" % i)
        written = (a["lines_h"][:, i] != S64).any()
        if written != b.included(i) or (written and (a["lines_h"][:, i, 0] == S64).all(axis=0).any()):
            bad.append("lines_h of instance %d: %s" % (i, "written" if written else "not written"))
    for g in range(G):
        s = group_sum(b, g)
        ok = all(b.included(i) for i in b.members(g))
        if int(a["gflag"][g]) != (VG_FLAG_OK if ok else 0) | (VG_FLAG_SUM if s is not None else 0):
            bad.append("gflag[%d] = %d" % (g, a["gflag"][g]))
        got = [F.dec(_int(a["sum_xy"][k, g])) for k in range(4)]
        if got != ([0] * 4 if s is None else [s[0][0], s[0][1], s[1][0], s[1][1]]):
            bad.append("sum_xy[%d]" % g)
        if (a["lines_g"][:, g] != S64).any() != (s is not None):
            bad.append("lines_g of group %d" % g)
        m = len(b.members(g))
        for q, (first, count) in enumerate(chunks_of(m, b.chunk, cpg)):
            folded = any(b.included(g * b.group + first + k) for k in range(count)) or (q == 0 and s is not None)
            if not folded and (a["partials"][g * cpg + q] != one12).any():
                bad.append("partial of chunk %d of group %d, which folds no pair, is not one" % (q, g))
            if folded and (a["partials"][g * cpg + q] == one12).all():
                bad.append("partial of chunk %d of group %d is one" % (q, g))
        if not ok and a["result"][g] != 0:
            bad.append("result[%d] without the group's flag" % g)
    return bad


def group_value(b, a, g):
    """conj(product of the partials of group g) as an Fp12 element: the Miller value the finish exponentiates"""
    f = F.F12_ONE
    for q in range(b.cpg):
        f = F.f12_mul(f, F.d12([_int(r) for r in a["partials"][g * b.cpg + q]]))
    return F.f12_conj(f)


def group_expected_gt(b, g):
    """prod e_ref(r_i pk_i, H_i) over the included instances, times e_ref(-g1, S_g) unless S_g is the identity"""
    from tests import pairing_ref as R
    out = F.F12_ONE
    for i in b.members(g):
        if b.included(i):
            out = F.f12_mul(out, R.e_ref(C.aff_mul(K1, b.scalars[i], b.pks[i]), b.hs[i]))
    s = group_sum(b, g)
    return out if s is None else F.f12_mul(out, R.e_ref(R.NEG_G1, s))


def values_batch(n):
    """launch_verify_values: the value cases of pairing_edges in rotation (relations and non-relations side by side in one wave, so that a
    neighbour's lines give another answer); instance 8 (where there is one) is a relation whose key did not decode"""
    cs = E.value_cases()
    cases = [cs[i % len(cs)] for i in range(n)]
    status = [(0, 0)] * n
    if n > 8:
        assert cases[8][4] == "relation"
        status[8] = (ST_BAD, 0)
    b = Batch([c[1] for c in cases], [c[3] for c in cases], [c[2] for c in cases], status, [1] * n, n, 8, seed=3)
    b.want = [int(c[4] == "relation" and st == (0, 0)) for c, st in zip(cases, status)]
    return b
