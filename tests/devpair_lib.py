"""ctypes loader for tests/devpair/libdevpair.so (TEST HARNESS ONLY): the table of pairing programs of tests/devpair/ops.hpp on the device, the
same table on the host (hostsim_pair_op), the items of tests/pairing_edges.py as operand blocks, and the compare steps the host test and the
device test share. Expected bits are the host single-lane form's (the team's for miller_values, which has no other); their MEANING is held to
tests/pairing_ref.py by the host test, through the reference's own gt."""
import ctypes
import os
import subprocess

import numpy as np

from tests import field_ref as F
from tests import hostsim_lib
from tests import pairing_edges as E
from tests import pairing_ref as R
from tests.field_ref import enc

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devpair")
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
PAD = 3  # witness slots behind an entry's stream: they keep the sentinel
FORMS = {"single": 0, "team": 1}
NO_CURSOR = 0xFFFFFFFF
TEAMS = 10
OP_NAMES = ["miller", "miller_pv", "miller_multi", "vlines2", "vlines3", "miller_values", "miller_groups", "groups_finish"]
VALUE_TEAM_OPS = ("miller_values", "miller_groups", "groups_finish")  # they run on a null cursor, which still counts the ops' witnesses
WITNESS_OPS = ("miller", "miller_pv", "miller_multi")
COEFFS, ROWS = 272, 408

_lib = None


def load():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-s", "-C", HERE])
        _lib = ctypes.CDLL(os.path.join(HERE, "libdevpair.so"))
    return _lib


def _host():
    L = hostsim_lib.load()
    L.hostsim_pair_op_name.restype = ctypes.c_char_p
    for f in (L.hostsim_pair_op_n_wit, L.hostsim_pair_op_n_in, L.hostsim_pair_op_n_out):
        f.restype = ctypes.c_int64
    L.hostsim_pair_spine_witnesses.restype = ctypes.c_uint32
    return L


def host_table():
    """[(name, forms)] of the compiled table, by entry index. forms: bit 0 single-lane, bit 1 team, bit 2 the single-lane form runs on the device too"""
    L = _host()
    return [(L.hostsim_pair_op_name(i).decode(), L.hostsim_pair_op_forms(i)) for i in range(L.hostsim_pair_op_count())]


def counts(op, K=1):
    """(operand elements, result elements, witnesses) of entry `op` at K pairs"""
    L, i = _host(), OP_NAMES.index(op)
    return L.hostsim_pair_op_n_in(i, K), L.hostsim_pair_op_n_out(i), L.hostsim_pair_op_n_wit(i, K)


def spine_witnesses():
    """(as miller_step_info() places them, from the op tables' counts)"""
    L = _host()
    return L.hostsim_pair_spine_witnesses(0), L.hostsim_pair_spine_witnesses(1)


def _pack(rows):
    """[n] equally long lists of stored integers -> uint64 [n, k, 6]"""
    raw = b"".join(x.to_bytes(48, "little") for r in rows for x in r)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(rows), len(rows[0]), 6).copy()


def ints(arr):
    """uint64 [k, 6] -> [k] integers"""
    return [int.from_bytes(arr[i].tobytes(), "little") for i in range(arr.shape[0])]


# ---------------------------------------------------------------- operand blocks
def coeffs(q):
    """the 272 stored line coefficients of the affine G2 point q, by the host's chain_prepare_g2"""
    def make():
        xy = _pack([E.st_g2(q)])
        out = np.zeros((COEFFS, 6), dtype=np.uint64)
        _host().hostsim_pair_prepare(xy.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        return tuple(ints(out))
    return F._memo(("devpair.coeffs", q), make)


def witness_item(q_sig, pairs):
    """the operand block of miller / miller_pv (one pair) and miller_multi: pairs = [(pk_j, Q_j)]"""
    blk = list(coeffs(q_sig))
    for p, q in pairs:
        blk += list(coeffs(q)) + E.st_g1(p)
    return tuple(blk)


def vlines2_item(q, p):
    return tuple(E.st_g2(q) + E.st_g1(p))


def vlines3_item(q, p, z):
    return tuple(E.st_g2(q) + [enc(m) for m in E.jacobian_multipliers(p, z)])


def lines(op, item):
    """the 408 stored line rows of a vlines item, by the host's vline_chain"""
    return F._memo(("devpair.lines", op, item), lambda: tuple(ints(run_host("single", op, [item])[0][0])))


def values_item(q_sig, p, q_h, z=None):
    """the operand block of miller_values: the lines of (-g1, Q_sig) and of (P, Q_h), two multipliers or, with z, the three of a Jacobian P"""
    ls = lines("vlines2", vlines2_item(q_sig, R.NEG_G1))
    lh = lines("vlines2", vlines2_item(q_h, p)) if z is None else lines("vlines3", vlines3_item(q_h, p, z))
    return ls + lh


# ---------------------------------------------------------------- runs
def run_host(form, op, items, K=1):
    """entry `op` over `items` through hostsim_pair_op -> (out uint64 [n, n_out, 6], wit [n, wcap, 6], npos uint32 [n])"""
    n = len(items)
    n_in, n_out, n_wit = counts(op, K)
    assert all(len(it) == n_in for it in items), (op, K, n_in, len(items[0]))
    wcap = n_wit + PAD
    A = _pack(items)
    out = np.full((n, n_out, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(n, NO_CURSOR, dtype=np.uint32)
    fn = _host().hostsim_pair_op
    fn.restype = ctypes.c_int
    rc = fn(FORMS[form], OP_NAMES.index(op), ctypes.c_uint32(K), ctypes.c_uint64(n), A.ctypes.data_as(u64p), out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p),
            ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "host %s %s: %d items returned %d" % (form, op, n, rc)
    return out, wit, npos


def run_device(form, op, items, K=1):
    """one launch on the device -> (out, wit [n, wcap, 6], npos uint32 [lanes]); out: team form uint64 [lanes, 2, 6] with 64 lanes per wave of ten
    items, single form [lanes, n_out, 6] with 64 lanes per wave of 64 items"""
    n = len(items)
    n_in, n_out, n_wit = counts(op, K)
    wcap = n_wit + PAD
    per = TEAMS if form == "team" else 64
    lanes = 64 * ((n + per - 1) // per)
    A = _pack(items)
    out = np.full((lanes, 2 if form == "team" else n_out, 6), F.SENTINEL, dtype=np.uint64)
    wit = np.full((n, wcap, 6), F.SENTINEL, dtype=np.uint64)
    npos = np.full(lanes, NO_CURSOR, dtype=np.uint32)
    fn = load().devpair_run
    fn.restype = ctypes.c_int
    rc = fn(FORMS[form], OP_NAMES.index(op), ctypes.c_uint32(K), ctypes.c_uint64(n), A.ctypes.data_as(u64p), out.ctypes.data_as(u64p), wit.ctypes.data_as(u64p),
            ctypes.c_uint32(wcap), npos.ctypes.data_as(u32p))
    assert rc == 0, "device %s %s: the launch over %d items returned %d" % (form, op, n, rc)
    return out, wit, npos


_expected = {}


def expected(op, items, K=1):
    """(out uint64 [n, n_out, 6], wit [n, wcap, 6], cursor [n]) per item, formed once per distinct item: the host's single-lane form (miller_values:
    the host team, it has no other), its cursor held to the table's count and the slots behind its stream to the sentinel. The cursor expected of
    a TEAM form is the count; for the value entries, whose null cursor still counts the witnesses of the ops they run, it is the host team's."""
    memo = _expected.setdefault((op, K), {})
    new = list(dict.fromkeys(it for it in items if it not in memo))
    if new:
        n_wit = counts(op, K)[2]
        out, wit, npos = run_host("team" if op == "miller_values" else "single", op, new, K)
        if op != "miller_values":
            assert (npos == n_wit).all(), "%s: the cursor is not the table's count %d: %s" % (op, n_wit, sorted(set(npos.tolist())))
        assert (wit[:, n_wit:] == np.uint64(F.SENTINEL)).all() and not (wit[:, :n_wit, 0] == np.uint64(F.SENTINEL)).all(axis=1).any() or n_wit == 0, op
        if op in VALUE_TEAM_OPS:
            npos = run_host("team", op, new, K)[2]
        for i, it in enumerate(new):
            memo[it] = (out[i], wit[i], int(npos[i]))
    return np.stack([memo[it][0] for it in items]), np.stack([memo[it][1] for it in items]), np.array([memo[it][2] for it in items], dtype=np.uint32)


def check_host_team(op, items, K=1):
    """the team form on the looped host team against expected(), bit for bit: value, stream, the sentinel behind it, the team's cursor -> mismatches"""
    want_out, want_wit, want_pos = expected(op, items, K)
    out, wit, npos = run_host("team", op, items, K)
    bad = []
    for i in range(len(items)):
        what = []
        if (out[i] != want_out[i]).any():
            what.append("value")
        if npos[i] != want_pos[i]:
            what.append("cursor %d" % npos[i])
        if (wit[i] != want_wit[i]).any():
            what.append("witness %d" % int(np.flatnonzero((wit[i] != want_wit[i]).any(axis=1))[0]))
        if what:
            bad.append((op, K, i, "; ".join(what)))
    return bad


def check_device(form, op, items, K=1):
    """one launch on the device against expected(), bit for bit. Team form: lane j of item i's team holds coefficient j of the value (a verdict: the
    flag on all six) and the team's cursor. Single form: lane i holds item i's whole result. Every other lane of the grid keeps the sentinel in
    its result and cursor slots; the stream, and the sentinel behind it -> mismatches"""
    n = len(items)
    n_wit = counts(op, K)[2]
    want_res, want_wit, item_pos = expected(op, items, K)
    out, wit, npos = run_device(form, op, items, K)
    lanes = out.shape[0]
    want_out = np.full(out.shape, F.SENTINEL, dtype=np.uint64)
    want_pos = np.full(lanes, NO_CURSOR, dtype=np.uint32)
    item = np.arange(n)
    if form == "team":
        lane0 = (item // TEAMS) * 64 + (item % TEAMS) * 6
        owned = (lane0[:, None] + np.arange(6)[None, :]).reshape(-1)
        want_out[owned] = want_res.reshape(n * 6, 2, 6)
        want_pos[owned] = np.repeat(item_pos, 6)
    else:
        owned = item
        want_out[owned] = want_res
        want_pos[owned] = n_wit
    bad = []
    for ln in np.flatnonzero((out != want_out).reshape(lanes, -1).any(axis=1) | (npos != want_pos))[:10].tolist():
        bad.append((form, op, K, "lane %d (wave %d, thread %d): %s%s" % (ln, ln // 64, ln % 64, "result " if (out[ln] != want_out[ln]).any() else "",
                                                                       "cursor %d" % npos[ln] if npos[ln] != want_pos[ln] else "")))
    for i in np.flatnonzero((wit != want_wit).reshape(n, -1).any(axis=1))[:10].tolist():
        bad.append((form, op, K, "item %d: witness %d" % (i, int(np.flatnonzero((wit[i] != want_wit[i]).any(axis=1))[0]))))
    return bad


# ---------------------------------------------------------------- the items of the tests
def case_items(op):
    """[(case name, item)] of a one-pair entry over pairing_edges.cases()"""
    if op in ("miller", "miller_pv"):
        return [(c[0], witness_item(c[2], [(c[1], c[3])])) for c in E.cases()]
    if op == "vlines2":
        out = [(c[0] + " / sig", vlines2_item(c[2], R.NEG_G1)) for c in E.value_cases()] + [(c[0] + " / h", vlines2_item(c[3], c[1])) for c in E.value_cases()]
        return list(dict((it, (nm, it)) for nm, it in out).values())
    if op == "vlines3":
        return [("%s / Z[%d]" % (c[0], k), vlines3_item(c[3], c[1], z)) for c in E.value_cases() for k, z in enumerate(E.jacobian_zs())]
    if op == "miller_values":
        out = [(c[0], values_item(c[2], c[1], c[3])) for c in E.value_cases()]
        c = E.cases()[E.JACOBIAN_MEANING_CASE]
        return out + [("%s / Jacobian Z[%d]" % (c[0], k), values_item(c[2], c[1], c[3], z)) for k, z in enumerate(E.jacobian_zs())]
    raise KeyError(op)


def multi_item(K):
    return witness_item(E.g2(E.MULTI_QSIG), E.multi_pool()[:K])


def launch(items, n):
    """n items for one launch: the case items in rotation, so that the teams of one wave hold different operands"""
    return [items[i % len(items)] for i in range(n)]


# ---------------------------------------------------------------- the pair-parallel product (csrc/miller_par.hpp, k_miller_par.hip)
STEPS = 68
PAR_SHAPES = ((1, 2), (2, 2), (3, 2), (5, 2), (5, 3), (4, 12), (12, 12), (13, 12), (25, 12))  # (K, B)


def par_items(K):
    """three synthetic items (the programs are algebra over any rows): all rows seeded random; the pairs' rows in rotation random, all ones, all
    p - 1; random with pair 0's point at x = 0 and an all-zero last pair, after which every value is 0. For K <= 5 the real item as well. Three or
    four items leave the launches over n 68 C and n 68 tasks with ragged last waves."""
    def make():
        import random
        from tests.field_edges import ONE, P
        rng = random.Random(0x9A7 + K)
        rnd = lambda k: [rng.randrange(P) for _ in range(k)]
        a = rnd(COEFFS + K * (COEFFS + 2))
        b = rnd(COEFFS)
        for j in range(K):
            b += (rnd(COEFFS + 2), [ONE] * (COEFFS + 2), [P - 1] * (COEFFS + 2))[j % 3]
        c = rnd(COEFFS + K * (COEFFS + 2))
        c[COEFFS + COEFFS] = 0
        c[len(c) - (COEFFS + 2):] = [0] * (COEFFS + 2)
        out = [tuple(a), tuple(b), tuple(c)]
        if K in E.MULTI_K:
            out.append(multi_item(K))
        return out
    return F._memo(("devpair.par_items", K), make)


def _par_arrays(n, K, B):
    C = (K + B - 1) // B
    n_wit = counts("miller_multi", K)[2]
    fe, tail = _final_exp_counts()
    wcap = n_wit + fe + PAD
    S = np.uint64(F.SENTINEL)
    return dict(C=C, n_wit=n_wit, wcap=wcap, off_is_one=n_wit + fe - tail, ffinal=np.full((12, n, 6), S), wit=np.full((n, wcap, 6), S), f1=np.full((12, n * STEPS, 6), S),
                t=np.full((12, n * STEPS, 6), S), q=np.full((12, n * STEPS * C, 6), S), result=np.full(n, -7, dtype=np.int32))


def _final_exp_counts():
    from tests import devteam_lib
    return devteam_lib.counts("final_exp_is_one")


def run_par_host(items, K, B):
    """the four phases on the host (the single-lane spine) -> the arrays of _par_arrays; the final exponentiation is not run"""
    n = len(items)
    a = _par_arrays(n, K, B)
    A = _pack(items)
    fn = _host().hostsim_pair_par
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_uint32(K), ctypes.c_uint32(B), ctypes.c_uint64(n), A.ctypes.data_as(u64p), a["ffinal"].ctypes.data_as(u64p), a["wit"].ctypes.data_as(u64p),
            ctypes.c_uint32(a["wcap"]), a["f1"].ctypes.data_as(u64p), a["t"].ctypes.data_as(u64p), a["q"].ctypes.data_as(u64p))
    assert rc == 0, "host miller_par K=%d B=%d returned %d" % (K, B, rc)
    return a


def run_par_device(items, K, B, spine_lane):
    """launch_miller_par on the device, with the final exponentiation of k_final_team behind the Miller segment"""
    n = len(items)
    a = _par_arrays(n, K, B)
    A = _pack(items)
    fn = load().devpair_par
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_uint32(K), ctypes.c_uint32(B), ctypes.c_uint32(spine_lane), ctypes.c_uint64(n), A.ctypes.data_as(u64p), a["ffinal"].ctypes.data_as(u64p),
            a["wit"].ctypes.data_as(u64p), ctypes.c_uint32(a["wcap"]), ctypes.c_uint32(a["off_is_one"]), ctypes.c_uint32(_final_exp_counts()[1]), a["f1"].ctypes.data_as(u64p),
            a["t"].ctypes.data_as(u64p), a["q"].ctypes.data_as(u64p), a["result"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == 0, "device miller_par K=%d B=%d spine_lane=%d returned %d" % (K, B, spine_lane, rc)
    return a


def check_par_host(K, B):
    """the phases against chain_miller_multi bit for bit: the stream (and the sentinel behind it), the final value; Q[k][0] keeps its sentinel and
    every other slot of f1, T, Q is written; Q[k][1], the first chunk's product, is the dense product of its pairs' embedded lines in integers
    -> (mismatches, the arrays)"""
    from tests import team_ref as T
    items = par_items(K)
    n = len(items)
    want_out, want_wit, _ = expected("miller_multi", items, K)
    a = run_par_host(items, K, B)
    C, n_wit = a["C"], a["n_wit"]
    bad = []
    if (a["wit"][:, :n_wit + PAD] != want_wit).any():
        i = int(np.flatnonzero((a["wit"][:, :n_wit + PAD] != want_wit).reshape(n, -1).any(axis=1))[0])
        bad.append("item %d: witness %d" % (i, int(np.flatnonzero((a["wit"][i, :n_wit + PAD] != want_wit[i]).any(axis=1))[0])))
    if (a["wit"][:, n_wit:] != np.uint64(F.SENTINEL)).any():
        bad.append("a write behind the Miller segment")
    if (a["ffinal"].transpose(1, 0, 2) != want_out).any():
        bad.append("final value")
    q = a["q"].reshape(12, n * STEPS, C, 6)
    S = np.uint64(F.SENTINEL)
    if (q[:, :, 0] != S).any():
        bad.append("Q[k][0] is stored")
    if (q[:, :, 1:, 0] == S).all(axis=0).any() or (a["f1"][:, :, 0] == S).all(axis=0).any() or (a["t"][:, :, 0] == S).all(axis=0).any():
        bad.append("an unwritten slot of f1, T or Q")
    if C >= 2:
        for i, k in ((0, 0), (n - 1, 1), (1, STEPS - 1)):
            it = items[i]
            want = F.F12_ONE
            for j in range(B):
                pr = it[COEFFS + j * (COEFFS + 2):COEFFS + (j + 1) * (COEFFS + 2)]
                want = F.f12_mul(want, T.line_var_p(pr, F.dec(pr[COEFFS]), F.dec(pr[COEFFS + 1]), k))
            if F.d12(ints(q[:, i * STEPS + k, 1])) != want:
                bad.append("Q[%d][1] of item %d is not the first chunk's product" % (k, i))
    return bad, a


def check_par_device(K, B, spine_lane, host=None):
    """launch_miller_par against the host phases, every array whole: the Miller segment, f1, T, Q (sentinels included), the final value; behind the
    segment the stream of chain_final_exp_is_one on that value, and its verdict as the result -> mismatches"""
    from tests import devteam_lib
    items = par_items(K)
    n = len(items)
    h = host or run_par_host(items, K, B)
    d = run_par_device(items, K, B, spine_lane)
    n_wit = h["n_wit"]
    fe, tail = _final_exp_counts()
    bad = [name for name in ("ffinal", "f1", "t", "q") if (h[name] != d[name]).any()]
    if (h["wit"][:, :n_wit] != d["wit"][:, :n_wit]).any():
        bad.append("the Miller segment")
    zero = F.blk([])
    vals = [(tuple(ints(h["ffinal"][:, i])), zero, zero) for i in range(n)]
    fout, fwit, _ = devteam_lib.run_host("single", "final_exp_is_one", vals)
    if (d["wit"][:, n_wit:n_wit + fe] != fwit[:, :fe]).any() or (d["wit"][:, n_wit + fe:] != np.uint64(F.SENTINEL)).any():
        bad.append("the final exponentiation behind the segment")
    if d["result"].tolist() != [int(fout[i, 0, 0]) for i in range(n)]:
        bad.append("result %s" % d["result"].tolist())
    return bad


# ---------------------------------------------------------------- the two group entries (csrc/vpairing.hpp: team_miller_groups; vgroups.hpp: team_groups_finish)
SETS = 9


def group_line_sets():
    """nine line sets and the pairs they are the lines of: [(P, Q, lines)], P Q over the operands on which the reference has been evaluated"""
    def make():
        ps, qs = [E.g1(2), E.g1(3), E.g1(-1)], [E.g2(2), E.g2(3), E.g2(-1)]
        return [(p, q, lines("vlines2", vlines2_item(q, p))) for p in ps for q in qs]
    return F._memo("devpair.group_line_sets", make)


def groups_item(count, own, mask):
    """`count` instance sets and (own) the group's own pair, the nine sets in their fixed order; a set beyond count + own is all zero"""
    sets = group_line_sets()
    blk = [count, own, mask]
    for j in range(SETS):
        blk += list(sets[j][2]) if j < count + own else [0] * ROWS
    return tuple(blk)


def groups_cases():
    """[(count, own, mask)]: nine sets with all bits set, one bit cleared in each position, all cleared; eight instance sets and the own pair the
    same way at its ends; the shorter chunks 1 + own, 3, 0 + own; n_pairs = 0; a mask with bits beyond n_pairs"""
    full = (1 << SETS) - 1
    out = [(9, 0, full)] + [(9, 0, full & ~(1 << p)) for p in range(SETS)] + [(9, 0, 0)]
    out += [(8, 1, full), (8, 1, full & ~(1 << 8)), (8, 1, full & ~1), (8, 1, 1 << 8), (8, 1, 0)]
    out += [(1, 1, 3), (1, 1, 1), (1, 1, 2), (3, 0, 7), (3, 0, 5), (0, 1, 1), (0, 1, 0), (0, 0, 0), (0, 0, full), (2, 0, full)]
    return out


def groups_expected_gt(count, own, mask):
    """the product of e_ref over the folded pairs: what gt(conj(partial)) must be (a partial is not conjugated)"""
    sets = group_line_sets()
    return R.product([R.e_ref(sets[p][0], sets[p][1]) for p in range(count + own) if (mask >> p) & 1])


def finish_item(partials):
    """1 to 3 partial products (twelve stored integers each)"""
    blk = [len(partials)]
    for q in range(3):
        blk += list(partials[q]) if q < len(partials) else [0] * 12
    return tuple(blk)


def _bits(*ps):
    return sum(1 << p for p in ps)


# the exponents of e(g1, g2) in the nine pairs are 4, 6, -2, 6, 9, -3, -2, -3, 1: pairs {0, 2, 6} and {1, 5, 7} multiply to one
FINISH_PARTS = {"X": _bits(0, 2), "Y": _bits(6), "Z": _bits(1, 5, 7), "W": _bits(4), "XY": _bits(0, 2, 6), "one": 0}
FINISH_CASES = (("XY",), ("X",), ("X", "Y"), ("X", "W"), ("X", "Y", "Z"), ("X", "one", "W"), ("one",), ("Z", "one", "one"))


def finish_partial(name):
    """the partial product of the nine sets under the mask of that name, by the single-lane statement of miller_groups"""
    return tuple(ints(expected("miller_groups", [groups_item(SETS, 0, FINISH_PARTS[name])])[0][0]))


def finish_items():
    return [finish_item([finish_partial(nm) for nm in names]) for names in FINISH_CASES]


def finish_reference_verdict(names):
    """gt(conj(product of the partials)) == 1, by the reference's gt on the integer product"""
    f = F.F12_ONE
    for nm in names:
        f = F.f12_mul(f, F.d12(list(finish_partial(nm))))
    return R.gt(F.f12_conj(f)) == F.F12_ONE
