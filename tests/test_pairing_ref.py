"""The table of pairing programs (tests/devpair/ops.hpp: the Miller programs of csrc/chains.hpp, team.hpp and vpairing.hpp) on the host, against an
INDEPENDENT pairing: tests/pairing_ref.py, the textbook optimal-ate Miller function over Python integers, proved here before use.

Two kinds of statement. Bits: every form of an entry equals the entry's single-lane form, values and witness streams and cursors (the device test
then holds the device to the same bits). Meaning: gt(the code's Miller value) == e_ref(-g1, Q_sig) * prod e_ref(P_j, Q_j), both sides through
the reference's own gt = f^((p^12 - 1) / r), never through the code's final exponentiation; on signature relations (the product is 1), on a
tampered one and on as many non-relations, whose product is a generic GT element: twelve coefficients compared, not one bit."""
import time

import pytest

from tests import chain_edges
from tests import devpair_lib as D
from tests import devteam_lib
from tests import field_ref as F
from tests import hostsim_lib
from tests import pairing_edges as E
from tests import pairing_ref as R
from tests.curve_ref import K1, K2, R_ORDER
from tests import curve_ref as C


def test_reference_is_a_pairing():
    """non-degenerate, of order r, bilinear in both arguments for a, b in {2, 3, r - 1}, additive in the second argument"""
    t0 = time.time()
    assert R.prove()
    print("pairing_ref.prove(): %.1f s" % (time.time() - t0))


def test_table_is_the_compiled_table():
    """the entry list and its forms; the witness counts, formed from the op tables' counts and miller_step_info(), are the layouts' Miller segments"""
    assert [n for n, _ in D.host_table()] == D.OP_NAMES
    forms = dict(D.host_table())
    assert forms == {"miller": 7, "miller_pv": 3, "miller_multi": 3, "vlines2": 5, "vlines3": 5, "miller_values": 2, "miller_groups": 3, "groups_finish": 3}
    placed, from_tables = D.spine_witnesses()
    assert placed == from_tables
    lay, lay_pv = hostsim_lib.layout(32), hostsim_lib.layout(32, 1)
    assert D.counts("miller") == (546, 12, lay["off_final_exp"] - lay["off_miller"])
    assert D.counts("miller_pv") == (546, 12, lay_pv["off_final_exp"] - lay_pv["off_miller"])
    ellv = devteam_lib.counts("ELLV")[0]
    for K in E.MULTI_K:
        assert D.counts("miller_multi", K) == (272 + 274 * K, 12, placed + 68 * K * ellv)
    assert D.counts("miller_multi", 1)[2] == D.counts("miller")[2]
    assert D.counts("vlines2") == (6, 408, 0) and D.counts("vlines3") == (7, 408, 0) and D.counts("miller_values") == (816, 12, 0)
    assert D.counts("miller_groups") == (3 + 9 * 408, 12, 0) and D.counts("groups_finish") == (37, 12, 0)


def test_operands_cover_what_they_claim():
    cs = E.cases()
    g1, g2 = E.g1(1), E.g2(1)
    ps, qs = {c[1] for c in cs}, {c[2] for c in cs} | {c[3] for c in cs}
    s, h = E.seeds()
    assert {g1, E.g1(-1), E.g1(2), E.g1(s), E.ORDER3} <= ps and E.g1(-1) == C.aff_neg(K1, g1)
    assert {g2, C.aff_neg(K2, g2), E.g2(h), E.g2(s * h)} <= qs and any(c[2] == c[3] for c in cs)
    assert C.aff_mul(K1, 3, E.ORDER3) is None and E.ORDER3[0] == 0 and ("order 3: (0, 2)", E.ORDER3, 3) in chain_edges.g1_operands()
    assert all(C.aff_mul(K2, R_ORDER, q) is None for q in qs) and all(C.aff_mul(K1, R_ORDER, p) is None for p in ps - {E.ORDER3})
    kinds = [c[4] for c in cs]
    assert kinds.count("relation") == 3 and kinds.count("tampered") == 1 and kinds.count("generic") >= 4 and kinds.count("off-subgroup") == 1
    # the relations are relations by the group law: sig = [sk] H with pk = [sk] g1, for sk = 1, r - 1 and the seeded one; the tampered one is not
    for c, sk in zip(cs[:3], (1, R_ORDER - 1, s)):
        assert c[1] == E.g1(sk) and c[2] == C.aff_mul(K2, sk, c[3])
    assert cs[3][1] == E.g1(2) and cs[3][2] != C.aff_mul(K2, 2, cs[3][3])
    assert all(c[4] != "off-subgroup" for c in E.value_cases()) and len(E.value_cases()) == len(cs) - 1
    # every kind of operand has its meaning checked in a program
    covered = {cs[i][4] for i in E.WITNESS_MEANING} | {cs[i][4] for i in E.VALUES_MEANING}
    assert covered == set(E.KINDS) and {0, 1, 2} <= set(E.WITNESS_MEANING) | set(E.VALUES_MEANING)
    zs = E.jacobian_zs()
    assert zs[:3] == [1, 2, E.P - 1] and zs[3] not in zs[:3]
    assert E.jacobian_multipliers(g1, 1) == (1, g1[0], g1[1])


def test_prepared_coefficients_are_the_circuit_arithmetic():
    """the operands of the witness entries: the host's chain_prepare_g2 gives the coefficients chain_edges.prepare_reference states in integers"""
    for q in (E.g2(1), E.g2(-1), E.g2(E.seeds()[1])):
        assert list(D.coeffs(q)) == chain_edges.prepare_reference(q)[1]


def _gt_of(out_row):
    return R.gt_of_block(D.ints(out_row))


@pytest.mark.parametrize("op", ["miller", "miller_pv"])
def test_witness_programs(op):
    """team == single lane bit for bit (value, stream, cursor, sentinel) on every case; the meaning of the value on E.WITNESS_MEANING"""
    named = D.case_items(op)
    items = [it for _, it in named]
    bad = D.check_host_team(op, items)
    assert not bad, bad
    out, _, _ = D.expected(op, items)
    t0 = time.time()
    for i in E.WITNESS_MEANING:
        name, p, q_sig, q_h, kind = E.cases()[i]
        got, want = _gt_of(out[i]), E.expected_gt(p, q_sig, q_h)
        assert got == want, "%s: gt(value) is not e_ref(-g1, Q_sig) e_ref(P, Q_h): %s" % (op, name)
        assert (want == F.F12_ONE) == (kind == "relation"), name
    print("%s: %d cases, meaning on %d, reference %.1f s" % (op, len(items), len(E.WITNESS_MEANING), time.time() - t0))


def test_witness_programs_agree_on_the_value():
    """team_miller_pv allocates the generator, which changes witnesses and not the value; one pair through miller_multi is miller, stream included"""
    a, b = (D.expected(op, [it for _, it in D.case_items(op)]) for op in ("miller", "miller_pv"))
    assert (a[0] == b[0]).all()
    items = [it for _, it in D.case_items("miller")]
    m = D.expected("miller_multi", items, 1)
    assert (m[0] == a[0]).all() and (m[1] == a[1]).all()


@pytest.mark.parametrize("K", E.MULTI_K)
def test_miller_multi(K):
    """chain_miller_multi == team_miller_multi bit for bit; at K = 2, 3, 5 gt(value) == e_ref(-g1, Q_sig) prod e_ref(pk_j, Q_j)"""
    items = [D.multi_item(K)] + [D.witness_item(c[2], [(c[1], c[3])] * K) for c in E.cases()[:2]]
    bad = D.check_host_team("miller_multi", items, K)
    assert not bad, bad
    if K in E.MULTI_MEANING_K:
        out, _, _ = D.expected("miller_multi", items[:1], K)
        want = R.product([R.e_ref(R.NEG_G1, E.g2(E.MULTI_QSIG))] + [R.e_ref(p, q) for p, q in E.multi_pool()[:K]])
        assert want != F.F12_ONE and _gt_of(out[0]) == want


def test_vlines_and_miller_values():
    """the lines are operands here (the device test holds the device's to the host's); their meaning is checked through team_miller_values: for
    the two-multiplier lines on E.VALUES_MEANING, for the three-multiplier lines of a Jacobian P against the same affine P"""
    named = D.case_items("miller_values")
    items = [it for _, it in named]
    out, _, _ = D.expected("miller_values", items)
    t0 = time.time()
    cs = E.value_cases()
    for i in E.VALUES_MEANING:
        name, p, q_sig, q_h, kind = E.cases()[i]
        k = cs.index(E.cases()[i])
        assert _gt_of(out[k]) == E.expected_gt(p, q_sig, q_h), "miller_values: %s" % name
    name, p, q_sig, q_h, _ = E.cases()[E.JACOBIAN_MEANING_CASE]
    want = E.expected_gt(p, q_sig, q_h)
    jac = out[len(cs):]
    assert (jac[0] == out[cs.index(E.cases()[E.JACOBIAN_MEANING_CASE])]).all()  # Z = 1: the multipliers (1, x, y), the same lines
    assert len({tuple(D.ints(j)) for j in jac}) == len(jac)  # another Z, another value: a factor in Fp
    assert _gt_of(jac[3]) == want, "miller_values on three-multiplier lines, seeded Z"
    print("miller_values: %d items, reference %.1f s" % (len(items), time.time() - t0))
    # the three-multiplier form is the two-multiplier form with c0 scaled: rows 0, 1 of a step times p0, rows 2..5 those of (px, py)
    c = E.cases()[E.JACOBIAN_MEANING_CASE]
    z = E.jacobian_zs()[3]
    p0, px, py = E.jacobian_multipliers(c[1], z)
    l3 = D.lines("vlines3", D.vlines3_item(c[3], c[1], z))
    l2 = D.lines("vlines2", D.vlines2_item(c[3], (px, py)))
    assert all(F.dec(l3[i]) == (F.dec(l2[i]) * p0 % E.P if i % 6 < 2 else F.dec(l2[i])) for i in range(D.ROWS))


def test_vlines_are_the_lines_of_the_walk():
    """the 408 rows of vline_chain in integers: step k's triple (c0, c1 x_P, c2 y_P) is the reference's line of step k, (s x_T - y_T, -s x_P, y_P),
    up to one non-zero factor in Fp2 (the projective walk's denominator); for the three-multiplier form the same against the affine P"""
    def proportional(rows, steps):
        for k, (_, ref) in enumerate(steps):
            got = [F.d2(rows, 6 * k + 2 * j) for j in range(3)]
            assert got[2] != F.F2_ZERO and all(F.f2_mul(got[i], ref[2]) == F.f2_mul(ref[i], got[2]) for i in range(2)), k
    for name, p, q_sig, q_h, _ in E.value_cases()[:4]:
        proportional(D.lines("vlines2", D.vlines2_item(q_h, p)), R.line_steps(p, q_h))
        proportional(D.lines("vlines2", D.vlines2_item(q_sig, R.NEG_G1)), R.line_steps(R.NEG_G1, q_sig))
    c = E.cases()[E.JACOBIAN_MEANING_CASE]
    for z in E.jacobian_zs():
        proportional(D.lines("vlines3", D.vlines3_item(c[3], c[1], z)), R.line_steps(c[1], c[3]))


@pytest.mark.parametrize("K,B", D.PAR_SHAPES)
def test_miller_par_phases_equal_the_serial_chain(K, B):
    """the four phases of miller_par.hpp as loops, on synthetic rows (zeros, ones, p - 1, random) and, for K <= 5, real points: the stream and the
    final value are chain_miller_multi's bit for bit; Q[k][0] keeps its sentinel; Q[k][1] is the first chunk's product in integers. The shapes:
    one chunk (C = 1: K <= B), a last chunk of one pair ((3, 2), (5, 2), (13, 12), (25, 12)), full chunks ((2, 2), (12, 12)), B = 3"""
    bad, a = D.check_par_host(K, B)
    assert a["C"] == (K + B - 1) // B and not bad, bad


def test_miller_groups():
    """team_miller_groups on the host team against its single-lane statement (per line index one square, then the dense product with the embedded
    line of every pair whose mask bit is set), bit for bit, on up to nine line sets: all bits set, one bit cleared in EACH position, all cleared,
    the own pair at position 8 and at position 1 and 0, n_pairs = 0. All cleared and n_pairs = 0 give exactly one. Meaning: the conjugated partial
    against the product of e_ref over the folded pairs only, with all nine folded, with position 4 skipped and with only the own pair folded"""
    cases = D.groups_cases()
    full = (1 << D.SETS) - 1
    assert all((9, 0, full & ~(1 << p)) in cases for p in range(D.SETS)) and (9, 0, full) in cases and (9, 0, 0) in cases and (0, 0, 0) in cases
    items = [D.groups_item(*c) for c in cases]
    bad = D.check_host_team("miller_groups", items)
    assert not bad, bad
    out, _, _ = D.expected("miller_groups", items)
    for c, o in zip(cases, out):
        folded = c[2] & ((1 << (c[0] + c[1])) - 1)
        assert (F.d12(D.ints(o)) == F.F12_ONE) == (folded == 0), c
    t0 = time.time()
    for c in ((9, 0, full), (9, 0, full & ~(1 << 4)), (8, 1, 1 << 8)):
        got = R.gt(F.f12_conj(F.d12(D.ints(out[cases.index(c)]))))
        assert got == D.groups_expected_gt(*c) != F.F12_ONE, c
    print("miller_groups: %d cases, reference %.1f s" % (len(cases), time.time() - t0))


def test_groups_finish():
    """team_groups_finish at 1, 2 and 3 partials on the host team against its single-lane statement, and both against the reference:
    verdict == (gt(conj(product of the partials)) == 1), on products that are one and on generic ones, with a partial that is exactly one"""
    items = D.finish_items()
    bad = D.check_host_team("groups_finish", items)
    assert not bad, bad
    out, _, _ = D.expected("groups_finish", items)
    t0 = time.time()
    want = [D.finish_reference_verdict(names) for names in D.FINISH_CASES]
    assert want == [True, False, True, False, True, False, True, True] and {len(n) for n in D.FINISH_CASES} == {1, 2, 3}
    assert [int(D.ints(o)[0]) for o in out] == [int(w) for w in want]
    print("groups_finish: %d cases, reference %.1f s" % (len(items), time.time() - t0))


# ---------------------------------------------------------------- the stages of the shipped value kernels, on the host
from tests import vstages_lib as V  # noqa: E402


def test_value_cases_are_what_their_kind_says():
    """the verdict the value kernels owe on a case: the reference's product is 1 exactly on the relations"""
    for name, p, q_sig, q_h, kind in E.value_cases():
        assert (E.expected_gt(p, q_sig, q_h) == F.F12_ONE) == (kind == "relation"), name


@pytest.mark.parametrize("n,group,chunk", V.SHAPES)
def test_group_stages_on_the_host(n, group, chunk):
    """vgroups_stages (the host's run of the five stages over many groups) against the group law and the rules of vgroups.hpp: r_i pk_i, S_g, the
    flags, a skipped pair's rows keep the sentinel, the partial of a chunk that folds nothing is exactly one, the verdicts by bilinearity"""
    b = V.groups_batch(n, group, chunk)
    a = V.groups_host(b)
    bad = V.check_group_arrays(b, a)
    assert not bad, bad[:10]
    assert a["result"].tolist() == V.want_results(b)
    if (n, group, chunk) == (23, 5, 2):
        assert b.cpg == 3 and V.chunks_of(3, 2, 3)[2] == (0, 0) and 1 in a["result"].tolist() and 0 in a["result"].tolist()
    if (n, group, chunk) == (23, 7, 3):  # the last group is two valid signatures that cancel: it PASSES, on a skipped own pair and two empty chunks
        assert len(b.members(3)) == 2 and V.group_sum(b, 3) is None and all(b.included(i) for i in b.members(3)) and b.cpg == 3
        assert a["result"][3] == 1 and a["gflag"][3] == V.VG_FLAG_OK and V.chunks_of(2, 3, 3)[1:] == [(0, 0), (0, 0)]
    if (n, group, chunk) == (70, 17, 8):
        pats = {g % 5 for g in range(b.G)}
        assert pats == {0, 1, 2, 3, 4} and any(V.group_sum(b, g) is None and any(b.included(i) for i in b.members(g)) for g in range(b.G))
        assert any(not any(b.included(i) for i in b.members(g)) for g in range(b.G)) and {1, 1 << 63, (1 << 64) - 1} <= set(b.scalars)


def test_group_stages_mean_the_pairing():
    """per group gt(conj(product of the partials)) == prod e_ref(r_i pk_i, H_i) e_ref(-g1, S_g) over the included instances, and the verdict is that
    value's == 1 ANDed with the flags: a valid group, a generic product with an excluded instance, a generic product with an empty chunk"""
    b = V.meaning_batch()
    a = V.groups_host(b)
    assert not V.check_group_arrays(b, a)
    t0 = time.time()
    want = [V.group_expected_gt(b, g) for g in range(b.G)]
    assert [w == F.F12_ONE for w in want] == [True, False, False]
    for g in range(b.G):
        assert R.gt(V.group_value(b, a, g)) == want[g], "group %d" % g
        assert a["result"][g] == int(want[g] == F.F12_ONE and a["gflag"][g] & V.VG_FLAG_OK)
    assert a["result"].tolist() == [1, 0, 0]
    print("group meaning: reference %.1f s" % (time.time() - t0))
