"""The team operation table (tests/devteam/ops.hpp: the six-lane executor of csrc/team.hpp, its lane routines and its op tables) on the host:
the team form, run by the looped host team of tests/hostsim, against the single-lane statement it claims to equal and against the big-integer
reference tests/team_ref.py, bit for bit, on every launch the device test (test_team_device_gpu.py) makes: the six coefficients, the witness
stream, the cursors, the sentinel behind the stream. This evaluates every op table numerically on chosen operands: 0, 1, a single non-zero
coefficient, p - 1 everywhere, a == b, sparse lines with a zero coefficient, points at infinity. The device test then holds the device's
TeamLanes to the same expected values."""
import pytest

from tests import devteam_lib as D
from tests import field_ref as F
from tests import hostsim_lib
from tests import team_ref as T
from tests.field_edges import ONE, P


def test_table_is_the_compiled_table():
    """the reference's entry list names the entries of the compiled table, in its order, with its exec / exec_hot split; the stream lengths are
    the compiled table's own (formed from the op tables' counts), and those of the whole final exponentiation are the layout's"""
    table = D.host_table()
    assert [(n, d) for n, _, _, d in table] == [(n, T.OPS[n][0]) for n in T.OP_NAMES]
    w = {n: (nw, tail) for n, nw, tail, _ in table}
    lay = hostsim_lib.layout(32)
    assert w["final_exp_is_one"] == (lay["n_witness"] - lay["off_final_exp"], lay["n_witness"] - lay["off_is_one"])
    assert w["is_one_w"] == (T.IS_ONE_WITNESSES, T.IS_ONE_WITNESSES) and w["inverse_w"] == (54, 0) and w["ELLGS"] == w["ELLGH"] == (0, 0)
    assert all(tail == 0 for n, (_, tail) in w.items() if n not in T.VERDICT_OPS)


def test_reference_is_consistent():
    """the reference against itself: the generators are on their curves and of order r; the cyclotomic map is the square on the cyclotomic subgroup
    and not elsewhere; the verdict cases of the final exponentiation are what they are meant to be; the is_one cases have exactly one false flag,
    in every position; the sparse embeddings multiply as the dense elements they are"""
    assert (T.G1_GEN[1] ** 2 - T.G1_GEN[0] ** 3 - 4) % P == 0
    g, p5, p7 = T.g2_points()  # asserts on-curve and [r] G = O
    assert all(T.g2_on_curve(x) for x in (g, p5, p7)) and T.g2_add(p5, T.g2_neg(p5)) is None and T.g2_add(T.g2_add(g, g), T.g2_add(g, T.g2_add(g, g))) == p5
    for blk in F.cyclotomic_elements():
        x = F.d12(blk)
        assert T.is_cyclotomic(x) and T.f12_cyc_formula(x) == F.f12_mul(x, x)
    rnd = F.d12(F.fp12_elements()[-1])
    assert not T.is_cyclotomic(rnd) and T.f12_cyc_formula(rnd) != F.f12_mul(rnd, rnd)
    assert T.f12_cyc_formula((F.F6_ZERO, F.F6_ZERO)) == (F.F6_ZERO, F.F6_ZERO)
    fe = T.final_exp_elements()
    assert [T.final_exp_is_one(F.d12(x)) for x, _ in fe] == [v for _, v in fe] == [True, True, True, True, False, False]
    assert all(F.d12(x) != F.F12_ONE for x, _ in fe[1:])
    false_at = []
    for blk in T.is_one_elements()[3:]:
        v, w = T.is_one_stream(F.d12(blk))
        flags = [w[h * 17 + k * 5 + 4] for h in range(2) for k in range(3)]
        assert not v and flags.count(0) == 1 and w[34] == 0
        false_at.append(flags.index(0))
    assert false_at == [k // 4 for k in range(24)]  # two coordinates per coefficient, two replacements per coordinate
    assert T.is_one_stream(F.F12_ONE)[0] and T.is_one_stream(F.F12_ONE)[1][15:17] == [ONE, ONE]


def test_inputs_cover_what_they_claim():
    """the lines hold a zero c0, a zero c1, a zero c4, the all-zero line and the all-(p - 1) line; the variable point meets all 25 combinations of
    its coordinates; the Fp12 operands hold 0, 1 and a single non-zero coefficient in each of the six positions; MUL has its diagonal; the G2
    cases hold the identity on either side and on both, P + P, P + (-P) and operands with Z != 1; every launch arrangement is there"""
    l4, l6, lv = T.lines4(), T.lines6(), T.lines_var()
    assert (0, 0, 0, 0) in l4 and (P - 1,) * 4 in l4 and any(x[:2] == (0, 0) != x[2:] for x in l4) and any(x[2:] == (0, 0) != x[:2] for x in l4)
    assert (0,) * 6 in l6 and (P - 1,) * 6 in l6 and all(any(x[2 * k:2 * k + 2] == (0, 0) and x.count(0) == 2 for x in l6) for k in range(3))
    g = T.g1_coords()
    assert {x[4:] for x in lv} == {(a, b) for a in g for b in g} and {0, 1, P - 1, ONE} <= set(g)
    els = [F.d12(x) for x in F.fp12_elements()]
    flat = [F.flat12(x) for x in els]
    assert (0,) * 12 in flat and F.flat12(F.F12_ONE) in flat
    for j in range(6):
        assert any(any(f[2 * j:2 * j + 2]) and not any(f[:2 * j]) and not any(f[2 * j + 2:]) for f in flat), j
    assert sum(a is b for a, b, _ in T.cases("MUL")) == len(F.fp12_elements())
    add = [(T.g2_affine_of_block(a), T.g2_affine_of_block(b), F.d2(a, 4), F.d2(b, 4)) for a, b, _ in T.cases("G2ADD")]
    kinds = {(p is None, q is None) for p, q, _, _ in add}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert any(p is not None and p == q for p, q, _, _ in add) and any(p is not None and q == T.g2_neg(p) for p, q, _, _ in add)
    assert any(zp == (P - 1, 0) for _, _, zp, _ in add) and any(zp not in (F.F2_ONE, (P - 1, 0)) and zq != F.F2_ONE for _, _, zp, zq in add)
    assert any(T.g2_affine_of_block(a) is None for a, _, _ in T.cases("G2DBL"))
    for op in T.OP_NAMES:
        names = [n for n, _ in T.launches(op)]
        assert names[:4] == ["edges", "shift3", "shift9", "teams"] and ["n=%d" % k for k in T.item_counts(op)] == names[4:4 + len(T.item_counts(op))], op
        assert ("mixed" in names) == (op in ("seq", "exp_by_x")), op
        assert {1, 9, 10, 11, 19, 20, 21} <= set(T.item_counts(op)) and (op in T.LONG_OPS or T.item_counts(op) == (1, 9, 10, 11, 19, 20, 21, 60, 64, 100)), op
        src = T.cases(op)
        teams = dict(T.launches(op))["teams"]
        assert all(teams[10 * i] == teams[10 * i + 4] == teams[10 * i + 9] == it for i, it in enumerate(src)), op


@pytest.mark.parametrize("op", T.OP_NAMES)
def test_host_team_equals_single_lane_and_reference(op):
    """every launch of the entry through the looped host team (exec; exec_hot, the same text on the host, on the edge launch): the six coefficients,
    the stream and the cursor equal the single-lane form's, which D.expected holds to the reference's values (the G2 entries: to the group law), to
    the reference's stream where it states one, and to the table's witness count; the slots behind the stream keep the sentinel"""
    bad, items = [], 0
    for name, launch in T.launches(op):
        bad += [(name,) + b for b in D.check_host("exec", op, launch)]
        items += len(launch)
    bad += [("edges",) + b for b in D.check_host("exec_hot", op, T.cases(op))]
    print("%s: %d launches, %d items, %d mismatches" % (op, len(T.launches(op)), items, len(bad)))
    assert not bad, bad[:10]

