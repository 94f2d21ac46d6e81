"""The curve operation table (tests/devcurve/ops.hpp: csrc/decode.hpp, vcurve.hpp, curve.hpp, vsign.hpp, vgroups.hpp) through the host compilation
(hostsim_curve_op) against the big-integer reference tests/curve_ref.py, bit for bit, on every launch the device test
(test_curve_device_gpu.py) makes: results, witness streams, cursors, untouched slots. The reference holds every expected value to the meaning
of the operation (affine arithmetic, [k]P ladders, RFC 9380) before it is used for its bits. Without a GPU this validates the reference, the
inputs and the host compilation; the device test then holds the three device compilations to the same expected values."""
import math
import random

import pytest

from tests import curve_edges as X
from tests import curve_ref as C
from tests import devcurve_lib as D
from tests import field_ref as F
from tests.curve_ref import K1, K2, R_ORDER, X_ABS
from tests.field_edges import P


def test_table_is_the_compiled_table():
    """the reference's table names the operations of the compiled table, in its order, with its result and witness counts and its quad column"""
    assert D.host_table() == [(n,) + C.OPS[n] for n in C.OP_NAMES]


def test_witness_counts_follow_from_the_field_table():
    """the witness column of the curve.hpp programs equals the counts formed from the field table's (fp_mul_w 1, fp2_mul_w 3, fp2_sqr_w 2,
    fp2_div_w 3) and the products each program makes; every other entry emits nothing"""
    w = C.witness_counts()
    assert (F.OPS["fp2_mul_w"][1], F.OPS["fp2_sqr_w"][1], F.OPS["fp2_div_w"][1]) == (3, 2, 3)
    assert (w["proj_double_w_fp"], w["proj_double_w_fp2"]) == (11, 30)
    assert (w["proj_add_w_fp_z0"], w["proj_add_w_fp2_z0"]) == (12, 36)
    assert (w["proj_add_w_fp_z1"], w["proj_add_w_fp2_z1"], w["proj_add_w_fp_z2"], w["proj_add_w_fp2_z2"]) == (11, 33, 11, 33)
    assert {w[n] for n in w if n.startswith("nz_double")} == {10} and {w[n] for n in w if n.startswith("nz_add")} == {8}
    for name, n_out, n_wit, _ in D.host_table():
        assert n_wit == w.get(name, 0), name


def test_reference_is_consistent():
    """the reference against itself: the isogeny coefficients are proven (images on y^2 = x^3 + 4(1 + u), additive on random pairs); psi is an
    endomorphism of the whole twist (additive on points outside the subgroup) that acts on the subgroup as [-|x|] and whose square is psi^2;
    phi(x, y) = (beta x, y) does not enter the reference at all; the two square-root methods agree up to sign; the window table of g1 holds
    d 16^w g1; a compressed point decodes to itself with either sort flag naming its own y"""
    assert C.prove_isogeny()
    pts = X.points(K2)
    a, b = pts["random"][0], pts["mixed"][0]
    psi = lambda q: C.jac_affine(K2, C.jac_psi((q[0], q[1], K2.one)))
    assert psi(C.aff_add(K2, a, b)) == C.aff_add(K2, psi(a), psi(b)) and C.on_curve(K2, psi(a))
    g = pts["subgroup"][2]
    assert psi(g) == C.aff_mul(K2, R_ORDER - X_ABS, g)
    assert psi(psi(a)) == C.jac_affine(K2, C.jac_psi2((a[0], a[1], K2.one)))
    rng = random.Random(0x5A17)
    for _ in range(6):
        x = (rng.randrange(P), rng.randrange(P))
        ok, r, _ = C.fp2_sqrt(x)
        g2 = C.fp2_sqrt_generic(x)
        assert ok == (g2 is not None) == C.fp2_is_square(x) and (not ok or g2 in (r, F.f2_neg(r)))
    tab = C.g1_window_table()
    assert tab[0][0] == C.G1_GEN and tab[3][6] == C.aff_mul(K1, 7 * 16 ** 3, C.G1_GEN) and tab[63][14] == C.aff_mul(K1, 15 * 16 ** 63 % R_ORDER, C.G1_GEN)
    for K, comp, kind in ((K1, C.g1_compress, "g1"), (K2, C.g2_compress, "g2")):
        for q in X.points(K)["subgroup"]:
            assert C.decode(kind, comp(q)) == (C.DEC_OK,) + q
            assert C.decode(kind, comp(q, not C.lex_largest(K, q[1]))) == (C.DEC_OK,) + C.aff_neg(K, q)
        assert C.decode(kind, comp(None))[0] == C.DEC_IDENTITY


def test_coverage_conditions():
    """Conditions on the inputs, reported by the reference alone: at least 8 cases for each of the five decode statuses per group, 4 for each of
    the six exits of fp2_sqrt (zero has one operand: it is listed four times), 8 on each side of the gx1 split of the map, 4 for each branch
    (identity in, doubling, cancelling, general) of each addition, for v_add also with both Z != 1, and the same for the complete formulas in
    every Z mode that admits the branch (mode 2, both z = 1, admits no identity).

    The exits of the endomorphism subgroup tests. g1_in_subgroup: "[|x|]P = +-P" is taken by the order-3 points (0, +-2) (|x| = 2 (mod 3), so
    [|x|]P = -P) and by every torsion point whose order divides |x| + 1; the others by points inside and outside the subgroup. No curve point
    but the identity takes "[|x|]P = O" or "[x^2]P = O": its order would divide |x| or x^2 and #E(Fp) = (x - 1)^2 / 3 * r, with
    gcd(|x|, |x| + 1) = 1 and r a prime above |x| (asserted below). g2_in_subgroup: "[|x|]P = O" needs an order dividing |x| and
    #E'(Fp2) = h2 r with gcd(|x|, h2) = 1 (asserted below, h2 from the polynomial of RFC 9380 8.8.2's curve family), so no curve point takes
    it either; both outcomes of the final comparison are covered."""
    x = -X_ABS
    h1 = (x - 1) ** 2 // 3
    h2 = (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    assert x ** 4 - x ** 2 + 1 == R_ORDER and X_ABS % 3 == 2
    assert math.gcd(X_ABS, h1 * R_ORDER) == 1 and math.gcd(X_ABS, h2 * R_ORDER) == 1
    assert C.aff_mul(K2, h2, X.points(K2)["random"][0]) is not None and C.aff_mul(K2, h2 * R_ORDER, X.points(K2)["random"][0]) is None
    assert C.aff_mul(K1, h1 * R_ORDER, X.points(K1)["random"][0]) is None
    for kind in ("g1", "g2"):
        counts = X.branch_counts(kind + "_decode")
        assert set(counts) == {"status %d" % s for s in range(5)} and min(counts.values()) >= 8, counts
    counts = X.branch_counts("fp2_sqrt")
    assert len(counts) == 6 and min(counts.values()) >= 4, counts
    counts = X.branch_counts("v_map_to_curve")
    assert len(counts) == 2 and min(counts.values()) >= 8, counts
    four = {"identity", "doubling", "cancelling", "general"}
    for op in C.ADDITIONS + tuple("proj_add_w_%s_z%d" % (f, m) for f in ("fp", "fp2") for m in (0, 1, 2)):
        counts = X.branch_counts(op)
        off = counts.pop("off contract", 0)  # modes 1 and 2 on a z that is not the constant one: the formula alone, which tells the modes apart
        assert off >= 4 or op[-1] == "0" or not op.startswith("proj"), (op, counts)
        assert set(counts) == (four - {"identity"} if op.endswith("z2") else four) and min(counts.values()) >= 4, (op, counts)
    assert set(X.branch_counts("jac1_add_mixed")) == {"general"}  # its domain only
    both = {}
    one2 = tuple(F.e2(K2.one))
    for (a, b), e in zip(X.cases("v_add"), C.expected("v_add", X.cases("v_add"))):
        if a[4:6] != one2 and b[4:6] != one2:
            both[e[2]] = both.get(e[2], 0) + 1
    assert set(both) == four and min(both.values()) >= 4, both
    assert set(X.branch_counts("g1_in_subgroup")) == {"phi(P) = -[x^2]P", "phi(P) != -[x^2]P", "[|x|]P = +-P"}
    assert set(X.branch_counts("g2_in_subgroup")) == {"psi(P) = [x]P", "psi(P) != [x]P"}
    assert min(X.branch_counts("g1_in_subgroup").values()) >= 4 and min(X.branch_counts("g2_in_subgroup").values()) >= 4
    for kind in ("g1", "g2"):  # decoding the order-3 points and the torsion points gives DEC_NOT_IN_SUBGROUP
        K, comp = (K1, C.g1_compress) if kind == "g1" else (K2, C.g2_compress)
        for q in X.points(K)["torsion"] + X.points(K).get("order3", []):
            assert C.decode(kind, comp(q))[0] == C.DEC_NOT_IN_SUBGROUP
    assert any(n % 64 and n > 64 for n in X.ITEM_COUNTS) and any(n % 2 for n in X.ITEM_COUNTS if n > 1) and 1 in X.ITEM_COUNTS


def test_decode_reference_equals_oracle(oracle):
    """the status the reference derives from the bytes equals the oracle's on every record, exactly; DEC_IDENTITY is the oracle's 0 with its
    infinity flag, as agree() in test_device_logic_host.py maps it"""
    for kind, recs, fn in (("g1", X.g1_records(), oracle.g1_decompress), ("g2", X.g2_records(), oracle.g2_decompress)):
        for r in recs:
            st = C.decode(kind, r)[0]
            ost, _, oinf = fn(r)
            assert (st if st != C.DEC_IDENTITY else 0) == ost and (ost != 0 or oinf == (st == C.DEC_IDENTITY)), (kind, r.hex(), st, ost, oinf)


@pytest.mark.parametrize("op", C.OP_NAMES)
def test_host_compilation_equals_reference(op):
    """every launch of the operation (all cases in order and shuffled, each branch filling a wave alone, the item counts) through
    hostsim_curve_op_batch: results, witness streams and cursors equal the reference, unowned slots keep the sentinel"""
    bad, items = [], 0
    for name, launch in X.launches(op):
        bad += [(name,) + b for b in D.run_launch("host", op, launch, D.host_runner(), 1)]
        items += len(launch)
    print("%s: %d launches, %d items, %d mismatches" % (op, len(X.launches(op)), items, len(bad)))
    assert not bad, bad[:10]
