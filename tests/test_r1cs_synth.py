"""The device R1CS evaluator's host-compilable parts on synthetic systems at their arithmetic edges (tests/r1cs_synth.py), without a GPU: the
encoder's coefficient classes and block cut (csrc/r1cs_encode.hpp through hostsim_r1cs_encode), the kernel's row arithmetic (csrc/r1cs_row.hpp
through hostsim_r1cs_row: accumulator, class dispatch, redc14) against big integers, the big-integer reference against the independent host check
hostsim_lib.r1cs_check, and fp.hpp's products and inversions against Python integers."""
import importlib

import numpy as np
import pytest

from tests import hostsim_lib, r1cs_synth as S
from tests.field_edges import field_edge_values
from tests.r1cs_synth import GEN, NEG, P, POS, R, R_INV, SMALL

SHAPES = (1, 3)  # n_instance_vars
_SYS = {}


def system(ni):
    if ni not in _SYS:
        sys = S.make_system(ni)
        rc, enc = hostsim_lib.r1cs_encode(sys)
        assert rc == 0
        _SYS[ni] = (sys, enc)
    return _SYS[ni]


def row_codes(sys, enc, r, m):
    rp, col, _ = sys["ABC"[m]]
    lo, hi = int(rp[r]), int(rp[r + 1])
    return col[lo:hi], enc["codes"][m][lo:hi]


@pytest.mark.parametrize("ni", SHAPES)
def test_encoder_classes_and_block_cut(ni):
    """every entry's code is the class and payload the encoding's definition gives its canonical coefficient (the boundary coefficients: the stated
    table); a table entry is the entry's Montgomery integer, one per distinct coefficient; the blocks partition the rows, there are at least 9 of
    them, their number is no multiple of the 4 waves of a workgroup, and the 6 000-entry row is a block of its own; blsw_r1cs_device_bytes accepts
    the system and reports the encoder's size"""
    sys, enc = system(ni)
    seen, table = {}, [S.to_int(t) for t in enc["table"]]
    assert len(set(table)) == len(table)
    for r, row in enumerate(sys["rows"]):
        for m in range(3):
            cols, codes = row_codes(sys, enc, r, m)
            assert [k for k, _ in row[m]] == cols.tolist()
            for (_, c), code in zip(row[m], codes.tolist()):
                cls, payload = S.expected_class(c)
                assert code >> 30 == cls, (r, m, hex(c))
                if cls == GEN:
                    assert table[code & SMALL] == c * R % P
                else:
                    assert code & SMALL == payload
                seen[c] = (code >> 30, (code & SMALL) if cls != GEN else None)
    for c, want in S.BOUNDARY.items():
        assert seen[c] == want == S.expected_class(c), hex(c)
    assert set(S.coefficients()) <= set(seen) and len(table) == sum(v[0] == GEN for v in seen.values())
    blk = enc["blk"].tolist()
    n_blk = len(blk) - 1
    assert blk[0] == 0 and blk[-1] == sys["n_constraints"] and all(a < b for a, b in zip(blk, blk[1:]))
    assert n_blk >= 9 and n_blk % 4 != 0, blk
    big = sys["tags"]["big"]
    assert big in blk and blk[blk.index(big) + 1] == big + 1 and 0 < blk.index(big) < n_blk - 1
    pkg = importlib.import_module("bls-verify-gadget_amd")
    assert pkg.r1cs_device_bytes(sys) == enc["bytes"]


def test_encoder_return_codes_on_malformed_systems():
    """the exported encoder refuses what blsw_r1cs_device_bytes refuses, with the same code: a zero coefficient, one equal to p, columns out of
    order, a column beyond z"""
    pkg = importlib.import_module("bls-verify-gadget_amd")
    sys, _ = system(1)

    def both(change):
        bad = {k: (tuple(a.copy() for a in v) if k in "ABC" else v) for k, v in sys.items()}
        change(bad)
        rc, _ = hostsim_lib.r1cs_encode(bad)
        with pytest.raises(pkg.BlswError, match="failed: %d" % rc):
            pkg.r1cs_device_bytes(bad)
        return rc

    def set_val(name, k, v):
        def f(bad):
            bad[name][2][k] = S.limbs([v])[0]
        return f

    def swap_columns(bad):
        rp, col, _ = bad["A"]
        r = sys["tags"]["big"]
        col[int(rp[r])], col[int(rp[r]) + 1] = col[int(rp[r]) + 1], col[int(rp[r])]

    def column_beyond(bad):
        bad["C"][1][-1] = sys["n_instance_vars"] + sys["n_witness"]

    assert both(set_val("A", 0, 0)) == 1 and both(set_val("B", 5, P)) == 1 and both(set_val("C", 7, P + 1)) == 1
    assert both(swap_columns) == 1 and both(column_beyond) == 1


def kernel_accumulator(entries, z):
    """the integer the kernel's 14-limb accumulator holds before redc14: a small positive coefficient adds v z, a small negative one v (p - z), a table
    coefficient the reduced product"""
    x = 0
    for k, c in entries:
        cls, v = S.expected_class(c)
        x += v * z[k] if cls == POS else (v * (P - z[k]) if cls == NEG else c * z[k] % P)
    return x


@pytest.mark.parametrize("ni", SHAPES)
def test_row_arithmetic_equals_big_integers(ni):
    """hostsim_r1cs_row (row_term per entry, redc14) == (sum of c z) R^-1 mod p on every row and matrix of the system, for 16 assignments in which
    the pool columns take every edge value of z, in both forms: always below p; the cancelling pairs give exactly 0 although their accumulator
    holds a non-zero multiple of p; in the limb-13 rows and the 6 000-entry row the accumulator's limb 13 is non-zero (the premise, checked)"""
    sys, enc = system(ni)
    tags = sys["tags"]
    seen_z = set()
    for form in (0, 1):
        for d in range(16 if form == 0 else 3):
            z = S.assignment(sys, d, form)
            seen_z.update(z[k] for k in sys["blocks"]["pool"])
            zl = S.limbs(z)
            for r, row in enumerate(sys["rows"]):
                for m in range(3):
                    cols, codes = row_codes(sys, enc, r, m)
                    got = hostsim_lib.r1cs_row(cols, codes, enc["table"], zl)
                    assert got == S.redc_ref(row[m], z), (form, d, r, m)
                    assert got < P
            if d == 0:
                for tag, r in tags.items():
                    if tag.startswith("cancel_"):
                        m = 1 if "_in_B" in tag else (2 if tag.endswith("_in_C") else 0)
                        pair = [e for e in sys["rows"][r][m] if e[0] != sys["slack"][r]]
                        cols, codes = row_codes(sys, enc, r, m)
                        acc = kernel_accumulator(pair, z)
                        assert len(pair) == 2 and acc % P == 0 and (acc > 0) == ("gen_zero" not in tag), tag  # table products of z = 0 are 0
                        assert hostsim_lib.r1cs_row(cols[:2], codes[:2], enc["table"], zl) == 0, tag
                    if tag.startswith("limb13_") or tag == "big":
                        m = "ABC".index(tag[-1]) if tag != "big" else 0
                        assert kernel_accumulator(sys["rows"][r][m], z) >> 416, tag
    assert set(S.EDGE_Z) <= seen_z


def test_row_arithmetic_every_coefficient_on_every_edge_value():
    """one-entry and two-entry rows: every coefficient of the generator (the class borders among them) on every edge value of z, 0 and p - 1 under
    the largest small negative coefficient included, and on stored values the kernel does not reduce (p, p + 1, 2^384 - 1) under the small classes"""
    coeffs = S.coefficients()
    mont = S.limbs([c * R % P for c in coeffs])
    n = len(coeffs)
    one = (np.arange(n + 1, dtype=np.uint64), np.ones(n, dtype=np.uint32), mont)
    sys = {"n_constraints": n, "n_instance_vars": 1, "n_witness": 1, "A": one, "B": one, "C": one}
    rc, enc = hostsim_lib.r1cs_encode(sys)
    assert rc == 0
    codes, table = enc["codes"][0], enc["table"]
    for zv in S.EDGE_Z:
        zl = S.limbs([1, zv])
        for j, c in enumerate(coeffs):
            assert hostsim_lib.r1cs_row([1], codes[j:j + 1], table, zl) == c * zv * R_INV % P, (hex(c), hex(zv))
            k = (j + 1) % n
            assert hostsim_lib.r1cs_row([0, 1], [codes[k], codes[j]], table, zl) == (coeffs[k] + c * zv) * R_INV % P
    # unreduced input: the accumulator takes the stored integer as it is (a positive small coefficient), the result is still reduced
    for zv in (P, P + 1, (1 << 384) - 1):
        zl = S.limbs([1, zv])
        for j, c in enumerate(coeffs):
            if S.expected_class(c)[0] == POS:
                got = hostsim_lib.r1cs_row([1], codes[j:j + 1], table, zl)
                assert got == c * zv * R_INV % P and got < P


@pytest.mark.parametrize("ni", SHAPES)
def test_reference_agrees_with_the_host_check(ni):
    """the big-integer reference and hostsim_lib.r1cs_check (the suite's independent host check, Montgomery form) agree: -1 on satisfied assignments,
    and the bumped row for each single-slack corruption (+1, -1 or 2^352 in turn; with three instance variables: each of the special rows and every
    fourth of the others, the rows being the same kinds); the canonical-form assignment of the same system is satisfied too"""
    sys, _ = system(ni)
    special = set(sys["tags"].values())

    def host(z):
        zl = S.limbs(z)
        return hostsim_lib.r1cs_check(sys, zl[ni:], zl[:ni]) if ni > 1 else hostsim_lib.r1cs_check(sys, zl[ni:])

    for d in (0, 1, 7):
        z = S.assignment(sys, d, 0)
        assert S.first_unsatisfied(sys, z, 0) == -1 == host(z)
        assert S.first_unsatisfied(sys, S.assignment(sys, d, 1), 1) == -1
    z0 = S.assignment(sys, 2, 0)
    n_slack = 0
    for r, s in enumerate(sys["slack"]):
        if s is None or (ni == 3 and r not in special and r % 4):
            continue
        z = list(z0)
        S.bump(sys, z, r, (1, P - 1, 1 << 352)[n_slack % 3])
        n_slack += 1
        assert S.first_unsatisfied(sys, z, 0) == r == host(z), r
    assert n_slack >= (250 if ni == 1 else 100) and (ni == 3 or n_slack == sum(s is not None for s in sys["slack"]))


def test_field_micro_checks():
    """fp_mul (28-bit limbs) and fp_mul32 == a b R^-1 mod p on all ordered pairs of the edge set plus 20 seeded random values; fp_inv (safegcd) and
    fp_inv_fermat == a^-1 R^2 mod p (0 for 0) on every value"""
    vals = field_edge_values()
    assert len(vals) == 110 and len(set(vals)) >= 100 and all(0 <= v < P for v in vals)
    bad = []
    for a in vals:
        for b in vals:
            want = a * b * R_INV % P
            if hostsim_lib.fp_mul(a, b) != want:
                bad.append(("fp_mul", hex(a), hex(b)))
            if hostsim_lib.fp_mul32(a, b) != want:
                bad.append(("fp_mul32", hex(a), hex(b)))
        want = pow(a, -1, P) * R * R % P if a else 0
        if hostsim_lib.fp_inv(a) != want:
            bad.append(("fp_inv", hex(a)))
        if hostsim_lib.fp_inv_fermat(a) != want:
            bad.append(("fp_inv_fermat", hex(a)))
    print("%d values: %d pairs x 2 products, %d x 2 inversions, %d mismatches" % (len(vals), len(vals) ** 2, len(vals), len(bad)))
    assert not bad, bad[:10]
