"""Every host form of the witness chains (tests/hostsim: csrc/chains.hpp serial, prepare_vf.hpp, cofactor_par.hpp, cofactor_vf.hpp, the six-lane
team programs) on keys and signatures OFF the prime-order subgroup (tests/chain_edges.py), whole vectors and result against the oracle; and the
oracle and the host both against a Python restatement of the three segments where these inputs bite (chain_edges.prepare_reference, the
allocation chains by curve_ref.aff_mul). No GPU: the device test (test_chain_edges_gpu.py) holds the kernels to the same oracle vectors."""
import numpy as np
import pytest

from tests import chain_edges as E
from tests import curve_ref as C
from tests import field_ref as F
from tests import hostsim_lib as H
from tests import synth
from tests.curve_ref import K1, K2, R_ORDER
from tests.field_edges import P

FORMS = {"serial": (0, 0, 0), "prepare_vf": (1, 0, 0), "cofactor_par": (0, 1, 0), "cofactor_vf": (0, 2, 0), "team": (0, 0, 1)}


def _set_form(form):
    vf, par, team = FORMS[form]
    lib = H.load()
    lib.hostsim_prepare_vf(vf)
    lib.hostsim_cofactor_par(par)
    lib.hostsim_use_team(team)


@pytest.fixture(autouse=True)
def _serial_after():
    yield
    _set_form("serial")


def segment_of(marks, idx):
    """the name of the segment that holds witness index idx, from the oracle's layout marks [(name, start)]"""
    name = None
    for n, s in sorted(marks, key=lambda m: m[1]):
        if s <= idx:
            name = n
    return name


def assert_same(tag, marks, want, got):
    assert want.shape == got.shape, (tag, want.shape, got.shape)
    if not np.array_equal(want, got):
        idx = int(np.nonzero((want != got).any(axis=1))[0][0])
        seg = segment_of(marks, idx)
        start = dict(marks)[seg]
        raise AssertionError("%s: first difference at witness %d = %s + %d" % (tag, idx, seg, idx - start))


def _valid(oracle):
    pk, msg, sig, expect = synth.make_batch(oracle, 4)
    assert expect[0]
    return pk[0], msg[0].tobytes(), sig[0]


def test_encoder_equals_oracle_decode(oracle):
    """the Montgomery encoder of chain_edges on the generators equals the oracle's decompression of their compressed forms"""
    st, xy, inf = oracle.g1_decompress(C.g1_compress(C.G1_GEN))
    assert st == 0 and not inf and np.array_equal(xy, E.enc_g1(C.G1_GEN))
    st, xy, inf = oracle.g2_decompress(C.g2_compress(C.G2_GEN))
    assert st == 0 and not inf and np.array_equal(xy, E.enc_g2(C.G2_GEN))


def test_coverage_conditions():
    """Which exceptional steps the operand list meets, from the orders alone, each event named with an operand that gives it.

    Native ladder [h1^-1 mod r] pk: acc = O, acc = pk and acc = -pk all occur for the keys of order 3 and 11. An END result of O is not
    reachable for a key other than the identity: [c]pk = O needs ord(pk) | c for c = h1^-1 mod r < r, so ord(pk) | gcd(c, h1), and c is
    non-zero modulo every prime factor of h1 (1 mod 3, 9 mod 11, -2 modulo 10177, 859267 and 52437899; asserted below). So the allocation of a
    non-identity key never is (0, 1, 0).

    Prepare chain over |x|: the doubling of O is the identity signature's (the pair (0, 0)); the addition r = -q is met by the points of order
    13 (prefixes 1, 3, 6, 12 = -1). The addition r = q is met by NO curve point: the first event of a point of order n at an addition needs
    n | prefix - 1 or n | prefix + 1 with prefix < 2^64, so n <= 2^64 + 1 divides h2 r, which leaves the divisors of 13^2 23^2 2713 11953 262069
    (r and the last prime of h2 exceed 2^64); over all of those the walk finds only r = -q events or none (asserted below). In particular
    points of order 23 and 169 meet no exceptional step: they are ordinary inputs to the prepare chain, exceptional only to (r - 1) sigma = -sigma."""
    g1, g2 = E.g1_operands(), E.g2_operands()
    seen = {}
    for name, q, n in g1:
        if q is None:
            continue
        ev, end = E.g1_ladder_events(n)
        assert end != 0, name
        assert C.aff_mul(K1, E.H1_INV, q) is not None
        for k, cnt in ev.items():
            if cnt:
                seen.setdefault(k, name)
        assert any(ev.values()) == (n in (3, 11)), name  # a sum with a subgroup point has an order above every prefix: no event
    for q in E.H1_FACTORS:
        assert E.H1_INV % q != 0
    assert (E.H1_INV % 3, E.H1_INV % 11) == (1, 9) and all(E.H1_INV % q == q - 2 for q in (10177, 859267, 52437899))
    assert {n for _, _, n in g1} >= {1, 3, 11, 10177, R_ORDER, 3 * R_ORDER, 11 * R_ORDER}
    for name, q, n in g2:
        for k, _ in E.prepare_events(n):
            seen.setdefault(k, name)
    print("events:", seen)
    assert set(seen) == set(E.G1_EVENTS) | {"doubling of O", "addition r = -q"}, seen
    assert seen["addition r = -q"] == "order 13" and seen["doubling of O"] == "identity"
    kinds = {d: E.prepare_events(d) for d in E.small_divisors()}
    assert all(not ev or ev[0][0] == "addition r = -q" for d, ev in kinds.items() if d > 1)
    assert kinds[13] == [("addition r = -q", 4)] and not kinds[23] and not kinds[169] and not kinds[529]
    orders = {n for _, _, n in g2}
    assert orders >= {1, 13, 23, R_ORDER, 13 * R_ORDER, 23 * R_ORDER}
    print("order 169:", "present" if 169 in orders else "absent: [r h2 / 169] Q had order 13 or 1 for every Q tried (the 13-part is not cyclic, or by chance)")
    for name, q, n in g2:  # the event list is what the group law says: the walk on the point itself, by the affine law
        if q is None or n > 1 << 64:
            continue
        acc, first, k = q, None, 0
        for i in range(62, -1, -1):
            acc, k = C.aff_add(K2, acc, acc), k + 1
            if (C.X_ABS >> i) & 1:
                if first is None and acc == q:
                    first = ("addition r = q", k)
                if first is None and acc == C.aff_neg(K2, q):
                    first = ("addition r = -q", k)
                acc, k = C.aff_add(K2, acc, q), k + 1
        assert ([first] if first else []) == E.prepare_events(n), (name, first)


def _check_tiers(tag, marks, w, pk_pt, sig_pt, input_modes=(False, False)):
    """the three segments of one vector against the Python restatement"""
    off = dict(marks)
    order = sorted(marks, key=lambda m: m[1])
    end_of = lambda name: order[[n for n, _ in order].index(name) + 1][1]
    seg = E.els(w[off["prepare.sig"]:off["prepare.sig"] + 1096])
    want, coeff = E.prepare_reference(sig_pt)
    bad = [i for i in range(1096) if seg[i] != want[i]]
    assert not bad, "%s: prepare.sig differs from the restatement first at element %d" % (tag, bad[0])
    assert E.prepare_coefficients_of(seg) == coeff, tag
    if not input_modes[0]:
        a, b = off["pk_alloc"], end_of("pk_alloc")
        pre = None if pk_pt is None else C.aff_mul(K1, E.H1_INV, pk_pt)
        want3 = [0, F.enc(1), 0] if pre is None else [F.enc(pre[0]), F.enc(pre[1]), F.enc(1)]
        assert E.els(w[a:a + 3]) == want3, "%s: pk_alloc allocates something else than [h1^-1 mod r] pk" % tag
        m = [F.dec(v) for v in E.els(w[b - 6:b])]  # the last statement is an addition (h1 is odd): X3 = m0 - m1, Y3 = m2 + m3, Z3 = m4 + m5
        assert E.H1 & 1
        assert E.proj_is(K1, ((m[0] - m[1]) % P, (m[2] + m[3]) % P, (m[4] + m[5]) % P), C.aff_mul(K1, E.H1, pre)), "%s: pk_alloc chain end is not [h1] of the allocation" % tag
    if not input_modes[1]:
        a, b = off["sig_alloc"], end_of("sig_alloc")
        want6 = [0, 0, F.enc(1), 0, 0, 0] if sig_pt is None else F.e2(sig_pt[0]) + F.e2(sig_pt[1]) + F.e2((1, 0))
        assert E.els(w[a:a + 6]) == want6, "%s: sig_alloc's first six elements are not the input" % tag
        # r - 1 is even: the (r - 1) chain ends with a doubling (30 witnesses) before the 35 of enforce_equal and the zero tests
        assert (R_ORDER - 1) & 1 == 0
        d = [F.dec(v) for v in E.els(w[b - 65:b - 35])]
        mul = lambda i: ((d[i] - d[i + 1]) % P, (d[i + 2] - d[i] - d[i + 1]) % P)
        y_frag, x_frag, t, t2, z3 = mul(12), mul(15), mul(18), mul(24), mul(27)
        end = (F.f2_sub(x_frag, t2), F.f2_add(y_frag, t), C.T.f2_scale(z3, 4))
        assert E.proj_is(K2, end, C.aff_mul(K2, R_ORDER - 1, sig_pt) if sig_pt is not None else None), "%s: sig_alloc chain end is not [r - 1] sigma" % tag


def _cases():
    out = [("key: " + name, i, None) for i, (name, _, _) in enumerate(E.g1_operands())]
    out += [("sig: " + name, None, j) for j, (name, _, _) in enumerate(E.g2_operands())]
    names1 = [n for n, _, _ in E.g1_operands()]
    names2 = [n for n, _, _ in E.g2_operands()]
    out.append(("both: order 3 key, order 13 signature", names1.index("order 3: (0, 2)"), names2.index("order 13")))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_forms_equal_oracle(oracle, case):
    """each operand through hostsim_lib.witness in every host form: the whole vector and the result equal the oracle's; the oracle's and the
    serial host's prepare.sig, pk_alloc and sig_alloc hold the Python restatement"""
    tag, i, j = case
    pk, msg, sig = _valid(oracle)
    pk_pt = sig_pt = False
    if i is not None:
        pk_pt = E.g1_operands()[i][1]
        pk = E.enc_g1(pk_pt)
    if j is not None:
        sig_pt = E.g2_operands()[j][1]
        sig = E.enc_g2(sig_pt)
    marks, _, _ = oracle.layout(32)
    nw, _, res, want = oracle.witness(pk, msg, sig)
    if pk_pt is False:
        pk_pt = (F.dec(E.el(pk[:6])), F.dec(E.el(pk[6:])))
    if sig_pt is False:
        s = [F.dec(E.el(sig[6 * k:6 * k + 6])) for k in range(4)]
        sig_pt = ((s[0], s[1]), (s[2], s[3]))
    _check_tiers(tag + " [oracle]", marks, want, pk_pt, sig_pt)
    failures = []
    for form in FORMS:
        _set_form(form)
        r, got = H.witness(pk, msg, sig)
        try:
            assert bool(r) == res, "%s [%s]: result %r, oracle %r" % (tag, form, r, res)
            assert_same("%s [%s]" % (tag, form), marks, want, got)
            if form == "serial":
                _check_tiers(tag + " [host]", marks, got, pk_pt, sig_pt)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


IO_CASES = [("order 3 key, order 13 signature", "order 3: (0, 2)", "order 13"), ("order 11 key, order 23 signature", "order 11", "order 23"),
            ("subgroup + order 3 key, subgroup + order 13 signature", "subgroup + order 3", "subgroup + order 13")]


@pytest.mark.parametrize("modes", [(1, 0), (0, 1), (1, 1)], ids=["pk input", "sig input", "both input"])
def test_witness_io_equals_oracle(oracle, modes):
    """keys / signatures allocated as public inputs skip the prime-order chain: vector, instance and result still equal the oracle's witness_io"""
    g1 = {n: q for n, q, _ in E.g1_operands()}
    g2 = {n: q for n, q, _ in E.g2_operands()}
    _, msg, _ = _valid(oracle)
    marks, _, _ = oracle.layout_io(32, bool(modes[0]), bool(modes[1]))
    failures = []
    for tag, kn, sn in IO_CASES:
        pk, sig = E.enc_g1(g1[kn]), E.enc_g2(g2[sn])
        _, _, res, want, winst = oracle.witness_io(pk, msg, sig, bool(modes[0]), bool(modes[1]))
        _check_tiers(tag + " [oracle io]", marks, want, g1[kn], g2[sn], (bool(modes[0]), bool(modes[1])))
        for form in ("serial", "prepare_vf", "team"):
            _set_form(form)
            r, got, inst = H.witness_io(pk, msg, sig, modes[0], modes[1])
            try:
                assert bool(r) == res and np.array_equal(inst, winst), (tag, form, r, res)
                assert_same("%s [%s]" % (tag, form), marks, want, got)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, failures


@pytest.mark.parametrize("selected", [1, 0], ids=["selected", "not selected"])
def test_witness_aggregate_equals_oracle(oracle, selected):
    """aggregate_verify with K = 3 and one key of small order, selected by the bitmap or not"""
    g1 = {n: q for n, q, _ in E.g1_operands()}
    failures = []
    for kn in ("order 3: (0, 2)", "order 11"):
        bitmap = [1, selected, 1]
        pks, bm, msg, sig, _ = synth.make_aggregate(oracle, 3, bitmap)
        pks = pks.copy()
        pks[1] = E.enc_g1(g1[kn])
        nw, res, cnt, marks, want = oracle.witness_aggregate(pks, bm, msg.tobytes(), sig)
        for form in ("serial", "prepare_vf", "team"):
            _set_form(form)
            r, c, got, _ = H.witness_aggregate(pks, bm, msg.tobytes(), sig)
            try:
                assert bool(r) == res and c == cnt, (kn, form, r, res, c, cnt)
                assert_same("aggregate %s [%s]" % (kn, form), [m for m in marks.items() if m[0]], want, got)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, failures


def test_witness_multi_equals_oracle(oracle):
    """the N+1-pair product with K = 3, one key of small order and a signature of order 13"""
    g1 = {n: q for n, q, _ in E.g1_operands()}
    g2 = {n: q for n, q, _ in E.g2_operands()}
    failures = []
    for kn, sn in (("order 3: (0, p - 2)", None), ("order 11", "order 13")):
        pks, msgs, sig, _ = synth.make_multi(oracle, 3)
        pks = pks.copy()
        pks[2] = E.enc_g1(g1[kn])
        if sn:
            sig = E.enc_g2(g2[sn])
        nw, res, marks, want = oracle.witness_multi(pks, msgs, sig)
        for form in ("serial", "prepare_vf", "team"):
            _set_form(form)
            r, got, _ = H.witness_multi(pks, msgs, sig)
            try:
                assert bool(r) == res, (kn, form, r, res)
                assert_same("multi %s [%s]" % (kn, form), [m for m in marks if m[0]], want, got)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, failures
