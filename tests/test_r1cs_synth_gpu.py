"""The device R1CS evaluator (blsw_r1cs_*, ConstraintChecker.from_matrices) on the MI355X against the big-integer reference of tests/r1cs_synth.py, on
synthetic systems at the kernel's arithmetic edges (accumulator limb 13, the coefficient class borders, edge values of z) and at the edges of its
block and wave mapping (a row that is a block of its own, a block count that is no multiple of the waves of a workgroup, failures in two
workgroups, one-row evaluate windows at block edges, padded strides). Every comparison is exact integer equality. The CPU half (encoder, row
arithmetic on the host, the reference against the host check) is tests/test_r1cs_synth.py."""
import importlib
import random

import numpy as np
import pytest

from tests import hostsim_lib, r1cs_synth as S
from tests.r1cs_synth import P

pytestmark = pytest.mark.gpu
N = 130  # not a multiple of 64: a full wave, a second one, and two lanes of a third
LANES = (0, 63, 64, 129)
DISTINCT = 16  # instance i carries base assignment i % 16
SENTINEL = 0x5A5A5A5A5A5A5A5A
_SYS, _DATA = {}, {}


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return importlib.import_module("bls-verify-gadget_amd")


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def set_elem(t, i, k, v):
    """t[i, k] = the integer v in a [n, stride, 6] int64 cuda tensor"""
    t[i, k] = to_dev(S.limbs([v])[0])


class Data:
    """a system, its encoding and checker, and N satisfied instances of one form as device tensors with padded strides full of junk"""

    def __init__(self, pkg, ni, form):
        if ni not in _SYS:
            sys = S.make_system(ni)
            rc, enc = hostsim_lib.r1cs_encode(sys)
            assert rc == 0
            _SYS[ni] = (sys, enc, pkg.ConstraintChecker.from_matrices(sys, "cuda:0"))
        self.sys, self.enc, self.chk = _SYS[ni]
        self.ni, self.form, self.nw = ni, form, self.sys["n_witness"]
        self.base = [S.assignment(self.sys, d, form) for d in range(DISTINCT)]
        pick = np.arange(N) % DISTINCT
        self.w = to_dev(S.witness_array(self.sys, self.base, pad=5)[pick])
        self.inst = to_dev(S.instance_array(self.sys, self.base, pad=2 if ni > 1 else 0)[pick])
        assert self.w.shape == (N, self.nw + 5, 6) and self.inst.shape[1] == (5 if ni > 1 else 1)

    def z(self, i):
        return list(self.base[i % DISTINCT])

    def instances(self):
        """the instance arguments the shape allows: the tensor, and for a circuit without public inputs also none"""
        return (self.inst,) if self.ni > 1 else (None, self.inst)


def data(pkg, ni, form):
    if (ni, form) not in _DATA:
        _DATA[(ni, form)] = Data(pkg, ni, form)
    return _DATA[(ni, form)]


def interior_block(sys, enc):
    """(first row, last row) of a block that is neither the first nor the last nor the one-row block, both rows with a slack"""
    blk = enc["blk"].tolist()
    for b in range(1, len(blk) - 2):
        first, last = blk[b], blk[b + 1] - 1
        if last > first and sys["slack"][first] is not None and sys["slack"][last] is not None:
            return first, last
    raise AssertionError("no interior block with slacks at both ends: %r" % blk)


def block_of(enc, row):
    return int(np.searchsorted(enc["blk"], row, side="right")) - 1


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("ni", (1, 3))
def test_satisfied(pkg, ni, form):
    """130 instances with padded strides of junk (most of it not below p): every instance satisfies every row, nothing of z is unreduced; without
    public inputs both with the library's constant one and with an explicit instance tensor"""
    d = data(pkg, ni, form)
    blk = d.enc["blk"]
    assert len(blk) - 1 >= 9 and (len(blk) - 1) % 4 != 0  # three workgroups of waves, the last one not full
    for inst in d.instances():
        assert d.chk.which_is_unsatisfied(d.w, inst, form=form).tolist() == [-1] * N
        assert d.chk.first_unreduced(d.w, inst, form=form).tolist() == [-1] * N
        assert bool(d.chk.is_satisfied(d.w, inst, form=form).all())


@pytest.mark.parametrize("ni", (1, 3))
def test_unsatisfied_rows(pkg, ni):
    """a slack bumped by +1, -1 or 2^352 (mod p) in row 0, the last row, the first and the last row of an interior block and the 6 000-entry row,
    each in instances 0, 63, 64 and 129 at once, both forms: the first unsatisfied row is the bumped one (the construction's, the reference's and,
    for +1 in Montgomery form, the host check's), every other instance stays -1. One instance with failures in blocks of two workgroups, the later block's
    written first: the smaller row"""
    for form in (0, 1):
        d = data(pkg, ni, form)
        sys, enc = d.sys, d.enc
        first, last = interior_block(sys, enc)
        rows = [0, sys["n_constraints"] - 1, first, last, sys["tags"]["big"]]
        for row, delta in [(r, delta) for delta in (1, P - 1, 1 << 352) for r in rows]:
            w = d.w.clone()
            want = [-1] * N
            for i in LANES:
                z = d.z(i)
                S.bump(sys, z, row, delta)
                set_elem(w, i, sys["slack"][row] - ni, z[sys["slack"][row]])
                want[i] = row
                assert S.first_unsatisfied(sys, z, form) == row
                if form == 0 and delta == 1:
                    zl = S.limbs(z)
                    assert (hostsim_lib.r1cs_check(sys, zl[ni:], zl[:ni]) if ni > 1 else hostsim_lib.r1cs_check(sys, zl[ni:])) == row
            for inst in d.instances():
                assert d.chk.which_is_unsatisfied(w, inst, form=form).tolist() == want, (form, row, delta)
            assert d.chk.is_satisfied(w, d.inst, form=form).tolist() == [x < 0 for x in want]
        # two failures of one instance in the blocks of two workgroups
        slack_rows = [r for r, s in enumerate(sys["slack"]) if s is not None]
        early = next(r for r in slack_rows if block_of(enc, r) == 1)
        late = next(r for r in reversed(slack_rows) if block_of(enc, r) == len(enc["blk"]) - 2)
        assert block_of(enc, early) // 4 != block_of(enc, late) // 4
        w = d.w.clone()
        want = [-1] * N
        for i in (64, 129):
            z = d.z(i)
            for row in (late, early):
                S.bump(sys, z, row, 1 + i)
                set_elem(w, i, sys["slack"][row] - ni, z[sys["slack"][row]])
            assert S.first_unsatisfied(sys, z, form) == early
            want[i] = early
        assert d.chk.which_is_unsatisfied(w, d.inst, form=form).tolist() == want


@pytest.mark.parametrize("ni", (1, 3))
def test_evaluate_rows_and_windows(pkg, ni):
    """A z, B z, C z of every row, both forms: instances 0, 63 and 129 equal the reference (below p, the cancelling rows exactly 0), and every
    instance equals the one that carries the same assignment. The raw call into oversized sentinel-filled buffers writes [n][count][6] and nothing
    else, for one-row windows at a block's first and last row, the one-row block, and a window over three blocks"""
    import torch

    L = pkg.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for form in (0, 1):
        d = data(pkg, ni, form)
        sys, enc = d.sys, d.enc
        nc = sys["n_constraints"]
        full = d.chk.evaluate(d.w, d.inst, form=form)
        host = [t.cpu().numpy().view(np.uint64) for t in full]
        assert host[0].shape == (N, nc, 6)
        for i in (0, 63, 129):
            ref = S.evaluate_ref(sys, d.z(i), form)
            for m in range(3):
                got = [S.to_int(x) for x in host[m][i]]
                assert got == [t[m] for t in ref], (form, i, m)
                assert max(got) < P
        for tag, r in sys["tags"].items():
            if tag.startswith("cancel_") and not tag.endswith("_in_C"):
                assert not host[1 if "_in_B" in tag else 0][:, r].any(), tag
        for m in range(3):
            assert np.array_equal(host[m], host[m][np.arange(N) % DISTINCT])
        if ni == 1:
            for a, b in zip(full, d.chk.evaluate(d.w, None, form=form)):
                assert torch.equal(a, b)
        first, last = interior_block(sys, enc)
        big = sys["tags"]["big"]
        assert block_of(enc, big - 2) + 2 == block_of(enc, big) + 1 == block_of(enc, big + 2)
        for begin, count in ((first, 1), (last, 1), (big, 1), (big - 2, 5)):
            lead, body, tail = 6, N * count * 6, 48
            bufs = [torch.full((lead + body + tail,), SENTINEL, dtype=torch.int64, device="cuda:0") for _ in range(3)]
            rc = L.blsw_r1cs_evaluate(d.chk._r, d.inst.data_ptr(), d.inst.stride(0) // 6, d.w.data_ptr(), d.w.stride(0) // 6, N, form, begin, count,
                                      *(b.data_ptr() + lead * 8 for b in bufs), stream)
            assert rc == 0
            torch.cuda.synchronize()
            for m in range(3):
                assert torch.equal(bufs[m][lead:lead + body].view(N, count, 6), full[m][:, begin:begin + count]), (form, begin, count, m)
                assert bool((bufs[m][:lead] == SENTINEL).all()) and bool((bufs[m][lead + body:] == SENTINEL).all()), (form, begin, count, m)


@pytest.mark.parametrize("ni", (1, 3))
def test_first_unreduced(pkg, ni):
    """a stored p, p + 1 or 2^384 - 1 is reported at its index of z = [instance | witness], p - 1 is not: at witness 0, at the last witness and in
    the instance vector; of two the smaller index is reported, whichever was written first"""
    d = data(pkg, ni, 0)
    w, inst = d.w.clone(), d.inst.clone()
    nw = d.nw
    want = [-1] * N
    set_elem(w, 0, 0, P)
    want[0] = ni
    set_elem(w, 63, nw - 1, P + 1)
    want[63] = ni + nw - 1
    set_elem(w, 64, 0, (1 << 384) - 1)
    want[64] = ni
    set_elem(w, 129, nw - 1, P)
    want[129] = ni + nw - 1
    set_elem(w, 1, 0, P - 1)  # reduced: not reported
    set_elem(w, 2, nw - 1, P - 1)
    set_elem(w, 65, nw - 1, P)  # two in one instance, the later one written first
    set_elem(w, 65, 300, P + 1)
    want[65] = ni + 300
    set_elem(w, 3, nw, P)  # the padding is not part of z
    assert d.chk.first_unreduced(w, inst).tolist() == want
    set_elem(inst, 5, ni - 1, P)  # the last instance variable (the one itself without public inputs)
    want[5] = ni - 1
    set_elem(inst, 6, ni - 1, P - 1)
    set_elem(inst, 129, ni - 1, (1 << 384) - 1)  # instance vector and witness: the instance index is smaller
    want[129] = ni - 1
    set_elem(inst, 64, ni - 1, P + 1)
    want[64] = ni - 1
    if ni > 1:
        set_elem(inst, 7, ni, P)  # the instance padding is not part of z
    assert d.chk.first_unreduced(w, inst).tolist() == want
    assert d.chk.first_unreduced(w, inst, form=1).tolist() == want


# ------------------------------------------------------------------------------------------------------------------ the compact source
def compact_system(pkg, c, seed=5):
    """about 40 rows over the witness columns of a compact step at the borders of its regions (pkg.compact_locate): SHA bits, tile rows, pairing
    rows. The leading rows are booleanity rows (1 - b) b = 0 on SHA bits; the others mix regions and carry a slack each, alternately a tile row
    and a pairing row that no other row uses -> (system, {witness index: region})"""
    rng = random.Random(seed)
    nw, lo, bits = c.n_witness, c.off_expand, c.sha_bits
    assert lo > 0 and lo + bits < nw

    def row_of(k):
        region, off, _ = pkg.compact_locate(c, k, 0)
        assert region != pkg.COMPACT_BIT
        return (off - c.off_staging) // (64 * 48) if region == pkg.COMPACT_TILE else c.split_row + (off - c.off_pair) // 48

    # the runs of witness indices whose staged rows are consecutive: before and after the SHA segment, a moved segment cut out of the first
    cuts = sorted({0, lo, c.moved_lo, c.moved_lo + c.moved_len} if c.moved_len else {0, lo})
    runs = [(a, b - 1) for a, b in zip(cuts, cuts[1:]) if b > a] + [(lo + bits, nw - 1)]
    for a, b in runs:
        assert row_of(b) - row_of(a) == b - a

    def k_of_row(row):
        for a, b in runs:
            if row_of(a) <= row <= row_of(b):
                return a + row - row_of(a)
        raise AssertionError(row)

    sha = [lo, lo + 31, lo + 32, lo + 63, lo + 64, lo + bits // 2, lo + bits - 2, lo + bits - 1]
    staged = {lo - 1, lo + bits, nw - 1, k_of_row(0), k_of_row(c.split_row - 1), k_of_row(c.split_row), k_of_row(c.split_row + 1), k_of_row(c.staging_rows - 1)}
    for a, b in runs:
        staged |= {a, b}
    region = {k: pkg.compact_locate(c, k, 0)[0] for k in sorted(staged) + sha}
    assert all(region[k] == pkg.COMPACT_BIT for k in sha)
    assert region[k_of_row(c.split_row - 1)] == pkg.COMPACT_TILE and region[k_of_row(c.split_row)] == pkg.COMPACT_PAIR == region[k_of_row(c.staging_rows - 1)]
    assert row_of(nw - 1) < c.staging_rows
    coeffs = S.coefficients()
    cols = [1 + k for k in sorted(staged)] + [1 + k for k in sha] + [0]
    order = [("bool_%d" % j, [[(0, 1), (1 + k, P - 1)], [(1 + k, 1)], []], None) for j, k in enumerate(sha)]
    n_mixed = 32
    slacks = []
    for j in range(n_mixed):  # free rows of both staged regions, away from the borders
        k = k_of_row(7 + 3 * j) if j % 2 == 0 else k_of_row(c.split_row + 11 + 5 * j)
        assert k not in staged and k not in slacks
        slacks.append(k)
        region[k] = pkg.compact_locate(c, k, 0)[0]
        assert region[k] == (pkg.COMPACT_TILE if j % 2 == 0 else pkg.COMPACT_PAIR)

    def entries(must):
        pick = set(rng.sample(cols, rng.randint(1, 4))) | {must}
        return sorted((k, rng.choice(coeffs)) for k in pick)

    for j in range(n_mixed):  # every border column is in some row; bits and staged elements meet in one row
        a, b = cols[j % len(cols)], cols[(j + n_mixed) % len(cols)]
        order.append((None, [entries(a), entries(1 + sha[j % len(sha)]), entries(b)], coeffs[j % len(coeffs)], 1 + slacks[j]))
    sys = S.system_from_rows(order, 1, n_witness=nw)
    used = {k for row in sys["rows"] for mat in row for k, _ in mat}
    assert {1 + k for k in staged} | {1 + k for k in sha} <= used
    return sys, region


def test_compact_source(pkg):
    """z read from a step's compact wire form: a synthetic system over the columns at the borders of the compact regions, satisfied in all 128 lanes
    of an engine's step by slacks written into the buffer and into the plain vectors, then with a slack bumped in every third lane: evaluate_compact
    == evaluate(plain) == the reference for lanes 0, 63, 64 and 127, and which_is_unsatisfied_compact == which_is_unsatisfied(plain) == the
    reference's first bad row for all lanes"""
    import torch

    from tests.test_r1cs_compact_gpu import single_key_step

    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    step = single_key_step(pkg, workload, 128)
    try:
        c, comp, plain = step.lay, step.comp, step.plain
        sys, region = compact_system(pkg, c)
        chk = pkg.ConstraintChecker.from_matrices(sys, "cuda:0")
        used = sorted({k for row in sys["rows"] for mat in row for k, _ in mat} - {0})
        vals = plain[:, torch.tensor([k - 1 for k in used], device=plain.device)].cpu().numpy().view(np.uint64)  # [128, used, 6]
        one = S.encode(1, 0)
        zs = []
        for i in range(128):
            z = {k: S.to_int(vals[i, j]) for j, k in enumerate(used)}
            z[0] = one
            for k in used:
                if region[k - 1] == pkg.COMPACT_BIT:
                    assert z[k] in (0, one)
            S.solve_slacks(sys, z, 0)
            zs.append(z)
        slack_rows = [r for r, s in enumerate(sys["slack"]) if s is not None]
        limbs64 = comp.view(torch.int64)
        six = torch.arange(6, device=comp.device)

        def write_slacks():
            """the slack values of zs into the compact buffer (through the locator) and into the plain vectors"""
            offs, rows = [], []
            for r in slack_rows:
                k = sys["slack"][r] - 1
                col = S.limbs([zs[i][k + 1] for i in range(128)]).view(np.int64)
                plain[:, k] = torch.from_numpy(col).to(plain.device)
                for i in range(128):
                    reg, off, _ = pkg.compact_locate(c, k, i)
                    assert reg == region[k] and off % 8 == 0 and off + 48 <= c.total
                    offs.append(off // 8)
                rows.append(col)
            idx = torch.tensor(offs, device=comp.device)[:, None] + six[None, :]
            limbs64[idx] = torch.from_numpy(np.concatenate(rows)).to(comp.device)

        def compare(want):
            assert [S.first_unsatisfied(sys, z, 0) for z in zs] == want
            assert chk.which_is_unsatisfied_compact(c, comp).tolist() == want
            assert chk.which_is_unsatisfied(plain).tolist() == want
            a, b = chk.evaluate_compact(c, comp), chk.evaluate(plain)
            for m in range(3):
                assert torch.equal(a[m], b[m])
                host = a[m].cpu().numpy().view(np.uint64)
                for i in (0, 63, 64, 127):
                    ref = S.evaluate_ref(sys, zs[i], 0)
                    assert [S.to_int(x) for x in host[i]] == [t[m] for t in ref], (i, m)

        write_slacks()
        assert torch.equal(step.expansion(), plain)  # the buffer and the vectors still hold the same step
        compare([-1] * 128)
        want = [-1] * 128
        for i in range(0, 128, 3):  # lanes 0, 63 and 126 among them; 64 and 127 stay satisfied
            r = slack_rows[(i // 3) % len(slack_rows)]
            S.bump(sys, zs[i], r, (1, P - 1, 1 << 352)[(i // 3) % 3])
            want[i] = r
        write_slacks()
        compare(want)
    finally:
        step.close()
