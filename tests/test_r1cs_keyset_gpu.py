"""The compact checker of shared-keys steps (ABI 16) on the MI355X: a step of a shared-keys engine validated straight from its compact buffer plus the
receiver's KeySet (every row, or only the rows behind the head rows), and the committee validated once per set (check_keyset).

References are never the new code: ConstraintChecker.which_is_unsatisfied / evaluate on expand_compact(.., keyset=) — the route the receiver had
before — and hostsim_lib.r1cs_check on the full matrices and on the matrices sliced to the rows from P on with numpy. K = 5, committee "A" of
tests/test_keyset_gpu.py with its identity key; n = 128 (two tiles; P = 9 695 falls inside a row block), and one n = 64 step each at K = 1 and at
mask 14 (13 instance variables). Corruptions change data only, never a pointer, a size or a stride."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import hostsim_lib
from tests import test_keyset_gpu as KS
from tests import test_r1cs_compact_gpu as C
from tests.oracle_lib import P_MOD

pytestmark = pytest.mark.gpu
K, SEG, HEAD_ROWS = 5, 1942, 1939
P5 = K * HEAD_ROWS  # the head rows of five keys
_MATS = {}


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def mats(pkg, n_keys, mask=0):
    if (n_keys, mask) not in _MATS:
        P = pkg.matrices(32, n_keys=n_keys, agg_inputs=mask)
        _MATS[n_keys, mask] = (P, pkg.ConstraintChecker.from_matrices(P, "cuda:0"))
    return _MATS[n_keys, mask]


def sliced(P, first):
    """the matrices with rows [first, n_constraints) only: the system a skip_head_rows check evaluates, for the host reference"""
    out = {"n_constraints": P["n_constraints"] - first, "n_instance_vars": P["n_instance_vars"], "n_witness": P["n_witness"]}
    for name in "ABC":
        rp, col, val = P[name]
        lo = int(rp[first])
        out[name] = (np.ascontiguousarray(rp[first:] - rp[first]), np.ascontiguousarray(col[lo:]), np.ascontiguousarray(val[lo:]))
    return out


class KeysetStep:
    """one step of n instances over one committee, produced by the same shared-keys engine as a compact buffer and as plain vectors (the way Step of
    tests/test_r1cs_compact_gpu.py does it); bitmaps vary per instance, every sixth instance has a tampered message"""

    def __init__(self, pkg, torch, oracle, n, k=K, mask=0):
        self.dev = torch.device("cuda:0")
        self.n, self.k, self.head_len = n, k, k * SEG
        name = "A" if k == K else "B"
        self.ks = pkg.KeySet(KS.to_dev(torch, KS.set_keys(oracle, name, k)))
        start, ident = KS.SETS[name]
        cases = []
        for i in range(6):  # six distinct instances, repeated
            bm = [(i >> b) & 1 for b in range(k)]
            bm[i % k] = 1
            bm[0] = 1
            signed = [b if (j != ident or k != K) else 0 for j, b in enumerate(bm)]
            _, _, msg, sig, _ = KS.synth.make_aggregate(oracle, k, signed, start=start, tamper=(i == 4))
            cases.append((np.array(bm, dtype=np.uint8), msg, sig))
        self.expect = [int(i % 6 != 4) for i in range(n)]
        bm, msg, sig = (KS.to_dev(torch, np.stack([cases[i % 6][j] for i in range(n)])) for j in range(3))
        self.eng = pkg.WitnessEngine(n, 32, max_steps=2, device=self.dev, n_buffers=2, n_keys=k, shared_keys=1, agg_inputs=mask)
        self.lay = self.eng.compact_layout()
        lay2, head_len = pkg.compact_layout_keyset(n, 32, n_keys=k, shared_keys=1, agg_inputs=mask)
        assert bytes(self.lay) == bytes(lay2) and head_len == self.head_len
        assert self.lay.total == self.eng.compact_bytes() and self.lay.n == n and self.lay.n_witness + self.head_len == self.eng.n_witness
        self.comp = self.eng.new_compact_buffer(1)[0]
        self.plain = self.eng.new_witness_tensor()
        self.inst = self.eng.new_instance_tensor() if self.eng.n_instance_vars > 1 else None
        r = [torch.empty(n, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self.eng.submit_aggregate_keyset_compact(self.ks, bm, sig, msg, self.comp, result=r[0])
        self.eng.submit_aggregate_keyset(self.ks, bm, sig, msg, witness=self.plain, result=r[1], instance=self.inst)
        self.eng.flush()
        torch.cuda.synchronize()
        assert r[0].tolist() == r[1].tolist() == self.expect
        self.torch = torch

    def expansion(self, comp=None, ks=None):
        """the receiver's route before this checker: blsw_engine_expand_compact_keyset of (a possibly corrupted copy of) the buffer with the set"""
        out = self.eng.new_witness_tensor()
        self.eng.expand_compact(self.comp if comp is None else comp, out, keyset=ks or self.ks)
        self.torch.cuda.synchronize()
        return out

    def close(self):
        self.eng.close()
        self.ks.close()


@pytest.fixture(scope="module")
def step(pkg, torch, oracle):
    s = KeysetStep(pkg, torch, oracle, 128)
    yield s
    s.close()


def both(chk, s, comp=None, ks=None):
    """(CHECK, SKIP) of the step from its compact buffer"""
    comp = s.comp if comp is None else comp
    kw = dict(instance=s.inst, keyset=ks or s.ks)
    return chk.which_is_unsatisfied_compact(s.lay, comp, **kw).tolist(), chk.which_is_unsatisfied_compact(s.lay, comp, skip_head_rows=True, **kw).tolist()


def test_clean_step(pkg, torch, oracle, step):
    """CHECK and SKIP are [-1] * n, as the full-vector check of the expansion; the committee is satisfied in both element forms; nothing unreduced"""
    P, chk = mats(pkg, K)
    assert chk.head_rows(K) == P5 and chk.head_rows(0) == 0 and chk.head_rows(2) == 2 * HEAD_ROWS
    w = step.expansion()
    assert torch.equal(w, step.plain)
    check, skip = both(chk, step)
    assert check == skip == [-1] * 128 == chk.which_is_unsatisfied(w).tolist()
    assert bool(chk.is_satisfied_compact(step.lay, step.comp, keyset=step.ks).all())
    assert bool(chk.is_satisfied_compact(step.lay, step.comp, keyset=step.ks, skip_head_rows=True).all())
    assert chk.first_unreduced_compact(step.lay, step.comp, keyset=step.ks).tolist() == [-1] * 128
    assert chk.check_keyset(step.ks) == (-1, -1)
    canon = pkg.KeySet(KS.to_dev(torch, KS.set_keys(oracle, "A")), output_form=1)
    assert chk.check_keyset(canon) == (-1, -1)
    canon.close()


def test_corrupted_buffer_fails_at_the_host_checks_row(pkg, step):
    """the corruptions of tests/test_r1cs_compact_gpu.py, in both tiles, with the caller's witness index k located at k - head_len in the buffer: a
    flipped SHA bit, a tile-row element of the map segment + 1, a pairing row + 1, the last element + 1. All of them lie behind the head, so the
    rows they break are behind P: CHECK == SKIP == the host's row == the full-vector check of the corrupted buffer's expansion"""
    P, chk = mats(pkg, K)
    L, c, h = pkg.layout_aggregate(32, K), step.lay, step.head_len
    comp = step.comp.clone()
    where = {3: L["off_expand"] + 1000, 40: L["off_map0"] + 50, 77: L["off_miller"] + 123, 127: L["n_witness"] - 1}
    C.flip_bit(pkg, c, comp, where[3] - h, 3)
    assert C.add_one(pkg, c, comp, where[40] - h, 40) == pkg.COMPACT_TILE
    assert C.add_one(pkg, c, comp, where[77] - h, 77) == pkg.COMPACT_PAIR
    assert C.add_one(pkg, c, comp, where[127] - h, 127) == pkg.COMPACT_PAIR
    w = step.expansion(comp)
    assert (w != step.plain).any(dim=2).nonzero().tolist() == [[i, k] for i, k in sorted(where.items())]
    expect = {i: C.host_row(P, w, i) for i in where}
    print("host rows:", expect)
    assert sum(e >= P5 for e in expect.values()) >= 3, expect
    want = [expect.get(i, -1) for i in range(128)]
    check, skip = both(chk, step, comp)
    assert check == want and skip == want
    assert chk.which_is_unsatisfied(w).tolist() == want
    # an unreduced staged element is reported at n_instance_vars + head_len + k of the buffer, i.e. at 1 + its index in the caller's vector
    C.set_elem(comp, pkg.compact_locate(c, where[40] - h, 40)[1], P_MOD + 1)
    assert chk.first_unreduced_compact(c, comp, keyset=step.ks).tolist() == [1 + where[40] if i == 40 else -1 for i in range(128)]
    assert chk.first_unreduced(step.expansion(comp)).tolist() == [1 + where[40] if i == 40 else -1 for i in range(128)]


def _with_table_element(step, torch, at, value):
    """context: ks.table[at] = value (data only), restored afterwards"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        torch.cuda.synchronize()
        saved = step.ks.table[at].clone()
        step.ks.table[at] = torch.from_numpy(C.to_limbs(value).view(np.int64)).to(step.dev)
        torch.cuda.synchronize()
        try:
            yield
        finally:
            step.ks.table[at] = saved
            torch.cuda.synchronize()

    return cm()


def test_corrupted_table_inside_a_keys_block(pkg, torch, step):
    """element 3 * 1942 + 1000 of the table + 1 — not one of the six elements later rows read: the committee check finds it in key 3's rows, at
    the host's row; CHECK finds that row for every instance; SKIP sees nothing"""
    P, chk = mats(pkg, K)
    at = 3 * SEG + 1000
    v = (C.to_int(step.ks.table[at].cpu().numpy().view(np.uint64)) + 1) % P_MOD
    with _with_table_element(step, torch, at, v):
        row, unreduced = chk.check_keyset(step.ks)
        w = step.expansion()
        assert (w != step.plain).any(dim=2).nonzero().tolist() == [[i, at] for i in range(128)]
        host = C.host_row(P, w, 0)
        print("committee row:", row, "host row:", host)
        assert 3 * HEAD_ROWS <= row < 4 * HEAD_ROWS and row == host and unreduced == -1
        check, skip = both(chk, step)
        assert check == [row] * 128 == chk.which_is_unsatisfied(w).tolist()
        assert skip == [-1] * 128
    assert chk.check_keyset(step.ks) == (-1, -1)


def test_corrupted_table_element_that_later_rows_read(pkg, torch, step):
    """element 1 * 1942 + 1938 of the table + 1: one of the six elements of key 1's block that rows behind the head read (the allocated point, which the
    aggregation adds when the bitmap selects the key). Of the instances 0, 5, 64 and 127 only 127 selects key 1 (bitmaps repeat with i % 6; 127 % 6 = 1
    is [1, 1, 0, 0, 0]): the host reference on the system sliced to the rows from P on reports a row >= P for it and -1 for the other three — chosen
    with that reference alone, on the CPU. SKIP equals it for those four and for every instance with the same inputs (i % 6 in 0, 1, 4, 5); the
    other two bitmaps select key 1 and fail behind the head as well. CHECK is the full-vector check's row, a head row of key 1 for every instance"""
    P, chk = mats(pkg, K)
    tail = sliced(P, P5)
    at = 1 * SEG + 1938
    v = (C.to_int(step.ks.table[at].cpu().numpy().view(np.uint64)) + 1) % P_MOD
    with _with_table_element(step, torch, at, v):
        w = step.expansion()
        check, skip = both(chk, step)
        full = chk.which_is_unsatisfied(w).tolist()
        host_tail = {}
        for i in (0, 5, 64, 127):
            r = hostsim_lib.r1cs_check(tail, w[i].cpu().numpy().view(np.uint64))
            host_tail[i] = r + P5 if r >= 0 else -1
        print("host rows behind the head:", host_tail, "full-vector rows:", {i: full[i] for i in host_tail})
        assert host_tail[127] >= P5 and [host_tail[i] for i in (0, 5, 64)] == [-1] * 3, host_tail
        by_class = {i % 6: r for i, r in host_tail.items()}
        assert sorted(by_class) == [0, 1, 4, 5]
        assert all(skip[i] == by_class[i % 6] if i % 6 in by_class else skip[i] >= P5 for i in range(128)), skip
        assert check == full and full[0] == C.host_row(P, w, 0) and HEAD_ROWS <= full[0] < 2 * HEAD_ROWS


def test_unreduced_table_element(pkg, torch, step):
    """a table element set to p + 1: check_keyset reports index n_instance_vars + k of z; the step's own unreduced pass never covers the head"""
    _, chk = mats(pkg, K)
    at = 2 * SEG + 77
    with _with_table_element(step, torch, at, P_MOD + 1):
        assert chk.check_keyset(step.ks)[1] == 1 + at
        assert chk.first_unreduced_compact(step.lay, step.comp, keyset=step.ks).tolist() == [-1] * 128
    with _with_table_element(step, torch, 5 * SEG - 1, P_MOD):  # the last element, with an earlier one: the first is reported
        with _with_table_element(step, torch, at, P_MOD + 1):
            assert chk.check_keyset(step.ks)[1] == 1 + at
        assert chk.check_keyset(step.ks)[1] == 5 * SEG


def test_evaluate_compact_equals_evaluate_bit_for_bit(pkg, torch, step):
    """A z, B z, C z over a window straddling P, the last 5 000 rows and a window of key 0's rows"""
    P, chk = mats(pkg, K)
    nc = P["n_constraints"]
    for begin, count in ((P5 - 50, 100), (nc - 5000, 5000), (100, 300)):
        a = chk.evaluate_compact(step.lay, step.comp, rows=(begin, count), keyset=step.ks)
        b = chk.evaluate(step.plain, rows=(begin, count))
        assert a[0].shape == (128, count, 6)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (begin, count)
        assert bool((a[0] != 0).any()) and bool((a[2] != 0).any())


@pytest.mark.parametrize("shape", ["one_key", "mask_14"])
def test_other_shapes(pkg, torch, oracle, shape):
    """n = 64 at K = 1 (P = 1 939, head_len 1 942) and at K = 5 with mask 14 (13 instance variables, the instance tensor passed): clean, then one
    corruption behind the head and one in the table"""
    k, mask = (1, 0) if shape == "one_key" else (K, 14)
    s = KeysetStep(pkg, torch, oracle, 64, k=k, mask=mask)
    P, chk = mats(pkg, k, mask)
    p_rows = k * HEAD_ROWS
    assert chk.head_rows(k) == p_rows and chk.n_instance_vars == (13 if mask else 1) and (s.inst is not None) == bool(mask)
    assert torch.equal(s.expansion(), s.plain)
    check, skip = both(chk, s)
    assert check == skip == [-1] * 64 == chk.which_is_unsatisfied(s.plain, s.inst).tolist()
    assert chk.check_keyset(s.ks) == (-1, -1)
    assert chk.first_unreduced_compact(s.lay, s.comp, instance=s.inst, keyset=s.ks).tolist() == [-1] * 64
    if mask:
        with pytest.raises(pkg.BlswError):
            chk.which_is_unsatisfied_compact(s.lay, s.comp, keyset=s.ks)  # instance required
    comp = s.comp.clone()
    at = pkg.layout_aggregate(32, k, mask)["off_agg"] + 5
    C.add_one(pkg, s.lay, comp, at - s.head_len, 37)
    w = s.expansion(comp)
    expect = C.host_row(P, w, 37, s.inst)
    assert expect >= p_rows
    want = [expect if j == 37 else -1 for j in range(64)]
    check, skip = both(chk, s, comp)
    assert check == skip == want == chk.which_is_unsatisfied(w, s.inst).tolist()
    at = (k - 1) * SEG + 1000
    s.torch.cuda.synchronize()
    saved = s.ks.table[at].clone()
    s.ks.table[at, 0] ^= 1
    row, _ = chk.check_keyset(s.ks)
    w = s.expansion()
    check, skip = both(chk, s)
    s.ks.table[at] = saved
    assert (k - 1) * HEAD_ROWS <= row < p_rows and row == C.host_row(P, w, 0, s.inst)
    assert check == [row] * 64 == chk.which_is_unsatisfied(w, s.inst).tolist() and skip == [-1] * 64
    s.close()


def test_refusals_that_need_a_device(pkg, torch, oracle, step):
    """a canonical-form set for the compact calls, a set of 3 keys, a layout of another K, a mode of 2: BLSW_ERR_ARG, the sentinel-filled outputs stay"""
    L = pkg.lib()
    _, chk = mats(pkg, K)
    c, comp, dev = step.lay, step.comp, step.dev
    canon = pkg.KeySet(KS.to_dev(torch, KS.set_keys(oracle, "A")), output_form=1)
    small = pkg.KeySet(KS.to_dev(torch, KS.set_keys(oracle, "A")[:3]))
    other, _ = pkg.compact_layout_keyset(128, 32, n_keys=3, shared_keys=1)
    assert other.n_witness != c.n_witness and other.total <= c.total
    out = torch.full((128,), 7, dtype=torch.int64, device=dev)
    az = torch.full((128, 4, 6), 7, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def check(ks, lay=c, mode=0, r=chk._r):
        return L.blsw_r1cs_check_compact_keyset(r, ctypes.byref(lay), comp.data_ptr(), ks._ks if ks else None, mode, None, 0, out.data_ptr(), out.data_ptr(), s)

    def evaluate(ks, lay=c, begin=0, count=4):
        return L.blsw_r1cs_evaluate_compact_keyset(chk._r, ctypes.byref(lay), comp.data_ptr(), ks._ks if ks else None, None, 0, begin, count, az.data_ptr(), az.data_ptr(),
                                                   az.data_ptr(), s)

    for mode in (0, 1):
        assert check(canon, mode=mode) == 1 and check(small, mode=mode) == 1 and check(step.ks, lay=other, mode=mode) == 1 and check(None, mode=mode) == 1
    assert check(small, lay=other) == 1  # the set and the layout agree with each other, not with the handle
    assert check(step.ks, mode=2) == 1 and check(step.ks, mode=1 << 31) == 1
    assert evaluate(canon) == 1 and evaluate(small) == 1 and evaluate(step.ks, lay=other) == 1 and evaluate(None) == 1
    assert evaluate(step.ks, begin=chk.n_constraints - 2) == 1 and evaluate(step.ks, count=0) == 1
    bad = pkg.blsw_compact_layout_t.from_buffer_copy(c)
    bad.n = 100
    assert check(step.ks, lay=bad) == 1 and evaluate(step.ks, lay=bad) == 1
    assert L.blsw_r1cs_check_keyset(chk._r, step.ks._ks, None, None, s) == 1 and L.blsw_r1cs_check_keyset(chk._r, None, out.data_ptr(), None, s) == 1
    with pytest.raises(pkg.BlswError):
        chk.which_is_unsatisfied_compact(c, comp, skip_head_rows=True)  # nothing to skip without a set
    if torch.cuda.device_count() > 1:
        far = pkg.KeySet(KS.to_dev(torch, KS.set_keys(oracle, "A")).to("cuda:1"))
        assert check(far) == 1 and evaluate(far) == 1 and L.blsw_r1cs_check_keyset(chk._r, far._ks, out.data_ptr(), None, s) == 1
        far.close()
    torch.cuda.synchronize()
    assert out.tolist() == [7] * 128 and bool((az == 7).all())
    bz, cz = az.clone(), az.clone()  # every rule kept: it runs
    assert L.blsw_r1cs_evaluate_compact_keyset(chk._r, ctypes.byref(c), comp.data_ptr(), step.ks._ks, None, 0, 0, 4, az.data_ptr(), bz.data_ptr(), cz.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert not bool((az == 7).all())
    for h in (canon, small):
        h.close()
