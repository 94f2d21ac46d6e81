"""The compact checker (blsw_r1cs_check_compact / _evaluate_compact, ABI 14) on the MI355X: a step is validated straight from its compact wire
form. The locator reproduces every element of the expanded vectors; satisfied steps are satisfied; data corrupted IN THE COMPACT BUFFER (a SHA
bit, a tile row, a pairing row, the last element) fails at the row the host check finds in that buffer's expansion, which is also the row the
full-vector device check finds; unreduced staged elements are reported; every shape a compact step exists for; A z, B z, C z equal the
full-vector evaluation bit for bit; the argument rules. The corruptions change data only, never a pointer, a size or a stride."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import hostsim_lib, synth
from tests.oracle_lib import P_MOD

pytestmark = pytest.mark.gpu
ONE = (1 << 384) % P_MOD  # the Montgomery form of 1: what a set bit stands for
_MATS = {}


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def workload():
    return importlib.import_module("bls-verify-gadget_amd.workload")


def mats(pkg, **shape):
    key = tuple(sorted(shape.items()))
    if key not in _MATS:
        P = pkg.matrices(32, **shape)
        _MATS[key] = (P, pkg.ConstraintChecker.from_matrices(P, "cuda:0"))
    return _MATS[key]


def to_int(limbs):
    return sum(int(x) << (64 * k) for k, x in enumerate(np.asarray(limbs, dtype=np.uint64)))


def to_limbs(v):
    return np.array([(v >> (64 * k)) & ((1 << 64) - 1) for k in range(6)], dtype=np.uint64)


def elem_view(comp, off):
    """the six int64 limbs of the element at byte offset off of a uint8 cuda buffer (a view: assignments go to the buffer)"""
    import torch

    assert off % 8 == 0
    return comp.view(torch.int64)[off // 8:off // 8 + 6]


def get_elem(comp, off):
    return to_int(elem_view(comp, off).cpu().numpy().view(np.uint64))


def set_elem(comp, off, v):
    import torch

    elem_view(comp, off).copy_(torch.from_numpy(to_limbs(v).view(np.int64)))


def add_one(pkg, c, comp, k, lane):
    """witness k of instance `lane` += 1 (mod p) in the compact buffer: a staged element"""
    region, off, _ = pkg.compact_locate(c, k, lane)
    assert region != pkg.COMPACT_BIT
    set_elem(comp, off, (get_elem(comp, off) + 1) % P_MOD)
    return region


def flip_bit(pkg, c, comp, k, lane):
    import torch

    region, off, bit = pkg.compact_locate(c, k, lane)
    assert region == pkg.COMPACT_BIT
    word = comp.view(torch.int32)[off // 4:off // 4 + 1]
    word ^= (1 << bit) if bit < 31 else -(1 << 31)


class Step:
    """one step of n instances, produced both as a compact buffer and as plain vectors by the same staged engine"""

    def __init__(self, pkg, n, submit, **options):
        import torch

        self.dev = torch.device("cuda:0")
        self.eng = pkg.WitnessEngine(n, 32, max_steps=2, device=self.dev, n_buffers=2, **options)
        self.lay = self.eng.compact_layout()
        assert self.lay.total == self.eng.compact_bytes() and self.lay.n == n and self.lay.n_witness == self.eng.n_witness
        self.comp = self.eng.new_compact_buffer(1)[0]
        self.plain = self.eng.new_witness_tensor()
        self.inst = self.eng.new_instance_tensor() if self.eng.n_instance_vars > 1 else None
        self.result = [torch.empty(n, dtype=torch.int32, device=self.dev) for _ in range(2)]
        submit(self)
        self.eng.flush()
        torch.cuda.synchronize()
        assert torch.equal(self.result[0], self.result[1])

    def expansion(self, comp=None):
        """the receiver's route: blsw_engine_expand_compact of (a possibly corrupted copy of) the buffer"""
        import torch

        out = self.eng.new_witness_tensor()
        self.eng.expand_compact(self.comp if comp is None else comp, out)
        torch.cuda.synchronize()
        return out

    def close(self):
        self.eng.close()


def single_key_step(pkg, workload, n, **options):
    import torch

    pk, msg, sig, expect = workload.make_batch(pkg, n, device=torch.device("cuda:0"))

    def submit(s):
        s.eng.submit_compact(pk, sig, msg, s.comp, result=s.result[0])
        s.eng.submit(pk, sig, msg, witness=s.plain, result=s.result[1], instance=s.inst)

    s = Step(pkg, n, submit, **options)
    assert np.array_equal(s.result[0].cpu().numpy().astype(bool), expect) and not expect.all()  # every 16th is a valid assignment whose Boolean is false
    return s


@pytest.fixture(scope="module")
def step(pkg, workload):
    s = single_key_step(pkg, workload, 128)
    yield s
    s.close()


def host_row(P, w, i, inst=None):
    hw = w[i].cpu().numpy().view(np.uint64)
    return hostsim_lib.r1cs_check(P, hw, inst[i].cpu().numpy().view(np.uint64)) if inst is not None else hostsim_lib.r1cs_check(P, hw)


def test_locator_reproduces_every_element_of_the_plain_vectors(pkg, step):
    """the compact buffer gathered through the locator table, in torch on the device == the plain vector of every one of the 128 instances. The
    table is blsw_compact_locate at lanes 0, 1 and 64 (offsets are affine in lane & 63 and lane >> 6: checked on ALL indices at lanes 63 and 127)"""
    import torch

    c, dev = step.lay, step.dev
    region, off0, bit = pkg.compact_locate_all(c, 0)
    d1 = pkg.compact_locate_all(c, 1)[1] - off0
    d64 = pkg.compact_locate_all(c, 64)[1] - off0
    for lane in (63, 127):
        r, o, b = pkg.compact_locate_all(c, lane)
        assert np.array_equal(r, region) and np.array_equal(b, bit) and np.array_equal(o, off0 + (lane & 63) * d1 + (lane >> 6) * d64)
    is_bit = torch.from_numpy(region == pkg.COMPACT_BIT).to(dev)
    off0_t, d1_t, d64_t = (torch.from_numpy(a).to(dev) for a in (off0, d1, d64))
    shift = torch.from_numpy(bit.astype(np.int32)).to(dev)[is_bit]
    one = torch.from_numpy(to_limbs(ONE).view(np.int64)).to(dev)
    words, limbs = step.comp.view(torch.int32), step.comp.view(torch.int64)
    six = torch.arange(6, device=dev)
    for i in range(128):
        off = off0_t + (i & 63) * d1_t + (i >> 6) * d64_t
        z = torch.empty((c.n_witness, 6), dtype=torch.int64, device=dev)
        z[is_bit] = ((words[off[is_bit] // 4] >> shift) & 1).to(torch.int64)[:, None] * one[None, :]
        z[~is_bit] = limbs[(off[~is_bit] // 8)[:, None] + six[None, :]]
        assert torch.equal(z, step.plain[i]), i
    assert torch.equal(step.expansion(), step.plain)


def test_satisfied(pkg, step):
    """128 instances, every 16th tampered (a valid assignment whose Boolean is false): all satisfied, as the full-vector check says"""
    _, chk = mats(pkg)
    got = chk.which_is_unsatisfied_compact(step.lay, step.comp).tolist()
    assert got == [-1] * 128 == chk.which_is_unsatisfied(step.plain).tolist()
    assert bool(chk.is_satisfied_compact(step.lay, step.comp).all())
    assert chk.first_unreduced_compact(step.lay, step.comp).tolist() == [-1] * 128


def test_corrupted_buffer_fails_at_the_host_checks_row(pkg, step):
    """four instances corrupted in the compact buffer, two of them in the second tile: a flipped SHA bit, a tile-row element of the map segment + 1,
    a pairing row + 1, the last element + 1 (indices for which the host check alone finds a bad row: checked on the CPU when they were chosen)"""
    P, chk = mats(pkg)
    L, c = pkg.layout(32), step.lay
    comp = step.comp.clone()
    where = {3: L["off_expand"] + 1000, 40: L["off_map0"] + 50, 77: L["off_miller"] + 123, 127: c.n_witness - 1}
    flip_bit(pkg, c, comp, where[3], 3)
    assert add_one(pkg, c, comp, where[40], 40) == pkg.COMPACT_TILE
    assert add_one(pkg, c, comp, where[77], 77) == pkg.COMPACT_PAIR
    assert add_one(pkg, c, comp, where[127], 127) == pkg.COMPACT_PAIR
    w = step.expansion(comp)
    changed = (w != step.plain).any(dim=2).nonzero().tolist()
    assert changed == [[i, k] for i, k in sorted(where.items())]  # the corruption is those four elements of the expansion and nothing else
    expect = {i: host_row(P, w, i) for i in where}
    print("host rows:", expect)
    assert sum(e >= 0 for e in expect.values()) >= 3, expect
    want = [expect.get(i, -1) for i in range(128)]
    assert chk.which_is_unsatisfied_compact(c, comp).tolist() == want
    assert chk.which_is_unsatisfied(w).tolist() == want
    assert chk.is_satisfied_compact(c, comp).tolist() == [x < 0 for x in want]


def test_unreduced_staged_element(pkg, step):
    """a staged element set to p + 1 is reported at 1 + k for its instance only (a tile row in the second tile, then a pairing row as well)"""
    _, chk = mats(pkg)
    L, c = pkg.layout(32), step.lay
    comp = step.comp.clone()
    k = L["off_map0"] + 7
    region, off, _ = pkg.compact_locate(c, k, 70)
    assert region == pkg.COMPACT_TILE
    set_elem(comp, off, P_MOD + 1)
    assert chk.first_unreduced_compact(c, comp).tolist() == [1 + k if i == 70 else -1 for i in range(128)]
    k2 = L["off_final_exp"] + 11
    region, off, _ = pkg.compact_locate(c, k2, 5)
    assert region == pkg.COMPACT_PAIR
    set_elem(comp, off, P_MOD + 1)
    set_elem(comp, pkg.compact_locate(c, c.n_witness - 1, 5)[1], P_MOD)  # a later one of the same instance: the first is reported
    assert chk.first_unreduced_compact(c, comp).tolist() == [1 + k if i == 70 else (1 + k2 if i == 5 else -1) for i in range(128)]


def _satisfied_then_one_corruption(pkg, s, P, chk, i, k):
    """the step is satisfied from its compact buffer and from its plain vectors; witness k of instance i + 1 in the buffer is found at the host's row"""
    n = int(s.lay.n)
    assert chk.which_is_unsatisfied_compact(s.lay, s.comp, s.inst).tolist() == [-1] * n == chk.which_is_unsatisfied(s.plain, s.inst).tolist()
    assert chk.first_unreduced_compact(s.lay, s.comp, s.inst).tolist() == [-1] * n
    comp = s.comp.clone()
    add_one(pkg, s.lay, comp, k, i)
    w = s.expansion(comp)
    expect = host_row(P, w, i, s.inst)
    assert expect >= 0
    want = [expect if j == i else -1 for j in range(n)]
    assert chk.which_is_unsatisfied_compact(s.lay, comp, s.inst).tolist() == want == chk.which_is_unsatisfied(w, s.inst).tolist()


def test_every_shape(pkg, workload, oracle):
    """aggregate_verify with 2 keys (all-Witness and all-Input), Witness parameters, and pk / sig / msg Input with the instance tensor of a
    submit_io run of the same inputs: satisfied, one corruption each, and a corrupted public input found at the host check's row"""
    import torch

    dev = torch.device("cuda:0")
    n = 64
    # four distinct aggregate instances (one tampered: false, still satisfied), sixteen times each
    cases = [synth.make_aggregate(oracle, 2, bm, start=10 * j, tamper=(j == 3)) for j, bm in enumerate(([1, 0], [0, 1], [1, 1], [1, 1]))]
    cases = [cases[i % 4] for i in range(n)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
    pks, bm, msg, sig = (t(np.stack([cs[j] for cs in cases])) for j in range(4))
    for mask in (0, 15):

        def submit(s):
            s.eng.submit_aggregate_compact(pks, bm, sig, msg, s.comp, result=s.result[0])
            s.eng.submit_aggregate(pks, bm, sig, msg, witness=s.plain, result=s.result[1], instance=s.inst)

        s = Step(pkg, n, submit, n_keys=2, agg_inputs=mask)
        assert s.result[0].tolist() == [int(cs[4]) for cs in cases]
        assert (s.inst is not None) == (mask == 15) and torch.equal(s.expansion(), s.plain)
        P, chk = mats(pkg, n_keys=2, agg_inputs=mask)
        _satisfied_then_one_corruption(pkg, s, P, chk, 37, pkg.layout_aggregate(32, 2, mask)["off_agg"] + 5)
        s.close()
    # Witness parameters
    s = single_key_step(pkg, workload, n, params_mode=1)
    P, chk = mats(pkg, params_mode=1)
    _satisfied_then_one_corruption(pkg, s, P, chk, 2, pkg.layout(32, params_mode=1)["off_params_alloc"] + 3)
    s.close()
    # pk / sig / msg Input: z = [instance | witness], the compact form carries the witnesses only
    s = single_key_step(pkg, workload, n, pk_mode=1, sig_mode=1, msg_mode=1)
    P, chk = mats(pkg, pk_mode=1, sig_mode=1, msg_mode=1)
    assert chk.n_instance_vars == 1 + 1 + 3 + 6 == s.inst.shape[1]
    with pytest.raises(pkg.BlswError):
        chk.which_is_unsatisfied_compact(s.lay, s.comp)  # instance required
    _satisfied_then_one_corruption(pkg, s, P, chk, 9, pkg.layout(32, pk_mode=1, sig_mode=1, msg_mode=1)["off_msg"] + 5)
    # a corrupted public input (the key's x) with the buffer as it is
    inst = s.inst.clone()
    v = (to_int(inst[20, 2].cpu().numpy().view(np.uint64)) + 1) % P_MOD
    inst[20, 2] = torch.from_numpy(to_limbs(v).view(np.int64)).to(dev)
    expect = hostsim_lib.r1cs_check(P, s.plain[20].cpu().numpy().view(np.uint64), inst[20].cpu().numpy().view(np.uint64))
    assert expect >= 0
    assert chk.which_is_unsatisfied_compact(s.lay, s.comp, inst).tolist() == [expect if j == 20 else -1 for j in range(n)]
    inst[21, 3] = torch.from_numpy(to_limbs(P_MOD + 1).view(np.int64)).to(dev)
    assert chk.first_unreduced_compact(s.lay, s.comp, inst).tolist() == [3 if j == 21 else -1 for j in range(n)]
    s.close()


def test_evaluate_compact_equals_evaluate_bit_for_bit(pkg, step):
    """A z, B z, C z over 20 000 rows at the pairing tail (general coefficients, pairing rows) and over a window inside the SHA segment (bits)"""
    import torch

    P, chk = mats(pkg)
    nc = P["n_constraints"]
    for begin, count in ((nc - 20000 - 7, 20000), (200000, 5000)):
        a = chk.evaluate_compact(step.lay, step.comp, rows=(begin, count))
        b = chk.evaluate(step.plain, rows=(begin, count))
        assert a[0].shape == (128, count, 6)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (begin, count)
        assert bool((a[0] != 0).any()) and bool((a[2] != 0).any())


def test_argument_rules_before_any_launch(pkg, step):
    """every rule of blsw_r1cs_check_compact / _evaluate_compact returns BLSW_ERR_ARG and the sentinel-filled outputs stay as they were"""
    import torch

    L = pkg.lib()
    P, chk = mats(pkg)
    _, chki = mats(pkg, pk_mode=1, sig_mode=0)
    c, comp, dev = step.lay, step.comp, step.dev
    ci = pkg.compact_layout(128, 32, pk_mode=1)
    assert ci.n_witness == chki.n_witness != c.n_witness and ci.total <= c.total
    out = torch.full((128,), 7, dtype=torch.int64, device=dev)
    az = torch.full((128, 4, 6), 7, dtype=torch.int64, device=dev)
    inst = torch.zeros((128, 4, 6), dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    nc = P["n_constraints"]
    cp = comp.data_ptr()

    def check(r, lay, buf, ip=None, ist=0, bad=out.data_ptr()):
        return L.blsw_r1cs_check_compact(r, ctypes.byref(lay) if lay is not None else None, buf, ip, ist, bad, out.data_ptr(), s)

    def evaluate(begin, count, r=chk._r, lay=c, buf=cp, z=az.data_ptr()):
        return L.blsw_r1cs_evaluate_compact(r, ctypes.byref(lay), buf, None, 0, begin, count, z, az.data_ptr(), az.data_ptr(), s)

    def changed(**kw):
        bad = pkg.blsw_compact_layout_t.from_buffer_copy(c)
        for k, v in kw.items():
            setattr(bad, k, v)
        return bad

    assert check(None, c, cp) == 1 and check(chk._r, None, cp) == 1 and check(chk._r, c, None) == 1 and check(chk._r, c, cp, bad=None) == 1
    assert check(chk._r, ci, cp, inst.data_ptr(), 4) == 1 and check(chki._r, c, cp, inst.data_ptr(), 4) == 1  # n_witness of another circuit
    assert check(chk._r, changed(n=100), cp) == 1 and check(chk._r, changed(n=0), cp) == 1
    assert check(chk._r, changed(total=c.total - 256), cp) == 1  # rows beyond the stated size
    assert check(chki._r, ci, cp) == 1  # n_instance_vars = 4: instance required
    assert check(chki._r, ci, cp, inst.data_ptr(), 3) == 1  # instance stride below n_instance_vars
    assert check(chk._r, c, cp, inst.data_ptr(), 0) == 1
    assert evaluate(nc, 1) == 1 and evaluate(nc - 2, 4) == 1 and evaluate(0, 0) == 1
    assert evaluate(0, 4, r=None) == 1 and evaluate(0, 4, buf=None) == 1 and evaluate(0, 4, z=None) == 1 and evaluate(0, 4, lay=changed(n=100)) == 1
    torch.cuda.synchronize()
    assert out.tolist() == [7] * 128 and bool((az == 7).all())
    bz, cz = az.clone(), az.clone()
    assert L.blsw_r1cs_evaluate_compact(chk._r, ctypes.byref(c), cp, None, 0, 0, 4, az.data_ptr(), bz.data_ptr(), cz.data_ptr(), s) == 0  # every rule kept: it runs
    torch.cuda.synchronize()
    assert not bool((az == 7).all())


def test_bench_shape_step_all_satisfied(pkg, workload):
    """the engine's bench shape (1 024 instances through the grouped engine) validated from its compact step: 2.6 GB read, no 34.8 GB tensor"""
    import torch

    dev = torch.device("cuda:0")
    n = 1024
    pk, msg, sig, expect = workload.make_batch(pkg, n, device=dev)
    eng = pkg.WitnessEngine(n, 32, max_steps=16, device=dev, n_buffers=3)
    comp = eng.new_compact_buffer(1)[0]
    r = torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_compact(pk, sig, msg, comp, result=r)
    eng.flush()
    torch.cuda.synchronize()
    lay = eng.compact_layout()
    eng.close()
    assert lay.total == comp.numel() == 2593280 * n
    assert np.array_equal(r.cpu().numpy().astype(bool), expect) and not expect.all()
    _, chk = mats(pkg)
    assert chk.which_is_unsatisfied_compact(lay, comp).tolist() == [-1] * n
    assert chk.first_unreduced_compact(lay, comp).tolist() == [-1] * n
