"""aggregate_verify with public inputs (options.agg_inputs, ABI 13) on the GPU: every witness element, instance element, result and count of the
engine (grouped, direct mode, the latency modes, canonical output form, compact wire form, the reference's 512-key case) against tests/agg_inputs'
shim; the device R1CS check of the aggregate_inputs matrices; the Python gadget and the C++ caller."""
import hashlib
import importlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import agg_inputs_lib as A
from tests import synth
from tests.oracle_lib import P_MOD, R_MOD

pytestmark = pytest.mark.gpu
RINV = pow(1 << 384, -1, P_MOD)
K, N, STEPS = 5, 6, 3


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def limbs(v):
    return np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


def value(e):
    return sum(int(x) << (64 * k) for k, x in enumerate(e))


def canonical_rows(a):
    """[m, 6] Montgomery limbs -> canonical integers; the booleans (zero and R mod p) without big-integer arithmetic"""
    one = limbs((1 << 384) % P_MOD)
    out = np.zeros_like(a)
    is_one = (a == one).all(axis=1)
    out[is_one, 0] = 1
    for k in np.nonzero(~is_one & a.any(axis=1))[0]:
        out[k] = limbs(value(a[k]) * RINV % P_MOD)
    return out


def batches(oracle):
    """three steps of 6 instances of 5 keys, bitmaps and a tampered instance as test_engine_aggregate_grouped builds them"""
    out = []
    for k in range(STEPS):
        batch = []
        for i in range(N):
            bm = [(i >> b) & 1 for b in range(K)]
            bm[(i + k) % K] = 1  # at least one key selected
            batch.append(synth.make_aggregate(oracle, K, bm, start=100 * k + 10 * i, tamper=(i == 4)))
        out.append(batch)
    return out


_SHIM = {}


def shim_case(case, mask):
    """the shim's (result, count, witness, instance, n_constraints) of one instance, computed once per (instance, mask)"""
    pks, bm, msg, sig, _ = case
    key = (pks.tobytes(), bm.tobytes(), msg.tobytes(), sig.tobytes(), mask)
    if key not in _SHIM:
        if len(_SHIM) >= 40:  # ~35 MB each
            _SHIM.clear()
        _SHIM[key] = A.witness(pks, bm, msg.tobytes(), sig, mask)
    return _SHIM[key]


def to_dev(torch, a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def stack(torch, batch, dev):
    return (to_dev(torch, np.stack([c[0] for c in batch]), dev), to_dev(torch, np.stack([c[1] for c in batch]), dev), to_dev(torch, np.stack([c[3] for c in batch]), dev),
            to_dev(torch, np.stack([c[2] for c in batch]), dev))  # pks, bitmap, sig, msg


def run_engine(pkg, torch, all_batches, mask, max_steps, n_buffers, **opt):
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, 32, max_steps=max_steps, n_buffers=n_buffers, device=dev, n_keys=K, agg_inputs=mask, **opt)
    assert eng.n_instance_vars == A.n_instance_vars(K, 32, mask) and eng.n_witness == pkg.layout_aggregate(32, K, mask)["n_witness"]
    outs = []
    for k, batch in enumerate(all_batches):
        pks, bmt, sig, msg = stack(torch, batch, dev)
        w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
        w.fill_(-1)
        inst.fill_(-1)
        r = torch.empty(N, dtype=torch.int32, device=dev)
        c = torch.empty(N, dtype=torch.int32, device=dev)
        assert eng.submit_aggregate(pks, bmt, sig, msg, witness=w, result=r, count=c, instance=inst) == k
        outs.append((r, c, w, inst))
    eng.flush()
    torch.cuda.synchronize()
    got = [(r.cpu().numpy(), c.cpu().numpy(), w.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64)) for r, c, w, inst in outs]
    eng.close()
    return got


def check_all(all_batches, got, mask, form=0):
    for k, (batch, (res, cnt, wit, inst)) in enumerate(zip(all_batches, got)):
        for i, case in enumerate(batch):
            r, c, w, ins, _ = shim_case(case, mask)
            assert r == case[4] == bool(res[i]) and c == int(cnt[i]) == int(case[1].sum()), (k, i)
            if form:
                w, ins = canonical_rows(w), canonical_rows(ins)
            assert wit[i].shape == w.shape
            bad = np.nonzero((w != wit[i]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
            assert np.array_equal(inst[i], ins), "step %d instance %d: instance vector differs" % (k, i)


CONFIGS = {"grouped": dict(max_steps=2, n_buffers=2), "direct": dict(max_steps=1, n_buffers=1), "latency_mode_1": dict(max_steps=2, n_buffers=2, latency_mode=1),
           "latency_mode_2": dict(max_steps=2, n_buffers=2, latency_mode=2)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("mask", [3, 4, 8, 15])
def test_engine_matches_the_shim(pkg, torch, oracle, mask, config):
    b = batches(oracle)
    check_all(b, run_engine(pkg, torch, b, mask, **CONFIGS[config]), mask)


@pytest.mark.parametrize("mask", [3, 4, 8, 15])
def test_canonical_output_form(pkg, torch, oracle, mask):
    b = batches(oracle)
    check_all(b, run_engine(pkg, torch, b, mask, max_steps=2, n_buffers=2, output_form=1), mask, form=1)


def test_mask_0_through_submit_aggregate_io(pkg, torch, oracle):
    """every aggregate engine takes submit_aggregate_io: with no Input argument the witness tensor is bit-equal to submit_aggregate's, instance = [1]"""
    b = batches(oracle)
    dev = torch.device("cuda:0")
    got = run_engine(pkg, torch, b, 0, max_steps=2, n_buffers=2)
    eng = pkg.WitnessEngine(N, 32, max_steps=2, n_buffers=2, device=dev, n_keys=K)
    one = limbs((1 << 384) % P_MOD)
    outs = []
    for batch in b:
        pks, bmt, sig, msg = stack(torch, batch, dev)
        w = eng.new_witness_tensor()
        r = torch.empty(N, dtype=torch.int32, device=dev)
        c = torch.empty(N, dtype=torch.int32, device=dev)
        eng.submit_aggregate(pks, bmt, sig, msg, witness=w, result=r, count=c)
        outs.append((r, c, w))
    eng.flush()
    torch.cuda.synchronize()
    for (res, cnt, wit, inst), (r, c, w), batch in zip(got, outs, b):
        assert np.array_equal(wit, w.cpu().numpy().view(np.uint64)) and np.array_equal(res, r.cpu().numpy()) and np.array_equal(cnt, c.cpu().numpy())
        assert inst.shape == (N, 1, 6) and all(np.array_equal(inst[i, 0], one) for i in range(N))
        assert res.astype(bool).tolist() == [case[4] for case in batch]
    eng.close()
    check_all(b[:1], got[:1], 0)  # and the all-Witness circuit is the shim's mask 0
    # a single-key engine refuses the aggregate step
    single = pkg.WitnessEngine(N, 32, device=dev)
    pks, bmt, sig, msg = stack(torch, b[0], dev)
    assert pkg.lib().blsw_engine_submit_aggregate_io(single._e, pks.data_ptr(), bmt.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
    single.close()


@pytest.mark.parametrize("mask", [3, 15])
def test_reference_512_key_case(pkg, torch, oracle, mask):
    """constraints.rs:378-441 (key 1, 511 x key 2): the first two selected -> true, count 2; every key selected -> false, count 512"""
    pks, msg, sig, _ = A.reference_case(oracle)
    bms = np.zeros((2, 512), dtype=np.uint8)
    bms[0, :2] = 1
    bms[1, :] = 1
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(2, 32, device=dev, n_keys=512, agg_inputs=mask)
    if mask == 3:
        assert eng.n_witness == 730081 and eng.n_instance_vars == 2049
    w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
    w.fill_(-1)
    inst.fill_(-1)
    r = torch.empty(2, dtype=torch.int32, device=dev)
    c = torch.empty(2, dtype=torch.int32, device=dev)
    eng.submit_aggregate(to_dev(torch, np.stack([pks, pks]), dev), to_dev(torch, bms, dev), to_dev(torch, np.stack([sig, sig]), dev),
                         to_dev(torch, np.stack([np.frombuffer(msg, dtype=np.uint8)] * 2), dev), witness=w, result=r, count=c, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    assert r.cpu().tolist() == [1, 0] and c.cpu().tolist() == [2, 512]
    wit, ins = w.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64)
    for i in range(2):
        res, cnt, sw, si, _ = A.witness(pks, bms[i], msg, sig, mask)
        assert (res, cnt) == ((True, 2) if i == 0 else (False, 512))
        bad = np.nonzero((sw != wit[i]).any(axis=1))[0]
        assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (i, bad[0])
        assert np.array_equal(ins[i], si), i
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_inputs_digests.json")))["agg_inputs"]["mask_%d" % mask]
    case = gold["cases"]["constraints_rs_378_first_two_selected"]
    b = np.ascontiguousarray(wit[0]).view(np.uint8).reshape(wit.shape[1], 48)
    assert (case["n_instance_vars"], case["n_witness"], case["result"], case["count"]) == (ins.shape[1], wit.shape[1], True, 2)
    assert case["sha256_instance"] == hashlib.sha256(np.ascontiguousarray(ins[0]).tobytes()).hexdigest()
    assert case["sha256_all"] == hashlib.sha256(b.tobytes()).hexdigest()
    for name, lo, hi in gold["segments"]:
        assert case["sha256_segments"][name] == hashlib.sha256(b[lo:hi].tobytes()).hexdigest(), name


def test_device_r1cs_check(pkg, torch, oracle):
    mask = 15
    b = batches(oracle)[0]
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, 32, device=dev, n_keys=K, agg_inputs=mask)
    pks, bmt, sig, msg = stack(torch, b, dev)
    w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
    r = torch.empty(N, dtype=torch.int32, device=dev)
    eng.submit_aggregate(pks, bmt, sig, msg, witness=w, result=r, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    chk = pkg.ConstraintChecker(32, n_keys=K, agg_inputs=mask, device=dev)
    assert chk.n_instance_vars == inst.shape[1] and chk.n_witness == w.shape[1]
    assert chk.which_is_unsatisfied(w, inst).cpu().tolist() == [-1] * N  # a tampered message is a false result, not an unsatisfied system
    # one bitmap input := the field element 2 (Montgomery form, the tensor's): the row the shim's own check gives for the same z
    bad = inst.clone()
    at = 1 + 3 * K + 2
    bad[3, at] = torch.from_numpy(limbs((2 << 384) % P_MOD).view(np.int64))
    pk3, bm3, msg3, sig3, _ = b[3]
    host = A.check(pk3, bm3, msg3.tobytes(), sig3, mask, bad[3].cpu().numpy().view(np.uint64), w[3].cpu().numpy().view(np.uint64))
    assert host == 2  # bit 2's booleanity row: Input keys have no constraints, the bitmap's K rows come first
    assert chk.which_is_unsatisfied(w, bad).cpu().tolist() == [-1, -1, -1, host, -1, -1]
    chk.close()


def test_compact_form_round_trip(pkg, torch, oracle):
    mask, n = 15, 64
    b = batches(oracle)[0]
    dev = torch.device("cuda:0")
    rep = lambda t: t.repeat((n + N - 1) // N, *([1] * (t.dim() - 1)))[:n].contiguous()
    pks, bmt, sig, msg = (rep(t) for t in stack(torch, b, dev))
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_keys=K, agg_inputs=mask)
    recv = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=1, n_keys=K, agg_inputs=mask)
    comp, plain = eng.new_compact_buffer(1), eng.new_witness_tensor()
    r1, r2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    c1, c2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_aggregate_compact(pks, bmt, sig, msg, comp[0], result=r1, count=c1)
    eng.submit_aggregate(pks, bmt, sig, msg, witness=plain, result=r2, count=c2)  # no instance vector asked for
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor()
    out.fill_(-1)
    recv.expand_compact(comp[0], out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(r1, r2) and torch.equal(c1, c2)
    wit = plain.cpu().numpy().view(np.uint64)
    for i in (0, 4, 63):
        res, cnt, w, _, _ = shim_case(b[i % N], mask)
        assert np.array_equal(wit[i], w) and bool(r2[i]) == res and int(c2[i]) == cnt, i
    eng.close()
    recv.close()


def test_python_aggregate_verify_with_input_wrappers(pkg, torch, oracle):
    b = batches(oracle)[1]
    dev = torch.device("cuda:0")
    pks, bmt, sig, msg = stack(torch, b, dev)
    out = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(pks), pkg.Boolean.new_input(bmt), pkg.UInt8.new_input_vec(msg), pkg.SignatureVar.new_input(sig))
    assert len(out) == 4
    res, cnt, wit, inst = out
    check_all([b], [(res.cpu().numpy(), cnt.cpu().numpy(), wit.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64))], 15)
    # the mask follows the wrappers: keys and bitmap only
    res, cnt, wit, inst = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(pks), pkg.Boolean.new_input(bmt), msg, pkg.SignatureVar.new_witness(sig))
    assert inst.shape == (N, 1 + 4 * K, 6)
    check_all([b], [(res.cpu().numpy(), cnt.cpu().numpy(), wit.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64))], 3)
    # all-Witness calls behave and return as before: three values, the direct call's witness vectors (bare tensors and Witness wrappers alike)
    r0, c0, w0 = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), bmt, msg, pkg.SignatureVar.new_witness(sig))
    r1, c1, w1 = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), pkg.Boolean.new_witness(bmt), pkg.UInt8.new_witness_vec(msg),
                                      pkg.SignatureVar.new_witness(sig))
    assert torch.equal(r0, r1) and torch.equal(c0, c1) and torch.equal(w0, w1)
    check_all([b], [(r0.cpu().numpy(), c0.cpu().numpy(), w0.cpu().numpy().view(np.uint64), np.stack([limbs((1 << 384) % P_MOD)[None]] * N))], 0)
    with pytest.raises(pkg.BlswError):
        pkg.aggregate_verify(pkg.ParametersVar.new_witness(), pkg.PublicKeyVar.new_input(pks), bmt, msg, pkg.SignatureVar.new_witness(sig))


def _digest(a):
    w = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    return int((w * (2 * np.arange(w.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def test_cpp_caller_aggregate_inputs(oracle):
    """include/blsw.hpp: aggregate_verify with Input keys, bitmap, message and signature from compressed bytes (tests/agg_inputs/cpp_caller.cpp)"""
    Kc, n = 3, 3
    lines, cases = [], []
    for i in range(n):
        bm = [1, (i >> 0) & 1, (i >> 1) & 1]
        m = synth._h(0x5EED, b"am", 50 + i)
        sks = [int.from_bytes(synth._h(0x5EED, b"sk", 50 + i + j), "big") % R_MOD or 1 for j in range(Kc)]
        pk48 = [bytes(oracle.sk_to_pk(sk)) for sk in sks]
        sig96 = bytes(oracle.aggregate_g2([oracle.sign(sk, m) for sk, b in zip(sks, bm) if b]))
        mm = bytearray(m)
        if i == 2:
            mm[9] ^= 16  # tampered after signing: false, still satisfied
        lines.append("%s %s %s %s" % ("".join(str(b) for b in bm), bytes(mm).hex(), sig96.hex(), " ".join(p.hex() for p in pk48)))
        cases.append((np.stack([oracle.g1_decompress(p)[1] for p in pk48]), np.array(bm, dtype=np.uint8), bytes(mm), oracle.g2_decompress(sig96)[1], i != 2))
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agg_inputs", "cpp_caller")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.check_output([exe, f.name], text=True, timeout=300).split("\n")
    finally:
        os.unlink(f.name)
    for i, (pks, bm, m, sig, want) in enumerate(cases):
        r, cnt, w, inst, _ = A.witness(pks, bm, m, sig, 15)
        assert r == want
        assert out[i].split() == [str(int(want)), str(cnt), str(inst.shape[0]), str(w.shape[0]), str(_digest(inst)), str(_digest(w)), "-1"], i
