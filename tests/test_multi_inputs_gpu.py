"""The N+1-pair product with public inputs (blsw_engine_create_multi_inputs) on the GPU: every witness element, instance element and result of the engine
(grouped, the latency modes, a wave boundary inside an instance's pairs, the pair-parallel Miller product, canonical output form, compact wire form)
against tests/multi_inputs' shim; the device R1CS check of the multi_inputs matrices; the Python verify_multi and the C++ caller."""
import importlib
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import multi_inputs_lib as M
from tests import synth
from tests.oracle_lib import P_MOD, R_MOD

pytestmark = pytest.mark.gpu
RINV = pow(1 << 384, -1, P_MOD)
K, N, STEPS, MSG_LEN = 3, 3, 3, 50  # 9 pair lanes per step; two chunks per message, the second of 3 bytes


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


ONE = limbs((1 << 384) % P_MOD)


def canonical_rows(a):
    """[m, 6] Montgomery limbs -> canonical integers; the booleans (zero and R mod p) without big-integer arithmetic"""
    out = np.zeros_like(a)
    is_one = (a == ONE).all(axis=1)
    out[is_one, 0] = 1
    for k in np.nonzero(~is_one & a.any(axis=1))[0]:
        out[k] = limbs(value(a[k]) * RINV % P_MOD)
    return out


_DISTINCT = {}


def distinct(oracle, k=K, msg_len=MSG_LEN):
    """at most four distinct instances per (K, msg_len): valid, tampered (message 1 flipped after signing), key 1 = (0, 0), another valid one.
    Each is (pks [K, 12], msgs [K, msg_len], sig [24], expected result)."""
    if (k, msg_len) not in _DISTINCT:
        a = synth.make_multi(oracle, k, msg_len=msg_len, start=30)
        t = synth.make_multi(oracle, k, msg_len=msg_len, start=40, tamper=1)
        z = synth.make_multi(oracle, k, msg_len=msg_len, start=50)
        zp = z[0].copy()
        zp[1] = 0  # the (0, 0) encoding of the point at infinity: pk != 0 fails for it, the result is false
        b = synth.make_multi(oracle, k, msg_len=msg_len, start=60)
        _DISTINCT[(k, msg_len)] = [a, t, (zp, z[1], z[2], False), b]
    return _DISTINCT[(k, msg_len)]


def tiled(cases, n, first=0):
    return [cases[(first + i) % len(cases)] for i in range(n)]


def batches(oracle):
    """three steps of 3 instances: step 0 = [valid, tampered, zero key], the next ones rotated by one"""
    d = distinct(oracle)
    return [tiled(d, N, k) for k in range(STEPS)]


_SHIM = {}


def shim_case(case, mask, form=0):
    """the shim's (result, witness, instance) of one instance, computed once per (instance, mask, element form)"""
    pks, msgs, sig, _ = case
    key = (pks.tobytes(), msgs.tobytes(), sig.tobytes(), mask)
    if key not in _SHIM:
        if len(_SHIM) >= 24:  # up to ~250 MB each
            _SHIM.clear()
        _SHIM[key] = {0: M.witness(pks, msgs, sig, mask)[:3]}
    e = _SHIM[key]
    if form not in e:
        r, w, ins = e[0]
        e[form] = (r, canonical_rows(w), canonical_rows(ins))
    return e[form]


def to_dev(torch, a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def stack(torch, batch, dev):
    return (to_dev(torch, np.stack([c[0] for c in batch]), dev), to_dev(torch, np.stack([c[1] for c in batch]), dev), to_dev(torch, np.stack([c[2] for c in batch]), dev))


def run_engine(pkg, torch, all_batches, mask, max_steps, n_buffers, k=K, msg_len=MSG_LEN, **opt):
    dev = torch.device("cuda:0")
    n = len(all_batches[0])
    eng = pkg.WitnessEngine(n, msg_len, max_steps=max_steps, n_buffers=n_buffers, device=dev, n_pairs=k, multi_inputs=mask, **opt)
    assert eng.n_instance_vars == M.n_instance_vars(k, msg_len, mask) and eng.n_witness == pkg.layout_multi(msg_len, k, mask)["n_witness"]
    outs = []
    for s, batch in enumerate(all_batches):
        pks, msgs, sig = stack(torch, batch, dev)
        w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
        w.fill_(-1)
        inst.fill_(-1)
        r = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert eng.submit_multi(pks, msgs, sig, witness=w, result=r, instance=inst) == s
        outs.append((r, w, inst))
    eng.flush()
    torch.cuda.synchronize()
    got = [(r.cpu().numpy(), w.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64)) for r, w, inst in outs]
    eng.close()
    return got


def check_all(all_batches, got, mask, form=0):
    for s, (batch, (res, wit, inst)) in enumerate(zip(all_batches, got)):
        for i, case in enumerate(batch):
            r, w, ins = shim_case(case, mask, form)
            assert r == case[3] and int(res[i]) == int(r), (s, i)
            assert wit[i].shape == w.shape
            bad = np.nonzero((w != wit[i]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (s, i, bad[0])
            assert np.array_equal(inst[i], ins), "step %d instance %d: instance vector differs" % (s, i)


# three steps through max_steps = 2: a launch group of two steps and one of one
CONFIGS = {"grouped": dict(max_steps=2, n_buffers=2), "latency_mode_1": dict(max_steps=2, n_buffers=2, latency_mode=1),
           "latency_mode_2": dict(max_steps=2, n_buffers=2, latency_mode=2)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("mask", [1, 4, 8, 13])
def test_engine_matches_the_shim(pkg, torch, oracle, mask, config):
    b = batches(oracle)
    assert [c[3] for c in b[0]] == [True, False, False]
    check_all(b, run_engine(pkg, torch, b, mask, **CONFIGS[config]), mask)


def test_wave_boundary_inside_an_instance(pkg, torch, oracle):
    """22 instances of 3 pairs: 66 pair lanes, the last instance's pairs on two waves"""
    b = [tiled(distinct(oracle), 22)]
    check_all(b, run_engine(pkg, torch, b, 13, max_steps=2, n_buffers=2), 13)


@pytest.mark.parametrize("mask", [8, 13])
def test_pair_parallel_miller_product(pkg, torch, oracle, mask):
    """8 pairs (BLSW_MILLER_PAR_MIN_PAIRS): the pair-parallel Miller product reads the prepared Input keys and the Input signature's coefficients"""
    d = distinct(oracle, 8, MSG_LEN)
    b = [[d[0], d[1]]]
    check_all(b, run_engine(pkg, torch, b, mask, max_steps=2, n_buffers=2, k=8), mask)


@pytest.mark.parametrize("mask", [4, 13])
def test_canonical_output_form(pkg, torch, oracle, mask):
    b = batches(oracle)
    check_all(b, run_engine(pkg, torch, b, mask, max_steps=2, n_buffers=2, output_form=1), mask, form=1)


def test_mask_0_through_submit_multi_io(pkg, torch, oracle):
    """every N+1-pair engine takes submit_multi_io: with no Input argument the witness tensor is bit-equal to submit_multi's, instance = [1]"""
    b = batches(oracle)
    dev = torch.device("cuda:0")
    got = run_engine(pkg, torch, b, 0, max_steps=2, n_buffers=2)
    eng = pkg.WitnessEngine(N, MSG_LEN, max_steps=2, n_buffers=2, device=dev, n_pairs=K)
    outs = []
    for batch in b:
        pks, msgs, sig = stack(torch, batch, dev)
        w = eng.new_witness_tensor()
        r = torch.empty(N, dtype=torch.int32, device=dev)
        eng.submit_multi(pks, msgs, sig, witness=w, result=r)
        outs.append((r, w))
    eng.flush()
    torch.cuda.synchronize()
    for (res, wit, inst), (r, w), batch in zip(got, outs, b):
        assert np.array_equal(wit, w.cpu().numpy().view(np.uint64)) and np.array_equal(res, r.cpu().numpy())
        assert inst.shape == (N, 1, 6) and all(np.array_equal(inst[i, 0], ONE) for i in range(N))
        assert res.astype(bool).tolist() == [case[3] for case in batch]
    eng.close()
    check_all(b[:1], got[:1], 0)  # and the all-Witness circuit is the shim's mask 0 (= the oracle's product, tests/test_multi_inputs.py)
    # a single-key engine refuses the step
    single = pkg.WitnessEngine(N, MSG_LEN, device=dev)
    pks, msgs, sig = stack(torch, b[0], dev)
    assert pkg.lib().blsw_engine_submit_multi_io(single._e, pks.data_ptr(), msgs.data_ptr(), sig.data_ptr(), None, None, 0, None, None) == 1
    single.close()


def test_compact_form_round_trip_and_golden_digests(pkg, torch, oracle):
    mask, n, k = 13, 32, 2  # 64 pair lanes: one pair tile, the instance lanes a part of one tile
    cases = [M.golden_case(oracle)] + distinct(oracle, k, MSG_LEN)[:3]
    batch = tiled(cases, n)
    dev = torch.device("cuda:0")
    pks, msgs, sig = stack(torch, batch, dev)
    eng = pkg.WitnessEngine(n, MSG_LEN, max_steps=2, device=dev, n_buffers=2, n_pairs=k, multi_inputs=mask)
    recv = pkg.WitnessEngine(n, MSG_LEN, max_steps=2, device=dev, n_buffers=1, n_pairs=k, multi_inputs=mask)
    comp, plain, inst = eng.new_compact_buffer(1), eng.new_witness_tensor(), eng.new_instance_tensor()
    plain.fill_(-1)
    r1, r2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_multi_compact(pks, msgs, sig, comp[0], result=r1)
    eng.submit_multi(pks, msgs, sig, witness=plain, result=r2, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor()
    out.fill_(-1)
    recv.expand_compact(comp[0], out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(r1, r2)
    for i in (0, 1, 2, 31):
        res, w, ins = shim_case(batch[i], mask)
        assert np.array_equal(plain[i].cpu().numpy().view(np.uint64), w) and bool(r2[i]) == res == batch[i][3], i
        assert np.array_equal(inst[i].cpu().numpy().view(np.uint64), ins), i
    # instance 0 is the golden file's case: the digests recorded from the shim
    g = json.load(open(M.GOLDEN))["multi_inputs"]["mask_%d" % mask]
    d = M.digests(plain[0].cpu().numpy().view(np.uint64), inst[0].cpu().numpy().view(np.uint64), pkg.layout_multi(MSG_LEN, k, mask))
    assert (g["n_witness"], g["n_instance_vars"], g["result"]) == (plain.shape[1], inst.shape[1], bool(r2[0]))
    for name in ("sha256_all", "sha256_instance", "sha256_segments"):
        assert g[name] == d[name], name
    eng.close()
    recv.close()


def test_device_r1cs_check(pkg, torch, oracle):
    mask = 13
    d = distinct(oracle)
    b = [d[0], d[1], d[3]]  # valid, tampered, valid: a (0, 0) key violates the enforced pk != 0 and is no satisfied system
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, MSG_LEN, max_steps=1, n_buffers=2, device=dev, n_pairs=K, multi_inputs=mask)
    pks, msgs, sig = stack(torch, b, dev)
    w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
    r = torch.empty(N, dtype=torch.int32, device=dev)
    eng.submit_multi(pks, msgs, sig, witness=w, result=r, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    assert r.cpu().tolist() == [1, 0, 1]
    chk = pkg.ConstraintChecker(MSG_LEN, n_pairs=K, multi_inputs=mask, device=dev)
    assert chk.n_instance_vars == inst.shape[1] and chk.n_witness == w.shape[1]
    assert chk.which_is_unsatisfied(w, inst).cpu().tolist() == [-1] * N  # a false result is not an unsatisfied system
    two = torch.from_numpy(limbs((2 << 384) % P_MOD).view(np.int64))
    c = M.chunks(MSG_LEN)
    # one message input (chunk 1 of pair 2 of instance 1), and separately one key's z (key 1 of instance 0): the row the shim's own check gives for
    # the same z, for that instance alone
    for i, at in ((1, 1 + 2 * c + 1), (0, 1 + K * c + 3 * 1 + 2)):
        bad = inst.clone()
        bad[i, at] = two
        pk_i, msg_i, sig_i, _ = b[i]
        host = M.check(pk_i, msg_i, sig_i, mask, bad[i].cpu().numpy().view(np.uint64), w[i].cpu().numpy().view(np.uint64))
        assert host >= 0
        want = [-1] * N
        want[i] = host
        assert chk.which_is_unsatisfied(w, bad).cpu().tolist() == want
    chk.close()


def test_python_verify_multi_with_input_wrappers(pkg, torch, oracle):
    b = batches(oracle)[1]
    dev = torch.device("cuda:0")
    pks, msgs, sig = stack(torch, b, dev)
    out = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(pks), pkg.UInt8.new_input_vec(msgs), pkg.SignatureVar.new_input(sig))
    assert len(out) == 3
    res, wit, inst = out
    check_all([b], [(res.cpu().numpy(), wit.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64))], 13)
    # the mask follows the wrappers: keys only
    res, wit, inst = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(pks), msgs, pkg.SignatureVar.new_witness(sig))
    assert inst.shape == (N, 1 + 3 * K, 6)
    check_all([b], [(res.cpu().numpy(), wit.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64))], 1)
    # all-Witness calls behave and return as before: two values, the direct call's witness vectors (bare tensors and Witness wrappers alike)
    r0, w0 = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), msgs, pkg.SignatureVar.new_witness(sig))
    r1, w1 = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), pkg.UInt8.new_witness_vec(msgs), pkg.SignatureVar.new_witness(sig))
    assert torch.equal(r0, r1) and torch.equal(w0, w1)
    check_all([b], [(r0.cpu().numpy(), w0.cpu().numpy().view(np.uint64), np.stack([ONE[None]] * N))], 0)
    with pytest.raises(pkg.BlswError):
        pkg.verify_multi(pkg.ParametersVar.new_witness(), pkg.PublicKeyVar.new_input(pks), msgs, pkg.SignatureVar.new_witness(sig))


def _digest(a):
    w = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    return int((w * (2 * np.arange(w.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def test_cpp_caller_multi_inputs(oracle):
    """include/blsw.hpp: verify_multi with Input keys, messages and signature from compressed bytes (tests/multi_inputs/cpp_caller.cpp)"""
    Kc, n = 3, 3
    lines, cases = [], []
    for i in range(n):
        sks = [int.from_bytes(synth._h(0x5EED, b"sk", 70 + 5 * i + j), "big") % R_MOD or 1 for j in range(Kc)]
        ms = [(synth._h(0x5EED, b"mm", 70 + 5 * i + j) * 2)[:MSG_LEN] for j in range(Kc)]
        pk48 = [bytes(oracle.sk_to_pk(sk)) for sk in sks]
        sig96 = bytes(oracle.aggregate_g2([oracle.sign(sk, m) for sk, m in zip(sks, ms)]))
        if i == 2:
            mm = bytearray(ms[1])
            mm[9] ^= 16  # tampered after signing: false, still satisfied
            ms[1] = bytes(mm)
        lines.append(sig96.hex() + " " + " ".join("%s %s" % (p.hex(), m.hex()) for p, m in zip(pk48, ms)))
        cases.append((np.stack([oracle.g1_decompress(p)[1] for p in pk48]), np.stack([np.frombuffer(m, dtype=np.uint8) for m in ms]), oracle.g2_decompress(sig96)[1], i != 2))
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_inputs", "cpp_caller")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.check_output([exe, f.name], text=True, timeout=300).split("\n")
    finally:
        os.unlink(f.name)
    for i, (pks, msgs, sig, want) in enumerate(cases):
        r, w, inst, _ = M.witness(pks, msgs, sig, 13)
        assert r == want
        assert out[i].split() == [str(int(want)), str(inst.shape[0]), str(w.shape[0]), str(_digest(inst)), str(_digest(w))], i
