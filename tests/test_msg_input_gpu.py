"""The message allocated as public inputs (UInt8::new_input_vec, options.msg_mode 1) on the GPU: witness vectors, instance vectors and results
of the engine (direct mode, grouped engine in every latency mode, ragged batches with tampered signatures and identity points, canonical
output form, compact wire form) against tests/msg_input's shim; the device R1CS check of the _inputs matrices; the Python gadget."""
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import msg_input_lib as M
from tests import synth
from tests.oracle_lib import P_MOD, R_MOD

pytestmark = pytest.mark.gpu
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (pk_mode, sig_mode)
RINV = pow(1 << 384, -1, P_MOD)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make_batch(o, n, msg_len, seed=0x3E55, tamper_every=4, identity=None):
    """n instances over synth's 16 keys with messages of msg_len bytes; every tamper_every-th message is flipped after signing; instance
    `identity` gets the point at infinity as key and signature (e(-g1, O) e(O, H(m)) = 1: the gadget's Boolean is true, while the circuit's
    pk != 0 constraint is left unsatisfied). -> (pk [n,12], msg [n,msg_len], sig [n,24], expect)"""
    sks = [int.from_bytes(synth._h(0x5EED, b"sk", k), "big") % R_MOD or 1 for k in range(16)]
    pk = np.zeros((n, 12), dtype=np.uint64)
    sig = np.zeros((n, 24), dtype=np.uint64)
    msg = np.zeros((n, msg_len), dtype=np.uint8)
    expect = np.ones(n, dtype=bool)
    for i in range(n):
        m = (synth._h(seed, b"m", i) * (msg_len // 32 + 1))[:msg_len]
        st, xy, _ = o.g1_decompress(o.sk_to_pk(sks[i % 16]))
        st2, sxy, _ = o.g2_decompress(o.sign(sks[i % 16], m))
        assert st == 0 and st2 == 0
        pk[i], sig[i] = xy, sxy
        mb = bytearray(m)
        if msg_len and tamper_every and i % tamper_every == tamper_every - 1:
            mb[i % msg_len] ^= 1
            expect[i] = False
        msg[i] = np.frombuffer(bytes(mb), dtype=np.uint8)
        if i == identity:
            pk[i], sig[i], expect[i] = 0, 0, True
    return pk, msg, sig, expect


def canonical(limbs):
    a = sum(int(x) << (64 * k) for k, x in enumerate(limbs))
    v = a * RINV % P_MOD
    return np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


def check_against_shim(pk, msg, sig, expect, res, wit, inst, pm, sm, idx=None):
    for i in (range(len(pk)) if idx is None else idx):
        r, w, ins, _ = M.witness(pk[i], msg[i].tobytes(), sig[i], pm, sm)
        assert r == bool(expect[i]) == bool(res[i]), i
        assert wit[i].shape[0] >= w.shape[0] and np.array_equal(wit[i][:w.shape[0]], w), "witness of instance %d differs" % i
        assert np.array_equal(inst[i], ins), "instance of instance %d differs" % i


def run_engine(pkg, torch, batches, msg_len, pm, sm, max_steps=1, n_buffers=1, **opt):
    dev = torch.device("cuda:0")
    n = batches[0][0].shape[0]
    eng = pkg.WitnessEngine(n, msg_len, max_steps=max_steps, n_buffers=n_buffers, device=dev, msg_mode=1, pk_mode=pm, sig_mode=sm, **opt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
    outs = []
    for pk, msg, sig, _ in batches:
        w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
        w.fill_(-1)
        inst.fill_(-1)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(t(pk), t(sig), t(msg), witness=w, result=r, instance=inst)
        outs.append((r, w, inst))
    eng.flush()
    torch.cuda.synchronize()
    got = [(r.cpu().numpy(), w.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64)) for r, w, inst in outs]
    eng.close()
    return got


@pytest.mark.parametrize("msg_len", [32, 47, 48, 120, 0])
@pytest.mark.parametrize("pk_mode,sig_mode", MODES)
def test_direct_engine_matches_the_shim(pkg, torch, oracle, msg_len, pk_mode, sig_mode):
    b = make_batch(oracle, 4, msg_len)
    (res, wit, inst), = run_engine(pkg, torch, [b], msg_len, pk_mode, sig_mode)
    assert inst.shape[1] == 1 + M.chunks(msg_len) + 3 * pk_mode + 6 * sig_mode
    check_against_shim(*b, res, wit, inst, pk_mode, sig_mode)


@pytest.mark.parametrize("latency_mode", [0, 1, 2])
def test_grouped_engine_ragged_batches(pkg, torch, oracle, latency_mode):
    """three steps of 5 instances in groups of 2 over 2 group buffers; tampered messages and one instance with identity key and signature"""
    msg_len = 95
    batches = [make_batch(oracle, 5, msg_len, seed=0x100 + s, tamper_every=3, identity=2 if s == 1 else None) for s in range(3)]
    for pm, sm in ((1, 1), (0, 1)):
        got = run_engine(pkg, torch, batches, msg_len, pm, sm, max_steps=2, n_buffers=2, latency_mode=latency_mode)
        for b, (res, wit, inst) in zip(batches, got):
            check_against_shim(*b, res, wit, inst, pm, sm)


def test_canonical_output_form(pkg, torch, oracle):
    msg_len = 48
    b = make_batch(oracle, 4, msg_len)
    (res, wit, inst), = run_engine(pkg, torch, [b], msg_len, 1, 1, max_steps=2, n_buffers=1, output_form=1)
    c = M.chunks(msg_len)
    for i in range(4):
        r, w, ins, _ = M.witness(b[0][i], b[1][i].tobytes(), b[2][i], 1, 1)
        assert bool(res[i]) == r
        assert all(np.array_equal(inst[i][k], canonical(ins[k])) for k in range(ins.shape[0])), i
        for k in list(range(0, 761 * c, 97)) + [761 * c - 1]:  # the message segment's elements as canonical integers
            assert np.array_equal(wit[i][k], canonical(w[k])), (i, k)


def test_device_r1cs_check(pkg, torch, oracle):
    msg_len, pm, sm = 48, 1, 1
    b = make_batch(oracle, 4, msg_len)
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(4, msg_len, device=dev, msg_mode=1, pk_mode=pm, sig_mode=sm)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
    w, inst = eng.new_witness_tensor(), eng.new_instance_tensor()
    r = torch.empty(4, dtype=torch.int32, device=dev)
    eng.submit(t(b[0]), t(b[2]), t(b[1]), witness=w, result=r, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    chk = pkg.ConstraintChecker(msg_len, pk_mode=pm, sig_mode=sm, msg_mode=1, device=dev)
    assert chk.n_instance_vars == inst.shape[1] and chk.n_witness == w.shape[1]
    assert chk.which_is_unsatisfied(w, inst).cpu().tolist() == [-1] * 4
    # the first message input + 1 (Montgomery one added): the packing constraint of chunk 0, row 381
    one = (1 << 384) % P_MOD
    bad_inst = inst.clone()
    for i in range(4):
        e = sum(int(x) << (64 * k) for k, x in enumerate(bad_inst[i, 1].cpu().numpy().view(np.uint64)))
        v = (e + one) % P_MOD
        bad_inst[i, 1] = torch.from_numpy(np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64).view(np.int64))
    assert chk.which_is_unsatisfied(w, bad_inst).cpu().tolist() == [381] * 4
    # a flipped message bit (chunk 1, bit 5) fails where the host check of the shim's system fails
    lay = eng.layout
    k = lay["off_msg"] + 761 + 5
    bad_w = w.clone()
    wk = bad_w[1, k].cpu().numpy().view(np.uint64)
    flipped = np.zeros(6, np.uint64) if wk.any() else np.array([(one >> (64 * q)) & (2**64 - 1) for q in range(6)], dtype=np.uint64)
    bad_w[1, k] = torch.from_numpy(flipped.view(np.int64))
    got = chk.which_is_unsatisfied(bad_w, inst).cpu().tolist()
    host = M.check(b[0][1], b[1][1].tobytes(), b[2][1], pm, sm, inst[1].cpu().numpy().view(np.uint64), bad_w[1].cpu().numpy().view(np.uint64))
    assert host >= 0 and got == [-1, host, -1, -1]
    eng.close()


def test_compact_form_round_trip(pkg, torch, oracle):
    msg_len, n = 32, 64
    pk, msg, sig, expect = make_batch(oracle, n, msg_len)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
    eng = pkg.WitnessEngine(n, msg_len, max_steps=2, device=dev, n_buffers=2, msg_mode=1, pk_mode=1)
    recv = pkg.WitnessEngine(n, msg_len, max_steps=2, device=dev, n_buffers=1, msg_mode=1, pk_mode=1)
    d = (t(pk), t(sig), t(msg))
    comp, plain = eng.new_compact_buffer(1), eng.new_witness_tensor()
    r1, r2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_compact(d[0], d[1], d[2], comp[0], result=r1)
    eng.submit(d[0], d[1], d[2], witness=plain, result=r2)
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor()
    out.fill_(-1)
    recv.expand_compact(comp[0], out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(r1, r2)
    assert r2.cpu().numpy().astype(bool).tolist() == expect.tolist()
    wit = plain.cpu().numpy().view(np.uint64)
    for i in (0, 3, 63):
        rr, w, _, _ = M.witness(pk[i], msg[i].tobytes(), sig[i], 1, 0)
        assert np.array_equal(wit[i], w), i
    eng.close()
    recv.close()


def test_python_gadget_new_input_vec(pkg, torch, oracle):
    msg_len = 47
    pk, msg, sig, expect = make_batch(oracle, 4, msg_len)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)
    g = pkg.BlsSignatureVerifyGadget(4, msg_len, device=dev, msg_mode="input", pk_mode="input")
    with pytest.raises(pkg.BlswError):  # a bare tensor is UInt8::new_witness_vec: not this gadget's circuit
        g.verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(t(pk)), t(msg), pkg.SignatureVar.new_witness(t(sig)))
    res = g.verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_input(t(pk)), pkg.UInt8.new_input_vec(t(msg)), pkg.SignatureVar.new_witness(t(sig)))
    torch.cuda.synchronize()
    assert g.instance.shape == (4, 1 + 2 + 3 - 1, 6)
    check_against_shim(pk, msg, sig, expect, res.cpu().numpy(), g.witness.cpu().numpy().view(np.uint64), g.instance.cpu().numpy().view(np.uint64), 1, 0)
    g.engine.close()
    w = pkg.BlsSignatureVerifyGadget(4, msg_len, device=dev, want_witness=False)
    with pytest.raises(pkg.BlswError):
        w.verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(t(pk)), pkg.UInt8.new_input_vec(t(msg)), pkg.SignatureVar.new_witness(t(sig)))
    w.engine.close()
    with pytest.raises(pkg.BlswError):
        pkg.verify_mixed_lengths(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(t(pk)), [bytes(m) for m in msg], pkg.SignatureVar.new_witness(t(sig)), msg_mode=1)


def _digest(a):
    w = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    return int((w * (2 * np.arange(w.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def test_cpp_caller_new_input_vec(oracle):
    """include/blsw.hpp: UInt8::new_input_vec with an Input key from compressed bytes (tests/msg_input/cpp_caller.cpp) against the shim"""
    msg_len, n = 48, 3
    sks = [int.from_bytes(synth._h(0x5EED, b"sk", k), "big") % R_MOD or 1 for k in range(n)]
    lines, cases = [], []
    for i, sk in enumerate(sks):
        m = (synth._h(0x77, b"m", i) * 2)[:msg_len]
        pk48, sig96 = oracle.sk_to_pk(sk), oracle.sign(sk, m)
        mm = bytearray(m)
        if i == 2:
            mm[40] ^= 4  # tampered after signing: false, still satisfied
        lines.append("%s %s %s" % (bytes(pk48).hex(), bytes(mm).hex(), bytes(sig96).hex()))
        cases.append((oracle.g1_decompress(pk48)[1], bytes(mm), oracle.g2_decompress(sig96)[1], i != 2))
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "msg_input", "cpp_caller")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        out = subprocess.check_output([exe, f.name], text=True, timeout=300).split("\n")
    finally:
        os.unlink(f.name)
    for i, (pk, m, sig, want) in enumerate(cases):
        r, w, inst, _ = M.witness(pk, m, sig, 1, 0)
        assert r == want
        assert out[i].split() == [str(int(want)), str(inst.shape[0]), str(w.shape[0]), str(_digest(inst)), str(_digest(w)), "-1"], i
