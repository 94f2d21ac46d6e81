"""GPU parity (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against the CPU oracle on the
same inputs — bit-exact on every witness element — plus the reference's golden vectors."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import hostsim_lib, synth
from tests.oracle_lib import GOLDEN, eth_cases, unhex

pytestmark = pytest.mark.gpu
LIT = json.load(open(os.path.join(GOLDEN, "literals.json")))


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = importlib.import_module("bls-verify-gadget_amd")
    p.lib()
    return p


def _run(pkg, pk, msg, sig, want_witness=True, **options):
    import torch

    dev = torch.device("cuda:0")
    n, msg_len = msg.shape
    g = pkg.BlsSignatureVerifyGadget(n, msg_len, device=dev, want_witness=want_witness, **options)
    res = g.verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.from_numpy(pk.view(np.int64)).to(dev)), torch.from_numpy(msg).to(dev),
                   pkg.SignatureVar.new_witness(torch.from_numpy(sig.view(np.int64)).to(dev)))
    torch.cuda.synchronize()
    w = g.witness.cpu().numpy().view(np.uint64) if want_witness else None
    return res.cpu().numpy().astype(bool), w


def _compare(oracle, pk, msg, sig, got, w, idx):
    for i in idx:
        n, _, r, ow = oracle.witness(pk[i], msg[i].tobytes(), sig[i])
        assert r == bool(got[i]), "result mismatch at instance %d" % i
        assert w.shape[1] == n
        bad = np.nonzero((ow != w[i]).any(axis=1))[0]
        assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (i, bad[0])


def test_batch_bit_exact(pkg, oracle):
    # 70 instances: one full wave + a ragged one; includes tampered messages (every 16th)
    n = 70
    pk, msg, sig, expect = synth.make_batch(oracle, n)
    got, w = _run(pkg, pk, msg, sig)
    assert np.array_equal(got, expect)
    _compare(oracle, pk, msg, sig, got, w, range(n))


def _grouped_engine_against_oracle(pkg, oracle, n=35, steps=2, identity_at=None, **options):
    """n * steps instances (a full wave and a ragged one per step) through a grouped engine (two steps per group) with the given options;
    every fourth instance on all elements against the oracle. identity_at: that instance gets the all-zero (identity) key and signature."""
    import torch

    pk, msg, sig, expect = synth.make_batch(oracle, n * steps)
    if identity_at is not None:
        pk, sig, expect = pk.copy(), sig.copy(), expect.copy()
        pk[identity_at] = 0
        sig[identity_at] = 0
        expect[identity_at] = oracle.witness(pk[identity_at], msg[identity_at].tobytes(), sig[identity_at])[2]  # the gadget's Boolean on defined values
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, **options)
    outs, ress, keep = [], [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        d = (torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev))
        w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(d[0], d[1], d[2], witness=w, result=r)
        outs.append(w), ress.append(r), keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect[sl])
        idx = sorted(set(range(0, n, 4)) | ({identity_at - k * n} if identity_at is not None and k * n <= identity_at < (k + 1) * n else set()))
        _compare(oracle, pk[sl], msg[sl], sig[sl], got, outs[k].cpu().numpy().view(np.uint64), idx)
    eng.close()


@pytest.mark.parametrize("chain_variant,cofactor_mode", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_kernel_variants_bit_exact(pkg, oracle, chain_variant, cofactor_mode):
    """Every compilation of the chain kernels and both forms of the cofactor chain write the same bytes: out-of-line / inlined
    (options.chain_variant) x one chain per lane / three chunks + join (options.cofactor_mode), a full wave and a ragged one, through a
    grouped engine (two steps per group); the latency kernels are switched off here (next test)."""
    _grouped_engine_against_oracle(pkg, oracle, chain_variant=chain_variant, cofactor_mode=cofactor_mode, latency_mode=1)


@pytest.mark.parametrize("latency_mode", [0, 2, 3, 4])
def test_latency_kernels_bit_exact(pkg, oracle, latency_mode):
    """options.latency_mode: the chains of a small launch group on quads (k_map_q, k_prepare_q, k_g2_alloc_q: the Fp products of every Fp2
    operation on different lanes, DPP broadcasts) and clear_cofactor2 values first (cofactor_vf.hpp: Jacobian value chains, one lane per
    doubling / addition for the witnesses) write the same bytes as the one-instance-per-lane chains: 0 = the default rule (the first group
    finds the chains idle and takes them, the second does not), 2 = every group, 3 = values-first cofactor only, 4 = quads only. Three steps
    (groups of two and one), ragged waves, one instance with the identity as key and signature."""
    _grouped_engine_against_oracle(pkg, oracle, n=35, steps=3, identity_at=37, latency_mode=latency_mode)


@pytest.mark.parametrize("pk_mode,sig_mode,max_steps", [(1, 1, 1), (1, 0, 2), (0, 1, 2), (1, 1, 2)])
def test_public_input_allocation_modes(pkg, oracle, pk_mode, sig_mode, max_steps):
    """PublicKeyVar / SignatureVar::new_variable with AllocationMode::Input (constraints.rs:214-249; options.pk_mode / sig_mode, blsw_engine_submit_io):
    witness vectors AND instance_assignment against the oracle, direct mode (max_steps 1) and through the grouped engine (latency kernels and the
    ordinary ones), a ragged batch with tampered instances and one identity key + signature; the GPU assignment satisfies the product's matrices."""
    import torch

    n, steps = 35, 3 if max_steps > 1 else 1
    pk, msg, sig, expect = synth.make_batch(oracle, n * steps)
    pk, sig = pk.copy(), sig.copy()
    pk[5] = 0
    sig[5] = 0
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=max_steps, device=dev, n_buffers=2 if max_steps > 1 else 1, pk_mode=pk_mode, sig_mode=sig_mode)
    lay = eng.layout
    assert eng.n_instance_vars == 1 + 3 * pk_mode + 6 * sig_mode and eng.n_witness == pkg.layout(32)["n_witness"] - 1942 * pk_mode - 12413 * sig_mode
    outs, insts, ress, keep = [], [], [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        d = (torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev))
        w, inst, r = eng.new_witness_tensor(), eng.new_instance_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(d[0], d[1], d[2], witness=w, result=r, instance=inst)
        outs.append(w), insts.append(inst), ress.append(r), keep.append(d)
        if max_steps == 1:
            eng.flush()
    eng.flush()
    torch.cuda.synchronize()
    P = None
    for k in range(steps):
        got = ress[k].cpu().numpy().astype(bool)
        w = outs[k].cpu().numpy().view(np.uint64)
        inst = insts[k].cpu().numpy().view(np.uint64)
        for i in sorted(set(range(0, n, 6)) | ({5} if k == 0 else set())):
            g = k * n + i
            nw, _, res, ow, oinst = oracle.witness_io(pk[g], msg[g].tobytes(), sig[g], pk_mode, sig_mode)
            assert res == bool(got[i]) and nw == eng.n_witness, (k, i)
            assert np.array_equal(inst[i], oinst), "instance_assignment of instance %d" % g
            bad = np.nonzero((ow != w[i]).any(axis=1))[0]
            assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (g, bad[0])
            if P is None and g != 5:
                P = pkg.matrices(32, pk_mode=pk_mode, sig_mode=sig_mode)
                assert hostsim_lib.r1cs_check(P, w[i], inst[i]) == -1
        assert np.array_equal(got[np.arange(n) != 5] if k == 0 else got, expect[k * n:(k + 1) * n][np.arange(n) != 5] if k == 0 else expect[k * n:(k + 1) * n])
    eng.close()


def test_reference_gadget_case(pkg, oracle):
    # constraints.rs:318-376: [true, false, false]
    g = LIT["gadget_verify"]
    _, pk1, _ = oracle.g1_decompress(bytes.fromhex(g["pubkey"]))
    _, sig1, _ = oracle.g2_decompress(bytes.fromhex(g["signature"]))
    msgs = np.stack([np.frombuffer(bytes.fromhex(m), dtype=np.uint8) for m in g["messages"]])
    pk = np.stack([pk1] * 3)
    sig = np.stack([sig1] * 3)
    got, w = _run(pkg, pk, msgs, sig)
    assert got.tolist() == g["expected"]
    _compare(oracle, pk, msgs, sig, got, w, range(3))


def test_verify_fixtures(pkg, oracle):
    # tests/test_cases/verify/*.json: every case whose key and signature decode (the gadget takes decoded points)
    rows = []
    for name, case in eth_cases("verify"):
        i = case["input"]
        st1, pk, inf1 = oracle.g1_decompress(unhex(i["pubkey"]))
        st2, sig, inf2 = oracle.g2_decompress(unhex(i["signature"]))
        if st1 or st2 or inf1 or inf2 or len(unhex(i["message"])) != 32:
            continue
        rows.append((pk, np.frombuffer(unhex(i["message"]), dtype=np.uint8), sig, case["output"]))
    assert len(rows) >= 19  # 9 valid + 9 wrong-pubkey + sk=1 case; tampered signatures do not decode
    pk = np.stack([r[0] for r in rows])
    msg = np.stack([r[1] for r in rows])
    sig = np.stack([r[2] for r in rows])
    got, _ = _run(pkg, pk, msg, sig, want_witness=False)
    assert got.tolist() == [r[3] for r in rows]


def test_edge_inputs(pkg, oracle):
    # identity key / identity signature keep defined values (verify_infinity_pubkey_and_infinity_signature.json)
    pk, msg, sig, _ = synth.make_batch(oracle, 16)
    pk = pk[:3].copy()
    sig = sig[:3].copy()
    msg = msg[:3].copy()
    pk[0] = 0
    sig[0] = 0
    sig[1] = 0
    pk[2] = 0
    got, w = _run(pkg, pk, msg, sig)
    _compare(oracle, pk, msg, sig, got, w, range(3))


@pytest.mark.parametrize("msg_len", [0, 3, 119])
def test_other_message_lengths(pkg, oracle, msg_len):
    pk, _, sig, _ = synth.make_batch(oracle, 16)
    msg = (np.arange(2 * max(msg_len, 1), dtype=np.uint8).reshape(2, -1))[:, :msg_len].copy()
    got, w = _run(pkg, pk[:2].copy(), msg.reshape(2, msg_len), sig[:2].copy())
    _compare(oracle, pk, msg.reshape(2, msg_len), sig, got, w, range(2))


@pytest.mark.parametrize("msg_len", [55, 56, 119, 120, 251, 8, 9, 17, 63, 73])
def test_engine_grouped_padding_boundary_lengths(pkg, oracle, msg_len):
    """The witness path on long and block-boundary messages through the GROUPED engine (staging, streamed expansion and
    placement). msg' = Z_pad || msg || ... of expand_message (hasher.rs:110-173) is 111 bytes longer than the message (sha.hpp: total =
    msg_len + 111), so its SHA-256 block count is (msg_len + 183) / 64 and changes at 8 / 9, 72 / 73, 136 / 137 and 200 / 201 bytes (NOT at
    55 / 56 and 119 / 120, which are the borders of a bare message and stay here as ordinary lengths); the 0x80 byte opens a block of its
    own at msg_len = 17 (mod 64), and the two lib_str witness bytes straddle a block at msg_len = 63 (mod 64). sha_bits, and with it the
    tail shape of the expansion, changes exactly there. 251 bytes is the longest of the reference's own strings (hasher.rs:1006-1012). Two steps of 70
    instances fused into one group (140 lanes: two full waves and a ragged one); valid and tampered signatures; every
    fifth vector and the ragged tail, element by element, against the oracle."""
    import torch

    n, steps = 70, 2
    pk16, _, _, _ = synth.make_batch(oracle, 16)
    sks = [int.from_bytes(synth._h(0x5EED, b"sk", k), "big") % synth.R_MOD or 1 for k in range(16)]
    total = n * steps
    msg = np.stack([np.frombuffer((synth._h(0x5EED, b"pb", i) * 8)[:msg_len], dtype=np.uint8) for i in range(total)]).copy()
    pk = np.stack([pk16[i % 16] for i in range(total)])
    sig = np.zeros((total, 24), dtype=np.uint64)
    signed = {}
    for i in range(total):  # a few distinct valid signatures (CPU hash-to-G2 is the slow part); the rest reuse them on other messages
        j = i % 7
        if j not in signed:
            st, sxy, _ = oracle.g2_decompress(oracle.sign(sks[j % 16], msg[j].tobytes()))
            assert st == 0
            signed[j] = sxy
        sig[i] = signed[j]
    expect = np.array([i < 7 for i in range(total)])  # instance i < 7 carries its own signature under key i % 16 = i
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, msg_len, max_steps=2, device=dev, n_buffers=2)
    outs, ress, keep = [], [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        d = (torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev))
        w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(d[0], d[1], d[2], witness=w, result=r)
        outs.append(w)
        ress.append(r)
        keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect[sl])
        w = outs[k].cpu().numpy().view(np.uint64)
        _compare(oracle, pk[sl], msg[sl], sig[sl], got, w, sorted(set(range(0, n, 5)) | {n - 1, n - 2, 63, 64}))
    eng.close()


def test_engine_grouped_batches(pkg, oracle):
    # engine mode: 5 different batches of 8 instances, fused 3 per launch group (3 + 2: both ping-pong buffers, staging,
    # per-step placement), each with its own witness tensor
    import torch

    n, steps = 8, 5
    pk, msg, sig, expect = synth.make_batch(oracle, n * steps, tamper_every=3)
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=3, device=dev)
    outs, ress, ins = [], [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        d = (torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev))
        w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(d[0], d[1], d[2], witness=w, result=r)
        outs.append(w)
        ress.append(r)
        ins.append(d)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect[sl])
        w = outs[k].cpu().numpy().view(np.uint64)
        _compare(oracle, pk[sl], msg[sl], sig[sl], got, w, range(0, n, 3))
    eng.close()


def test_params_allocated_as_witnesses(pkg, oracle):
    """ParametersVar::new_variable with AllocationMode::Witness (constraints.rs:198-211 takes any mode; the reference's tests use
    Constant): the generator's G1Var::new_variable segment, prepare_g1(-g1) and the variable-point ell of the (-g1, sig) pair.
    Direct mode (70 instances: a full wave and a ragged one, every vector against the oracle), then the grouped engine (staging,
    streamed placement, compact wire form expanded by a second engine), with g2_mode team as well (its staging coordinates move
    the new segments); a gadget built for Constant parameters refuses a Witness ParametersVar."""
    import torch

    dev = torch.device("cuda:0")
    n = 70
    pk, msg, sig, expect = synth.make_batch(oracle, n)
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)

    def compare(got, w, idx, lo=0):
        for i in idx:
            nw, _, r, ow = oracle.witness(pk[lo + i], msg[lo + i].tobytes(), sig[lo + i], params_mode=1)
            assert r == bool(got[i]) and w.shape[1] == nw
            bad = np.nonzero((ow != w[i]).any(axis=1))[0]
            assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (lo + i, bad[0])

    g = pkg.BlsSignatureVerifyGadget(n, 32, device=dev, params_mode="witness")
    assert g.layout["params_mode"] == 1 and g.n_witness == pkg.layout(32)["n_witness"] + 1942 + 7 + 67 * 8 + 2
    res = g.verify(pkg.ParametersVar.new_witness(), pkg.PublicKeyVar.new_witness(t(pk)), t(msg), pkg.SignatureVar.new_witness(t(sig)))
    torch.cuda.synchronize()
    got = res.cpu().numpy().astype(bool)
    assert np.array_equal(got, expect)
    compare(got, g.witness.cpu().numpy().view(np.uint64), range(n))
    with pytest.raises(pkg.BlswError):
        g.verify(pkg.ParametersVar.new_constant(), pkg.PublicKeyVar.new_witness(t(pk)), t(msg), pkg.SignatureVar.new_witness(t(sig)))
    g.engine.close()
    # grouped engine: 3 steps of 20 instances, groups of 2; the last step leaves in compact form and is expanded by a direct-mode engine
    ns, steps = 20, 3
    for opts in (dict(), dict(g2_mode="team")):
        eng = pkg.WitnessEngine(ns, 32, max_steps=2, device=dev, n_buffers=2, params_mode=1, **opts)
        outs, ress, keep = [], [], []
        for k in range(steps):
            sl = slice(k * ns, (k + 1) * ns)
            d = (t(pk[sl]), t(sig[sl]), t(msg[sl]))
            w, r = eng.new_witness_tensor(), torch.empty(ns, dtype=torch.int32, device=dev)
            eng.submit(d[0], d[1], d[2], witness=w, result=r)
            outs.append(w)
            ress.append(r)
            keep.append(d)
        eng.flush()
        torch.cuda.synchronize()
        for k in range(steps):
            got = ress[k].cpu().numpy().astype(bool)
            assert np.array_equal(got, expect[k * ns:(k + 1) * ns])
            compare(got, outs[k].cpu().numpy().view(np.uint64), (0, 7, ns - 1), lo=k * ns)
        eng.close()
    # compact wire form: one step of 64 instances leaves as bit words + staged rows and is expanded by a receiving engine of the same circuit
    eng = pkg.WitnessEngine(64, 32, max_steps=2, device=dev, n_buffers=2, params_mode=1)
    recv = pkg.WitnessEngine(64, 32, max_steps=2, device=dev, n_buffers=1, params_mode=1)
    d = (t(pk[:64]), t(sig[:64]), t(msg[:64]))
    comp, plain = eng.new_compact_buffer(1), eng.new_witness_tensor()
    r1, r2 = torch.empty(64, dtype=torch.int32, device=dev), torch.empty(64, dtype=torch.int32, device=dev)
    eng.submit_compact(d[0], d[1], d[2], comp[0], result=r1)
    eng.submit(d[0], d[1], d[2], witness=plain, result=r2)
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor()
    out.fill_(-1)
    recv.expand_compact(comp[0], out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(r1, r2)
    compare(r2.cpu().numpy().astype(bool), plain.cpu().numpy().view(np.uint64), (5, 63))
    eng.close()
    recv.close()
    with pytest.raises(pkg.BlswError):  # the aggregate and N+1-pair circuits take Constant parameters only
        pkg.WitnessEngine(8, 32, device=dev, n_keys=4, params_mode=1)


def test_hash_to_g2_batch(pkg, oracle):
    import torch

    # instance 0 is the bls.rs:645 literal (32 zero bytes)
    n = 10
    msgs = np.zeros((n, 32), dtype=np.uint8)
    for i in range(1, n):
        msgs[i] = np.frombuffer(synth._h(0x5EED, b"h", i), dtype=np.uint8)
    out = pkg.hash_to_g2_batch(torch.from_numpy(msgs).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy().view(np.uint64)
    assert oracle.g2_compress(out[0]).hex() == LIT["hash_to_g2"]["compressed"]
    for i in range(n):
        c, aff = oracle.hash_to_g2(msgs[i].tobytes())
        assert np.array_equal(aff, out[i])


@pytest.mark.parametrize("msg_len", [32, 55, 120])
def test_hash_to_g2_batch_ragged_multi_wave(pkg, oracle, msg_len):
    """blsw_hash_to_g2_batch over several waves with a ragged tail (n = 200 = 3 full waves + 8 lanes per one-lane kernel, 6 + 16 for
    the two-lane map kernel): every point against the oracle. The value-only kernels (k_map_values, k_cofactor_values: SSWU without
    witnesses, psi-based cofactor clearing) must give the point of hash_to_g2_with_cons (hasher.rs:727-740, :1004-1026)."""
    import torch
    from concurrent.futures import ThreadPoolExecutor

    n = 200
    msgs = np.stack([np.frombuffer((synth._h(0x5EED, b"rg", i) * 4)[:msg_len], dtype=np.uint8) for i in range(n)])
    out = pkg.hash_to_g2_batch(torch.from_numpy(msgs).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy().view(np.uint64)
    with ThreadPoolExecutor(max_workers=8) as ex:
        want = list(ex.map(lambda i: oracle.hash_to_g2(msgs[i].tobytes())[1], range(n)))
    bad = [i for i in range(n) if not np.array_equal(want[i], out[i])]
    assert bad == [], bad[:8]


def test_hash_to_g2_one_million_messages_sampled(pkg, oracle):
    """BASELINE configs[4] at its full size: msg_i = SHA-256(seed || "h" || i) for i < 2^20, message 0 replaced by the 32 zero bytes of
    bls.rs:645, hashed in four chunks of 262 144. A fixed-stride sample of 64 outputs (every chunk, both ends) against the oracle, output 0 against the
    reference's literal, and a size-independent property of the whole batch: the second half re-hashed after a permutation equals the permuted outputs."""
    import torch
    from concurrent.futures import ThreadPoolExecutor

    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    n, chunk = 1 << 20, 1 << 18
    dev = torch.device("cuda:0")
    msgs = workload.messages(0x5EED, 0, n, tag=b"h")
    msgs[0] = 0
    d = torch.from_numpy(msgs).to(dev)
    out = torch.empty((n, 24), dtype=torch.int64, device=dev)
    for c0 in range(0, n, chunk):
        pkg.hash_to_g2_batch(d[c0:c0 + chunk], out=out[c0:c0 + chunk])
    torch.cuda.synchronize()
    sample = sorted(set([0, 1, chunk - 1, chunk, n - 1] + list(range(7, n, n // 59))))
    got = out[sample].cpu().numpy().view(np.uint64)
    with ThreadPoolExecutor(max_workers=8) as ex:
        want = list(ex.map(lambda i: oracle.hash_to_g2(msgs[i].tobytes()), sample))
    bad = [i for k, i in enumerate(sample) if not np.array_equal(want[k][1], got[k])]
    assert bad == [], bad[:8]
    assert want[0][0].hex() == LIT["hash_to_g2"]["compressed"] and bytes(msgs[0]).hex() == LIT["hash_to_g2"]["message"]  # bls.rs:645-651
    perm = torch.randperm(chunk, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    again = pkg.hash_to_g2_batch(d[n - chunk:][perm].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(again, out[n - chunk:][perm])


def test_sign_batch_ragged_multi_wave(pkg, oracle):
    """blsw_sign_batch over several waves (n = 200): sig = sk * H(m) through the four-digit psi ladder and pk = sk * g1 through the
    fixed-base windows (vsign.hpp), scalars with special digit patterns and random ones, against the oracle's signer."""
    import random

    import torch
    from concurrent.futures import ThreadPoolExecutor

    r_mod = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    z = 0xD201000000010000
    rng = random.Random(11)
    n = 200
    sks = [1, 2, 15, 16, z - 1, z, z + 1, z * z, z * z - 1, z ** 3, z ** 3 + z * z + z + 1, r_mod - 1, r_mod - 2, (1 << 254) + 1]
    sks += [rng.randrange(1, r_mod) for _ in range(n - len(sks))]
    msgs = [synth._h(0x5EED, b"sg", i) for i in range(n)]
    sk = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(-1, 32).copy()
    msg = np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(-1, 32).copy()
    r = pkg.sign_batch(torch.from_numpy(sk).cuda(), torch.from_numpy(msg).cuda())
    assert (r["status"].cpu().numpy() == 0).all()
    sig, pk = r["sig96"].cpu().numpy(), r["pk48"].cpu().numpy()
    with ThreadPoolExecutor(max_workers=8) as ex:
        want = list(ex.map(lambda i: (oracle.sign(sks[i], msgs[i]), oracle.sk_to_pk(sks[i])), range(n)))
    bad = [i for i in range(n) if sig[i].tobytes() != want[i][0] or pk[i].tobytes() != want[i][1]]
    assert bad == [], bad[:8]


def test_hash_to_curve_reference_strings(pkg, oracle):
    """hasher.rs:1004-1026 (test_hash_to_curve) on the GPU: the reference's five messages — lengths 0, 3, 7, 23 and 251 bytes,
    i.e. up to five SHA-256 blocks of msg' — through blsw_hash_to_g2_batch, against the frozen oracle outputs."""
    import torch

    frozen = json.load(open(os.path.join(GOLDEN, "oracle_hash_strings.json")))
    for s, want in zip(LIT["hash_strings"], frozen["compressed"]):
        m = np.frombuffer(s.encode("utf-8"), dtype=np.uint8).reshape(1, -1).repeat(3, axis=0).copy()
        out = pkg.hash_to_g2_batch(torch.from_numpy(m).cuda())
        torch.cuda.synchronize()
        out = out.cpu().numpy().view(np.uint64)
        for i in range(3):
            assert oracle.g2_compress(out[i]).hex() == want, "message %r" % s[:24]


def test_decode_and_verify_bytes_fixtures(pkg, oracle):
    """tests/tests.rs:239-268 end to end on the GPU: all 29 verify/*.json cases from their compressed bytes
    (decode kernel -> gadget), plus the deserialization_G1/G2 accept/reject fixtures through the decode kernel."""
    import torch

    cases = [c for _, c in eth_cases("verify")]
    pk = np.stack([np.frombuffer(unhex(c["input"]["pubkey"]), dtype=np.uint8) for c in cases])
    sig = np.stack([np.frombuffer(unhex(c["input"]["signature"]), dtype=np.uint8) for c in cases])
    msg = np.stack([np.frombuffer(unhex(c["input"]["message"]), dtype=np.uint8) for c in cases])
    got = pkg.verify_bytes_batch(torch.from_numpy(pk).cuda(), torch.from_numpy(msg).cuda(), torch.from_numpy(sig).cuda())
    assert got.cpu().numpy().tolist() == [c["output"] for c in cases]
    # decoded coordinates equal the oracle's wherever the point decodes
    pk_xy, sig_xy, status = pkg.decode_batch(torch.from_numpy(pk).cuda(), torch.from_numpy(sig).cuda())
    torch.cuda.synchronize()
    pk_xy, sig_xy, status = pk_xy.cpu().numpy().view(np.uint64), sig_xy.cpu().numpy().view(np.uint64), status.cpu().numpy()
    for i, c in enumerate(cases):
        st, xy, inf = oracle.g1_decompress(unhex(c["input"]["pubkey"]))
        assert (st == 0) == (status[i, 0] in (0, 4))
        if status[i, 0] == 0:
            assert np.array_equal(xy, pk_xy[i])
        st, xy, inf = oracle.g2_decompress(unhex(c["input"]["signature"]))
        assert (st == 0) == (status[i, 1] in (0, 4))
        if status[i, 1] == 0:
            assert np.array_equal(xy, sig_xy[i])
    # accept / reject fixtures with the right length
    g1 = [(unhex(c["input"]["pubkey"]), c["output"]) for _, c in eth_cases("deserialization_G1") if len(unhex(c["input"]["pubkey"])) == 48]
    g2 = [(unhex(c["input"]["signature"]), c["output"]) for _, c in eth_cases("deserialization_G2") if len(unhex(c["input"]["signature"])) == 96]
    m = max(len(g1), len(g2))
    p = np.zeros((m, 48), dtype=np.uint8)
    s = np.zeros((m, 96), dtype=np.uint8)
    p[:, 0] = 0xC0
    s[:, 0] = 0xC0
    for i, (b, _) in enumerate(g1):
        p[i] = np.frombuffer(b, dtype=np.uint8)
    for i, (b, _) in enumerate(g2):
        s[i] = np.frombuffer(b, dtype=np.uint8)
    _, _, st = pkg.decode_batch(torch.from_numpy(p).cuda(), torch.from_numpy(s).cuda())
    st = st.cpu().numpy()
    assert [bool(st[i, 0] in (0, 4)) for i in range(len(g1))] == [o for _, o in g1]
    assert [bool(st[i, 1] in (0, 4)) for i in range(len(g2))] == [o for _, o in g2]


def _agg_run(pkg, pks, bm, msg, sig):
    import torch

    res, cnt, wit = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.from_numpy(pks.view(np.int64)).cuda()),
                                         torch.from_numpy(bm).cuda(), torch.from_numpy(msg).cuda(), pkg.SignatureVar.new_witness(torch.from_numpy(sig.view(np.int64)).cuda()))
    return res.cpu().numpy().astype(bool), cnt.cpu().numpy(), wit.cpu().numpy().view(np.uint64)


def test_aggregate_verify_reference_512_keys(pkg, oracle):
    # constraints.rs:378-521: 512 keys (key1 + 511 x key2); bitmap first two -> true, all -> false. Two instances in one batch.
    pk1 = "a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a"
    pk2 = "b301803f8b5ac4a1133581fc676dfedc60d891dd5fa99028805e5ea5b08d3491af75d0707adab3b70c6a6a580217bf81"
    sigh = "912c3615f69575407db9392eb21fee18fff797eeb2fbe1816366ca2a08ae574d8824dbfafb4c9eaa1cf61b63c6f9b69911f269b664c42947dd1b53ef1081926c1e82bb2a465f927124b08391a5249036146d6f3f1e17ff5f162f779746d830d1"
    _, p1, _ = oracle.g1_decompress(bytes.fromhex(pk1))
    _, p2, _ = oracle.g1_decompress(bytes.fromhex(pk2))
    _, s, _ = oracle.g2_decompress(bytes.fromhex(sigh))
    K = 512
    one = np.stack([p1] + [p2] * (K - 1))
    pks = np.stack([one, one])
    bm = np.zeros((2, K), dtype=np.uint8)
    bm[0, :2] = 1
    bm[1, :] = 1
    msg = np.full((2, 32), 0x56, dtype=np.uint8)
    sig = np.stack([s, s])
    got, cnt, w = _agg_run(pkg, pks, bm, msg, sig)
    assert got.tolist() == [True, False] and cnt.tolist() == [2, 512]
    for i in range(2):
        n, res, c, _, ow = oracle.witness_aggregate(pks[i], bm[i], msg[i].tobytes(), sig[i])
        assert n == w.shape[1] and res == bool(got[i]) and c == cnt[i]
        bad = np.nonzero((ow != w[i]).any(axis=1))[0]
        assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (i, bad[0])


def test_fast_aggregate_verify_fixtures(pkg, oracle):
    # tests/test_cases/fast_aggregate_verify/*.json (tests.rs:296-334) with every key selected
    done = 0
    for name, c in eth_cases("fast_aggregate_verify"):
        i = c["input"]
        pks = [oracle.g1_decompress(unhex(p)) for p in i["pubkeys"]]
        st, sxy, sinf = oracle.g2_decompress(unhex(i["signature"]))
        if not pks or any(p[0] for p in pks) or st or sinf:
            assert c["output"] is False  # undecodable / empty inputs are rejected before the gadget
            continue
        pk = np.stack([p[1] for p in pks])[None]
        bm = np.ones((1, pk.shape[1]), dtype=np.uint8)
        msg = np.frombuffer(unhex(i["message"]), dtype=np.uint8)[None].copy()
        got, cnt, w = _agg_run(pkg, pk, bm, msg, sxy[None])
        assert bool(got[0]) == c["output"] and cnt[0] == pk.shape[1]
        n, res, cc, _, ow = oracle.witness_aggregate(pk[0], bm[0], msg[0].tobytes(), sxy)
        assert np.array_equal(ow, w[0])
        done += 1
    assert done >= 6


def test_native_verify_batch_fixtures_and_gadget_agreement(pkg, oracle):
    """blsw_verify_batch = BLS::verify as values (bls.rs:427-458; vpairing.hpp): all 29 verify/*.json cases from their compressed bytes in ONE call
    (tests/tests.rs:239-268: tampered, wrong-key, infinity and non-subgroup inputs), all 11 fast_aggregate_verify/*.json cases through
    PublicKey::aggregate + verify (tests/tests.rs:296-334: empty list, infinity key, extra key, tampered signature), and on the 1024-instance
    synthetic batch of the bench the verdicts equal the gadget's Booleans (a ragged batch too: 70 instances)."""
    import torch

    dev = torch.device("cuda:0")
    rows = [(name, unhex(c["input"]["pubkey"]), unhex(c["input"]["message"]), unhex(c["input"]["signature"]), c["output"]) for name, c in eth_cases("verify")]
    assert len(rows) == 29 and all(len(r[1]) == 48 and len(r[3]) == 96 and len(r[2]) == 32 for r in rows)
    t = lambda xs, w: torch.from_numpy(np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(len(xs), w).copy()).to(dev)
    res, st = pkg.verify_batch(t([r[1] for r in rows], 48), t([r[2] for r in rows], 32), t([r[3] for r in rows], 96), want_status=True)
    got = res.cpu().numpy().astype(bool).tolist()
    assert got == [r[4] for r in rows], [r[0] for r, g in zip(rows, got) if g != r[4]]
    assert sum(got) >= 9 and got == [oracle.verify_bytes(r[1], r[2], r[3]) for r in rows]
    # fast_aggregate_verify: one call per list length (the lists are ragged)
    done = 0
    for name, c in eth_cases("fast_aggregate_verify"):
        i = c["input"]
        pks = [unhex(p) for p in i["pubkeys"]]
        sig = unhex(i["signature"])
        assert len(sig) == 96 and all(len(p) == 48 for p in pks)
        pk_t = torch.from_numpy(np.frombuffer(b"".join(pks), dtype=np.uint8).reshape(1, len(pks), 48).copy()).to(dev) if pks else torch.zeros((1, 0, 48), dtype=torch.uint8, device=dev)
        r = pkg.fast_aggregate_verify_batch(pk_t, t([unhex(i["message"])], 32), t([sig], 96))
        assert bool(r[0].item()) == c["output"], name
        done += 1
    assert done == 11
    # the synthetic workload: verdict == the gadget's Boolean (every 16th instance is tampered)
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    for n in (1024, 70):
        pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev)
        sk = np.frombuffer(b"".join(workload.secret_keys(0x5EED, 16)[i % 16].to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()
        signed = pkg.sign_batch(torch.from_numpy(sk).to(dev), torch.from_numpy(workload.messages(0x5EED, 0, n)).to(dev))
        r = pkg.verify_batch(signed["pk48"], msg, signed["sig96"]).cpu().numpy().astype(bool)
        eng = pkg.WitnessEngine(n, 32, device=dev)
        g = torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(pk, sig, msg, witness=None, result=g)
        eng.flush()
        torch.cuda.synchronize()
        eng.close()
        assert np.array_equal(r, g.cpu().numpy().astype(bool)) and np.array_equal(r, expect) and 0 < r.sum() < n


def test_sign_batch_fixtures_and_synthetic_workload(pkg, oracle):
    """blsw_sign_batch (bls.rs:411-425, 183-195) against tests/test_cases/sign/*.json, the CPU oracle, and the oracle-built
    synthetic batch of tests/synth.py (the bench's inputs are minted by this entry point)."""
    import torch

    dev = torch.device("cuda:0")
    cases = [c for _, c in eth_cases("sign")]
    r_mod = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    sks = [int.from_bytes(unhex(c["input"]["privkey"]), "big") for c in cases] + [r_mod, r_mod - 1]
    msgs = [unhex(c["input"]["message"]) for c in cases] + [b"\x11" * 32, b"\x22" * 32]
    sk = np.frombuffer(b"".join(s.to_bytes(32, "little") for s in sks), dtype=np.uint8).reshape(-1, 32).copy()
    msg = np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(-1, 32).copy()
    r = pkg.sign_batch(torch.from_numpy(sk).to(dev), torch.from_numpy(msg).to(dev))
    st = r["status"].cpu().numpy()
    sig = r["sig96"].cpu().numpy()
    pk = r["pk48"].cpu().numpy()
    n_zero = 0
    for i, c in enumerate(cases):
        if c["output"] is None:
            assert st[i] == pkg.ST_INVALID_SECRET_KEY and sig[i].tobytes() == bytes([0xC0]) + bytes(95)
            n_zero += 1
        else:
            assert st[i] == 0 and sig[i].tobytes() == unhex(c["output"])
            assert pk[i].tobytes() == oracle.sk_to_pk(sks[i])
    assert n_zero == 1
    assert st[-2] == pkg.ST_BAD_ENCODING and st[-1] == 0
    assert sig[-1].tobytes() == oracle.sign(r_mod - 1, msgs[-1])
    # affine limb outputs == decoding the compressed outputs
    pk_xy, sig_xy, dst = pkg.decode_batch(r["pk48"], r["sig96"])
    ok = st == 0
    assert (dst.cpu().numpy()[ok] == 0).all()
    assert (pk_xy.cpu().numpy()[ok] == r["pk_xy"].cpu().numpy()[ok]).all() and (sig_xy.cpu().numpy()[ok] == r["sig_xy"].cpu().numpy()[ok]).all()
    # the GPU-minted workload equals the oracle-minted one
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    gpk, gmsg, gsig, gexp = workload.make_batch(pkg, 48, seed=0x5EED, device=dev)
    opk, omsg, osig, oexp = synth.make_batch(oracle, 48, seed=0x5EED)
    assert (gpk.cpu().numpy().view(np.uint64) == opk).all() and (gsig.cpu().numpy().view(np.uint64) == osig).all()
    assert (gmsg.cpu().numpy() == omsg).all() and (gexp == oexp).all()


def test_aggregate_points_fixtures_and_batches(pkg, oracle):
    """Signature::aggregate / PublicKey::aggregate on the GPU (bls.rs:288-300, 183-195): the reference's test_sign_aggr over
    tests/test_cases/aggregate/*.json (tests/tests.rs:270-294; the empty list is None), the key sums of fast_aggregate_verify
    (tests/tests.rs:296-334), and ragged multi-wave batches of lists against the oracle — with repeated points (the addition runs into
    its doubling case), P + (-P) (the identity) and lists holding the encoding of the point at infinity; a point that does not decode
    gives its status for the list."""
    import torch

    dev = torch.device("cuda:0")
    t = lambda rows, nbytes: torch.from_numpy(np.frombuffer(b"".join(b"".join(r) for r in rows), dtype=np.uint8).reshape(len(rows), -1, nbytes).copy()).to(dev)
    n_cases = 0
    for name, c in eth_cases("aggregate"):
        sigs = [unhex(x) for x in c["input"]]
        if not sigs:
            assert c["output"] is None and pkg.aggregate_signatures(torch.empty((1, 0, 96), dtype=torch.uint8, device=dev)) is None
            continue
        out, st = pkg.aggregate_signatures(t([sigs], 96))
        assert int(st[0]) == 0 and out[0].cpu().numpy().tobytes() == unhex(c["output"]), name
        n_cases += 1
    assert n_cases == 5
    for name, c in eth_cases("fast_aggregate_verify"):
        pks = [unhex(x) for x in c["input"]["pubkeys"]]
        if not pks:
            continue
        out, st = pkg.aggregate_public_keys(t([pks], 48))
        exp = oracle.aggregate_g1(pks)
        if exp is None:  # a key that does not decode (the infinity encoding decodes)
            assert int(st[0]) != 0
        else:
            assert int(st[0]) == 0 and out[0].cpu().numpy().tobytes() == exp, name
    # batches: 150 lists of 5 (three waves of lists, 750 points), built from 12 distinct signatures / keys
    sks = [int.from_bytes(synth._h(0xA66, b"sk", j), "big") % synth.R_MOD or 1 for j in range(12)]
    sig = [oracle.sign(sk, b"aggregate me") for sk in sks]
    pk = [oracle.sk_to_pk(sk) for sk in sks]
    neg = lambda b: bytes([b[0] ^ 0x20]) + b[1:]  # the other root: -P
    inf2, inf1 = bytes([0xC0]) + bytes(95), bytes([0xC0]) + bytes(47)
    for group, pts, inf, agg, nbytes in ((2, sig, inf2, oracle.aggregate_g2, 96), (1, pk, inf1, oracle.aggregate_g1, 48)):
        rows = []
        for i in range(150):
            row = [pts[(i * 7 + 3 * j) % 12] for j in range(5)]
            if i % 10 == 1:
                row[2] = row[0]  # P + ... + P: doubling inside the mixed addition
            if i % 10 == 2:
                row = [row[0], neg(row[0]), inf, row[0], neg(row[0])]  # the identity
            if i % 10 == 3:
                row[4] = inf
            rows.append(row)
        out, st = pkg.aggregate_points(group, t(rows, nbytes))
        assert (st.cpu().numpy() == 0).all()
        got = out.cpu().numpy()
        for i in range(150):
            assert got[i].tobytes() == agg(rows[i]), "group %d list %d" % (group, i)
        assert got[2].tobytes() == inf
        # a point that is not on the curve / not in the subgroup: the list's status names it, the others are unaffected
        bad = bytearray(rows[5][3])
        bad[-1] ^= 1
        rows[5][3] = bytes(bad)
        out2, st2 = pkg.aggregate_points(group, t(rows, nbytes))
        st2 = st2.cpu().numpy()
        assert st2[5] in (pkg.ST_NOT_ON_CURVE, pkg.ST_NOT_IN_SUBGROUP, pkg.ST_BAD_ENCODING) and (np.delete(st2, 5) == 0).all()
        assert agg(rows[5]) is None and (np.delete(out2.cpu().numpy(), 5, axis=0) == np.delete(got, 5, axis=0)).all()


def test_gpu_matches_oracle_emitted_digests(pkg, oracle):
    """ORACLE-vs-GPU (T2), not a T3 check: tests/golden/witness_digests.json was emitted by this repository's own oracle
    (tests/golden/gen_oracle_vectors.py), so it pins the GPU to the oracle, not to real arkworks — the witness ORDER of real
    arkworks stays unpinned until tools/t3_dumper is run by someone with cargo. What it adds over the
    element-wise tests: the committed file freezes the oracle's output across rounds (SHA-256 of every witness vector and of its
    Miller-loop segment for the valid verify fixtures and the reference gadget case; inputs decoded from the compressed fixture
    bytes on the GPU)."""
    import hashlib

    import torch

    gold = json.load(open(os.path.join(GOLDEN, "witness_digests.json")))
    names = list(gold["cases"])
    dev = torch.device("cuda:0")
    pk48 = torch.tensor(np.frombuffer(b"".join(bytes.fromhex(gold["cases"][k]["pubkey"]) for k in names), dtype=np.uint8).reshape(-1, 48).copy(), device=dev)
    sig96 = torch.tensor(np.frombuffer(b"".join(bytes.fromhex(gold["cases"][k]["signature"]) for k in names), dtype=np.uint8).reshape(-1, 96).copy(), device=dev)
    msg = torch.tensor(np.frombuffer(b"".join(bytes.fromhex(gold["cases"][k]["message"]) for k in names), dtype=np.uint8).reshape(-1, 32).copy(), device=dev)
    pk_xy, sig_xy, st = pkg.decode_batch(pk48, sig96)
    assert int(st.abs().sum().item()) == 0
    g = pkg.BlsSignatureVerifyGadget(len(names), 32, device=dev)
    res = g.verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pk_xy), msg, pkg.SignatureVar.new_witness(sig_xy))
    torch.cuda.synchronize()
    w = g.witness.cpu().numpy().view(np.uint8).reshape(len(names), -1, 48)
    lo, hi = gold["segments"][-3][1], gold["segments"][-3][2]
    for i, k in enumerate(names):
        c = gold["cases"][k]
        assert w.shape[1] == c["n_witness"] and bool(res[i].item()) == c["result"]
        assert hashlib.sha256(w[i].tobytes()).hexdigest() == c["sha256_all"], k
        assert hashlib.sha256(w[i, lo:hi].tobytes()).hexdigest() == c["sha256_segments"]["miller"], k


def test_engine_ragged_tiles(pkg, oracle):
    """Grouped engine with N = 2 x 70 lanes: staging tiles of 64 instances and pairing waves of 10 instances are both ragged
    and straddled by the two batches; instances around every boundary are compared element by element with the oracle."""
    import torch

    n, steps = 70, 2
    pk, msg, sig, expect = synth.make_batch(oracle, 64, tamper_every=5)
    reps = (n * steps + 63) // 64
    pk, msg, sig, expect = np.tile(pk, (reps, 1))[: n * steps], np.tile(msg, (reps, 1))[: n * steps], np.tile(sig, (reps, 1))[: n * steps], np.tile(expect, reps)[: n * steps]
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev)
    outs, ress = [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev), witness=w, result=r)
        outs.append(w)
        ress.append(r)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect[sl])
        w = outs[k].cpu().numpy().view(np.uint64)
        # lanes 63|64 (tile edge in batch 0), 69|70 (batch edge), 127|128 (tile edge in batch 1 = local 57|58), last lane
        idx = [0, 9, 10, 63, 64, 69] if k == 0 else [0, 57, 58, 59, 60, 69]
        _compare(oracle, pk[sl], msg[sl], sig[sl], got, w, idx)
    eng.close()


def test_engine_results_only(pkg, oracle):
    """Grouped engine without witness tensors (value-only emitters, no SHA bit pass, no placement): gadget results only."""
    import torch

    n, steps = 16, 3
    pk, msg, sig, expect = synth.make_batch(oracle, n * steps, tamper_every=4)
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev)
    ress = []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev), witness=None, result=r)
        ress.append(r)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        assert np.array_equal(ress[k].cpu().numpy().astype(bool), expect[k * n:(k + 1) * n])
    eng.close()


def _grouped(pkg, oracle, n, steps, max_steps, check_idx, tamper_every=3, n_buffers=None, **options):
    """n * steps distinct instances through the grouped engine (one witness tensor per step); instances check_idx(k) of
    every step are compared element by element with the oracle, all results with the expected booleans."""
    import torch

    pk, msg, sig, expect = synth.make_batch(oracle, n * steps, tamper_every=tamper_every)
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=max_steps, device=dev, n_buffers=n_buffers, **options)
    outs, ress, keep = [], [], []
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        d = (torch.from_numpy(pk[sl].view(np.int64)).to(dev), torch.from_numpy(sig[sl].view(np.int64)).to(dev), torch.from_numpy(msg[sl]).to(dev))
        w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
        assert eng.submit(d[0], d[1], d[2], witness=w, result=r) == k
        outs.append(w)
        ress.append(r)
        keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    assert eng.submitted() == eng.launched() == steps
    for k in range(steps):
        sl = slice(k * n, (k + 1) * n)
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect[sl])
        idx = list(check_idx(k))
        w = outs[k][idx].cpu().numpy().view(np.uint64)
        for a, i in enumerate(idx):
            nw, _, r, ow = oracle.witness(pk[sl][i], msg[sl][i].tobytes(), sig[sl][i])
            assert r == bool(got[i]) and nw == w.shape[1]
            bad = np.nonzero((ow != w[a]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
    eng.close()


@pytest.mark.parametrize("options", [dict(g2_mode="team"), dict(pairing_mode="lane"), dict(expand_store=1, prio_mode=0)])
def test_engine_mode_options(pkg, oracle, options):
    """Kernel variants are engine-creation options (blsw_engine_options_t), not process state: the six-lane G2 allocation
    (its segment staged instance-major at the end of the staging coordinates), the single-lane pairing kernel and the
    store / priority knobs, each through the grouped engine with ragged tiles."""
    _grouped(pkg, oracle, 70, 2, 2, lambda k: [0, 9, 63, 64, 69] if k == 0 else [0, 57, 58, 69], tamper_every=5, **options)
    got, w = _run(pkg, *synth.make_batch(oracle, 70)[:3], **options)
    pk, msg, sig, expect = synth.make_batch(oracle, 70)
    assert np.array_equal(got, expect)
    _compare(oracle, pk, msg, sig, got, w, [0, 15, 63, 64, 69])


def test_lane_pairing_with_many_buffers_is_refused(pkg):
    """The single-lane pairing kernel's 9.7 KB stack x 64 lanes x wave slots per queue used to abort the process with
    HSA_STATUS_ERROR_OUT_OF_RESOURCES at >= 4 group buffers: blsw_engine_create_ex now returns BLSW_ERR_SCRATCH."""
    with pytest.raises(pkg.BlswError, match="5"):
        pkg.WitnessEngine(64, 32, max_steps=2, n_buffers=4, pairing_mode="lane")
    pkg.WitnessEngine(64, 32, max_steps=2, n_buffers=2, pairing_mode="lane").close()


def test_engine_1024_instances_grouped(pkg, oracle):
    """BASELINE configs[1] shape: batches of 1024 instances, grouped (max_steps = 2, three steps: a full group and a partial
    one). All 3072 results, and 18 instances spread over staging tiles / pairing waves / steps compared with the oracle on
    every one of their 707 427 witness elements."""
    import torch

    n, steps = 1024, 3
    pick = {0: [0, 63, 64, 500, 1009, 1023], 1: [0, 1, 639, 640, 777, 1023], 2: [5, 64, 127, 128, 1000, 1023]}
    # inputs minted by the product's signer (checked against the oracle's in test_sign_batch_...), expectations from its tamper rule
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2)
    outs = [eng.new_witness_tensor() for _ in range(steps)]
    ress, ins = [], []
    for k in range(steps):
        pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=k * n)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit(pk, sig, msg, witness=outs[k], result=r)
        ress.append(r)
        ins.append((pk, msg, sig, expect))
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        pk, msg, sig, expect = ins[k]
        got = ress[k].cpu().numpy().astype(bool)
        assert np.array_equal(got, expect)
        hp, hm, hs = pk.cpu().numpy().view(np.uint64), msg.cpu().numpy(), sig.cpu().numpy().view(np.uint64)
        w = outs[k][pick[k]].cpu().numpy().view(np.uint64)
        for a, i in enumerate(pick[k]):
            nw, _, r, ow = oracle.witness(hp[i], hm[i].tobytes(), hs[i])
            assert r == bool(got[i]) and nw == w.shape[1]
            bad = np.nonzero((ow != w[a]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
    eng.close()


def test_engine_bench_shape_against_oracle(pkg, oracle):
    """The engine shape bench.py times (BASELINE configs[1]): 1024 instances per step, launch groups of up to 10 steps (25 steps are
    balanced into 9 + 8 + 8), 3 group buffers, a ring of TWO output tensors, free running, 25 steps of DISTINCT batches. What the ring
    holds afterwards — steps 23 and 24 — against the oracle on every witness element of seven sampled instances per tensor (staging
    tile edges, pairing-wave edges), and all 25 x 1024 results against the tamper rule."""
    import torch

    bench_spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(bench_spec)
    bench_spec.loader.exec_module(bench)
    n, steps, ring = 1024, 25, 2
    coalesce = bench.balanced_coalesce(steps, 10)
    assert coalesce == 9
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=coalesce, device=dev, n_buffers=3)
    outs = [eng.new_witness_tensor() for _ in range(ring)]
    for o in outs:
        o.fill_(-1)
    ins, ress = [], []
    for k in range(steps):
        pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=(7 + k) * n)
        ins.append((pk, msg, sig, expect))
        ress.append(torch.empty(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    for k in range(steps):
        eng.submit(ins[k][0], ins[k][2], ins[k][1], witness=outs[k % ring], result=ress[k])
    eng.flush()
    torch.cuda.synchronize()
    assert eng.launched() == steps and eng.materialised() == steps
    for k in range(steps):
        assert np.array_equal(ress[k].cpu().numpy().astype(bool), ins[k][3]), "results of step %d" % k
    pick = [0, 63, 64, 127, 639, 640, 1023]
    for k in (steps - 2, steps - 1):
        pk, msg, sig, _ = ins[k]
        hp, hm, hs = pk.cpu().numpy().view(np.uint64), msg.cpu().numpy(), sig.cpu().numpy().view(np.uint64)
        w = outs[k % ring][pick].cpu().numpy().view(np.uint64)
        for a, i in enumerate(pick):
            nw, _, r, ow = oracle.witness(hp[i], hm[i].tobytes(), hs[i])
            assert nw == w.shape[1] and r == bool(ins[k][3][i])
            bad = np.nonzero((ow != w[a]).any(axis=1))[0]
            assert len(bad) == 0, "ring tensor %d (step %d) instance %d: first mismatching witness index %d" % (k % ring, k, i, bad[0])
    eng.close()


@pytest.mark.parametrize("msg_len", [32, 3])
def test_expansion_geometries_bit_exact(pkg, oracle, msg_len):
    """Every store geometry of the SHA expansion (options.expand_variant 1 .. 13: one piece per thread in 4 / 8 / 16 KiB chunks, 768-thread variants, scalar
    bit words, the light instruction stream at 8 / 16 / 32 pieces per thread) and the canonical output form through the light kernel write the tensors
    of the default engine, byte for byte; one instance per message length against the oracle. 70 instances (a ragged tile), two steps, two message lengths (different segment alignments and tail workgroups)."""
    import torch

    n = 70
    pk, _, _, _ = synth.make_batch(oracle, n)
    rng = np.random.default_rng(5 + msg_len)
    msg = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    dev = torch.device("cuda:0")
    # signatures need not verify: the witness bytes are what is compared (every 16th instance of make_batch is tampered anyway)
    _, _, sig, _ = synth.make_batch(oracle, n)
    d_pk, d_sig, d_msg = (torch.from_numpy(pk.view(np.int64)).to(dev), torch.from_numpy(sig.view(np.int64)).to(dev), torch.from_numpy(msg).to(dev))
    side = torch.cuda.Stream(device=dev)

    def run(**opts):
        eng = pkg.WitnessEngine(n, msg_len, max_steps=2, device=dev, n_buffers=2, **opts)
        outs = [eng.new_witness_tensor() for _ in range(2)]
        res = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
        for o in outs:
            o.fill_(-1)
        torch.cuda.synchronize()
        for k in range(2):
            eng.submit(d_pk, d_sig, d_msg, witness=outs[k], result=res[k], stream=side)
        eng.flush(stream=side)
        torch.cuda.synchronize()
        eng.close()
        return outs, res

    ref, ref_res = run()
    assert torch.equal(ref[0], ref[1])
    nw, _, r, ow = oracle.witness(pk[69], msg[69].tobytes(), sig[69])
    assert nw == ref[0].shape[1] and np.array_equal(ref[0][69].cpu().numpy().view(np.uint64), ow) and bool(ref_res[0][69].item()) == r
    for variant in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13):
        got, res = run(expand_variant=variant)
        for k in range(2):
            assert torch.equal(got[k], ref[k]), "expand_variant %d, step %d" % (variant, k)
            assert torch.equal(res[k], ref_res[k])
        del got
    for store in (1, 2, 3):  # nontemporal / sc1 / sc0 sc1 stores of the default geometry
        got, res = run(expand_store=store)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), "expand_store %d" % store
        del got
    canon_ref, _ = run(output_form=1)
    canon, _ = run(output_form=1, expand_variant=10)
    assert torch.equal(canon[0], canon_ref[0]) and not torch.equal(canon_ref[0], ref[0])


def test_verify_mixed_message_lengths(pkg, oracle):
    """verify_mixed_lengths: one batch whose messages have lengths 0, 3, 32, 32, 119, 120, 32 (constraints.rs:90-95 takes any &[UInt8]): grouped by
    length, one engine per length; every instance's result and whole witness vector against the oracle, in the caller's order."""
    import torch

    lens = [0, 3, 32, 32, 119, 120, 32]
    sks = [0x1234567 + 977 * i for i in range(len(lens))]
    msgs = [bytes((37 * i + 11 * j) & 0xFF for j in range(L)) for i, L in enumerate(lens)]
    pk = np.stack([oracle.g1_decompress(oracle.sk_to_pk(sk))[1] for sk in sks])
    sig = np.stack([oracle.g2_decompress(oracle.sign(sk, m))[1] for sk, m in zip(sks, msgs)])
    sent = list(msgs)
    sent[3] = bytes([sent[3][0] ^ 1]) + sent[3][1:]  # a tampered 32-byte message: false
    dev = torch.device("cuda:0")
    res, wit = pkg.verify_mixed_lengths(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.from_numpy(pk.view(np.int64)).to(dev)), sent,
                                        pkg.SignatureVar.new_witness(torch.from_numpy(sig.view(np.int64)).to(dev)))
    got = res.cpu().numpy().astype(bool)
    assert got.tolist() == [True, True, True, False, True, True, True]
    for i, m in enumerate(sent):
        nw, _, r, ow = oracle.witness(pk[i], m, sig[i])
        assert r == bool(got[i]) and tuple(wit[i].shape) == (nw, 6) and nw == pkg.layout(len(m))["n_witness"]
        assert np.array_equal(wit[i].cpu().numpy().view(np.uint64), ow), "instance %d (message length %d)" % (i, len(m))


def test_direct_calls_refuse_batches_beyond_free_hbm(pkg):
    """verify_multi / aggregate_verify / the gadget allocate n witness vectors per call (4.19 GB each at 128 pairs): a batch beyond the free
    HBM is refused with a BlswError that says so, before anything is allocated (round 3: torch.OutOfMemoryError half-way)."""
    import torch

    dev = torch.device("cuda:0")
    free0, _ = torch.cuda.mem_get_info(dev)
    n, K = 96, 128  # 96 x 4.19 GB = 402 GB
    pks = torch.zeros((n, K, 12), dtype=torch.int64, device=dev)
    msgs = torch.zeros((n, K, 32), dtype=torch.uint8, device=dev)
    sig = torch.zeros((n, 24), dtype=torch.int64, device=dev)
    with pytest.raises(pkg.BlswError, match="GB of HBM"):
        pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), msgs, pkg.SignatureVar.new_witness(sig))
    n2, K2 = 4096, 512  # 4096 x 82.8 MB = 339 GB
    with pytest.raises(pkg.BlswError, match="GB of HBM"):
        pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.zeros((n2, K2, 12), dtype=torch.int64, device=dev)),
                             torch.ones((n2, K2), dtype=torch.uint8, device=dev), torch.zeros((n2, 32), dtype=torch.uint8, device=dev),
                             pkg.SignatureVar.new_witness(torch.zeros((n2, 24), dtype=torch.int64, device=dev)))
    with pytest.raises(pkg.BlswError, match="GB of HBM"):
        pkg.BlsSignatureVerifyGadget(16384, 32, device=dev)  # 16 384 x 34 MB = 556 GB
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info(dev)
    assert free1 > free0 - (2 << 30)  # nothing of the refused calls stayed allocated


def test_release_table_full_is_busy_and_nothing_is_queued(pkg):
    """Consumer mode with more distinct outputs than the release table holds (64): every accepted step reserves its output's slot when it is
    submitted, so the 65th distinct output is refused with BUSY BEFORE anything is queued or launched (round 3: the group was launched
    and the step counted, then the call failed) — and goes through once an output has been released."""
    import torch

    n = 2
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=40)
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, consumer_mode=1)
    outs = [eng.new_witness_tensor() for _ in range(66)]
    res = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(66)]
    for k in range(64):
        eng.submit(pk, sig, msg, witness=outs[k], result=res[k])
    assert eng.submitted() == 64 and eng.launched() == 64 and eng.materialised() == 64
    with pytest.raises(pkg.BlswBusy):
        eng.submit(pk, sig, msg, witness=outs[64], result=res[64])
    assert eng.submitted() == 64 and eng.launched() == 64  # nothing taken, nothing launched
    with pytest.raises(pkg.BlswBusy):
        eng.output_consumed(outs[65])  # an output the engine has never seen needs a slot too
    eng.wait_step(0)
    eng.output_consumed(outs[0])
    torch.cuda.synchronize()  # the release has completed: its slot is recycled
    eng.submit(pk, sig, msg, witness=outs[64], result=res[64])
    eng.output_consumed(outs[1])
    torch.cuda.synchronize()
    eng.submit(pk, sig, msg, witness=outs[65], result=res[65])
    eng.flush()
    torch.cuda.synchronize()
    assert eng.submitted() == 66 and eng.materialised() == 66
    d = [pkg.witness_digest(outs[k]).cpu().numpy() for k in (0, 63, 64, 65)]
    assert all(np.array_equal(d[0], x) for x in d[1:]) and d[0].any()
    for k in (0, 63, 64, 65):
        assert np.array_equal(res[k].cpu().numpy().astype(bool), expect)
    eng.close()


def test_engine_compact_form_round_trip(pkg, oracle):
    """The compact wire form of a step (blsw_engine_submit_compact: bit-packed SHA witnesses + staged field witnesses, what the
    multi-GPU all-gather ships) expanded on the 'receiver' (blsw_engine_expand_compact, here a SECOND engine) gives bit for bit
    the witness tensor blsw_engine_submit writes: three steps with distinct inputs (a full group of two and a partial one),
    compact and plain submits mixed in one group; one instance per step also against the oracle."""
    import torch

    n, steps = 128, 3
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2)
    recv = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=1)  # the receiving rank's engine
    assert recv.compact_bytes() == eng.compact_bytes() and eng.compact_bytes() < 0.08 * n * eng.n_witness * 48
    plain = [eng.new_witness_tensor() for _ in range(steps)]
    comp = eng.new_compact_buffer(steps)
    ins, r_plain, r_comp = [], [], []
    for k in range(steps):
        pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=1000 + k * n)
        ins.append((pk, msg, sig, expect))
        r_plain.append(torch.empty(n, dtype=torch.int32, device=dev))
        r_comp.append(torch.empty(n, dtype=torch.int32, device=dev))
    # group 1: [compact 0, plain 0]; group 2: [compact 1, compact 2]; group 3: [plain 1, plain 2]
    eng.submit_compact(ins[0][0], ins[0][2], ins[0][1], comp[0], result=r_comp[0])
    eng.submit(ins[0][0], ins[0][2], ins[0][1], witness=plain[0], result=r_plain[0])
    eng.submit_compact(ins[1][0], ins[1][2], ins[1][1], comp[1], result=r_comp[1])
    eng.submit_compact(ins[2][0], ins[2][2], ins[2][1], comp[2], result=r_comp[2])
    eng.submit(ins[1][0], ins[1][2], ins[1][1], witness=plain[1], result=r_plain[1])
    eng.submit(ins[2][0], ins[2][2], ins[2][1], witness=plain[2], result=r_plain[2])
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor()
    for k in range(steps):
        out.fill_(-1)
        recv.expand_compact(comp[k], out)
        torch.cuda.synchronize()
        assert torch.equal(out, plain[k]), "step %d: expanded compact form differs from the plain witness tensor" % k
        assert torch.equal(r_comp[k], r_plain[k]) and np.array_equal(r_plain[k].cpu().numpy().astype(bool), ins[k][3])
        i = (17, 64, 127)[k]
        pk, msg, sig, _ = ins[k]
        nw, _, r, ow = oracle.witness(pk[i].cpu().numpy().view(np.uint64), msg[i].cpu().numpy().tobytes(), sig[i].cpu().numpy().view(np.uint64))
        assert nw == out.shape[1] and np.array_equal(ow, out[i].cpu().numpy().view(np.uint64))
    with pytest.raises(pkg.BlswError):
        pkg.WitnessEngine(n, 32, max_steps=1, device=dev, n_buffers=1).compact_bytes()  # direct mode stages nothing
    eng.close()
    recv.close()


@pytest.mark.parametrize("ramp", [0, 1])
def test_engine_consumer_mode_small_ring(pkg, oracle, ramp):
    """options.consumer_mode = 1: ten steps of 64 instances in groups of four through a ring of TWO output tensors (fewer than
    one group): a step is written into its tensor only after the consumer released the previous user of that tensor, so every
    step's digests must equal those of a free-running engine that had ten separate tensors. The consumer is the digest
    kernel on its own stream; submit returning BUSY is answered by draining. ramp = 1: options.group_ramp — the first groups are
    2 and 4 steps (the group of 2 is launched by the second submit), same bytes."""
    import torch

    n, steps, ring = 64, 10, 2
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    ins = [workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=5000 + k * n) for k in range(steps)]
    # reference: free running, one tensor per step
    ref = pkg.WitnessEngine(n, 32, max_steps=4, device=dev, n_buffers=2)
    ref_out = [ref.new_witness_tensor() for _ in range(steps)]
    ref_res = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(steps)]
    for k in range(steps):
        ref.submit(ins[k][0], ins[k][2], ins[k][1], witness=ref_out[k], result=ref_res[k])
    ref.flush()
    torch.cuda.synchronize()
    want = [pkg.witness_digest(t).cpu().numpy().copy() for t in ref_out]
    ref.close()
    del ref_out
    torch.cuda.empty_cache()
    # consumer mode, ring of two
    eng = pkg.WitnessEngine(n, 32, max_steps=4, device=dev, n_buffers=2, consumer_mode=1, group_ramp=ramp)
    outs = [eng.new_witness_tensor() for _ in range(ring)]
    res = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(steps)]
    got = [torch.empty((n, 2), dtype=torch.int64, device=dev) for _ in range(steps)]
    consumer = torch.cuda.Stream(device=dev)
    state = {"next": 0, "busy": 0}
    launched_after = []

    def drain():
        while state["next"] < eng.materialised():
            s = state["next"]
            eng.wait_step(s, consumer)
            pkg.witness_digest(outs[s % ring], out=got[s], stream=consumer)
            eng.output_consumed(outs[s % ring], consumer)
            state["next"] += 1

    for k in range(steps):
        while True:
            try:
                eng.submit(ins[k][0], ins[k][2], ins[k][1], witness=outs[k % ring], result=res[k])
                break
            except pkg.BlswBusy:
                state["busy"] += 1
                before = state["next"]
                drain()
                assert state["next"] > before, "BUSY with nothing to drain"
        launched_after.append(eng.launched())
        drain()
    eng.flush()
    while state["next"] < steps:
        before = state["next"]
        drain()
        assert state["next"] > before
    assert eng.materialised() == steps
    assert launched_after == ([0, 2, 2, 2, 2, 6, 6, 6, 6, 10] if ramp else [0, 0, 0, 4, 4, 4, 4, 8, 8, 8])
    with pytest.raises(pkg.BlswError):
        eng.wait_step(steps)  # not submitted
    consumer.synchronize()
    torch.cuda.synchronize()
    for k in range(steps):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), "step %d: digests differ from the free-running engine's" % k
        assert torch.equal(res[k], ref_res[k]) and np.array_equal(res[k].cpu().numpy().astype(bool), ins[k][3])
    eng.close()


def test_engine_canonical_output_form(pkg, oracle):
    """options.output_form = 1: every witness element as the canonical integer (48 bytes little-endian, CanonicalSerialize of an
    Fq) instead of Montgomery form. For a grouped engine, a direct-mode engine and an expanded compact batch: canonical * 2^384
    mod p == the Montgomery element of the default engine, for every one of the 707 427 elements of two instances; booleans are
    0 / 1."""
    import torch

    P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    R = (1 << 384) % P
    n = 64
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    pk, msg, sig, expect = workload.make_batch(pkg, n, seed=0x5EED, device=dev, start=9000)

    def ints(rows):  # [k, 6] uint64 -> python ints
        return [sum(int(v) << (64 * i) for i, v in enumerate(r)) for r in rows]

    mont = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2)
    canon = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, output_form=1)
    wm, wc, wx = mont.new_witness_tensor(), canon.new_witness_tensor(), canon.new_witness_tensor()
    cb = mont.new_compact_buffer(1)
    rm, rc = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    mont.submit(pk, sig, msg, witness=wm, result=rm)
    mont.submit_compact(pk, sig, msg, cb[0])
    canon.submit(pk, sig, msg, witness=wc, result=rc)
    mont.flush()
    canon.flush()
    torch.cuda.synchronize()
    canon.expand_compact(cb[0], wx)  # a Montgomery engine's compact batch expanded by a canonical engine
    torch.cuda.synchronize()
    assert torch.equal(rm, rc) and torch.equal(wc, wx)
    lay = pkg.layout(32)
    for i in (0, 37):
        m = ints(wm[i].cpu().numpy().view(np.uint64))
        c = ints(wc[i].cpu().numpy().view(np.uint64))
        assert all(x < P for x in c)
        bad = [k for k in range(len(m)) if c[k] * R % P != m[k]]
        assert not bad, "instance %d: first element whose canonical form is wrong: %d" % (i, bad[0])
        seg = c[lay["off_expand"]:lay["off_expand"] + lay["sha_bits"]]
        assert set(seg) <= {0, 1} and 0 < sum(seg) < len(seg)
    mont.close()
    canon.close()
    # direct mode (one step per launch, the chains write in place)
    direct = pkg.WitnessEngine(4, 32, max_steps=1, device=dev, n_buffers=1, output_form=1)
    wd = direct.new_witness_tensor()
    direct.submit(pk[:4].contiguous(), sig[:4].contiguous(), msg[:4].contiguous(), witness=wd)
    direct.flush()
    torch.cuda.synchronize()
    assert torch.equal(wd[0], wc[0]) and torch.equal(wd[3], wc[3])
    direct.close()


def test_witness_digest_kernel(pkg, oracle):
    """blsw_witness_digest against its host-side definition on real witness vectors (ragged: stride > n_witness)."""
    import torch

    pk, msg, sig, _ = synth.make_batch(oracle, 16)
    got, w = _run(pkg, pk[:3], msg[:3], sig[:3])
    dev = torch.device("cuda:0")
    nw = w.shape[1]
    padded = torch.zeros((3, nw + 5, 6), dtype=torch.int64, device=dev)
    padded[:, :nw] = torch.from_numpy(w.view(np.int64)).to(dev)
    padded[:, nw:] = 0x7777
    d = pkg.witness_digest(padded, n_witness=nw).cpu().numpy().view(np.uint64)
    for i in range(3):
        assert d[i].tolist() == pkg.witness_digest_reference(w[i])
    # a single flipped bit anywhere changes both words
    padded[1, nw // 2, 3] ^= 1
    d2 = pkg.witness_digest(padded, n_witness=nw).cpu().numpy().view(np.uint64)
    assert d2[0].tolist() == d[0].tolist() and d2[1, 0] != d[1, 0] and d2[1, 1] != d[1, 1]


def _multi_run(pkg, pks, msgs, sig):
    import torch

    res, wit = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.from_numpy(pks.view(np.int64)).cuda()), torch.from_numpy(msgs).cuda(),
                                pkg.SignatureVar.new_witness(torch.from_numpy(sig.view(np.int64)).cuda()))
    return res.cpu().numpy().astype(bool), wit


def test_verify_multi_small(pkg, oracle):
    """N+1-pair product (BASELINE configs[3]) at K = 1, 2, 3: K = 1 equals the single-key circuit; a batch of three K = 2
    instances (one with a tampered message); every witness element against the oracle."""
    pk, msg, sig, expect = synth.make_batch(oracle, 16)
    got, wit = _multi_run(pkg, pk[3:4, None, :].copy(), msg[3:4, None, :].copy(), sig[3:4].copy())
    n, _, r, ow = oracle.witness(pk[3], msg[3].tobytes(), sig[3])
    assert got.tolist() == [True] and np.array_equal(wit[0].cpu().numpy().view(np.uint64), ow)
    for K, tampers in ((2, [None, 1, None]), (3, [0, None])):
        cases = [synth.make_multi(oracle, K, tamper=t, start=7 * a) for a, t in enumerate(tampers)]
        pks = np.stack([c[0] for c in cases])
        msgs = np.stack([c[1] for c in cases])
        sigs = np.stack([c[2] for c in cases])
        got, wit = _multi_run(pkg, pks, msgs, sigs)
        assert got.tolist() == [c[3] for c in cases]
        for i, c in enumerate(cases):
            n, res, _, ow = oracle.witness_multi(c[0], c[1], c[2])
            w = wit[i].cpu().numpy().view(np.uint64)
            assert n == w.shape[0] and res == c[3]
            bad = np.nonzero((ow != w).any(axis=1))[0]
            assert len(bad) == 0, "K=%d instance %d: first mismatching witness index %d" % (K, i, bad[0])


def test_verify_multi_pair_parallel_batch(pkg, oracle):
    """The pair-parallel Miller product (miller_par.hpp; K >= 8) on a BATCH: three instances of K = 20 pairs (two chunks of 12 and
    8 pairs; one instance with a tampered message) — every witness element of every instance against the oracle."""
    K = 20
    cases = [synth.make_multi(oracle, K, tamper=t, start=11 * a) for a, t in enumerate([None, 13, None])]
    got, wit = _multi_run(pkg, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]))
    assert got.tolist() == [c[3] for c in cases]
    for i, c in enumerate(cases):
        n, res, _, ow = oracle.witness_multi(c[0], c[1], c[2])
        w = wit[i].cpu().numpy().view(np.uint64)
        assert n == w.shape[0] and res == c[3]
        bad = np.nonzero((ow != w).any(axis=1))[0]
        assert len(bad) == 0, "instance %d: first mismatching witness index %d" % (i, bad[0])


@pytest.mark.parametrize("K,tamper", [(7, None), (8, 5), (12, 0), (13, None)])
def test_verify_multi_at_the_chunk_borders(pkg, oracle, K, tamper):
    """The product at the borders of the pair-parallel path, one instance each: K = 7 (the largest K of the serial team chain), K = 8
    (BLSW_MILLER_PAR_MIN_PAIRS: one chunk, no prefix Q[k][c] is ever stored), K = 12 (one full chunk), K = 13 (a second chunk of one
    pair) — every witness element against the oracle; the oracle's seconds are printed."""
    import time

    c = synth.make_multi(oracle, K, tamper=tamper, start=3 * K)
    got, wit = _multi_run(pkg, c[0][None].copy(), c[1][None].copy(), c[2][None].copy())
    assert got.tolist() == [c[3]] and c[3] == (tamper is None)
    t0 = time.time()
    n, res, _, ow = oracle.witness_multi(c[0], c[1], c[2])
    print("K=%d: oracle.witness_multi %.2f s" % (K, time.time() - t0))
    w = wit[0].cpu().numpy().view(np.uint64)
    assert n == w.shape[0] and res == c[3]
    bad = np.nonzero((ow != w).any(axis=1))[0]
    assert len(bad) == 0, "K=%d: first mismatching witness index %d" % (K, bad[0])


@pytest.mark.parametrize("K,n,consumer", [(3, 2, 0), (20, 3, 0), (20, 2, 1)])
def test_engine_multi_grouped(pkg, oracle, K, n, consumer):
    """The N+1-pair product through the GROUPED engine (options.n_pairs = K; blsw_engine_submit_multi): pair tiles, instance tiles and
    instance-major rows staged per group, expansion of K SHA segments per instance and placement per step. Five steps of n instances
    fused two per group (2 + 2 + 1; pair lanes of a step start inside a 64-lane tile), valid and tampered instances, K = 3 (the
    serial team Miller chain) and K = 20 (the pair-parallel one); free running with one tensor per step, and consumer mode through a
    ring of two tensors. Every witness element of every instance against the oracle."""
    import torch

    steps = 5
    dev = torch.device("cuda:0")
    cases = [synth.make_multi(oracle, K, tamper=(a % K if a % 3 == 1 else None), start=5 * a) for a in range(steps * n)]
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_pairs=K, consumer_mode=consumer)
    assert eng.n_witness == pkg.layout_multi(32, K)["n_witness"]
    ring = 2 if consumer else steps
    outs = [eng.new_witness_tensor() for _ in range(ring)]
    ress = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(steps)]
    got_w, keep = {}, []
    state = {"next": 0}

    def drain():
        while state["next"] < eng.materialised():
            s = state["next"]
            eng.wait_step(s)
            torch.cuda.synchronize()
            got_w[s] = outs[s % ring].cpu().numpy().view(np.uint64).copy()
            eng.output_consumed(outs[s % ring])
            state["next"] += 1

    for k in range(steps):
        sl = cases[k * n:(k + 1) * n]
        d = (torch.from_numpy(np.stack([c[0] for c in sl]).view(np.int64)).to(dev), torch.from_numpy(np.stack([c[1] for c in sl])).to(dev),
             torch.from_numpy(np.stack([c[2] for c in sl]).view(np.int64)).to(dev))
        keep.append(d)
        while True:
            try:
                eng.submit_multi(d[0], d[1], d[2], witness=outs[k % ring], result=ress[k])
                break
            except pkg.BlswBusy:
                drain()
        if consumer:
            drain()
    eng.flush()
    if consumer:
        while state["next"] < steps:
            drain()
    torch.cuda.synchronize()
    for k in range(steps):
        w = got_w[k] if consumer else outs[k].cpu().numpy().view(np.uint64)
        got = ress[k].cpu().numpy().astype(bool)
        for i in range(n):
            c = cases[k * n + i]
            nw, res, _, ow = oracle.witness_multi(c[0], c[1], c[2])
            assert nw == w.shape[1] and res == c[3] == bool(got[i]), (k, i)
            bad = np.nonzero((ow != w[i]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
    eng.close()


def test_engine_multi_compact_round_trip(pkg, oracle):
    """Compact wire form of the N+1-pair engine (blsw_engine_submit_multi_compact; 4 instances of 16 pairs per step: one whole pair tile,
    a quarter of an instance tile, packed): three steps leave in compact form, a SECOND engine expands them
    (blsw_engine_expand_compact) and every witness element of every instance equals the oracle's."""
    import torch

    K, n, steps = 16, 4, 3
    dev = torch.device("cuda:0")
    cases = [synth.make_multi(oracle, K, tamper=(3 if a == 5 else None), start=3 * a) for a in range(steps * n)]
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_pairs=K)
    rx = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_pairs=K)
    cb = eng.compact_bytes()
    lay = pkg.layout_multi(32, K)
    assert cb < n * lay["n_witness"] * 48 / 10  # an order of magnitude below the vectors
    cbufs = eng.new_compact_buffer(steps)
    ress = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(steps)]
    keep = []
    for k in range(steps):
        sl = cases[k * n:(k + 1) * n]
        d = (torch.from_numpy(np.stack([c[0] for c in sl]).view(np.int64)).to(dev), torch.from_numpy(np.stack([c[1] for c in sl])).to(dev),
             torch.from_numpy(np.stack([c[2] for c in sl]).view(np.int64)).to(dev))
        keep.append(d)
        eng.submit_multi_compact(d[0], d[1], d[2], cbufs[k], result=ress[k])
    eng.flush()
    torch.cuda.synchronize()
    wit = rx.new_witness_tensor()
    for k in range(steps):
        wit.zero_()
        rx.expand_compact(cbufs[k], wit)
        torch.cuda.synchronize()
        w = wit.cpu().numpy().view(np.uint64)
        got = ress[k].cpu().numpy().astype(bool)
        for i in range(n):
            c = cases[k * n + i]
            nw, res, _, ow = oracle.witness_multi(c[0], c[1], c[2])
            assert nw == w.shape[1] and res == c[3] == bool(got[i]), (k, i)
            bad = np.nonzero((ow != w[i]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
    eng.close()
    rx.close()


def test_engine_multi_canonical_output_form(pkg, oracle):
    """options.output_form = 1 on the N+1-pair engine: canonical * 2^384 mod p == the oracle's Montgomery element for every element of
    an instance of 16 pairs (the K SHA segments hold 0 / 1), plain steps and an expanded compact batch."""
    import torch

    P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    R = (1 << 384) % P
    K, n = 16, 4
    dev = torch.device("cuda:0")
    cases = [synth.make_multi(oracle, K, start=3 * a) for a in range(n)]
    d = (torch.from_numpy(np.stack([c[0] for c in cases]).view(np.int64)).to(dev), torch.from_numpy(np.stack([c[1] for c in cases])).to(dev),
         torch.from_numpy(np.stack([c[2] for c in cases]).view(np.int64)).to(dev))
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_pairs=K, output_form=1)
    w, wx, cb = eng.new_witness_tensor(), eng.new_witness_tensor(), eng.new_compact_buffer(1)
    res = torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_multi(d[0], d[1], d[2], witness=w, result=res)
    eng.submit_multi_compact(d[0], d[1], d[2], cb[0])
    eng.flush()
    torch.cuda.synchronize()
    eng.expand_compact(cb[0], wx)
    torch.cuda.synchronize()
    assert torch.equal(w, wx) and res.cpu().numpy().astype(bool).tolist() == [c[3] for c in cases]
    lay = pkg.layout_multi(32, K)
    i = 2
    nw, _, _, ow = oracle.witness_multi(cases[i][0], cases[i][1], cases[i][2])
    got = w[i].cpu().numpy().view(np.uint64)
    # vectorised check of c * R mod p == m through python integers per element is slow for 11 M elements: compare a strided sample of
    # every segment plus the segment borders
    idx = sorted(set(list(range(0, nw, 997)) + [lay[k] + dlt for k in lay if k.startswith("off_") for dlt in (-1, 0, 1) if 0 <= lay[k] + dlt < nw] + [nw - 1]))
    for k in idx:
        c = sum(int(v) << (64 * t) for t, v in enumerate(got[k]))
        m = sum(int(v) << (64 * t) for t, v in enumerate(ow[k]))
        assert c < P and c * R % P == m, "element %d" % k
    for j in (0, K - 1):
        seg = got[lay["off_expand"] + j * lay["stride_hash"]:lay["off_expand"] + j * lay["stride_hash"] + lay["sha_bits"]]
        assert (seg[:, 1:] == 0).all() and set(np.unique(seg[:, 0]).tolist()) == {0, 1}
    eng.close()


def test_verify_multi_128_pairs(pkg, oracle):
    """BASELINE configs[3]: ONE signature over 128 (pk, msg) pairs, a 129-pair Miller product — all 87 295 138 witness
    elements (4.2 GB) against the oracle, plus the tampered variant's result."""
    K = 128
    pks, msgs, sig, _ = synth.make_multi(oracle, K)
    got, wit = _multi_run(pkg, pks[None], msgs[None], sig[None])
    n, res, _, ow = oracle.witness_multi(pks, msgs, sig)
    assert res is True and got.tolist() == [True] and n == wit.shape[1] == pkg.layout_multi(32, K)["n_witness"]
    w = wit[0].cpu().numpy().view(np.uint64)
    del wit
    step = 1 << 22
    for lo in range(0, n, step):
        blk = (ow[lo:lo + step] != w[lo:lo + step]).any(axis=1)
        assert not blk.any(), "first mismatching witness index %d" % (lo + int(np.nonzero(blk)[0][0]))
    del w, ow
    bad = msgs.copy()
    bad[77, 5] ^= 0x40
    got, _ = _multi_run(pkg, pks[None], bad[None], sig[None])
    assert got.tolist() == [False]


def test_sharded_stream_rehearsal(pkg, oracle):
    """BASELINE configs[2] procedure on one GPU: one rank's shard of 8 192 instances streamed in
    micro-batches of 1 024 through a ring of TWO witness tensors with a digest kernel as the consumer; all 8 192 results and
    the digests of a 1 % sample (82 instances, chosen by a fixed stride) against the oracle."""
    rehearsal = importlib.import_module("tools.shard_rehearsal")
    out = rehearsal.run_shard(pkg, n_shard=8192, batch=1024, ring=2, rank=0, world=8)
    assert out["results_ok"] and out["steps"] == 8
    bad = rehearsal.check_sample(pkg, oracle, out, frac=0.01, threads=8)
    assert bad == [], bad
    assert out["sampled"] >= 82


def test_config2_every_shard_of_the_65536_on_one_gpu(pkg, oracle):
    """BASELINE configs[2] at its full size, rank by rank on the one GPU at hand: the 65 536 instances of SURVEY 8d config 3 as the eight contiguous shards
    of 8 192 that eight ranks would own (sharding.shard_range), each streamed through a ring of two tensors with the digest kernel as the consumer. All
    65 536 result booleans against the tamper rule, a fixed-stride 1 % sample of EVERY shard (82 per shard, 656 in all) against the
    oracle's witness vectors on all host threads, and
    a size-independent property of the whole: the shards' digest sets are pairwise different (every rank processed ITS block of the global batch)."""
    import torch

    rehearsal = importlib.import_module("tools.shard_rehearsal")
    sums = []
    for rank in range(8):
        out = rehearsal.run_shard(pkg, n_shard=8192, batch=1024, ring=2, rank=rank, world=8)
        assert out["results_ok"] and out["steps"] == 8 and out["first_instance"] == rank * 8192, rank
        bad = rehearsal.check_sample(pkg, oracle, out, frac=0.01, threads=max(8, len(os.sched_getaffinity(0))))
        assert bad == [] and out["sampled"] >= 81, (rank, bad)
        sums.append(tuple(int(v) for v in out["digests"].sum(axis=0, dtype=np.uint64)))
        del out
        torch.cuda.empty_cache()
    assert len(set(sums)) == 8


def test_c_caller_on_the_gpu(pkg, oracle):
    """tests/c_caller (plain C against include/blsw.h): decode -> engine create / submit / flush / wait_step -> digest for the
    reference's gadget case (constraints.rs:337-343); result and witness digest against the oracle."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "c_caller")])
    g = LIT["gadget_verify"]
    out = subprocess.check_output([os.path.join(root, "tests", "c_caller", "caller"), "verify", g["pubkey"], g["messages"][0], g["signature"]], text=True, timeout=300)
    kv = dict(p.split("=") for p in out.split())
    _, pk, _ = oracle.g1_decompress(bytes.fromhex(g["pubkey"]))
    _, sig, _ = oracle.g2_decompress(bytes.fromhex(g["signature"]))
    n, _, res, w = oracle.witness(pk, bytes.fromhex(g["messages"][0]), sig)
    assert kv["status_pk"] == kv["status_sig"] == "0" and int(kv["result"]) == int(res) == 1 and int(kv["n_witness"]) == n
    assert [int(kv["digest0"]), int(kv["digest1"])] == pkg.witness_digest_reference(w)
    # the streaming side of the ABI from C: consumer-mode engine, one witness tensor + one compact buffer as the whole ring
    out = subprocess.check_output([os.path.join(root, "tests", "c_caller", "caller"), "stream", g["pubkey"], g["messages"][0], g["signature"]], text=True, timeout=300)
    kv = dict(p.split("=") for p in out.split())
    assert kv["steps"] == "5" and kv["all_digests_equal"] == "1" and kv["all_results_equal"] == "1" and kv["result"] == "1"
    assert [int(kv["digest0"]), int(kv["digest1"])] == pkg.witness_digest_reference(w)


def test_cpp_host_mirror_reference_gadget_test(pkg, oracle):
    """tests/cpp_caller/gadget_test.cpp = the reference's `test_verify` (constraints.rs:318-376) written against include/blsw.hpp, the C++ host side
    with the reference's names: the three messages as three systems of one batch, expected [true, false, false]; witness vectors of the valid and of an
    invalid system against the oracle (a position-weighted digest of the assignment), for Constant and for Witness parameters; `constraint size` against the oracle's. Then `test_aggregate_verify` and `test_aggregate_verify_neg`
    (constraints.rs:378-521) through BlsSignatureVerifyGadget::aggregate_verify of the same header: results, effective key counts, both witness vectors."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "cpp_caller")])
    g = LIT["gadget_verify"]
    _, pk, _ = oracle.g1_decompress(bytes.fromhex(g["pubkey"]))
    _, sig, _ = oracle.g2_decompress(bytes.fromhex(g["signature"]))

    def digest(a):  # the program's: sum of w_k (2 k + 1) over the u64 words, mod 2^64
        w = a.reshape(-1).astype(np.uint64)
        with np.errstate(over="ignore"):
            return int((w * (2 * np.arange(w.size, dtype=np.uint64) + 1)).sum(dtype=np.uint64))

    for mode, pm in (("constant", 0), ("witness", 1)):
        args = [os.path.join(root, "tests", "cpp_caller", "gadget_test"), mode] + (["count-constraints"] if pm == 0 else [])
        out = subprocess.check_output(args, text=True, timeout=600)
        kv = dict(p.split("=") for p in out.split())
        assert [kv["verification_result_%d" % i] for i in range(3)] == ["1", "0", "0"] and g["expected"] == [True, False, False]
        assert kv["status_pk"] == kv["status_sig"] == "0" and kv["num_instance_variables"] == "1"
        for k, key in ((0, "digest0"), (2, "digest2")):
            n, ncons, res, w = oracle.witness(pk, bytes.fromhex(g["messages"][k]), sig, params_mode=pm)
            assert int(kv["num_witness_variables"]) == n and res == g["expected"][k]
            assert int(kv[key]) == digest(w), "%s parameters, system %d" % (mode, k)
        if pm == 0:
            assert int(kv["constraint_size"]) == ncons
    # the same test with PublicKeyVar / SignatureVar allocated as public inputs (AllocationMode::Input): instance_assignment and witness_assignment
    out = subprocess.check_output([os.path.join(root, "tests", "cpp_caller", "gadget_test"), "input", "count-constraints"], text=True, timeout=600)
    kv = dict(p.split("=") for p in out.split())
    assert [kv["verification_result_%d" % i] for i in range(3)] == ["1", "0", "0"] and kv["num_instance_variables"] == "10"
    for k, key in ((0, "digest0"), (2, "digest2")):
        n, ncons, res, w, inst = oracle.witness_io(pk, bytes.fromhex(g["messages"][k]), sig, 1, 1)
        assert int(kv["num_witness_variables"]) == n and res == g["expected"][k] and int(kv[key]) == digest(w)
    assert int(kv["instance_digest0"]) == digest(inst) and int(kv["constraint_size"]) == ncons
    # the reference's two aggregate_verify tests (constraints.rs:378-521) as the two systems of one batch: 512 keys, bitmaps {first two} / {all}
    out = subprocess.check_output([os.path.join(root, "tests", "cpp_caller", "gadget_test"), "aggregate"], text=True, timeout=600)
    kv = dict(p.split("=") for p in out.split())
    assert (kv["verification_result_0"], kv["verification_result_1"], kv["effective_public_key_count_0"], kv["effective_public_key_count_1"]) == ("1", "0", "2", "512")
    _, p1, _ = oracle.g1_decompress(bytes.fromhex("a491d1b0ecd9bb917989f0e74f0dea0422eac4a873e5e2644f368dffb9a6e20fd6e10c1b77654d067c0618f6e5a7f79a"))
    _, p2, _ = oracle.g1_decompress(bytes.fromhex("b301803f8b5ac4a1133581fc676dfedc60d891dd5fa99028805e5ea5b08d3491af75d0707adab3b70c6a6a580217bf81"))
    _, s, _ = oracle.g2_decompress(bytes.fromhex(
        "912c3615f69575407db9392eb21fee18fff797eeb2fbe1816366ca2a08ae574d8824dbfafb4c9eaa1cf61b63c6f9b69911f269b664c42947dd1b53ef1081926c1e82bb2a465f927124b08391a5249036146d6f3f1e17ff5f162f779746d830d1"))
    keys = np.stack([p1] + [p2] * 511)
    for i, bits in enumerate((np.array([1, 1] + [0] * 510, dtype=np.uint8), np.ones(512, dtype=np.uint8))):
        n, res, c, _, ow = oracle.witness_aggregate(keys, bits, bytes([0x56]) * 32, s)
        assert int(kv["num_witness_variables"]) == n and res == (i == 0) and c == (2, 512)[i]
        assert int(kv["digest%d" % i]) == digest(ow), "aggregate system %d" % i
    # a well-formed identity key, masked out (system 0) and unmasked (system 1): the gadget's Boolean, not a forced false; verify() afterwards is refused
    out = subprocess.check_output([os.path.join(root, "tests", "cpp_caller", "gadget_test"), "aggregate-identity"], text=True, timeout=600)
    kv = dict(p.split("=") for p in out.split())
    keys3 = np.stack([p1, p2, np.zeros(12, dtype=np.uint64)])
    for i, bits in enumerate((np.array([1, 1, 0], dtype=np.uint8), np.array([1, 1, 1], dtype=np.uint8))):
        n, res, c, _, ow = oracle.witness_aggregate(keys3, bits, bytes([0x56]) * 32, s)
        assert int(kv["num_witness_variables"]) == n and kv["verification_result_%d" % i] == str(int(res)) and int(kv["effective_public_key_count_%d" % i]) == c
        assert int(kv["digest%d" % i]) == digest(ow), "aggregate system %d with an identity key" % i
        assert kv["status_pk_%d" % i] == "0"
    assert kv["verification_result_0"] == "1" and kv["verify_after_aggregate_refused"] == "1"


def test_c_caller_submit_bytes_fixtures(pkg, tmp_path):
    """blsw_engine_submit_bytes from plain C: all 29 verify/*.json cases of the reference (tests/tests.rs:239-268) as ONE batch of
    compressed bytes — decode, status rule (an undecodable / identity point is replaced by the default and the case is false) and
    gadget in one ABI call; the results must equal the fixtures' outputs."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "c_caller")])
    cases = [c for _, c in eth_cases("verify")]
    f = tmp_path / "cases.txt"
    f.write_text("".join("%s %s %s\n" % (c["input"]["pubkey"][2:], c["input"]["message"][2:], c["input"]["signature"][2:]) for c in cases))
    out = subprocess.check_output([os.path.join(root, "tests", "c_caller", "caller"), "bytes", str(f)], text=True, timeout=300)
    kv = dict(p.split("=") for p in out.split())
    assert int(kv["n"]) == len(cases)
    assert [ch == "1" for ch in kv["results"]] == [bool(c["output"]) for c in cases]
    st = [tuple(int(v) for v in pair.split(",")) for pair in kv["statuses"].strip(";").split(";")]
    assert all((a == 0 and b == 0) or not c["output"] for (a, b), c in zip(st, cases))


def test_cpp_host_mirror_native_scheme(pkg, oracle, tmp_path):
    """The native scheme through include/blsw.hpp: BLS::sign + PublicKey::from(&sk) over the reference's sign fixtures (tests/tests.rs:202-237; a zero
    key is Err(InvalidSecretKey)) and BLS::verify over all 29 verify fixtures (tests/tests.rs:239-268), each as one batch from a C++ host."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "cpp_caller")])
    exe = os.path.join(root, "tests", "cpp_caller", "gadget_test")
    cases = [c for _, c in eth_cases("sign")]
    f = tmp_path / "sign.txt"
    f.write_text("".join("%s %s\n" % (c["input"]["privkey"][2:], c["input"]["message"][2:]) for c in cases))
    lines = subprocess.check_output([exe, "sign", str(f)], text=True, timeout=300).split("\n")[:len(cases)]
    n_err = 0
    for ln, c in zip(lines, cases):
        st, sig, pk = ln.split()
        if c["output"] is None:
            assert int(st) == pkg.ST_INVALID_SECRET_KEY
            n_err += 1
        else:
            assert int(st) == 0 and sig == c["output"][2:]
            assert bytes.fromhex(pk) == oracle.sk_to_pk(int(c["input"]["privkey"], 16))
    assert n_err == 1
    cases = [c for _, c in eth_cases("verify")]
    f = tmp_path / "verify.txt"
    f.write_text("".join("%s %s %s\n" % (c["input"]["pubkey"][2:], c["input"]["message"][2:], c["input"]["signature"][2:]) for c in cases))
    lines = subprocess.check_output([exe, "verify", str(f)], text=True, timeout=300).split("\n")[:len(cases)]
    for ln, c in zip(lines, cases):
        ok, st_pk, st_sig = (int(v) for v in ln.split())
        assert bool(ok) == bool(c["output"])
        assert not c["output"] or (st_pk, st_sig) == (0, 0)


def test_gpu_witness_satisfies_product_matrices(pkg, oracle):
    """f1: witness vectors produced by the HIP kernels satisfy the constraint matrices emitted by the product
    (blsw_matrices_*: A z o B z = C z on every one of the 713 891 constraints; evaluator in the test harness) — single-key
    circuit through the grouped engine, aggregate_verify with 2 keys and the N+1-pair product with 2 pairs."""
    import torch

    from tests import hostsim_lib

    pk, msg, sig, expect = synth.make_batch(oracle, 16)
    got, w = _run(pkg, pk[:4].copy(), msg[:4].copy(), sig[:4].copy(), max_steps=2)
    P = pkg.matrices(32, 0, 1)
    assert w.shape[1] == P["n_witness"]
    for i in (0, 3):
        assert hostsim_lib.r1cs_check(P, w[i]) == -1
    # aggregate_verify, 2 keys (same message): sk0 + sk1 signature over msg of instance 0
    pks, msgs, sg, _ = synth.make_multi(oracle, 2)
    got, wit = _multi_run(pkg, pks[None], msgs[None], sg[None])
    PM = pkg.matrices(32, 0, 2)
    assert got.tolist() == [True] and hostsim_lib.r1cs_check(PM, wit[0].cpu().numpy().view(np.uint64)) == -1
    PA = pkg.matrices(32, 2, 1)
    keys = np.stack([pk[0], pk[1]])[None]
    bm = np.array([[1, 0]], dtype=np.uint8)
    g, cnt, wa = _agg_run(pkg, keys, bm, msg[0:1].copy(), sig[0:1].copy())  # bitmap selects key 0 only: sig of instance 0 verifies
    assert g.tolist() == [True] and cnt.tolist() == [1] and hostsim_lib.r1cs_check(PA, wa[0]) == -1


def test_engine_aggregate_grouped(pkg, oracle):
    """aggregate_verify through the grouped engine (options.n_keys; constraints.rs:153-191): three batches of 6 instances with 5
    keys each, fused two per launch group, staged + placed; every instance against the oracle (results, counts, all witnesses)."""
    import torch

    K, n, steps = 5, 6, 3
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, n_keys=K)
    assert eng.n_witness == pkg.layout_aggregate(32, K)["n_witness"]
    cases, outs = [], []
    for k in range(steps):
        batch = []
        for i in range(n):
            bm = [(i >> b) & 1 for b in range(K)]
            bm[(i + k) % K] = 1  # at least one key selected
            batch.append(synth.make_aggregate(oracle, K, bm, start=100 * k + 10 * i, tamper=(i == 4)))
        pks = torch.from_numpy(np.stack([c[0] for c in batch]).view(np.int64)).to(dev)
        bmt = torch.from_numpy(np.stack([c[1] for c in batch])).to(dev)
        msg = torch.from_numpy(np.stack([c[2] for c in batch])).to(dev)
        sig = torch.from_numpy(np.stack([c[3] for c in batch]).view(np.int64)).to(dev)
        w = eng.new_witness_tensor()
        r = torch.empty(n, dtype=torch.int32, device=dev)
        c = torch.empty(n, dtype=torch.int32, device=dev)
        assert eng.submit_aggregate(pks, bmt, sig, msg, witness=w, result=r, count=c) == k
        cases.append(batch)
        outs.append((w, r, c))
    eng.flush()
    torch.cuda.synchronize()
    for k in range(steps):
        w, r, c = outs[k]
        got, cnt, wh = r.cpu().numpy().astype(bool), c.cpu().numpy(), w.cpu().numpy().view(np.uint64)
        for i, (pks, bm, msg, sig, expect) in enumerate(cases[k]):
            nw, res, cc, _, ow = oracle.witness_aggregate(pks, bm, msg.tobytes(), sig)
            assert res == expect == bool(got[i]) and cc == cnt[i] == int(bm.sum()) and nw == wh.shape[1]
            bad = np.nonzero((ow != wh[i]).any(axis=1))[0]
            assert len(bad) == 0, "step %d instance %d: first mismatching witness index %d" % (k, i, bad[0])
    eng.close()
    # the aggregate engine's compact wire form: 64 instances (copies of step 0's six), compact submit + expansion on a second
    # engine == plain submit, every element
    n2 = 64
    rep = lambda t: t.repeat((n2 + n - 1) // n, *([1] * (t.dim() - 1)))[:n2].contiguous()
    batch = cases[0]
    pks = rep(torch.from_numpy(np.stack([c[0] for c in batch]).view(np.int64)).to(dev))
    bmt = rep(torch.from_numpy(np.stack([c[1] for c in batch])).to(dev))
    msg = rep(torch.from_numpy(np.stack([c[2] for c in batch])).to(dev))
    sig = rep(torch.from_numpy(np.stack([c[3] for c in batch]).view(np.int64)).to(dev))
    e2 = pkg.WitnessEngine(n2, 32, max_steps=2, device=dev, n_buffers=2, n_keys=K)
    e3 = pkg.WitnessEngine(n2, 32, max_steps=2, device=dev, n_buffers=1, n_keys=K)
    plain, cb, back = e2.new_witness_tensor(), e2.new_compact_buffer(1), e3.new_witness_tensor()
    r1, r2 = torch.empty(n2, dtype=torch.int32, device=dev), torch.empty(n2, dtype=torch.int32, device=dev)
    c1, c2 = torch.empty(n2, dtype=torch.int32, device=dev), torch.empty(n2, dtype=torch.int32, device=dev)
    e2.submit_aggregate(pks, bmt, sig, msg, witness=plain, result=r1, count=c1)
    e2.submit_aggregate_compact(pks, bmt, sig, msg, cb[0], result=r2, count=c2)
    e2.flush()
    torch.cuda.synchronize()
    e3.expand_compact(cb[0], back)
    torch.cuda.synchronize()
    assert torch.equal(back, plain) and torch.equal(r1, r2) and torch.equal(c1, c2)
    assert torch.equal(plain[:n], outs[0][0]) and torch.equal(plain[60], outs[0][0][60 % n])
    e2.close()
    e3.close()
