"""The kernels that run the witness chains (k_g1, k_g2, k_prepare, k_prepv_*, k_cofactor*, k_cofv_*, k_agg_keys, k_keyset_alloc, their _inl and _q
compilations, the team G2 allocation, the pairing forms) on keys and signatures OFF the prime-order subgroup, through the public API, against the
oracle's vectors (run with -m gpu). The operands are those of tests/chain_edges.py, which tests/test_chain_edges.py holds, with the oracle, to a
Python restatement on the host.

Every batch is 70 instances, a full wave and a ragged one. Batch MIXED has edge operands at lanes 0, 1, 31, 62, 63, 64 and 69 between ordinary
valid (and one tampered) instances: a wave mixes exceptional and ordinary chains, and fp_inv's wave-wide loop exit sees a zero beside slow
inversions. Batch WAVE fills lanes 0..63 with one instance whose key has order 3 and whose signature has order 13: a whole wave takes the
second walk of the G1 ladder and the affine fallback of the values-first prepare chain together. Whole vectors are compared for every edge
lane, the neighbours of the edge lanes and every eighth ordinary lane; the comparison runs on the device."""
import importlib

import numpy as np
import pytest

from tests import agg_inputs_lib as A
from tests import chain_edges as E
from tests import curve_ref as C
from tests import synth
from tests.edges_gpu_lib import same, to_dev

pytestmark = pytest.mark.gpu
N = 70
EDGE_LANES = (0, 1, 31, 62, 63, 64, 69)
CHECK_LANES = sorted(set(EDGE_LANES) | {2, 30, 32, 61, 65, 68} | set(range(0, N, 8)))


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = importlib.import_module("bls-verify-gadget_amd")
    p.lib()
    return p


def _g1(name):
    return E.enc_g1({n: q for n, q, _ in E.g1_operands()}[name])


def _g2(name):
    return E.enc_g2({n: q for n, q, _ in E.g2_operands()}[name])


def batches(oracle):
    """{name: (pk [70, 12], msg [70, 32], sig [70, 24])}, built once"""
    def make():
        pk0, msg0, sig0, expect = synth.make_batch(oracle, 16)
        pick = (0, 1, 2, 15)  # three valid instances and the tampered one
        assert list(expect[list(pick)]) == [True, True, True, False]
        base = [pick[i % 4] for i in range(N)]
        pk, msg, sig = pk0[base].copy(), msg0[base].copy(), sig0[base].copy()
        pk[0] = _g1("order 3: (0, 2)")
        sig[1] = _g2("order 13")
        pk[31] = _g1("order 11")
        sig[62] = _g2("-(order 13)")
        pk[63], sig[63] = _g1("order 3: (0, p - 2)"), _g2("order 23")
        sig[64] = 0  # the identity signature under a valid key
        pk[69], sig[69] = _g1("subgroup + order 3"), _g2("subgroup + order 13")
        wpk, wmsg, wsig = pk0[base].copy(), msg0[base].copy(), sig0[base].copy()
        wpk[:64], wsig[:64], wmsg[:64] = _g1("order 3: (0, 2)"), _g2("order 13"), msg0[0]
        return {"mixed": (pk, msg, sig), "wave": (wpk, wmsg, wsig)}
    return E.F._memo("chain_edges_gpu_batches", make)


_EXPECT = {}


def expected(oracle, torch, kind, *args):
    """(result, vector on the device[, instance / count]) of the oracle for one instance, computed once"""
    key = (kind,) + tuple(a.tobytes() if hasattr(a, "tobytes") else a for a in args)
    if key not in _EXPECT:
        if kind == "single":
            _, _, res, w = oracle.witness(*args)
            extra = None
        elif kind == "io":
            _, _, res, w, extra = oracle.witness_io(args[0], args[1], args[2], True, True)
        elif kind == "agg":
            _, res, extra, _, w = oracle.witness_aggregate(*args)
        elif kind == "agg_keys_input":
            res, extra, w, inst, _ = A.witness(args[0], args[1], args[2], args[3], A.KEYS)
            extra = (extra, inst)
        else:
            _, res, _, w = oracle.witness_multi(*args)
            extra = None
        _EXPECT[key] = (res, torch.from_numpy(w.view(np.int64)).cuda(), extra)
    return _EXPECT[key]


def run_single(pkg, oracle, tag, max_steps=2, io=False, **options):
    """batches MIXED and WAVE as two steps of one engine; every compared lane equals the oracle"""
    import torch

    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, 32, max_steps=max_steps, device=dev, n_buffers=2 if max_steps > 1 else 1, **options)
    outs, keep = [], []
    for name in ("mixed", "wave"):
        pk, msg, sig = batches(oracle)[name]
        d = (to_dev(torch, pk), to_dev(torch, sig), to_dev(torch, msg))
        w, r = eng.new_witness_tensor(), torch.empty(N, dtype=torch.int32, device=dev)
        inst = eng.new_instance_tensor() if io else None
        eng.submit(d[0], d[1], d[2], witness=w, result=r, instance=inst)
        if max_steps == 1:
            eng.flush()
        outs.append((name, w, r, inst)), keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    failures = []
    for name, w, r, inst in outs:
        pk, msg, sig = batches(oracle)[name]
        got = r.cpu().numpy().astype(bool)
        insts = inst.cpu().numpy().view(np.uint64) if io else None
        for i in (CHECK_LANES if name == "mixed" else sorted(set(range(64)) | {64, 69})):
            res, want, extra = expected(oracle, torch, "io" if io else "single", pk[i], msg[i].tobytes(), sig[i])
            try:
                assert res == bool(got[i]), "%s %s, lane %d: result %r, oracle %r" % (tag, name, i, bool(got[i]), res)
                same(torch, "%s %s" % (tag, name), i, w[i], want)
                if io:
                    assert np.array_equal(insts[i], extra), "%s %s, lane %d: instance vector differs" % (tag, name, i)
            except AssertionError as e:
                failures.append(str(e))
    eng.close()
    assert not failures, failures[:12]


def test_direct_call(pkg, oracle):
    """the direct call (max_steps = 1): one launch per chain kernel, no staging"""
    run_single(pkg, oracle, "direct", max_steps=1)


@pytest.mark.parametrize("latency_mode", [0, 1, 2, 3, 4])
def test_grouped_latency_modes(pkg, oracle, latency_mode):
    """0: the default rule (the group finds the chains idle: quads, values-first cofactor and prepare); 1: the ordinary kernels; 2: every group;
    3: values first only; 4: quads only"""
    run_single(pkg, oracle, "latency_mode %d" % latency_mode, latency_mode=latency_mode)


@pytest.mark.parametrize("chain_variant,cofactor_mode", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_kernel_variants(pkg, oracle, chain_variant, cofactor_mode):
    """out-of-line / inlined compilations x one cofactor chain per lane / three chunks and a join"""
    run_single(pkg, oracle, "chain_variant %d cofactor_mode %d" % (chain_variant, cofactor_mode), chain_variant=chain_variant, cofactor_mode=cofactor_mode, latency_mode=1)


@pytest.mark.parametrize("options", [dict(g2_mode="team"), dict(pairing_mode="lane")], ids=["g2_mode team", "pairing_mode lane"])
def test_team_g2_and_lane_pairing(pkg, oracle, options):
    """the G2DBL / G2ADD tables under the (r - 1) sigma chain, where (r - 1) sigma is not -sigma; the one-lane pairing on coefficients of a degenerate chain"""
    run_single(pkg, oracle, str(options), **options)


def test_public_inputs(pkg, oracle):
    """pk_mode = sig_mode = 1: no allocation chains, the instance vectors compared too"""
    run_single(pkg, oracle, "pk_mode sig_mode 1", io=True, pk_mode=1, sig_mode=1)


K = 3


def agg_batch(oracle):
    """70 aggregate_verify instances over 3 keys; at the edge lanes key 1 has order 3 or 11, selected by the bitmap at lanes 0, 31, 63, 69 and not
    at lanes 1, 62, 64; lane 62 also carries a signature of order 13"""
    def make():
        cases = []
        for i in range(N):
            bm = [1, (i >> 1) & 1, 1]
            pks, b, msg, sig, _ = synth.make_aggregate(oracle, K, bm, start=10 * (i % 4), tamper=(i % 4 == 3))
            pks, sig = pks.copy(), sig.copy()
            if i in EDGE_LANES:
                pks[1] = _g1("order 3: (0, 2)" if i in (0, 1, 63) else "order 11")
                b = np.array([1, int(i in (0, 31, 63, 69)), 1], dtype=np.uint8)
            if i == 62:
                sig = _g2("order 13")
            cases.append((pks, b, msg, sig))
        return cases
    return E.F._memo("chain_edges_gpu_agg", make)


@pytest.mark.parametrize("mode", ["agg_inputs 0", "keys input", "shared_keys"])
def test_aggregate(pkg, oracle, mode):
    """the aggregate engine with K = 3: k_agg_keys per (instance, key); keys as public inputs (no allocation chain: the small-order key enters
    the sum as it is); a KeySet that holds a small-order key, its table against the oracle's allocation segment"""
    import torch

    dev = torch.device("cuda:0")
    cases = agg_batch(oracle)
    if mode == "shared_keys":  # one committee for all: the keys of lane 31 (key 1 of order 11), bitmaps and signatures of the instances
        cases = [(cases[31][0], b, msg, sig) for _, b, msg, sig in cases]
    opts = {"keys input": dict(agg_inputs=A.KEYS), "shared_keys": dict(shared_keys=1)}.get(mode, {})
    eng = pkg.WitnessEngine(N, 32, max_steps=2, device=dev, n_buffers=2, n_keys=K, **opts)
    pks, bm, msg, sig = (to_dev(torch, np.stack([c[j] for c in cases])) for j in range(4))
    w, r, c = eng.new_witness_tensor(), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    inst = eng.new_instance_tensor() if mode == "keys input" else None
    ks = None
    if mode == "shared_keys":
        ks = pkg.KeySet(to_dev(torch, cases[0][0]))
        eng.submit_aggregate_keyset(ks, bm, sig, msg, witness=w, result=r, count=c)
    else:
        eng.submit_aggregate(pks, bm, sig, msg, witness=w, result=r, count=c, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    got, cnt = r.cpu().numpy().astype(bool), c.cpu().numpy()
    failures = []
    for i in CHECK_LANES:
        p, b, m, s = cases[i]
        res, want, extra = expected(oracle, torch, "agg_keys_input" if mode == "keys input" else "agg", p, b, m.tobytes(), s)
        count = extra[0] if mode == "keys input" else extra
        try:
            assert res == bool(got[i]) and count == cnt[i] == int(b.sum()), (mode, i, res, got[i], count, cnt[i])
            same(torch, mode, i, w[i], want)
            if mode == "keys input":
                assert np.array_equal(inst[i].cpu().numpy().view(np.uint64), extra[1]), (mode, i)
        except AssertionError as e:
            failures.append(str(e))
    if ks is not None:
        seg = pkg.layout_aggregate(32, K)["off_bitmap"]
        assert pkg.layout_aggregate(32, K)["off_keys"] == 0 and tuple(ks.table.shape) == (seg, 6)
        want = expected(oracle, torch, "agg", cases[0][0], cases[0][1], cases[0][2].tobytes(), cases[0][3])[1]
        same(torch, "KeySet.table", 0, ks.table, want[:seg])
        ks.close()
    eng.close()
    assert not failures, failures[:12]


@pytest.mark.parametrize("pairs", [3, 8])
def test_verify_multi(pkg, oracle, pairs):
    """the N+1-pair product: K = 3 (the serial Miller chain) and K = 8 (the pair-parallel one); at the edge lanes one key has small order
    (lanes 0, 31, 63, 69), the signature has order 13 (lanes 1, 62, 63) or is the identity (lane 64)"""
    import torch

    pks0, msgs0, sig0, _ = synth.make_multi(oracle, pairs)
    pks1, msgs1, sig1, _ = synth.make_multi(oracle, pairs, tamper=1, start=5)
    cases = []
    for i in range(N):
        pks, msgs, sig = (pks0, msgs0, sig0) if i % 4 != 3 else (pks1, msgs1, sig1)
        pks, sig = pks.copy(), sig.copy()
        if i in (0, 63):
            pks[pairs - 1] = _g1("order 3: (0, p - 2)")
        if i in (31, 69):
            pks[0] = _g1("order 11")
        if i in (1, 62, 63):
            sig = _g2("order 13")
        if i == 64:
            sig[:] = 0
        cases.append((pks, msgs, sig))
    res, wit = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(to_dev(torch, np.stack([c[0] for c in cases]))), to_dev(torch, np.stack([c[1] for c in cases])),
                                pkg.SignatureVar.new_witness(to_dev(torch, np.stack([c[2] for c in cases]))))
    torch.cuda.synchronize()
    got = res.cpu().numpy().astype(bool)
    failures = []
    for i in CHECK_LANES:
        r, want, _ = expected(oracle, torch, "multi", *cases[i])
        try:
            assert r == bool(got[i]), ("multi", pairs, i, r, got[i])
            same(torch, "verify_multi K = %d" % pairs, i, wit[i], want)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures[:12]


def test_value_entries_reject(pkg, oracle):
    """blsw_verify_batch and blsw_verify_groups_batch on the compressed forms of the same points: false, with status ST_NOT_IN_SUBGROUP where the
    point is outside the subgroup, as oracle.verify_bytes says; within a group only the affected triple fails after verify_batch_grouped's re-check"""
    import torch

    pk0, msg0, sig0, _ = synth.make_batch(oracle, 16)
    n = 16
    pk48 = [oracle.g1_compress(pk0[i]) for i in range(n)]
    sig96 = [oracle.g2_compress(sig0[i]) for i in range(n)]
    msgs = [msg0[i].tobytes() for i in range(n)]
    g1 = {nm: q for nm, q, _ in E.g1_operands()}
    g2 = {nm: q for nm, q, _ in E.g2_operands()}
    bad_pk = {1: "order 3: (0, 2)", 4: "order 11", 6: "order 10177", 9: "subgroup + order 3", 12: "random"}
    bad_sig = {2: "order 13", 4: "order 23", 7: "-(order 13)", 10: "subgroup + order 13", 13: "[r]Q"}
    for i, nm in bad_pk.items():
        pk48[i] = C.g1_compress(g1[nm])
    for i, nm in bad_sig.items():
        sig96[i] = C.g2_compress(g2[nm])
    u8 = lambda rows: torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n, -1).copy()).cuda()
    pk_t, msg_t, sig_t = u8(pk48), u8(msgs), u8(sig96)
    want = np.array([oracle.verify_bytes(pk48[i], msgs[i], sig96[i]) for i in range(n)])
    assert list(np.nonzero(~want)[0]) == sorted(set(bad_pk) | set(bad_sig) | {15})  # 15: the tampered message
    res, st = pkg.verify_batch(pk_t, msg_t, sig_t, want_status=True)
    st = st.cpu().numpy()
    assert np.array_equal(res.cpu().numpy().astype(bool), want)
    for i in range(n):
        assert st[i, 0] == (pkg.ST_NOT_IN_SUBGROUP if i in bad_pk else pkg.ST_OK) and st[i, 1] == (pkg.ST_NOT_IN_SUBGROUP if i in bad_sig else pkg.ST_OK), (i, st[i])
    gres, gst = pkg.verify_groups(pk_t, msg_t, sig_t, group=4, want_status=True)
    assert gres.cpu().numpy().astype(bool).tolist() == [False, False, False, False] and np.array_equal(gst.cpu().numpy(), st)
    gres, _ = pkg.verify_groups(pk_t[:1], msg_t[:1], sig_t[:1], group=4, want_status=True)
    assert gres.cpu().numpy().astype(bool).tolist() == [True]
    again = pkg.verify_batch_grouped(pk_t, msg_t, sig_t, group=4)
    assert np.array_equal(again.cpu().numpy().astype(bool), want)
    sel = [0, 2, 3, 5, 8, 11, 14, 0, 3, 5, 8, 11, 14, 0, 3, 5]  # one signature of order 13 in the first group of eight, a clean second group
    idx = torch.tensor(sel, device=pk_t.device)
    sub = (pk_t[idx].contiguous(), msg_t[idx].contiguous(), sig_t[idx].contiguous())
    assert pkg.verify_groups(*sub, group=8).cpu().numpy().astype(bool).tolist() == [False, True]
    assert pkg.verify_batch_grouped(*sub, group=8).cpu().numpy().astype(bool).tolist() == [i != 1 for i in range(16)]
