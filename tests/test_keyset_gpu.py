"""Shared key sets (options.shared_keys, ABI 15) on the GPU: the key table, every witness element / result / count of a shared-keys engine against
the CPU oracle and against an all-Witness engine fed the same keys replicated per instance (grouped with two sets in one launch group, a padded
stride, direct mode, results only, canonical form, a mask with public inputs, consumer mode, the compact form), the refusals that need an engine,
and the device R1CS check with the unchanged all-Witness matrices. All comparisons are bit-exact."""
import importlib

import numpy as np
import pytest

from tests import agg_inputs_lib as A
from tests import synth
from tests.oracle_lib import P_MOD

pytestmark = pytest.mark.gpu
K, N, SEG = 5, 6, 1942
RINV = pow(1 << 384, -1, P_MOD)
# two committees: (first secret key of synth.make_aggregate, index of the key that is the identity (0, 0) or None)
SETS = {"A": (100, 2), "B": (200, None)}
STEP_SETS = ["A", "B", "A"]  # steps 0 and 1 share a launch group of max_steps = 2


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def limbs(v):
    return np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


def canonical_rows(a):
    """[m, 6] Montgomery limbs -> canonical integers; the booleans (zero and R mod p) without big-integer arithmetic"""
    one = limbs((1 << 384) % P_MOD)
    out = np.zeros_like(a)
    is_one = (a == one).all(axis=1)
    out[is_one, 0] = 1
    for k in np.nonzero(~is_one & a.any(axis=1))[0]:
        out[k] = limbs(sum(int(x) << (64 * j) for j, x in enumerate(a[k])) * RINV % P_MOD)
    return out


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def set_keys(oracle, name, k=K):
    start, ident = SETS[name]
    pks = synth.make_aggregate(oracle, k, [1] * k, start=start)[0].copy()
    if ident is not None:
        pks[ident] = 0
    return pks


def instance(oracle, name, bitmap, tamper=False):
    """one instance over committee `name`: the signature is that of the selected keys that are not the identity (selecting the identity adds nothing)"""
    start, ident = SETS[name]
    signed = [b if j != ident else 0 for j, b in enumerate(bitmap)]
    _, _, msg, sig, _ = synth.make_aggregate(oracle, K, signed, start=start, tamper=tamper)
    return set_keys(oracle, name), np.array(bitmap, dtype=np.uint8), msg, sig


def steps(oracle):
    """three steps of N instances: bitmaps vary per instance, key 0 (never the identity) always signs, the identity key of set A is selected in
    half of its instances, instance 4 of every step has a tampered message"""
    out = []
    for k, name in enumerate(STEP_SETS):
        batch = []
        for i in range(N):
            bm = [(i >> b) & 1 for b in range(K)]
            bm[(i + k) % K] = 1
            bm[0] = 1
            bm[2] = (i + k) & 1
            batch.append(instance(oracle, name, bm, tamper=(i == 4)))
        out.append(batch)
    return out


_ORACLE = {}


def expected(oracle, case):
    """(result, count, witness [n_witness, 6]) of the CPU oracle, computed once per instance"""
    pks, bm, msg, sig = case
    key = (pks.tobytes(), bm.tobytes(), msg.tobytes(), sig.tobytes())
    if key not in _ORACLE:
        _, res, cnt, _, w = oracle.witness_aggregate(pks, bm, msg.tobytes(), sig)
        _ORACLE[key] = (res, cnt, w)
    return _ORACLE[key]


def stack(torch, batch):
    return tuple(to_dev(torch, np.stack([c[j] for c in batch])) for j in range(4))  # pks [N, K, 12], bitmap, msg, sig


def run(pkg, torch, oracle, all_steps, shared, max_steps, n_buffers, pad=0, witness=True, want_instance=False, **opt):
    """the steps through a shared-keys engine (one KeySet per committee) or through an ordinary engine fed the keys replicated [N, K, 12]
    -> [(result, count, witness or None, instance or None)] as numpy arrays; pad: extra elements of witness_stride, sentinel-filled"""
    dev = torch.device("cuda:0")
    form = int(opt.get("output_form", 0))
    eng = pkg.WitnessEngine(N, 32, max_steps=max_steps, n_buffers=n_buffers, device=dev, n_keys=K, **({"shared_keys": 1} if shared else {}), **opt)
    assert eng.n_witness == pkg.layout_aggregate(32, K, int(opt.get("agg_inputs", 0)))["n_witness"]
    sets = {name: pkg.KeySet(to_dev(torch, set_keys(oracle, name)), output_form=form) for name in SETS} if shared else {}
    outs = []
    for k, batch in enumerate(all_steps):
        pks, bm, msg, sig = stack(torch, batch)
        w = None
        if witness:
            w = torch.full((N, eng.n_witness + pad, 6), -1, dtype=torch.int64, device=dev)
        inst = eng.new_instance_tensor().fill_(-1) if want_instance else None
        r = torch.full((N,), -1, dtype=torch.int32, device=dev)
        c = torch.full((N,), -1, dtype=torch.int32, device=dev)
        if shared:
            assert eng.submit_aggregate_keyset(sets[STEP_SETS[k]], bm, sig, msg, witness=w, result=r, count=c, instance=inst) == k
        else:
            assert eng.submit_aggregate(pks, bm, sig, msg, witness=w, result=r, count=c, instance=inst) == k
        outs.append((r, c, w, inst))
    eng.flush()
    torch.cuda.synchronize()
    got = [(r.cpu().numpy(), c.cpu().numpy(), w.cpu().numpy().view(np.uint64) if w is not None else None,
            inst.cpu().numpy().view(np.uint64) if inst is not None else None) for r, c, w, inst in outs]
    eng.close()
    for s in sets.values():
        s.close()
    return got


def first_difference(a, b):
    bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
    return None if len(bad) == 0 else int(bad[0])


def check_against_oracle(oracle, all_steps, got, form=0):
    for k, (batch, (res, cnt, wit, _)) in enumerate(zip(all_steps, got)):
        for i, case in enumerate(batch):
            r, c, w = expected(oracle, case)
            assert r == (i != 4) == bool(res[i]) and c == int(cnt[i]) == int(case[1].sum()), (k, i)
            if wit is not None:
                w = canonical_rows(w) if form else w
                assert wit[i, :w.shape[0]].shape == w.shape
                assert first_difference(wit[i, :w.shape[0]], w) is None, "step %d instance %d: witness %d differs" % (k, i, first_difference(wit[i, :w.shape[0]], w))


def check_equal(got, ref):
    for k, ((r0, c0, w0, i0), (r1, c1, w1, i1)) in enumerate(zip(got, ref)):
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1), k
        assert (w0 is None) == (w1 is None) and (w0 is None or np.array_equal(w0, w1)), k
        assert (i0 is None) == (i1 is None) and (i0 is None or np.array_equal(i0, i1)), k


_RUNS = {}


def grouped(pkg, torch, oracle, shared):
    """the grouped run of test 2 (max_steps 2, n_buffers 2), computed once and left unchanged"""
    if shared not in _RUNS:
        _RUNS[shared] = run(pkg, torch, oracle, steps(oracle), shared, 2, 2)
    return _RUNS[shared]


@pytest.mark.parametrize("form", [0, 1])
def test_table(pkg, torch, oracle, form):
    """KeySet.table = the keys segment of the oracle's vector, one key the identity; K = 1: 93 216 bytes, no multiple of the copy's chunk"""
    for name, k in (("A", K), ("B", 1)):
        pks = set_keys(oracle, name, k)
        ks = pkg.KeySet(to_dev(torch, pks), output_form=form)
        torch.cuda.synchronize()
        assert ks.n_keys == k and tuple(ks.table.shape) == (k * SEG, 6) and ks.table.data_ptr() % 256 == 0
        table = ks.table.cpu().numpy().view(np.uint64)
        ks.close()
        bm = [1] * k
        if SETS[name][1] is not None and k == K:
            bm[SETS[name][1]] = 0
        _, _, msg, sig, _ = synth.make_aggregate(oracle, k, bm, start=SETS[name][0])
        _, _, _, marks, w = oracle.witness_aggregate(pks, np.array(bm, dtype=np.uint8), msg.tobytes(), sig)
        assert pkg.layout_aggregate(32, k)["off_keys"] == 0 and pkg.layout_aggregate(32, k)["off_bitmap"] == k * SEG
        want = canonical_rows(w[:k * SEG]) if form else w[:k * SEG]
        assert first_difference(table, want) is None, (name, k, first_difference(table, want))


def test_vectors_two_sets_in_one_group(pkg, torch, oracle):
    all_steps = steps(oracle)
    got = grouped(pkg, torch, oracle, True)
    check_against_oracle(oracle, all_steps, got)
    check_equal(got, grouped(pkg, torch, oracle, False))
    # the two sets differ, and set A's identity key is selected somewhere
    assert not np.array_equal(got[0][2][0, :K * SEG], got[1][2][0, :K * SEG])
    assert any(c[1][2] for c in all_steps[0]) and any(c[1][2] for c in all_steps[2])


def test_padded_stride_leaves_the_pad_untouched(pkg, torch, oracle):
    nw = pkg.layout_aggregate(32, K)["n_witness"]
    got = run(pkg, torch, oracle, steps(oracle), True, 2, 2, pad=5)
    for (r, c, w, _), (r1, c1, w1, _) in zip(got, grouped(pkg, torch, oracle, False)):
        assert w.shape == (N, nw + 5, 6) and np.array_equal(w[:, :nw], w1) and np.array_equal(r, r1) and np.array_equal(c, c1)
        assert (w[:, nw:] == np.uint64(2**64 - 1)).all()


@pytest.mark.parametrize("config", ["direct", "results_only", "canonical"])
def test_other_engine_shapes(pkg, torch, oracle, config):
    kw = {"direct": dict(max_steps=1, n_buffers=1), "results_only": dict(max_steps=2, n_buffers=2, witness=False),
          "canonical": dict(max_steps=2, n_buffers=2, output_form=1)}[config]
    all_steps = steps(oracle)
    got = run(pkg, torch, oracle, all_steps, True, **kw)
    check_equal(got, run(pkg, torch, oracle, all_steps, False, **kw))
    check_against_oracle(oracle, all_steps[:1], got[:1], form=kw.get("output_form", 0))
    if config == "direct":  # and direct mode in canonical form: the chains write in place, the conversion must leave the copied head alone
        kw = dict(kw, output_form=1)
        got = run(pkg, torch, oracle, all_steps[:2], True, **kw)
        check_equal(got, run(pkg, torch, oracle, all_steps[:2], False, **kw))
        check_against_oracle(oracle, all_steps[:1], got[:1], form=1)


def test_mask_14_keeps_the_keys_segment(pkg, torch, oracle):
    mask = 14
    all_steps = steps(oracle)[:2]
    got = run(pkg, torch, oracle, all_steps, True, 2, 2, want_instance=True, agg_inputs=mask)
    lay = pkg.layout_aggregate(32, K, mask)
    assert lay["off_keys"] == 0 and lay["off_bitmap"] == K * SEG and lay["off_msg"] == lay["off_bitmap"]
    for k, (batch, (res, cnt, wit, inst)) in enumerate(zip(all_steps, got)):
        for i, (pks, bm, msg, sig) in enumerate(batch):
            r, c, w, ins, _ = A.witness(pks, bm, msg.tobytes(), sig, mask)
            assert r == (i != 4) == bool(res[i]) and c == int(cnt[i]), (k, i)
            assert wit[i].shape == w.shape and first_difference(wit[i], w) is None, (k, i, first_difference(wit[i], w))
            assert np.array_equal(inst[i], ins), (k, i)
    check_equal(got, run(pkg, torch, oracle, all_steps, False, 2, 2, want_instance=True, agg_inputs=mask))


def test_consumer_mode_holds_the_head_back(pkg, torch, oracle):
    """a ring of ONE output: step 1 (set B) is accepted while step 0 (set A) still owns the tensor, and nothing of it — the broadcast head included —
    may reach the tensor before the consumer releases it"""
    all_steps = steps(oracle)[:2]
    want = grouped(pkg, torch, oracle, False)
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, 32, max_steps=2, n_buffers=2, device=dev, n_keys=K, shared_keys=1, consumer_mode=1)
    sets = {name: pkg.KeySet(to_dev(torch, set_keys(oracle, name))) for name in SETS}
    X = eng.new_witness_tensor().fill_(-1)
    res = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2)]
    keep = []
    for k, batch in enumerate(all_steps):
        pks, bm, msg, sig = stack(torch, batch)
        keep.append((bm, msg, sig))
        assert eng.submit_aggregate_keyset(sets[STEP_SETS[k]], bm, sig, msg, witness=X, result=res[k]) == k
    assert eng.launched() == 2 and eng.materialised() == 1
    eng.wait_step(0)
    torch.cuda.synchronize()
    x0 = X.cpu().numpy().view(np.uint64)
    assert first_difference(x0[:, :K * SEG], want[0][2][:, :K * SEG]) is None, "step 1's head reached the tensor before its release"
    assert np.array_equal(x0, want[0][2])
    with pytest.raises(pkg.BlswBusy):
        eng.wait_step(1)
    eng.output_consumed(X)
    assert eng.materialised() == 2
    eng.flush()
    torch.cuda.synchronize()
    assert np.array_equal(X.cpu().numpy().view(np.uint64), want[1][2])
    assert np.array_equal(res[0].cpu().numpy(), want[0][0]) and np.array_equal(res[1].cpu().numpy(), want[1][0])
    eng.close()
    for s in sets.values():
        s.close()


def test_compact_form_carries_no_key_rows(pkg, torch, oracle):
    n = 64
    batch = steps(oracle)[0]
    dev = torch.device("cuda:0")
    rep = lambda t: t.repeat((n + N - 1) // N, *([1] * (t.dim() - 1)))[:n].contiguous()
    pks, bm, msg, sig = (rep(t) for t in stack(torch, batch))
    ks = pkg.KeySet(to_dev(torch, set_keys(oracle, "A")))
    eng = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=2, device=dev, n_keys=K, shared_keys=1)
    recv = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=1, device=dev, n_keys=K, shared_keys=1)
    plain_eng = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=1, device=dev, n_keys=K)
    assert plain_eng.compact_bytes() - eng.compact_bytes() >= n * K * SEG * 48 and recv.compact_bytes() == eng.compact_bytes()
    comp, plain = eng.new_compact_buffer(1), eng.new_witness_tensor()
    r1, r2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    c1, c2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit_aggregate_keyset_compact(ks, bm, sig, msg, comp[0], result=r1, count=c1)
    eng.submit_aggregate_keyset(ks, bm, sig, msg, witness=plain, result=r2, count=c2)
    eng.flush()
    torch.cuda.synchronize()
    out = recv.new_witness_tensor().fill_(-1)
    recv.expand_compact(comp[0], out, keyset=ks)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and torch.equal(r1, r2) and torch.equal(c1, c2)
    wit = plain.cpu().numpy().view(np.uint64)
    for i in (0, 4, 63):
        r, c, w = expected(oracle, batch[i % N])
        assert np.array_equal(wit[i], w) and bool(r2[i]) == r and int(c2[i]) == c, i
    # a shared-keys step expands only with its set; the ordinary entry points refuse a shared-keys engine and the other way round
    L = pkg.lib()
    assert L.blsw_engine_expand_compact(recv._e, comp[0].data_ptr(), out.data_ptr(), out.shape[1], None) == 1
    assert L.blsw_engine_expand_compact_keyset(plain_eng._e, ks._ks, comp[0].data_ptr(), out.data_ptr(), out.shape[1], None) == 1
    assert L.blsw_engine_submit_aggregate(eng._e, pks.data_ptr(), bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, 0, None, None, None) == 1
    assert L.blsw_engine_submit_aggregate_io(eng._e, pks.data_ptr(), bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
    assert L.blsw_engine_submit_aggregate_compact(eng._e, pks.data_ptr(), bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), comp[0].data_ptr(), None, None, None) == 1
    assert L.blsw_engine_submit_aggregate_keyset(plain_eng._e, ks._ks, bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
    assert L.blsw_engine_submit_aggregate_keyset_compact(plain_eng._e, ks._ks, bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), comp[0].data_ptr(), None, None, None) == 1
    assert L.blsw_engine_submit_aggregate_keyset(eng._e, None, bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
    # a set of another size or another element form than the engine's
    small = pkg.KeySet(to_dev(torch, set_keys(oracle, "A")[:3]))
    canon = pkg.KeySet(to_dev(torch, set_keys(oracle, "A")), output_form=1)
    for other in (small, canon):
        assert L.blsw_engine_submit_aggregate_keyset(eng._e, other._ks, bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
        assert L.blsw_engine_expand_compact_keyset(recv._e, other._ks, comp[0].data_ptr(), out.data_ptr(), out.shape[1], None) == 1
    if torch.cuda.device_count() > 1:
        far = pkg.KeySet(to_dev(torch, set_keys(oracle, "A")).to("cuda:1"))
        assert L.blsw_engine_submit_aggregate_keyset(eng._e, far._ks, bm.data_ptr(), sig.data_ptr(), msg.data_ptr(), None, None, 0, None, None, None) == 1
        far.close()
    assert eng.submitted() == 2
    for h in (eng, recv, plain_eng, ks, small, canon):
        h.close()


def test_python_gadget_takes_a_keyset(pkg, torch, oracle):
    batch = steps(oracle)[0]
    pks, bm, msg, sig = stack(torch, batch)
    ks = pkg.KeySet(to_dev(torch, set_keys(oracle, "A")))
    res, cnt, wit = pkg.aggregate_verify(pkg.ParametersVar(), ks, bm, msg, pkg.SignatureVar.new_witness(sig))
    r0, c0, w0 = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), bm, msg, pkg.SignatureVar.new_witness(sig))
    assert torch.equal(res, r0) and torch.equal(cnt, c0) and torch.equal(wit, w0)
    ks.close()


def test_all_witness_matrices_are_satisfied(pkg, torch, oracle):
    """ConstraintChecker(32, n_keys=5) holds the unchanged all-Witness matrices. Every instance of test 2 satisfies them — the one with the
    tampered message too: a tampered message is a false result, not an unsatisfied system (tests/test_r1cs_device.py::test_every_shape). An
    instance whose copied head is tampered is found, at the row the same tampering gives in the all-Witness engine's tensor."""
    dev = torch.device("cuda:0")
    chk = pkg.ConstraintChecker(32, n_keys=K, device=dev)
    got, ref = grouped(pkg, torch, oracle, True), grouped(pkg, torch, oracle, False)
    for k in range(len(STEP_SETS)):
        w = to_dev(torch, got[k][2])
        assert chk.n_witness == w.shape[1]
        assert chk.which_is_unsatisfied(w).cpu().tolist() == [-1] * N, k
        assert got[k][0].tolist() == [int(i != 4) for i in range(N)]
    w, w_ref = to_dev(torch, got[1][2]).clone(), to_dev(torch, ref[1][2]).clone()
    at = 3 * SEG + 1000  # inside key 3's block of the head of instance 4
    w[4, at, 0] ^= 1
    w_ref[4, at, 0] ^= 1
    rows = chk.which_is_unsatisfied(w).cpu().tolist()
    assert rows[4] >= 0 and rows[:4] + rows[5:] == [-1] * (N - 1)
    assert rows == chk.which_is_unsatisfied(w_ref).cpu().tolist()
    chk.close()
