"""The kernels that run the in-circuit key sum of aggregate_verify (k_agg_keys, k_agg_sum, k_agg_sum_in, k_agg_sum_ks, k_agg_instance,
k_keyset_alloc and their compilations: chain_mapped_aggregate and chain_g1_post of csrc/chains.hpp) at the group law's edges, through the public
API, against the oracle's and the shim's vectors (run with -m gpu). The cases are those of tests/agg_edges.py, which tests/test_agg_edges.py
holds, with the oracle, to a Python restatement and to the meaning on the host. All comparisons are exact.

Batches of 70 instances, a full wave and a ragged one. "mixed 0..2" put the 21 cases at lanes 0, 1, 31, 62, 63, 64 and 69, seven each,
between ordinary valid and tampered instances: fp_inv's wave-wide loop exit sees a zero beside slow inversions. "wave" fills lanes 0..63 with
one case whose sum is the identity, lanes 64..69 with an ordinary selection, valid and tampered; keys 1, 2, 3 are O in all 70. A staged engine (max_steps = 2) takes "wave" as a launch group of its own,
then "mixed 0" and "mixed 1" as a full group and "mixed 2" as a last one: in the first group the hardware wave 0 of the sum kernel inverts
zero in every lane of chain_g1_post, and two whole waves of k_agg_keys (lane k N + I, N = 70: lanes 128..255) take the `inf` branch of
chain_g1_alloc_only. Whole vectors are compared, on the device, for every edge lane, its neighbours and every eighth ordinary lane; results
and counts for all 70 lanes.

What the Boolean is: the pairing equation alone (agg_edges' docstring). pk != 0 is a constraint, so a vector whose sum is the identity is the
reference's defined assignment that fails that one row first; the device checker is held to exactly that, lane by lane, and the value entry
(committee_verify), which folds "the aggregate is the identity" into its verdict, to `Boolean and sum != O`."""
import importlib

import numpy as np
import pytest

from tests import agg_edges as G
from tests import agg_inputs_lib as A
from tests.edges_gpu_lib import same, to_dev

pytestmark = pytest.mark.gpu
N, K = G.N, G.K


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = importlib.import_module("bls-verify-gadget_amd")
    p.lib()
    return p


_EXPECT = {}


def expected(oracle, torch, mask, row):
    """(Boolean, count, vector on the device, instance vector on the device or None) of the oracle (mask 0) or the shim for one instance, once"""
    key = (mask,) + tuple(a.tobytes() for a in row)
    if key not in _EXPECT:
        pks, bm, msg, sig = row
        if mask == 0:
            _, res, cnt, _, w = oracle.witness_aggregate(pks, bm, msg.tobytes(), sig)
            inst = None
        else:
            res, cnt, w, inst, _ = A.witness(pks, bm, msg.tobytes(), sig, mask)
            inst = to_dev(torch, inst)
        _EXPECT[key] = (res, cnt, to_dev(torch, w), inst)
    return _EXPECT[key]


def compare(oracle, torch, tag, mask, rows, lanes, w, r, c, inst=None, offset=0):
    """results and counts of every instance of `rows`, the whole vectors (and instance vectors) of `lanes`, at lane + offset of the outputs"""
    failures, whole = [], 0
    got, cnt = r.cpu().numpy().astype(bool), c.cpu().numpy()
    for i, row in enumerate(rows):
        res, count, want, winst = expected(oracle, torch, mask, row)
        whole += i in lanes
        try:
            assert (res, count) == (bool(got[offset + i]), int(cnt[offset + i])) and count == int(row[1].sum()), "%s, lane %d: result %r count %d, expected %r %d" % (
                tag, offset + i, bool(got[offset + i]), int(cnt[offset + i]), res, count)
            if i in lanes:
                same(torch, tag, offset + i, w[offset + i], want)
                if inst is not None:
                    assert torch.equal(inst[offset + i], winst), "%s, lane %d: instance vector differs" % (tag, offset + i)
        except AssertionError as e:
            failures.append(str(e))
    assert whole == len(set(lanes)) >= len(G.CHECK_LANES) and len(rows) >= N, (tag, whole)  # every lane asked for was there to compare
    return failures


def run_engine(pkg, oracle, tag, mask=0, **options):
    """the four batches through one staged engine in three launch groups -> {batch: (witness, result, count, instance)}; the engine is closed"""
    import torch

    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(N, G.MSG_LEN, max_steps=2, device=dev, n_buffers=2, n_keys=K, agg_inputs=mask, **options)
    b = G.batches(oracle)
    out, keep = {}, []
    for name in G.BATCHES:  # wave | mixed 0, mixed 1 | mixed 2
        d = tuple(to_dev(torch, a) for a in G.stacked(b[name][0]))
        w, r, c = eng.new_witness_tensor(), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        inst = eng.new_instance_tensor() if mask else None
        eng.submit_aggregate(d[0], d[1], d[3], d[2], witness=w, result=r, count=c, instance=inst)
        if name == "wave":
            eng.flush()
        out[name] = (w, r, c, inst)
        keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    return out


def check_engine(pkg, oracle, tag, mask=0, **options):
    import torch

    out = run_engine(pkg, oracle, tag, mask, **options)
    b = G.batches(oracle)
    failures = []
    for name, (w, r, c, inst) in out.items():
        failures += compare(oracle, torch, "%s %s" % (tag, name), mask, b[name][0], G.check_lanes(name), w, r, c, inst)
    assert not failures, failures[:12]


@pytest.mark.parametrize("options", [dict(chain_variant=1), dict(chain_variant=2), dict(latency_mode=2)], ids=["chain_variant 1", "chain_variant 2", "latency_mode 2"])
def test_witness_keys(pkg, oracle, options):
    """agg_inputs 0: the out-of-line, the inlined and the grouped compilation of k_agg_keys and k_agg_sum"""
    check_engine(pkg, oracle, str(options), **options)


@pytest.mark.parametrize("mask", [1, 2, 3, 15])
def test_input_arguments(pkg, oracle, mask):
    """agg_inputs 1, 2, 3, 15 through submit_aggregate(..., instance=): k_agg_sum_in on the affine inputs (masks with the keys Input: T itself is
    summed there), k_agg_sum over allocated keys with an empty bitmap segment (mask 2), k_agg_instance's vectors against the shim's"""
    check_engine(pkg, oracle, "agg_inputs %d" % mask, mask)


def test_direct_call(pkg, oracle):
    """pkg.aggregate_verify = blsw_aggregate_verify_batch, one launch per kernel and no staging, on the three mixed batches and on "wave\""""
    import torch

    b = G.batches(oracle)
    failures = []
    for name in G.BATCHES:
        pks, bm, msg, sig = (to_dev(torch, a) for a in G.stacked(b[name][0]))
        r, c, w = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), bm, msg, pkg.SignatureVar.new_witness(sig))
        failures += compare(oracle, torch, "direct " + name, 0, b[name][0], G.check_lanes(name), w, r, c)
        del w
    assert not failures, failures[:12]


def test_shared_keys(pkg, oracle):
    """shared_keys = 1: one KeySet holding P, -P, O, Q, the key of r - (s_P + s_Q) and T; the edges are reached by bitmaps alone (k_agg_sum_ks), and
    k_keyset_alloc allocates O and T: its table is the oracle's allocation segment"""
    import torch

    dev = torch.device("cuda:0")
    b = G.keyset_batches(oracle)
    keys = G.keyset_cases(oracle)[0].pks
    ks = pkg.KeySet(to_dev(torch, keys))
    eng = pkg.WitnessEngine(N, G.MSG_LEN, max_steps=2, device=dev, n_buffers=2, n_keys=K, shared_keys=1)
    out, keep = {}, []
    for name in ("wave", "mixed"):
        _, bm, msg, sig = (to_dev(torch, a) for a in G.stacked(b[name][0]))
        w, r, c = eng.new_witness_tensor(), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        eng.submit_aggregate_keyset(ks, bm, sig, msg, witness=w, result=r, count=c)
        eng.flush()
        out[name] = (w, r, c)
        keep.append((bm, msg, sig))
    torch.cuda.synchronize()
    failures = []
    for name, (w, r, c) in out.items():
        failures += compare(oracle, torch, "shared_keys " + name, 0, b[name][0], G.check_lanes(name), w, r, c)
    lay = pkg.layout_aggregate(G.MSG_LEN, K)
    seg = lay["off_bitmap"]
    assert lay["off_keys"] == 0 and seg == K * G.SEG_PK_ALLOC and tuple(ks.table.shape) == (seg, 6)
    same(torch, "KeySet.table", 0, ks.table, expected(oracle, torch, 0, b["mixed"][0][0])[2][:seg])
    eng.close()
    ks.close()
    assert not failures, failures[:12]


def test_compact_round_trip(pkg, oracle):
    """the three mixed batches through submit_aggregate_compact on one engine and expand_compact on a second: the plain vectors, bit for bit.
    The compact form takes n a multiple of 64: 128 instances, the 70 followed by their first 58"""
    import torch

    dev = torch.device("cuda:0")
    n = 128
    b = G.batches(oracle)
    eng = pkg.WitnessEngine(n, G.MSG_LEN, max_steps=2, device=dev, n_buffers=2, n_keys=K)
    recv = pkg.WitnessEngine(n, G.MSG_LEN, max_steps=2, device=dev, n_buffers=2, n_keys=K)
    names = ("mixed 0", "mixed 1", "mixed 2")
    comp = eng.new_compact_buffer(len(names))
    rows = {name: b[name][0] + b[name][0][:n - N] for name in names}
    res, keep = {}, []
    for k, name in enumerate(names):
        d = tuple(to_dev(torch, a) for a in G.stacked(rows[name]))
        r, c = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        eng.submit_aggregate_compact(d[0], d[1], d[3], d[2], comp[k], result=r, count=c)
        res[name] = (r, c)
        keep.append(d)
    eng.flush()
    torch.cuda.synchronize()
    failures = []
    w = recv.new_witness_tensor()
    for k, name in enumerate(names):
        recv.expand_compact(comp[k], w)
        torch.cuda.synchronize()
        lanes = set(G.check_lanes(name)) | {i + N for i in G.check_lanes(name) if i + N < n}
        failures += compare(oracle, torch, "compact " + name, 0, rows[name], lanes, w, *res[name])
    eng.close()
    recv.close()
    assert not failures, failures[:12]


def first_rows(oracle, rows, at, nz_row, keys_input):
    """the first unsatisfied row of every instance: -1, or pk != 0's row where the sum of the selected keys is the identity"""
    names = {c.name: c for c in G.cases(oracle) + [G.wave_case(oracle)] + G.wave_tail(oracle) + G.keyset_cases(oracle)}
    return [nz_row if i in at and G.selected_sum(names[at[i]], keys_input) is None else -1 for i in range(len(rows))]


@pytest.mark.parametrize("mask", [0, 15])
def test_device_checker(pkg, oracle, mask):
    """blsw_r1cs_check over the vectors (mask 15: and the instance tensors) of all four batches: every lane is satisfied, the tampered ones
    included, but for the lanes whose key sum is the identity, whose first unsatisfied row is the one that enforces pk != 0"""
    import torch

    mats, nz_row, _ = G.system(pkg, mask)
    chk = pkg.ConstraintChecker.from_matrices(mats, device=torch.device("cuda:0"))
    out = run_engine(pkg, oracle, "checker", mask)
    b = G.batches(oracle)
    for name, (w, r, c, inst) in out.items():
        want = first_rows(oracle, b[name][0], b[name][1], nz_row, bool(mask & A.KEYS))
        assert chk.which_is_unsatisfied(w, inst).cpu().tolist() == want, name
        assert chk.first_unreduced(w, inst).cpu().tolist() == [-1] * N, name
        assert any(x >= 0 for x in want) and any(not v for v, x in zip(r.cpu().tolist(), want) if x < 0)  # identity sums, and satisfied lanes whose Boolean is false
    chk.close()


def test_device_checker_keyset(pkg, oracle):
    """the key-set step: blsw_r1cs_check_keyset on the table that holds O and T (the head rows, once), blsw_r1cs_check on the step's vectors"""
    import torch

    dev = torch.device("cuda:0")
    mats, nz_row, _ = G.system(pkg, 0)
    chk = pkg.ConstraintChecker.from_matrices(mats, device=dev)
    b = G.keyset_batches(oracle)
    ks = pkg.KeySet(to_dev(torch, G.keyset_cases(oracle)[0].pks))
    assert chk.check_keyset(ks) == (-1, -1)
    for name in ("wave", "mixed"):
        _, bm, msg, sig = (to_dev(torch, a) for a in G.stacked(b[name][0]))
        r, c, w = pkg.aggregate_verify(pkg.ParametersVar(), ks, bm, msg, pkg.SignatureVar.new_witness(sig))
        want = first_rows(oracle, b[name][0], b[name][1], nz_row, False)
        assert chk.which_is_unsatisfied(w).cpu().tolist() == want and any(x >= 0 for x in want), name
        del w
    ks.close()
    chk.close()


def test_committee_cross_check(pkg, oracle):
    """two implementations of the key sum in one library: every case whose keys are in the subgroup or O through the circuit
    (pkg.aggregate_verify) and, compressed, through pkg.committee_verify(group = 0). The counts are equal; d_agg48 is oracle.g1_compress of the
    point prepare.pk ends with (the infinity encoding for (0, 0)); the value entry's verdict, which is false for an identity aggregate, is the
    circuit's Boolean and sum != O, and is the statement known by construction"""
    import torch

    dev = torch.device("cuda:0")
    cs = [c for c in G.cases(oracle) + [G.wave_case(oracle)] + G.wave_tail(oracle) if c.subgroup]
    assert {c.letter for c in cs} == set("abcdefgiw")
    rows = [(c.pks, c.bitmap, c.msg, c.sig) for c in cs]
    n = len(rows)
    pks, bm, msg, sig = (to_dev(torch, a) for a in G.stacked(rows))
    r, cnt, w = pkg.aggregate_verify(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(pks), bm, msg, pkg.SignatureVar.new_witness(sig))
    off = pkg.layout_aggregate(G.MSG_LEN, K)["off_prep_pk"]
    points = w[:, off + 5:off + 7].reshape(n, 12).cpu().numpy().view(np.uint64)
    boolean, count = r.cpu().numpy().astype(bool), cnt.cpu().tolist()
    del w
    u8 = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev)
    failures = []
    for i, c in enumerate(cs):
        pks48 = np.stack([np.frombuffer(oracle.g1_compress(xy), dtype=np.uint8) for xy in c.pks])
        sig96 = np.frombuffer(oracle.g2_compress(c.sig), dtype=np.uint8)[None]
        res, ccount, agg = pkg.committee_verify(u8(pks48), u8(c.bitmap[None]), u8(c.msg[None]), u8(sig96), group=0, want_count=True, want_aggregate=True)
        zero_sum = not points[i].any()
        try:
            assert zero_sum == (c.sum_secret == 0) and bool(boolean[i]) == c.boolean, (c.name, zero_sum, boolean[i])
            assert ccount.cpu().tolist() == [count[i]] == [int(c.bitmap.sum())], (c.name, ccount.cpu().tolist(), count[i])
            assert bytes(agg[0].cpu().numpy()) == oracle.g1_compress(points[i]), c.name
            assert bool(res.cpu().tolist()[0]) == (bool(boolean[i]) and not zero_sum) == c.expect, (c.name, res.cpu().tolist(), boolean[i], zero_sum)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures
