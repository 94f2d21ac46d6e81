"""The SHA-256 gadget and hash_to_field layer (csrc/sha.hpp) on the device: the operation table of tests/devsha/ops.hpp in the two compilations
csrc/k_sha.hip gets (the grouped engine's register policy, and "inl": tests/devsha/devsha.hip) against tests/sha_ref.py, on the launches
test_sha_ref.py validates on the host, bit for bit: results, the bit words at k_sha's tile addresses in a sentinel-filled guarded buffer compared
whole (only the words of a partial last run behind a stream are excepted), word counts. Then the shipped kernels and their grids through the
public API: hash_to_g2_batch (k_sha_values) over the length sweep and at 65 535 against the oracle, and whole witness vectors of the direct call
(k_sha_inl) and a grouped engine (k_sha) at lengths no other GPU test runs. The reference's walk of a length (about a second of Python) is cached
per process in devsha_lib.gadget_walk."""
import ctypes
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import devsha_lib as D
from tests import sha_edges as X
from tests import sha_ref as S
from tests import synth

pytestmark = pytest.mark.gpu

NO_MSG_OPS = [op for op in S.OP_NAMES if not S.OPS[op][2]]
GROUP = 4  # lengths per case of the sweeps
_SHORT = [n for n in X.STREAM_LENGTHS if n < 8000]
LENGTH_GROUPS = [_SHORT[i:i + GROUP] for i in range(0, len(_SHORT), GROUP)] + [[8080], [8081]]
_ids = lambda g: "%d-%d" % (g[0], g[-1])


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = importlib.import_module("bls-verify-gadget_amd")
    p.lib()
    return p


# ---------------------------------------------------------------- the operation table, entry by entry
@pytest.mark.parametrize("op", NO_MSG_OPS)
@pytest.mark.parametrize("build", list(D.BUILDS))
def test_device_compilation_equals_reference(build, op):
    bad, items = [], 0
    for name, msg_len, cases in X.launches(op):
        bad += [(name,) + b for b in D.run_device(build, op, msg_len, cases)]
        items += len(cases)
    print("%s %s: %d launches, %d items, %d mismatches" % (build, op, len(X.launches(op)), items, len(bad)))
    assert not bad, bad[:10]


@pytest.mark.parametrize("build", list(D.BUILDS))
def test_b0_block_every_byte(build):
    bad = []
    for msg_len in X.B0_LENGTHS:
        cases = X.msg_cases("b0_block", msg_len)
        bad += [(msg_len,) + b for b in D.run_device(build, "b0_block", msg_len, cases)]
        bad += [(msg_len, n) + b for n in X.ITEM_COUNTS for b in D.run_device(build, "b0_block", msg_len, [cases[i % len(cases)] for i in range(n)])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("lengths", LENGTH_GROUPS, ids=_ids)
def test_length_sweep_70_lanes(lengths):
    """expand_message_w (streams and words) and expand_message_values (words) with 70 lanes of different messages per launch, both compilations;
    the item counts 1, 63, 64, 65 at the first length of a group"""
    bad = []
    for n in lengths:
        cases = X.msg_cases("expand_message_w", n)
        for build in D.BUILDS:
            bad += [(n, build, "w") + b for b in D.run_device(build, "expand_message_w", n, cases)]
            bad += [(n, build, "values") + b for b in D.run_device(build, "expand_message_values", n, cases)]
            if n == lengths[0] and n < 8000:
                for k in X.ITEM_COUNTS[:-1]:
                    bad += [(n, build, "w", k) + b for b in D.run_device(build, "expand_message_w", n, cases[:k])]
                    bad += [(n, build, "values", k) + b for b in D.run_device(build, "expand_message_values", n, cases[:k])]
    assert not bad, bad[:10]


@pytest.mark.parametrize("build", list(D.BUILDS))
def test_expand_message_values_65535(build):
    """the longest message the API accepts: a three-byte bit length (0x080378 bits), 1 026 blocks"""
    for k in (1, 70):
        bad = D.run_device(build, "expand_message_values", 65535, X.msg_cases("expand_message_values", 65535, k))
        assert not bad, bad[:10]


# ---------------------------------------------------------------- the shipped kernels through the public API
def _hash_to_g2(pkg, msgs):
    import torch

    m = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(len(msgs), -1).copy()).cuda() if len(msgs[0]) else torch.empty((len(msgs), 0), dtype=torch.uint8, device="cuda")
    out = pkg.hash_to_g2_batch(m)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("lengths", [_SHORT[i:i + 8] for i in range(0, len(_SHORT), 8)] + [[8080, 8081, 65535]], ids=_ids)
def test_hash_to_g2_batch_over_the_sweep(pkg, oracle, lengths):
    """blsw_hash_to_g2_batch (k_sha_values and the value chain behind it) at every length of the sweep and at 65 535, against oracle.hash_to_g2:
    the all-0xFF, the counter and a random message per length"""
    with ThreadPoolExecutor(8) as pool:
        for n in lengths:
            msgs = X.messages(n)[1:4]
            want = list(pool.map(lambda m: oracle.hash_to_g2(m)[1], msgs))
            got = _hash_to_g2(pkg, msgs)
            for i in range(len(msgs)):
                assert np.array_equal(got[i], want[i]), "msg_len %d, message %d" % (n, i)


def test_hash_to_g2_batch_refuses_65536(pkg):
    import torch

    L = pkg.lib()
    wb = ctypes.c_uint64(0)
    err = pkg._header_define("BLSW_ERR_ARG")
    assert L.blsw_hash_to_g2_workspace_bytes(1, 65536, ctypes.byref(wb)) == err
    assert L.blsw_hash_to_g2_workspace_bytes(1, 65535, ctypes.byref(wb)) == 0
    msg = torch.zeros((1, 65536), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, 24), dtype=torch.int64, device="cuda")
    ws = torch.empty(wb.value, dtype=torch.uint8, device="cuda")
    rc = L.blsw_hash_to_g2_batch(msg.data_ptr(), 65536, 1, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == err and not out.any()


def _witness_case(pkg, oracle, msg_len, n, max_steps):
    import torch

    dev = torch.device("cuda:0")
    pk, _, sig, _ = synth.make_batch(oracle, 4)
    msgs = X.messages(msg_len)[1:1 + n]
    with ThreadPoolExecutor(n) as pool:
        want = list(pool.map(lambda i: oracle.witness(pk[1 + i % 3], msgs[i], sig[1 + i % 3]), range(n)))
    eng = pkg.WitnessEngine(n, msg_len, max_steps=max_steps, device=dev, n_buffers=2 if max_steps > 1 else 1)
    d_pk = torch.from_numpy(np.stack([pk[1 + i % 3] for i in range(n)]).view(np.int64)).to(dev)
    d_sig = torch.from_numpy(np.stack([sig[1 + i % 3] for i in range(n)]).view(np.int64)).to(dev)
    d_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(n, msg_len).copy()).to(dev)
    w, r = eng.new_witness_tensor(), torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit(d_pk, d_sig, d_msg, witness=w, result=r)
    eng.flush()
    torch.cuda.synchronize()
    got_r = r.cpu().numpy().astype(bool)
    lay = pkg.layout(msg_len)
    for i in range(n):
        nw, _, res, ow = want[i]
        assert nw == w.shape[1] and res == bool(got_r[i]), (msg_len, i, nw, w.shape, res, got_r[i])
        same = torch.equal(w[i], torch.from_numpy(ow.view(np.int64)).to(dev))
        if not same:
            k = int((w[i].cpu() != torch.from_numpy(ow.view(np.int64))).any(dim=1).nonzero()[0])
            raise AssertionError("msg_len %d, instance %d: witness %d differs (hash.expand is [%d, %d))" % (msg_len, i, k, lay["off_expand"], lay["off_expand"] + lay["sha_bits"]))
    eng.close()


@pytest.mark.parametrize("msg_len", [1, 2, 5, 6, 7, 10, 61, 66, 137])
@pytest.mark.parametrize("max_steps", [1, 2], ids=["direct", "grouped"])
def test_whole_witness_at_new_lengths(pkg, oracle, max_steps, msg_len):
    """whole witness vectors and results against oracle.witness, three instances: the direct call (k_sha_inl) and a grouped engine (k_sha)"""
    _witness_case(pkg, oracle, msg_len, 3, max_steps)


@pytest.mark.parametrize("max_steps", [1, 2], ids=["direct", "grouped"])
def test_whole_witness_at_8081(pkg, oracle, max_steps):
    """one instance at the first length whose bit length has a third byte: 5 883 166 elements, 282 MB"""
    _witness_case(pkg, oracle, 8081, 1, max_steps)
