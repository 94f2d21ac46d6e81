"""aggregate_verify with public inputs (options.agg_inputs, ABI 13), host side: the product's layout, matrices, device logic (compiled for the host)
and argument rules against tests/agg_inputs' shim — the circuit of constraints.rs:378-441 composed from the oracle's building blocks with each of its
four arguments Witness or Input (pv_new_input, an input boolean with its booleanity constraint, the message chunks, mapped_aggregate,
bls_verify_gadget). Exact comparisons, no tolerance. No GPU."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import agg_inputs_lib as A
from tests import synth
from tests.oracle_lib import P_MOD

ERR_ARG = 1  # BLSW_ERR_ARG
SEG_PK_ALLOC, SEG_SIG_ALLOC, SEG_MSG_CHUNK = 1942, 12413, 761


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def _mont(v):
    v = (v << 384) % P_MOD
    return np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


def _layout_cases():
    cases = [(2, 32, m) for m in range(16)]
    for K in (1, 5):
        for msg_len in (0, 47, 48):
            cases += [(K, msg_len, m) for m in (0, 3, 15)]
    return cases


@pytest.mark.parametrize("K,msg_len,mask", _layout_cases())
def test_layout_matches_the_shim(pkg, K, msg_len, mask):
    marks, nw, nc, ni = A.layout(K, msg_len, mask)
    lay = pkg.layout_aggregate(msg_len, K, mask)
    c = A.chunks(msg_len)
    assert lay["n_instance_vars"] == ni == A.n_instance_vars(K, msg_len, mask)
    assert lay["n_witness"] == nw and lay["n_keys"] == K and lay["msg_len"] == msg_len and lay["n_pairs"] == 1
    for name, field in A.MARKS:
        assert marks[name] == lay[field], name
    # what the header says a caller reads the modes from
    assert lay["pk_mode"] == (1 if mask & A.KEYS else 0) and lay["sig_mode"] == (1 if mask & A.SIG else 0)
    assert (lay["off_bitmap"] == lay["off_keys"]) == bool(mask & A.KEYS)
    assert (lay["off_msg"] == lay["off_bitmap"]) == bool(mask & A.BITMAP)
    assert lay["stride_msg"] == (SEG_MSG_CHUNK * c if mask & A.MSG else 8 * msg_len)
    base = pkg.layout_aggregate(msg_len, K)
    want = base["n_witness"] - (K * SEG_PK_ALLOC if mask & A.KEYS else 0) - (K if mask & A.BITMAP else 0) - (SEG_SIG_ALLOC if mask & A.SIG else 0) + \
        ((SEG_MSG_CHUNK * c - 8 * msg_len) if mask & A.MSG else 0)
    assert nw == want
    # mask 0 is blsw_layout_aggregate field for field, also through the new entry point
    L = pkg.blsw_layout_t()
    assert pkg.lib().blsw_layout_aggregate_inputs(msg_len, K, 0, ctypes.byref(L)) == 0
    assert {n: getattr(L, n) for n in pkg._LAYOUT_FIELDS} == base
    if mask == 0:
        assert lay == base
    # the host compilation of the key source's header computes the same table
    A.emit().aggemit_layout(msg_len, K, mask, ctypes.byref(L))
    assert {n: getattr(L, n) for n in pkg._LAYOUT_FIELDS} == lay


def test_layout_of_the_512_key_committee(pkg):
    """the figures the feature was specified with: 512 keys, a 32-byte message (no synthesis: the layout call alone)"""
    all_witness, keys_bitmap = pkg.layout_aggregate(32, 512), pkg.layout_aggregate(32, 512, A.KEYS | A.BITMAP)
    assert (all_witness["n_witness"], all_witness["n_instance_vars"]) == (1724897, 1)
    assert all_witness["off_bitmap"] - all_witness["off_keys"] == 994304
    assert (keys_bitmap["n_witness"], keys_bitmap["n_instance_vars"]) == (730081, 2049)
    assert keys_bitmap["off_keys"] == keys_bitmap["off_bitmap"] == keys_bitmap["off_msg"] == 0
    assert pkg.layout_aggregate(32, 512, 15)["n_instance_vars"] == 2049 + 1 + 6


def _same(mo, mp):
    return all(np.array_equal(x, y) for x, y in zip(mo, mp))


@pytest.mark.parametrize("mask", [1, 2, 12, 15])
def test_matrices_equal_the_shims(pkg, mask):
    K, msg_len = 2, 32
    nc, nw, ni, S = A.matrices(K, msg_len, mask)
    P = pkg.matrices(msg_len, n_keys=K, agg_inputs=mask)
    assert (P["n_constraints"], P["n_witness"], P["n_instance_vars"]) == (nc, nw, ni)
    for k, name in enumerate("ABC"):
        assert _same(S[k], P[name]), "matrix %s differs" % name
    assert int(max(P[n][1].max() for n in "ABC")) == ni + nw - 1  # the last witness's column
    # the constraint count differs from the all-Witness system's only by what key / signature / message allocation contributes: the K booleanity
    # rows of Input bits stay
    d = _allocation_rows(pkg)
    want = d["base"] - (K * d["key"] if mask & A.KEYS else 0) - (d["sig"] if mask & A.SIG else 0) + (d["msg"] if mask & A.MSG else 0)
    assert nc == want
    if mask & A.BITMAP:  # bit k's row: (1 - b_k) * b_k = 0 on the bit's instance column, wherever the keys' rows put it
        b0 = 1 + (3 * K if mask & A.KEYS else 0)
        r0 = 0 if mask & A.KEYS else K * d["key"]
        for k in range(K):
            rows = [list(col[rp[r0 + k]:rp[r0 + k + 1]]) for rp, col, _ in (P["A"], P["B"], P["C"])]
            assert rows == [[0, b0 + k], [b0 + k], []]


_ROWS = {}


def _allocation_rows(pkg):
    """constraints of the all-Witness system (K = 2, 32 bytes) and what one key's / the signature's / the message's allocation contributes, from the
    single-key systems"""
    if not _ROWS:
        n = lambda **kw: int(pkg.matrices(32, **kw)["n_constraints"])
        single = n()
        _ROWS.update(base=n(n_keys=2), key=single - n(pk_mode=1), sig=single - n(sig_mode=1), msg=n(msg_mode=1) - single)
    return _ROWS


def test_matrices_mask_0_is_the_all_witness_system(pkg):
    L = pkg.lib()
    base = pkg.matrices(32, n_keys=2, n_pairs=1)
    info = pkg.blsw_matrices_info_t()
    assert L.blsw_matrices_info_aggregate_inputs(32, 2, 0, ctypes.byref(info)) == 0
    assert (info.n_constraints, info.n_instance_vars, info.n_witness) == (base["n_constraints"], 1, base["n_witness"])
    assert [info.nnz[m] for m in range(3)] == [base[n][1].shape[0] for n in "ABC"]
    rp = [np.zeros(info.n_constraints + 1, dtype=np.uint64) for _ in range(3)]
    col = [np.zeros(info.nnz[m], dtype=np.uint32) for m in range(3)]
    val = [np.zeros((info.nnz[m], 6), dtype=np.uint64) for m in range(3)]
    out = pkg.blsw_matrices_t()
    for m in range(3):
        out.row_ptr[m] = rp[m].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        out.col[m] = col[m].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        out.val[m] = val[m].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.blsw_matrices_fill_aggregate_inputs(32, 2, 0, ctypes.byref(info), ctypes.byref(out)) == 0
    for m, name in enumerate("ABC"):
        assert _same((rp[m], col[m], val[m]), base[name])


def test_shim_assignment_satisfies_its_system(oracle):
    K = 3
    for mask, tamper in ((15, False), (3, True), (10, False)):  # valid and tampered instances
        pks, bm, msg, sig, expect = synth.make_aggregate(oracle, K, [1, 0, 1], start=40, tamper=tamper)
        res, cnt, w, inst, _ = A.witness(pks, bm, msg.tobytes(), sig, mask)
        assert res == expect and cnt == 2
        assert A.check(pks, bm, msg.tobytes(), sig, mask, inst, w) == -1
        assert A.check(pks, bm, msg.tobytes(), sig, mask) == -1
        b0 = 1 + (3 * K if mask & A.KEYS else 0)
        bad = inst.copy()
        bad[b0 + 1] = _mont(2)  # bit 1 := 2: its booleanity row (1 - b_1) * b_1 = 0 is the first one that fails
        got = A.check(pks, bm, msg.tobytes(), sig, mask, bad, w)
        S = A.matrices(K, 32, mask)[3]
        rows = [list(col[rp[got]:rp[got + 1]]) for rp, col, _ in S]
        assert rows == [[0, b0 + 1], [b0 + 1], []]
        if mask & A.KEYS:  # Input keys have no constraints: the bitmap's rows are the first K
            assert got == 1
            bad = inst.copy()
            bad[1] = _mont(5)  # a key input changed: the system no longer holds
            assert A.check(pks, bm, msg.tobytes(), sig, mask, bad, w) >= 0


def _logic_cases():
    K = 4
    return [("none", K, [0, 0, 0, 0], None), ("one", K, [0, 0, 1, 0], None), ("all", K, [1, 1, 1, 1], None), ("zero_key_selected", K, [1, 1, 0, 1], 1),
            ("zero_key_not_selected", K, [1, 0, 1, 1], 1), ("first", K, [1, 0, 0, 0], None), ("single_key", 1, [1], None)]


@pytest.mark.parametrize("mask", [1, 3, 15])
@pytest.mark.parametrize("name,K,bitmap,zero_at", _logic_cases())
def test_device_logic_on_the_host(pkg, oracle, name, K, bitmap, zero_at, mask):
    """csrc/agg_input.hpp's key source + chain_mapped_aggregate + chain_g1_post + the instance writer's element function, compiled for the CPU,
    against the shim's count / agg / pk_not_zero / prep_pk segments and instance elements"""
    pks, _, msg, sig, _ = synth.make_aggregate(oracle, K, [1] * K, start=7)
    pks = pks.copy()
    if zero_at is not None:
        pks[zero_at] = 0  # the (0, 0) encoding of the point at infinity
    bm = np.array(bitmap, dtype=np.uint8)
    res, cnt, w, inst, _ = A.witness(pks, bm, msg.tobytes(), sig, mask)
    lay = pkg.layout_aggregate(32, K, mask)
    got_cnt, gw, ginst = A.emit_instance(pks, bm, 32, mask, lay["n_witness"])
    assert got_cnt == cnt == int(bm.sum())
    for a, b in (("off_bitmap", "off_msg"), ("off_count", "off_agg"), ("off_agg", "off_pk_not_zero"), ("off_pk_not_zero", "off_expand"), ("off_prep_pk", "off_prep_sig")):
        assert np.array_equal(gw[lay[a]:lay[b]], w[lay[a]:lay[b]]), "segment %s differs" % a
    head = 1 + 3 * K + (K if mask & A.BITMAP else 0)
    assert ginst.shape[0] == head and np.array_equal(ginst, inst[:head])
    if zero_at is not None:  # (0, 1, 0)
        assert np.array_equal(inst[1 + 3 * zero_at:4 + 3 * zero_at], np.stack([_mont(0), _mont(1), _mont(0)]))


def test_argument_rules(pkg):
    L = pkg.lib()
    o = pkg.blsw_engine_options_t()
    assert L.blsw_engine_options_default(ctypes.byref(o)) == 0 and o.agg_inputs == 0
    assert pkg.engine_options().agg_inputs == 0 and pkg.engine_options(n_keys=4, agg_inputs=3).agg_inputs == 3

    def ws(n=64, max_steps=2, n_buffers=2, **kw):
        opt = pkg.engine_options(**kw)
        b = ctypes.c_uint64(0)
        rc = L.blsw_engine_workspace_bytes_ex(n, 32, max_steps, n_buffers, ctypes.byref(opt), ctypes.byref(b))
        return rc, b.value

    def create(**kw):
        opt = pkg.engine_options(**kw)
        e = ctypes.c_void_p()
        return L.blsw_engine_create_ex(ctypes.byref(e), 64, 32, 2, 2, ctypes.byref(opt), ctypes.c_void_p(1), 1 << 40)

    for m in range(16):
        assert ws(n_keys=4, agg_inputs=m)[0] == 0
    for bad in ({"n_keys": 4, "agg_inputs": 16}, {"agg_inputs": 1}, {"agg_inputs": 15, "n_pairs": 2}, {"n_keys": 4, "agg_inputs": 1, "g2_mode": 1},
                # the aggregate circuit's modes are agg_inputs: the single-key fields stay refused together with n_keys
                {"n_keys": 4, "pk_mode": 1}, {"n_keys": 4, "sig_mode": 1}, {"n_keys": 4, "msg_mode": 1}, {"n_keys": 4, "agg_inputs": 3, "pk_mode": 1},
                {"n_keys": 4, "agg_inputs": 4, "msg_mode": 1}, {"n_keys": 4, "agg_inputs": 1, "params_mode": 1}):
        assert ws(**bad)[0] == ERR_ARG, bad
        assert create(**bad) == ERR_ARG, bad  # before any device call
    # Input keys: nothing allocates keys, the workspace holds no projective keys (3 * N * K * 48 bytes per group buffer)
    K, n, steps, nb = 512, 64, 2, 2
    w0, w1, w2 = ws(n, steps, nb, n_keys=K)[1], ws(n, steps, nb, n_keys=K, agg_inputs=1)[1], ws(n, steps, nb, n_keys=K, agg_inputs=2)[1]
    assert w0 - w1 >= nb * 3 * (n * steps) * K * 48
    assert w2 < w0 and w0 - w2 < nb * 3 * (n * steps) * K * 48  # an Input bitmap only shortens the staged rows
    lay, info = pkg.blsw_layout_t(), pkg.blsw_matrices_info_t()
    assert L.blsw_layout_aggregate_inputs(32, 4, 16, ctypes.byref(lay)) == ERR_ARG
    assert L.blsw_layout_aggregate_inputs(32, 0, 1, ctypes.byref(lay)) == ERR_ARG
    assert L.blsw_layout_aggregate_inputs(32, 4, 15, None) == ERR_ARG
    assert L.blsw_matrices_info_aggregate_inputs(32, 4, 16, ctypes.byref(info)) == ERR_ARG
    assert L.blsw_matrices_info_aggregate_inputs(32, 0, 1, ctypes.byref(info)) == ERR_ARG
    assert L.blsw_matrices_fill_aggregate_inputs(32, 4, 16, ctypes.byref(info), None) == ERR_ARG
    # the single-key entry points do not reach the aggregate circuit
    assert L.blsw_matrices_info_io(32, 1, 0, ctypes.byref(info)) == 0 and info.n_instance_vars == 4
    assert L.blsw_engine_submit_aggregate_io(None, None, None, None, None, None, None, 0, None, None, None) == ERR_ARG
    for bad in (dict(msg_mode=1), dict(pk_mode=1), dict(sig_mode=1)):
        with pytest.raises(pkg.BlswError):
            pkg.matrices(32, n_keys=2, **bad)
        with pytest.raises(pkg.BlswError):
            pkg.matrices(32, n_keys=2, agg_inputs=3, **bad)
    with pytest.raises(pkg.BlswError):
        pkg.matrices(32, agg_inputs=3)
    with pytest.raises(pkg.BlswError):
        pkg.matrices(32, n_keys=2, agg_inputs=16)
    with pytest.raises(pkg.BlswError):
        pkg.layout_aggregate(32, 2, 16)
    with pytest.raises(pkg.BlswError):
        pkg.Boolean(None, "Constant")
    assert pkg.Boolean.new_input(None).mode == "Input" and pkg.Boolean.new_witness(None).mode == "Witness" and pkg.Boolean(None).mode == "Witness"
    assert (pkg.AGG_KEYS_INPUT, pkg.AGG_BITMAP_INPUT, pkg.AGG_MSG_INPUT, pkg.AGG_SIG_INPUT) == (1, 2, 4, 8)


def test_golden_digests_are_what_the_shim_emits(pkg, oracle):
    """tests/golden/agg_inputs_digests.json (the hand-off to a later real-arkworks comparison) against the shim, for the reference's 512-key case"""
    import hashlib
    import json
    import os

    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_inputs_digests.json")))["agg_inputs"]
    pks, msg, sig, hexes = A.reference_case(oracle)
    bm = np.zeros(512, dtype=np.uint8)
    bm[:2] = 1
    for mask in (3, 15):
        g = gold["mask_%d" % mask]
        res, cnt, w, inst, nc = A.witness(pks, bm, msg, sig, mask)
        c = g["cases"]["constraints_rs_378_first_two_selected"]
        assert (c["pubkey_first"], c["pubkey_rest"], c["signature"]) == hexes and c["message"] == msg.hex()
        assert (c["n_instance_vars"], c["n_witness"], c["n_constraints"], c["result"], c["count"]) == (inst.shape[0], w.shape[0], nc, res, cnt) and res and cnt == 2
        b = np.ascontiguousarray(w).view(np.uint8).reshape(w.shape[0], 48)
        assert c["sha256_instance"] == hashlib.sha256(np.ascontiguousarray(inst).tobytes()).hexdigest()
        assert c["sha256_all"] == hashlib.sha256(b.tobytes()).hexdigest()
        assert g["segments"] == A.segments(pkg.layout_aggregate(32, 512, mask))
        for name, lo, hi in g["segments"]:
            assert c["sha256_segments"][name] == hashlib.sha256(b[lo:hi].tobytes()).hexdigest(), name
