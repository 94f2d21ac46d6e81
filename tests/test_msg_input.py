"""The message allocated as public inputs (UInt8::new_input_vec, options.msg_mode 1, ABI 12), host side: the product's layout, matrices,
emitter (compiled for the host) and argument rules against tests/msg_input's shim — the circuit composed from the oracle's building blocks
(finput, fto_bits_le, U8 from the bits, bls_verify_gadget). No GPU."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import msg_input_lib as M
from tests import synth
from tests.oracle_lib import P_MOD

ERR_ARG = 1  # BLSW_ERR_ARG
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (pk_mode, sig_mode)
# the numbers the issue states for the rule (n_instance_vars, n_witness, constraints), composed from the oracle's blocks
TABLE = {(0, 0, 0): (1, 672864, 679061), (32, 0, 0): (2, 707932, 714549), (47, 0, 0): (2, 708163, 714780), (48, 0, 0): (3, 708937, 715707),
         (32, 1, 1): (11, 693577, 700194)}
MARKS = (("msg", "off_msg"), ("pk_alloc", "off_pk_alloc"), ("sig_alloc", "off_sig_alloc"), ("verify.pk_not_zero", "off_pk_not_zero"), ("hash.expand", "off_expand"),
         ("hash.map0", "off_map0"), ("hash.map1", "off_map1"), ("hash.add", "off_add"), ("hash.clear_cofactor", "off_cofactor"), ("prepare.h", "off_prep_h"),
         ("prepare.pk", "off_prep_pk"), ("prepare.sig", "off_prep_sig"), ("miller", "off_miller"), ("final_exp", "off_final_exp"), ("is_one", "off_is_one"))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


def _one_mont():
    v = (1 << 384) % P_MOD
    return np.array([(v >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


def _add_one(e):
    """e + 1 in Montgomery limbs"""
    a = sum(int(x) << (64 * k) for k, x in enumerate(e))
    b = (a + (1 << 384)) % P_MOD
    return np.array([(b >> (64 * k)) & (2**64 - 1) for k in range(6)], dtype=np.uint64)


@pytest.mark.parametrize("msg_len", [0, 1, 32, 46, 47, 48, 95, 120])
@pytest.mark.parametrize("pk_mode,sig_mode", MODES)
def test_layout_matches_the_shim(pkg, msg_len, pk_mode, sig_mode):
    marks, nw, nc, ni = M.layout(msg_len, pk_mode, sig_mode)
    lay = pkg.layout(msg_len, pk_mode=pk_mode, sig_mode=sig_mode, msg_mode="input")
    c = M.chunks(msg_len)
    assert lay["n_instance_vars"] == ni == 1 + c + 3 * pk_mode + 6 * sig_mode
    assert c == ni - 1 - 3 * lay["pk_mode"] - 6 * lay["sig_mode"] == pkg.msg_input_chunks(msg_len)  # the header's recovery rule
    assert lay["n_witness"] == nw and lay["stride_msg"] == 761 * c and lay["msg_len"] == msg_len
    for name, field in MARKS:
        assert marks[name] == lay[field], name
    if (msg_len, pk_mode, sig_mode) in TABLE:
        assert (ni, nw, nc) == TABLE[(msg_len, pk_mode, sig_mode)]
    # every segment behind the message moves by the difference of the two message segments, nothing else changes
    base = pkg.layout(msg_len, pk_mode=pk_mode, sig_mode=sig_mode)
    assert pkg.layout(msg_len, pk_mode=pk_mode, sig_mode=sig_mode, msg_mode=0) == base
    d = 761 * c - 8 * msg_len
    for name, field in MARKS[1:]:
        assert lay[field] == base[field] + d, field
    assert lay["n_witness"] == base["n_witness"] + d
    # the host compilation of the emitter's header computes the same table
    L = pkg.blsw_layout_t()
    M.emit().msgemit_layout(msg_len, 1, pk_mode, sig_mode, ctypes.byref(L))
    assert {n: getattr(L, n) for n in pkg._LAYOUT_FIELDS} == lay


def _same(mo, mp):
    return all(np.array_equal(x, y) for x, y in zip(mo, mp))


@pytest.mark.parametrize("msg_len,pk_mode,sig_mode", [(32, 0, 0), (48, 1, 1), (0, 0, 0)])
def test_matrices_equal_the_shims(pkg, msg_len, pk_mode, sig_mode):
    nc, nw, ni, S = M.matrices(msg_len, pk_mode, sig_mode)
    P = pkg.matrices(msg_len, pk_mode=pk_mode, sig_mode=sig_mode, msg_mode="input")
    assert (P["n_constraints"], P["n_witness"], P["n_instance_vars"]) == (nc, nw, ni)
    for k, name in enumerate("ABC"):
        assert _same(S[k], P[name]), "matrix %s differs" % name
    assert int(max(P[n][1].max() for n in "ABC")) == ni + nw - 1  # the last witness's column
    if msg_len == 0:  # no chunk: the Witness-mode system
        W = pkg.matrices(0, pk_mode=pk_mode, sig_mode=sig_mode)
        assert (W["n_constraints"], W["n_witness"], W["n_instance_vars"]) == (nc, nw, ni)
        for name in "ABC":
            assert _same(W[name], P[name])
    else:  # the packing constraint of chunk 0 is row 381: 0 * 0 = sum 2^i b_i - m_0
        rp, col, val = P["C"]
        row = col[rp[381]:rp[382]]
        assert list(row) == [1] + [ni + i for i in range(381)]


def _segment_cases():
    rng = np.random.default_rng(7)
    cases = [("ff47", bytes([0xFF]) * 47), ("ff94", bytes([0xFF]) * 94), ("zero48", bytes(48))]
    for n in (46, 47, 48, 93, 94, 95, 1, 120):
        cases.append(("rand%d" % n, rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    return cases


@pytest.mark.parametrize("name,msg", _segment_cases())
def test_emitter_equals_the_shims_message_segment(oracle, name, msg):
    pk, _, sig, _ = synth.make_batch(oracle, 1)
    _, w, inst, _ = M.witness(pk[0], msg, sig[0])
    seg, inp = M.emit_segment(msg)
    c = M.chunks(len(msg))
    assert seg.shape == (761 * c, 6) and inp.shape == (c, 6)
    assert np.array_equal(seg, w[:761 * c]), "message segment differs"
    assert np.array_equal(inp, inst[1:1 + c]), "message inputs differ"
    # the message's bits are the chunks' low 376 booleans, LSB first
    one = _one_mont()
    bits = [b for j in range(c) for b in seg[761 * j:761 * j + 376]]
    for k in range(8 * len(msg)):
        want = (msg[k // 8] >> (k % 8)) & 1
        assert np.array_equal(bits[k], one if want else np.zeros(6, np.uint64)), k


def test_argument_rules(pkg):
    L = pkg.lib()
    o = pkg.blsw_engine_options_t()
    assert L.blsw_engine_options_default(ctypes.byref(o)) == 0 and o.msg_mode == 0
    assert pkg.engine_options().msg_mode == 0

    def ws(**kw):
        opt = pkg.engine_options()
        for k, v in kw.items():
            setattr(opt, k, v)
        b = ctypes.c_uint64(0)
        rc = L.blsw_engine_workspace_bytes_ex(64, 32, 2, 2, ctypes.byref(opt), ctypes.byref(b))
        return rc, b.value

    rc0, b0 = ws()
    rc1, b1 = ws(msg_mode=1)
    assert rc0 == rc1 == 0 and b1 > b0  # the staging holds the larger message segment
    assert ws(msg_mode=1, pk_mode=1, sig_mode=1)[0] == 0
    for bad in ({"msg_mode": 2}, {"msg_mode": 1, "n_keys": 2}, {"msg_mode": 1, "n_pairs": 2}, {"msg_mode": 1, "params_mode": 1}, {"msg_mode": 1, "g2_mode": 1}):
        assert ws(**bad)[0] == ERR_ARG, bad
    # create_ex refuses the same sets before it looks at the device
    for bad in ({"msg_mode": 2}, {"msg_mode": 1, "n_keys": 2}, {"msg_mode": 1, "params_mode": 1}):
        opt = pkg.engine_options(**bad)
        e = ctypes.c_void_p()
        assert L.blsw_engine_create_ex(ctypes.byref(e), 64, 32, 2, 2, ctypes.byref(opt), ctypes.c_void_p(1), 1 << 40) == ERR_ARG
    lay = pkg.blsw_layout_t()
    assert L.blsw_layout_inputs(32, 2, 0, 0, ctypes.byref(lay)) == ERR_ARG
    assert L.blsw_layout_inputs(32, 0, 2, 0, ctypes.byref(lay)) == ERR_ARG
    info = pkg.blsw_matrices_info_t()
    assert L.blsw_matrices_info_inputs(32, 2, 0, 0, ctypes.byref(info)) == ERR_ARG
    # msg_mode 0 is the _io circuit
    assert L.blsw_layout_inputs(40, 0, 1, 0, ctypes.byref(lay)) == 0
    assert {n: getattr(lay, n) for n in pkg._LAYOUT_FIELDS} == pkg.layout(40, pk_mode=1)
    with pytest.raises(pkg.BlswError):
        pkg.layout(32, params_mode=1, msg_mode=1)
    with pytest.raises(pkg.BlswError):
        pkg.matrices(32, n_keys=2, msg_mode=1)
    with pytest.raises(pkg.BlswError):
        pkg.UInt8(None, "Constant")
    assert pkg.UInt8.new_input_vec(None).mode == "Input" and pkg.UInt8.new_witness_vec(None).mode == "Witness"


def test_shim_assignment_satisfies_its_system(oracle):
    pk, msg, sig, expect = synth.make_batch(oracle, 16)
    for i, (pm, sm) in ((0, (0, 0)), (15, (1, 1))):  # a valid and a tampered instance
        res, w, inst, _ = M.witness(pk[i], msg[i].tobytes(), sig[i], pm, sm)
        assert res == bool(expect[i])
        assert M.check(pk[i], msg[i].tobytes(), sig[i], pm, sm, inst, w) == -1
        bad = inst.copy()
        bad[1] = _add_one(bad[1])  # the first message input + 1: the packing constraint of chunk 0 fails first
        assert M.check(pk[i], msg[i].tobytes(), sig[i], pm, sm, bad, w) == 381
