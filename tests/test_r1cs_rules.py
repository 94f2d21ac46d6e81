"""Argument rules of the device R1CS evaluator (include/blsw.h: blsw_r1cs_*) that are checked on the host before any HIP call: a malformed
CSR is refused by blsw_r1cs_device_bytes and blsw_r1cs_create with BLSW_ERR_ARG (the buffer pointer is never dereferenced), and the
encoding of the real single-key matrices holds at least 8 bytes per non-zero. Runs without a GPU."""
import ctypes
import importlib

import numpy as np
import pytest

from tests.oracle_lib import P_MOD

BLSW_ERR_ARG = 1
R = 1 << 384


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def single_key(pkg):
    return pkg.matrices(32)


def limbs(v):
    return np.array([(v >> (64 * k)) & ((1 << 64) - 1) for k in range(6)], dtype=np.uint64)


def tiny(n_instance_vars=1):
    """3 constraints over z = [one | w0, w1]: w0 * w0 = w0, w0 * w1 = w1, (w0 + 2 w1) * 1 = 5 - (2^300) w1 (Montgomery coefficients)"""
    mont = lambda c: limbs(c % P_MOD * R % P_MOD)
    o = n_instance_vars
    A = ([0, 1, 2, 4], [o, o, o, o + 1], [mont(1), mont(1), mont(1), mont(2)])
    B = ([0, 1, 2, 3], [o, o, 0], [mont(1), mont(1), mont(1)])
    C = ([0, 1, 2, 4], [o, o + 1, 0, o + 1], [mont(1), mont(1), mont(5), mont(-(1 << 300))])
    out = {"n_constraints": 3, "n_instance_vars": n_instance_vars, "n_witness": 2}
    for name, (rp, col, val) in zip("ABC", (A, B, C)):
        out[name] = (np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), np.array(val, dtype=np.uint64).reshape(-1, 6))
    return out


def copy(mats):
    return {k: (tuple(a.copy() for a in v) if k in "ABC" else v) for k, v in mats.items()}


def refused(pkg, mats):
    L = pkg.lib()
    info, m = pkg._matrices_struct(mats)
    b = ctypes.c_uint64(0)
    r = ctypes.c_void_p()
    fake = ctypes.c_void_p(0x100000)  # never dereferenced: the calls fail before any device work
    return (L.blsw_r1cs_device_bytes(ctypes.byref(info), ctypes.byref(m), ctypes.byref(b)) == BLSW_ERR_ARG
            and L.blsw_r1cs_create(ctypes.byref(r), ctypes.byref(info), ctypes.byref(m), 0, fake, 1 << 40, None) == BLSW_ERR_ARG and not r.value)


def test_tiny_system_is_accepted(pkg):
    assert pkg.r1cs_device_bytes(tiny()) >= 8 * 11
    assert pkg.r1cs_device_bytes(tiny(4)) >= 8 * 11


def test_malformed_matrices_are_refused(pkg):
    good = tiny()
    cases = {}
    m = copy(good)
    m["A"][0][2] = 5  # row_ptr decreases
    cases["row_ptr decreasing"] = m
    m = copy(good)
    m["B"][0][3] = 2  # row_ptr does not end at nnz
    cases["row_ptr end"] = m
    m = copy(good)
    m["C"][1][3] = 3  # column = n_instance_vars + n_witness
    cases["column out of range"] = m
    m = copy(good)
    m["A"][1][2], m["A"][1][3] = 2, 1  # row 2 of A: columns descending
    cases["unsorted columns"] = m
    m = copy(good)
    m["A"][1][3] = 1  # row 2 of A: a repeated column
    cases["repeated column"] = m
    m = copy(good)
    m["C"][2][2] = limbs(P_MOD)  # coefficient == p
    cases["coefficient p"] = m
    m = copy(good)
    m["B"][2][0] = limbs(P_MOD + 5)
    cases["coefficient above p"] = m
    m = copy(good)
    m["C"][2][0] = 0  # zero coefficient
    cases["zero coefficient"] = m
    for what, m in cases.items():
        assert refused(pkg, m), what
    assert not refused(pkg, good)


def test_single_key_encoding_size(pkg, single_key):
    """the real single-key shape is accepted; its encoding holds an 8-byte entry per non-zero plus row pointers and the coefficient table"""
    nnz = sum(single_key[k][1].shape[0] for k in "ABC")
    b = pkg.r1cs_device_bytes(single_key)
    assert b >= 8 * nnz + 3 * 8 * (single_key["n_constraints"] + 1)
    m = copy(single_key)
    m["B"][1][m["B"][0][1000]] = single_key["n_instance_vars"] + single_key["n_witness"]  # one column out of range
    assert refused(pkg, m)


def test_io_argument_rules_need_a_handle(pkg):
    """check / evaluate refuse a missing handle and the other argument errors with BLSW_ERR_ARG before any HIP call"""
    L = pkg.lib()
    fake = ctypes.c_void_p(0x100000)
    assert L.blsw_r1cs_check(None, None, 0, fake, 10, 4, 0, fake, None, None) == BLSW_ERR_ARG
    assert L.blsw_r1cs_evaluate(None, None, 0, fake, 10, 4, 0, 0, 1, fake, fake, fake, None) == BLSW_ERR_ARG
    assert L.blsw_r1cs_destroy(None) == 0
