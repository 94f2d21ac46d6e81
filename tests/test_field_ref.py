"""The field and tower operation table (tests/devfield/ops.hpp: csrc/fp.hpp, gadgets.hpp, tower.hpp) through the host compilation
(hostsim_field_op) against the big-integer reference tests/field_ref.py, bit for bit, on every launch the device test
(test_field_device_gpu.py) makes: results, witness streams, cursors, untouched slots. Without a GPU this validates the reference, the inputs and
the host compilation; the device test then holds the three device compilations to the same expected values."""
import random

import pytest

from tests import devfield_lib as D
from tests import field_edges as E
from tests import field_ref as F
from tests.field_edges import P


def test_table_is_the_compiled_table():
    """the reference's table names the operations of the compiled table, in its order, with its result and witness counts"""
    assert D.host_table() == [(n,) + F.OPS[n] for n in F.OP_NAMES]


def test_inversion_model_reproduces_the_frozen_counts():
    """the divstep model gives the batch counts recorded beside the frozen stress values, 0 for the value 0, and stays within fp_inv's 37 batches on
    every edge value; the frozen values are the largest and the smallest count among them"""
    for v, n in E.INV_STRESS:
        assert E.inv_batches(v) == n, hex(v)
    assert E.inv_batches(0) == 0
    counts = {E.inv_batches(v) for v in E.field_edge_values() if v}
    assert counts == {26, 27}, counts
    assert E.inv_batches(E.INV_SLOW) == max(counts) and E.inv_batches(E.INV_FAST) < min(counts)


def test_reference_is_consistent():
    """the reference against itself where it can be: Frobenius = the p-th power (one full power, then composition), x x^-1 = 1 in Fp6 and Fp12,
    the cyclotomic elements have x conj(x) = 1 and are no trivial ones, Montgomery encode / decode are inverse"""
    rng = random.Random(0x5E1F)
    x = F.d12([rng.randrange(P) for _ in range(12)])
    f1 = F.f12_frobenius(x, 1)
    assert f1 == F.f12_pow(x, P)
    assert F.f12_frobenius(f1, 1) == F.f12_frobenius(x, 2) and F.f12_frobenius(F.f12_frobenius(x, 2), 1) == F.f12_frobenius(x, 3)
    assert F.f12_mul(x, F.f12_inv(x)) == F.F12_ONE and F.f6_mul(x[0], F.f6_inv(x[0])) == F.F6_ONE
    assert F.f12_inv((F.F6_ZERO, F.F6_ZERO)) == (F.F6_ZERO, F.F6_ZERO) and F.f2_inv((0, 0)) == (0, 0)
    assert len(F.cyclotomic_elements()) == 6
    for v in (0, 1, P - 1, rng.randrange(P)):
        assert F.dec(F.enc(v)) == v


def test_to_bits_witness_count_is_constant():
    """fp_to_bits_le_w's stream has 761 witnesses whatever the value: 381 bits, then enforce_in_field_le's ANDs against p - 1"""
    vals = E.to_bits_canonical_values()
    runs = E.runs_of_ones(P - 1)
    assert all(0 <= v < P for v in vals) and {0, 1, P - 1, P - 2, (P - 1) // 2, 1 << 380} <= set(vals)
    assert all((P - 1) ^ (1 << b) in vals for hi, lo in runs for b in (hi, lo)) and runs[0][0] == 380 and runs[-1][1] == 1
    for v in vals:
        assert len(F.w_to_bits_le(v)) == F.TO_BITS_WITNESSES == 761, hex(v)
    # p - 1 itself passes every run: all of its ANDs inside runs are true, every nand's AND is false
    w = F.w_to_bits_le(P - 1)[381:]
    assert w.count(F.ONE) == sum(hi - lo for hi, lo in runs) + len(runs) - 1  # a run of L ones: L - 1 ANDs, one more with last_run (a constant for the first run)


def test_inputs_cover_what_they_claim():
    """the Fp2 operand set has the four shapes of every reduced edge value; the arrangements of an inversion-bearing operation hold a zero next to
    the stress values in one wave; the item counts leave a partial last wave in both lane layouts"""
    s = set(E.fp2_operand_set())
    for x in E.fp_reduced_edges():
        assert {(x, 0), (0, x), (x, x), (x, (P - x) % P)} <= s
    assert {(0, 0), (1, 0), (0, 1), (P - 1, P - 1)} <= s
    for op in F.INVERSION_OPS:
        c = F.cases(op)
        assert len(c["uniform"]) % E.WAVE == 0 and all(len(set(c["uniform"][i:i + E.WAVE])) == 1 for i in range(0, len(c["uniform"]), E.WAVE)), op
        assert len(c["interleaved"]) >= 2 * E.WAVE and len(set(c["interleaved"][:16])) >= 8, op
    first_wave = [a[0] for a, _ in F.cases("fp_inv")["interleaved"][:16]]
    assert {0, 1, P - 1, E.INV_SLOW, E.INV_FAST} <= set(first_wave)
    eq = F.cases("fp2_is_eq_w")["edges"]
    kinds = {(a[0] == b[0], a[1] == b[1]) for a, b in eq}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    inv2 = F.cases("fp2_inv2")["edges"]
    assert {(a[:2] == (0, 0), b[:2] == (0, 0)) for a, b in inv2} == {(True, True), (True, False), (False, True), (False, False)} and any(a == b != F.ZERO_BLK for a, b in inv2)
    assert any(n % 64 and n > 64 for n in E.ITEM_COUNTS) and any(4 * n % 64 and 4 * n > 64 for n in E.ITEM_COUNTS) and 1 in E.ITEM_COUNTS


@pytest.mark.parametrize("op", F.OP_NAMES)
def test_host_compilation_equals_reference(op):
    """every launch of the operation (all edge operands; for the inversion-bearing ones the uniform and the interleaved arrangement; the item counts)
    through hostsim_field_op_batch: results, witness streams and cursors equal the reference, unowned slots keep the sentinel"""
    bad, items = [], 0
    for name, launch in F.all_launches(op):
        bad += [(name,) + b for b in D.run_launch("host", op, launch, D.host_runner(), 1)]
        items += len(launch)
    print("%s: %d launches, %d items, %d mismatches" % (op, len(F.all_launches(op)), items, len(bad)))
    assert not bad, bad[:10]
