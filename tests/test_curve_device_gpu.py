"""The curve operation table (tests/devcurve/ops.hpp: csrc/decode.hpp, vcurve.hpp, curve.hpp, vsign.hpp, vgroups.hpp) on the device, in the three
compilations the library gives its chain units (programs out of line, inlined, inlined on quads: tests/devcurve/devcurve.hip), against the
big-integer reference tests/curve_ref.py on the launches test_curve_ref.py validates on the host: every case in order, the same shuffled so
that every wave mixes branches, statuses and exits (lanes that left a decode at the flags beside lanes inside the second ladder's fp_inv), each
branch the reference names filling whole waves alone, and item counts 1, 63, 64, 65, 100 (a partial last wave, a wave with one item, odd row
strides for the PARK). Bit for bit, nothing sampled: results on every lane (the four lanes of a quad agree), witness streams, cursors, and the
sentinel in every slot an operation does not own. The quad build carries the entries the table marks for it."""
import pytest

from tests import curve_edges as X
from tests import curve_ref as C
from tests import devcurve_lib as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", C.OP_NAMES)
@pytest.mark.parametrize("build", list(D.BUILDS))
def test_device_compilation_equals_reference(build, op):
    lpi = D.lanes_per_item(build)
    assert lpi == (4 if build == "quad" else 1)
    runner = D.device_runner(build)
    if not D.in_build(build, op):  # the library compiles this code only without quads: the build says so itself
        import ctypes
        assert runner(C.OP_NAMES.index(op), ctypes.c_uint64(1), None, None, None, None, ctypes.c_uint32(C.OPS[op][1] + 1), None) == -3
        return
    bad, items = [], 0
    for name, launch in X.launches(op):
        bad += [(name,) + b for b in D.run_launch(build, op, launch, runner, lpi)]
        items += len(launch)
    print("%s %s: %d launches, %d items, %d mismatches" % (build, op, len(X.launches(op)), items, len(bad)))
    assert not bad, bad[:10]
