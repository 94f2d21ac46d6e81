"""The field and tower operation table (tests/devfield/ops.hpp: csrc/fp.hpp, gadgets.hpp, tower.hpp) on the device, in the three compilations
the library gives its chain units (programs out of line, inlined, inlined on quads: tests/devfield/devfield.hip), against the big-integer
reference tests/field_ref.py on the launches test_field_ref.py validates on the host: every edge operand, the inversion-bearing operations also
with each operand filling its waves alone (fp_inv's wave-wide exit taken by all lanes at once) and with 0, 1, p - 1, the slowest and fastest
inversions found and random values side by side in every wave (lanes idling past their convergence), and item counts that leave a partial last
wave and a wave with one item. Bit for bit, nothing sampled: results on every lane (the four lanes of a quad agree), witness streams, cursors,
and the sentinel in every slot an operation does not own."""
import pytest

from tests import devfield_lib as D
from tests import field_ref as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", F.OP_NAMES)
@pytest.mark.parametrize("build", list(D.BUILDS))
def test_device_compilation_equals_reference(build, op):
    lpi = D.lanes_per_item(build)
    assert lpi == (4 if build == "quad" else 1)
    runner = D.device_runner(build)
    bad, items = [], 0
    for name, launch in F.all_launches(op):
        bad += [(name,) + b for b in D.run_launch(build, op, launch, runner, lpi)]
        items += len(launch)
    print("%s %s: %d launches, %d items, %d mismatches" % (build, op, len(F.all_launches(op)), items, len(bad)))
    assert not bad, bad[:10]
