"""The team operation table (tests/devteam/ops.hpp) on the device: the six-lane executor of csrc/team.hpp as the library's team kernels run it
(tests/devteam/devteam.hip: ten teams per wave with lanes 60..63 idle, slot files in LDS, a ragged last wave whose idle teams sit on slot file 0
with a null cursor, descriptors prefetched from constant memory, exec out of line against exec_hot inlined, exp_by_x as an out-of-line member),
against the expected values test_team_ref.py validates on the host, on the same launches: all edge items; the same behind 3 and 9 filler items;
every edge item at team 0, at an inner team and at team 9 of a wave; item counts around the wave size; for seq and exp_by_x a wave of ten
different operand kinds. Bit for bit, nothing sampled: every lane's coefficient of the result (a verdict on all six lanes of its team), every
lane's cursor, the witness stream, the sentinel behind it, and the sentinel in the result and cursor slots of every idle lane of the grid."""
import pytest

from tests import devteam_lib as D
from tests import team_ref as T

pytestmark = pytest.mark.gpu

FORMS = [(op, form) for op in T.OP_NAMES for form in (("exec", "exec_hot") if T.OPS[op][0] else ("exec",))]


@pytest.mark.parametrize("op,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_device_team_equals_expected(op, form):
    bad, items = [], 0
    for name, launch in T.launches(op):
        bad += [(name,) + b for b in D.check_device(form, op, launch)]
        items += len(launch)
    print("%s %s: %d launches, %d items, %d mismatches" % (op, form, len(T.launches(op)), items, len(bad)))
    assert not bad, bad[:10]
