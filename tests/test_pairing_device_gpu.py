"""The table of pairing programs (tests/devpair/ops.hpp) on the device: every entry in every form the device has, on the library's own device teams
and lane shapes (tests/devpair/devpair.hip), bit for bit against the host forms: values, witness streams, cursors, and the sentinel in every
slot nothing may write (behind a stream, the result and cursor slots of lanes 60..63 and of the idle teams of a ragged last wave). The host
forms' MEANING is held to the independent pairing of tests/pairing_ref.py by test_pairing_ref.py; here one value per program goes through the
reference's gt as well, taken from the device's own output. Item counts are team_ref.LONG_ITEM_COUNTS: a one-team wave, full waves, one team
spilling into a new wave; the operands rotate, so the teams of one wave hold different cases."""
import time

import pytest

from tests import devpair_lib as D
from tests import field_ref as F
from tests import pairing_edges as E
from tests import pairing_ref as R
from tests import team_ref as T

pytestmark = pytest.mark.gpu


def _launches(form, op, items, K=1):
    bad, t0 = [], time.time()
    for n in T.LONG_ITEM_COUNTS:
        bad += [("n=%d" % n,) + b for b in D.check_device(form, op, D.launch(items, n), K)]
    print("%s %s K=%d: %d launches, %d mismatches, %.2f s" % (form, op, K, len(T.LONG_ITEM_COUNTS), len(bad), time.time() - t0))
    return bad


@pytest.mark.parametrize("form,op", [("single", "miller"), ("team", "miller"), ("team", "miller_pv")])
def test_witness_programs_on_the_device(form, op):
    items = [it for _, it in D.case_items(op)]
    bad = _launches(form, op, items)
    assert not bad, bad[:10]


@pytest.mark.parametrize("K", E.MULTI_K)
def test_miller_multi_on_the_device(K):
    items = [D.multi_item(K)] + [D.witness_item(c[2], [(c[1], c[3])] * K) for c in E.cases()[:2]]
    bad = _launches("team", "miller_multi", items, K)
    assert not bad, bad[:10]


@pytest.mark.parametrize("op", ["vlines2", "vlines3"])
def test_vlines_on_the_device(op):
    """device == host, 408 rows; 64 items per wave here, so the counts also include a second wave"""
    items = [it for _, it in D.case_items(op)]
    bad = _launches("single", op, items)
    bad += [("n=65",) + b for b in D.check_device("single", op, D.launch(items, 65))]
    assert not bad, bad[:10]


def test_miller_values_on_the_device():
    items = [it for _, it in D.case_items("miller_values")]
    bad = _launches("team", "miller_values", items)
    assert not bad, bad[:10]


def test_device_values_mean_the_pairing():
    """the device's own Miller values through the reference's gt: team_miller on a relation (1) and team_miller_values on a generic product"""
    t0 = time.time()
    c = E.cases()[E.WITNESS_MEANING[0]]
    out, _, _ = D.run_device("team", "miller", [D.witness_item(c[2], [(c[1], c[3])])])
    assert R.gt_of_block(D.ints(out[:6].reshape(12, 6))) == E.expected_gt(c[1], c[2], c[3]) == F.F12_ONE
    c = E.cases()[E.JACOBIAN_MEANING_CASE]
    out, _, _ = D.run_device("team", "miller_values", [D.values_item(c[2], c[1], c[3])])
    want = E.expected_gt(c[1], c[2], c[3])
    assert want != F.F12_ONE and R.gt_of_block(D.ints(out[:6].reshape(12, 6))) == want
    print("reference part: %.1f s" % (time.time() - t0))


@pytest.mark.parametrize("K,B", D.PAR_SHAPES)
def test_miller_par_on_the_device(K, B):
    """launch_miller_par unchanged (csrc/k_miller_par.hip compiled into the harness), B a runtime value, three or four instances so that the task
    counts n 68 C and n 68 end in ragged waves, with the team spine and with the single-lane spine: the Miller segment, f1, T, Q (Q[k][0] keeps
    its sentinel), the final value, the final exponentiation behind the segment and the verdict equal the host's bit for bit"""
    t0 = time.time()
    bad, host = D.check_par_host(K, B)
    assert not bad, bad
    for spine_lane in (0, 1):
        bad = D.check_par_device(K, B, spine_lane, host)
        assert not bad, ("spine_lane=%d" % spine_lane, bad)
    print("miller_par K=%d B=%d: %.2f s" % (K, B, time.time() - t0))


# ---------------------------------------------------------------- the shipped value kernels on chosen points
from tests import vstages_lib as V  # noqa: E402


@pytest.mark.parametrize("n,group,chunk", V.SHAPES)
def test_launch_verify_groups_equals_the_host_stages(n, group, chunk):
    """launch_verify_groups unchanged, chunk a runtime argument: p_scaled, s_scaled, sum_xy, gflag, lines_h, lines_g, partials and result equal the
    host stages bit for bit, sentinels included (a skipped pair writes nothing); the device's own arrays are what the group law says (the partial
    of a chunk that folds nothing is exactly one), and the verdicts are the ones bilinearity gives"""
    t0 = time.time()
    b = V.groups_batch(n, group, chunk)
    host, dev = V.groups_host(b), V.groups_device(b)
    diff = [k for k in V.ARRAYS if (host[k] != dev[k]).any()]
    assert not diff, diff
    bad = V.check_group_arrays(b, dev)
    assert not bad, bad[:10]
    assert dev["result"].tolist() == V.want_results(b)
    print("verify_groups n=%d group=%d chunk=%d: %d groups, %d teams, %.2f s" % (n, group, chunk, b.G, b.G * b.cpg, time.time() - t0))


def test_launch_verify_groups_on_the_meaning_batch():
    """the batch whose partials test_pairing_ref.py holds to the reference pairing: the device's arrays are the host's"""
    b = V.meaning_batch()
    host, dev = V.groups_host(b), V.groups_device(b)
    assert not [k for k in V.ARRAYS if (host[k] != dev[k]).any()] and dev["result"].tolist() == [1, 0, 0]


@pytest.mark.parametrize("n", V.VALUE_COUNTS)
def test_launch_verify_values(n):
    """launch_verify_values unchanged: lines_sig and lines_h equal the host's bit for bit; result is the reference's verdict (test_pairing_ref.py:
    1 exactly on the relations) ANDed with the statuses, relations and non-relations mixed in one wave"""
    b = V.values_batch(n)
    hs, hh = V.values_host(b)
    ds, dh, res = V.values_device(b)
    assert not (hs != ds).any() and not (hh != dh).any()
    assert res.tolist() == b.want and (n < 8 or (0 in b.want and 1 in b.want))


# ---------------------------------------------------------------- the two group entries on TeamLanesGroups
def test_miller_groups_on_the_device():
    """team_miller_groups on TeamLanesGroups, bound as k_vg_fold binds a chunk (instance sets from lines_h, the own pair from lines_g): up to nine
    line sets, all bits set, one cleared in each position, all cleared, n_pairs = 0; the cases rotate, so the ten teams of a wave hold different
    masks and counts (a barrier inside load_pair that only some teams reach)"""
    items = [D.groups_item(*c) for c in D.groups_cases()]
    bad = _launches("team", "miller_groups", items)
    bad += [("n=26",) + b for b in D.check_device("team", "miller_groups", items)]
    assert not bad, bad[:10]


def test_groups_finish_on_the_device():
    """team_groups_finish on TeamLanesGroups, bound as k_vg_finish binds a group: 1, 2 and 3 partials side by side in one wave, the verdicts
    test_pairing_ref.py holds to gt(conj(product of the partials)) == 1"""
    items = D.finish_items()
    bad = _launches("team", "groups_finish", items)
    assert not bad, bad[:10]
    out, _, _ = D.run_device("team", "groups_finish", items)
    assert [int(out[6 * i, 0, 0]) for i in range(len(items))] == [1, 0, 1, 0, 1, 0, 1, 1]
