"""blsw_combine_points_batch, blsw_lagrange_batch and blsw_recover_points_batch on the MI355X: the vectors of tests/combine_lib.py (the CPU file's)
through combine_points, lagrange_coefficients and recover_points in both groups, compared whole with the host stages and the Python reference.
Shapes: n in {1, 63, 65} — below and just above one wavefront, so a partial wave's inactive lanes are exercised — and k in {1, 2, 3, 9} with ragged
counts; at most 585 terms per call. Then the workspace's extent, a non-default stream, and threshold signing end to end on the device.
No test times anything."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import combine_lib as L

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = 0xA5, 4096
SHAPES = [(n, k) for k in (1, 2, 3, 9) for n in (1, 63, 65)]


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _rows(n, total, k):
    """n row indices cycling through the vectors, starting where this shape's k points so that n = 1 is not always row 0"""
    return [(k + i) % total for i in range(n)]


def _dev(dev, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _counts_t(dev, counts):
    return _dev(dev, np.array(counts, dtype=np.uint32).view(np.int32))


def _direct(pkg, dev, entry, group, points, rows32, counts, shave=0, stream=None):
    """the C entry itself on a workspace of exactly the stated size with guard bytes behind it and sentinel-filled outputs
    -> (rc, out, status, term_status or None, guard intact)"""
    import torch

    n, k = points.shape[:2]
    wb = ctypes.c_uint64(0)
    assert pkg.lib().blsw_combine_points_workspace_bytes(group, n, k, ctypes.byref(wb)) == 0
    ws = torch.full((wb.value + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((n, L.WIDTH[group]), SENTINEL, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    tst = torch.full((n, k, 2), -1, dtype=torch.int32, device=dev)
    s = (stream or torch.cuda.current_stream(dev)).cuda_stream
    cp = counts.data_ptr() if counts is not None else None
    if entry == "combine":
        rc = pkg.lib().blsw_combine_points_batch(group, points.data_ptr(), rows32.data_ptr(), cp, k, n, out.data_ptr(), st.data_ptr(), tst.data_ptr(), ws.data_ptr(), wb.value - shave, s)
    else:
        rc = pkg.lib().blsw_recover_points_batch(group, points.data_ptr(), rows32.data_ptr(), cp, k, n, out.data_ptr(), st.data_ptr(), ws.data_ptr(), wb.value - shave, s)
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy(), st.cpu().numpy(), tst.cpu().numpy() if entry == "combine" else None, bool((ws[wb.value:] == SENTINEL).all().item())


@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("group", [1, 2])
def test_combine_points(pkg, dev, group, n, k):
    names, points, scalars, counts, want_out, want_st = L.combine_vectors(group, k)
    idx = _rows(n, len(names), k)
    p, s, c = points[idx], scalars[idx], [counts[i] for i in idx]
    out, st, tst = pkg.combine_points(group, _dev(dev, p), _dev(dev, s), _counts_t(dev, c), want_term_status=True)
    h_out, h_st, h_tst = L.host_combine(group, p, s, c)
    out, st, tst = out.cpu().numpy(), st.cpu().numpy(), tst.cpu().numpy()
    assert st.tolist() == [want_st[i] for i in idx] == h_st.tolist()
    assert np.array_equal(out, want_out[idx]) and np.array_equal(out, h_out) and np.array_equal(tst, h_tst)
    # the entry itself: sentinel-filled outputs (a failing list holds zeros, not the sentinel), guard bytes behind the workspace, one byte less refused
    rc, d_out, d_st, d_tst, intact = _direct(pkg, dev, "combine", group, _dev(dev, p), _dev(dev, s), _counts_t(dev, c))
    assert rc == 0 and intact and np.array_equal(d_out, out) and np.array_equal(d_st, st) and np.array_equal(d_tst, tst)
    assert all(not d_out[i].any() for i in range(n) if st[i] != L.ST_OK)
    rc, d_out, d_st, _, intact = _direct(pkg, dev, "combine", group, _dev(dev, p), _dev(dev, s), _counts_t(dev, c), shave=1)
    assert rc == 2 and intact and (d_out == SENTINEL).all() and (d_st == -1).all()
    # terms beyond a count hold the bytes of an undecodable point and of a scalar >= r: nothing changes
    p2, s2 = p.copy(), s.copy()
    for i, cnt in enumerate(c):
        p2[i, min(cnt, k):] = 0xFF
        s2[i, min(cnt, k):] = 0xFF
    out2, st2 = pkg.combine_points(group, _dev(dev, p2), _dev(dev, s2), _counts_t(dev, c))
    assert np.array_equal(out2.cpu().numpy(), out) and np.array_equal(st2.cpu().numpy(), st)
    if all(cnt == k for cnt in c):  # counts None is every term
        out3, st3 = pkg.combine_points(group, _dev(dev, p), _dev(dev, s))
        assert np.array_equal(out3.cpu().numpy(), out) and np.array_equal(st3.cpu().numpy(), st)


@pytest.mark.parametrize("n,k", SHAPES)
def test_lagrange_coefficients(pkg, dev, n, k):
    import torch

    names, ids, counts, want_coeff, want_st = L.lagrange_vectors(k)
    idx = _rows(n, len(names), k)
    x, c = ids[idx], [counts[i] for i in idx]
    coeff, st = pkg.lagrange_coefficients(_dev(dev, x), _counts_t(dev, c))
    h_coeff, h_st = L.host_lagrange(x, c)
    assert st.cpu().numpy().tolist() == [want_st[i] for i in idx] == h_st.tolist()
    assert np.array_equal(coeff.cpu().numpy(), want_coeff[idx]) and np.array_equal(coeff.cpu().numpy(), h_coeff)
    # the entry on sentinel-filled outputs: zeros in every row of a failing list and beyond a count
    out = torch.full((n, k, 32), SENTINEL, dtype=torch.uint8, device=dev)
    sts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    assert pkg.lib().blsw_lagrange_batch(_dev(dev, x).data_ptr(), _counts_t(dev, c).data_ptr(), k, n, out.data_ptr(), sts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy(), want_coeff[idx]) and sts.cpu().numpy().tolist() == [want_st[i] for i in idx]
    if all(cnt == k for cnt in c):
        coeff2, st2 = pkg.lagrange_coefficients(_dev(dev, x))
        assert torch.equal(coeff2, coeff) and torch.equal(st2, st)


@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("group", [1, 2])
def test_recover_points(pkg, dev, group, n, k):
    names, points, ids, counts, want_out, want_st = L.recover_vectors(group, k)
    idx = _rows(n, len(names), k)
    p, x, c = points[idx], ids[idx], [counts[i] for i in idx]
    out, st = pkg.recover_points(group, _dev(dev, x), _dev(dev, p), _counts_t(dev, c))
    h_out, h_st = L.host_recover(group, p, x, c)
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [want_st[i] for i in idx] == h_st.tolist()
    assert np.array_equal(out, want_out[idx]) and np.array_equal(out, h_out)
    rc, d_out, d_st, _, intact = _direct(pkg, dev, "recover", group, _dev(dev, p), _dev(dev, x), _counts_t(dev, c))
    assert rc == 0 and intact and np.array_equal(d_out, out) and np.array_equal(d_st, st)
    rc, d_out, d_st, _, intact = _direct(pkg, dev, "recover", group, _dev(dev, p), _dev(dev, x), _counts_t(dev, c), shave=1)
    assert rc == 2 and intact and (d_out == SENTINEL).all() and (d_st == -1).all()
    p2, x2 = p.copy(), x.copy()
    for i, cnt in enumerate(c):
        p2[i, min(cnt, k):] = 0xFF
        x2[i, min(cnt, k):] = 0xFF
    out2, st2 = pkg.recover_points(group, _dev(dev, x2), _dev(dev, p2), _counts_t(dev, c))
    assert np.array_equal(out2.cpu().numpy(), out) and np.array_equal(st2.cpu().numpy(), st)


def test_two_calls_queued_on_a_side_stream(pkg, dev):
    """lagrange, then combine on the coefficients it is still writing, on one non-default stream with no host synchronisation between the two calls:
    both results are right, and the second is what recover_points gives"""
    import torch

    group, k, n = 2, 3, 65
    names, points, ids, counts, want_out, want_st = L.recover_vectors(group, k)
    idx = _rows(n, len(names), k)
    p, x, c = _dev(dev, points[idx]), _dev(dev, ids[idx]), _counts_t(dev, [counts[i] for i in idx])
    _, _, _, want_coeff, want_lst = L.lagrange_vectors(k)
    wb = ctypes.c_uint64(0)
    assert pkg.lib().blsw_combine_points_workspace_bytes(group, n, k, ctypes.byref(wb)) == 0
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    coeff = torch.full((n, k, 32), SENTINEL, dtype=torch.uint8, device=dev)
    lst = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out = torch.full((n, 96), SENTINEL, dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    rc1 = pkg.lib().blsw_lagrange_batch(x.data_ptr(), c.data_ptr(), k, n, coeff.data_ptr(), lst.data_ptr(), side.cuda_stream)
    rc2 = pkg.lib().blsw_combine_points_batch(group, p.data_ptr(), coeff.data_ptr(), c.data_ptr(), k, n, out.data_ptr(), st.data_ptr(), None, ws.data_ptr(), wb.value, side.cuda_stream)
    side.synchronize()
    assert rc1 == 0 and rc2 == 0
    n_lag = len(L.lagrange_vectors(k)[0])
    lag_rows = [i for i in range(n) if idx[i] < n_lag]  # the rows of recover_vectors that are the Lagrange rows
    assert np.array_equal(coeff.cpu().numpy()[lag_rows], want_coeff[[idx[i] for i in lag_rows]]) and [lst.cpu().numpy()[i] for i in lag_rows] == [want_lst[idx[i]] for i in lag_rows]
    # combine over the coefficients is recover wherever the ids are good; a failing id list leaves zero coefficients, which combine sums to the identity
    good = [i for i in range(n) if lst[i].item() == L.ST_OK]
    assert len(good) > n // 4
    assert np.array_equal(out.cpu().numpy()[good], want_out[[idx[i] for i in good]]) and [st.cpu().numpy()[i] for i in good] == [want_st[idx[i]] for i in good]


def test_cpp_host_mirror(pkg, dev, tmp_path):
    """BLS::recover_signature / recover_public_key / lagrange_coefficients / combine (include/blsw.hpp) from a C++ host on ragged lists equal the
    Python calls; the C++ side pads with zero bytes behind a list's length"""
    import os
    import subprocess

    subprocess.check_call(["make", "-s", "-C", os.path.join(L.HERE, "combine"), "cpp_caller"])
    lines, want = [], []
    for group in (1, 2):
        names, points, ids, counts, want_out, want_st = L.recover_vectors(group, 3)
        for i, cnt in enumerate(counts):
            if 1 <= cnt <= 3:
                lines.append("g%d %s %s" % (group, ",".join(bytes(p).hex() for p in points[i, :cnt]), ",".join(bytes(x).hex() for x in ids[i, :cnt])))
                want.append((want_st[i], bytes(want_out[i]).hex(), L.ref_lagrange([int.from_bytes(bytes(x), "little") for x in ids[i, :cnt]])[0]))
    f = tmp_path / "lists.txt"
    f.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([os.path.join(L.HERE, "combine", "cpp_caller"), str(f)], text=True, timeout=120).strip().split("\n")
    assert len(out) == len(want) > 20
    for ln, (st, hx, lst) in zip(out, want):
        st_r, rec, st_l, st_c, com = ln.split()
        assert (int(st_r), rec, int(st_l)) == (st, hx, lst), ln
        if lst == L.ST_OK:
            assert (int(st_c), com) == (st, hx), ln


def test_threshold_signing_end_to_end_on_the_device(pkg, dev):
    """sign_batch on share secrets -> recover_signature; recover_public_key on the share keys -> the group key; verify_batch accepts the pair, and
    refuses it when one share's id is swapped for another's"""
    import torch

    t, m, n = 3, 5, 4
    msg = np.frombuffer(b"threshold on the device, 32 b. .", np.uint8).copy()
    assert msg.size == 32
    sets = [L.shares(t, m, 0xD0E + i) for i in range(n)]
    pick = [[0, 1, 2], [4, 2, 0], [1, 3, 4], [0, 1, 2, 3, 4]]  # three t-subsets and a whole set, padded to m with counts
    counts = [len(q) for q in pick]
    sk = np.zeros((n, m, 32), np.uint8)
    ids = np.zeros((n, m, 32), np.uint8)
    for i, (secret, xs, sks) in enumerate(sets):
        for j, q in enumerate(pick[i]):
            sk[i, j] = np.frombuffer(L.le32(sks[q]), np.uint8)
            ids[i, j] = np.frombuffer(L.le32(xs[q]), np.uint8)
        sk[i, counts[i]:] = np.frombuffer(L.le32(1), np.uint8)  # unused lanes still need a valid key for sign_batch
    msgs = torch.from_numpy(np.tile(msg, (n * m, 1))).to(dev)
    signed = pkg.sign_batch(_dev(dev, sk.reshape(n * m, 32)), msgs)
    assert int(signed["status"].abs().sum().item()) == 0
    ids_t, cnt = _dev(dev, ids), _counts_t(dev, counts)
    sig, st_s = pkg.recover_signature(ids_t, signed["sig96"].reshape(n, m, 96).contiguous(), cnt)
    pk, st_p = pkg.recover_public_key(ids_t, signed["pk48"].reshape(n, m, 48).contiguous(), cnt)
    assert not st_s.any().item() and not st_p.any().item()
    whole = pkg.sign_batch(_dev(dev, np.stack([np.frombuffer(L.le32(s[0]), np.uint8) for s in sets])), msgs[:n].contiguous())
    assert torch.equal(sig, whole["sig96"]) and torch.equal(pk, whole["pk48"])
    assert pkg.verify_batch(pk, msgs[:n].contiguous(), sig).cpu().tolist() == [1] * n
    swapped = ids.copy()
    swapped[:, [0, 1]] = swapped[:, [1, 0]]  # the first two shares trade ids
    sig_bad, st_b = pkg.recover_signature(_dev(dev, swapped), signed["sig96"].reshape(n, m, 96).contiguous(), cnt)
    assert not st_b.any().item()
    assert pkg.verify_batch(pk, msgs[:n].contiguous(), sig_bad).cpu().tolist() == [0] * n
