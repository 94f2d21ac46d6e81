"""Device R1CS evaluator (blsw_r1cs_*, ConstraintChecker) on the MI355X: witness vectors written by the engine are checked against the
matrices the library emits, on every constraint, for every circuit shape; corrupted elements are found at the row the host check finds;
A z, B z, C z equal a big-integer evaluation of the CSR. Host matrix synthesis takes seconds per shape: cached per module."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import hostsim_lib, synth
from tests.oracle_lib import P_MOD

pytestmark = pytest.mark.gpu
R = 1 << 384
R_INV = pow(R, -1, P_MOD)
_MATS = {}


@pytest.fixture(scope="module")
def pkg():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return importlib.import_module("bls-verify-gadget_amd")


def mats(pkg, **shape):
    key = tuple(sorted(shape.items()))
    if key not in _MATS:
        P = pkg.matrices(32, **shape)
        _MATS[key] = (P, pkg.ConstraintChecker.from_matrices(P, "cuda:0"))
    return _MATS[key]


def to_int(limbs):
    return sum(int(x) << (64 * k) for k, x in enumerate(np.asarray(limbs, dtype=np.uint64)))


def to_limbs(v):
    return np.array([(v >> (64 * k)) & ((1 << 64) - 1) for k in range(6)], dtype=np.uint64)


def set_elem(t, i, k, v):
    """t[i, k] = the integer v (six u64 limbs) in a [n, stride, 6] int64 cuda tensor"""
    import torch

    t[i, k] = torch.from_numpy(to_limbs(v).view(np.int64)).to(t.device)


def single_key(pkg, n, pad=0, **options):
    """n single-key instances through a direct-mode engine (every 16th tampered: a valid assignment whose Boolean is false), written into a
    witness tensor whose rows are padded by `pad` elements of junk -> (engine, witness [n, n_witness + pad, 6], instance or None)"""
    import torch

    from importlib import import_module

    workload = import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    pk, msg, sig, _ = workload.make_batch(pkg, n, device=dev)
    eng = pkg.WitnessEngine(n, 32, max_steps=1, device=dev, n_buffers=1, **options)
    w = torch.randint(-(1 << 62), 1 << 62, (n, eng.n_witness + pad, 6), dtype=torch.int64, device=dev)
    inst = eng.new_instance_tensor() if eng.n_instance_vars > 1 else None
    eng.submit(pk, sig, msg, witness=w, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    return w, inst


def test_single_key_satisfied_and_corrupted(pkg):
    """n = 130 (not a multiple of 64) with a padded stride full of junk: every instance satisfies the system in both element forms. One
    element changed to another reduced element in four instances (an early message bit, a SHA-256 row, a Miller-loop element, the last
    element): the first bad row is the host check's, the other instances stay at -1; an element set to p + 1 is reported as unreduced."""
    import torch

    n = 130
    P, chk = mats(pkg)
    lay = pkg.layout(32)
    nw = P["n_witness"]
    w, _ = single_key(pkg, n, pad=5)
    wc, _ = single_key(pkg, n, pad=3, output_form=1)
    assert chk.n_witness == nw and w.shape[1] == nw + 5
    for t, form in ((w, 0), (wc, 1)):
        assert chk.which_is_unsatisfied(t, form=form).tolist() == [-1] * n
        assert chk.first_unreduced(t, form=form).tolist() == [-1] * n
        assert bool(chk.is_satisfied(t, form=form).all())
    # the non-padded view of the same tensor: the stride comes from the view
    assert chk.which_is_unsatisfied(w[:, :nw]).tolist() == [-1] * n
    # corruption: instance -> witness index
    where = {3: 0, 40: lay["off_expand"] + 1000, 77: lay["off_miller"] + 123, 129: nw - 1}
    expect = {}
    for i, k in where.items():
        h = w[i, :nw].cpu().numpy().view(np.uint64).copy()
        v = (to_int(h[k]) + 1) % P_MOD
        h[k] = to_limbs(v)
        expect[i] = hostsim_lib.r1cs_check(P, h)
        set_elem(w, i, k, v)
        set_elem(wc, i, k, v * R_INV % P_MOD)  # the same field element in canonical form
    assert sum(e >= 0 for e in expect.values()) >= 3, expect
    want = [expect.get(i, -1) for i in range(n)]
    assert chk.which_is_unsatisfied(w).tolist() == want
    assert chk.which_is_unsatisfied(wc, form=1).tolist() == want
    assert chk.is_satisfied(w).tolist() == [x < 0 for x in want]
    set_elem(w, 64, 777, P_MOD + 1)
    set_elem(wc, 65, nw - 2, P_MOD + 1)
    assert chk.first_unreduced(w).tolist() == [1 + 777 if i == 64 else -1 for i in range(n)]
    assert chk.first_unreduced(wc, form=1).tolist() == [1 + nw - 2 if i == 65 else -1 for i in range(n)]
    torch.cuda.synchronize()


def test_argument_rules_before_any_launch(pkg):
    """blsw_r1cs_check / _evaluate refuse form 2, n 0, a stride below n_witness, a missing instance vector where the circuit has public
    inputs and a row range outside the matrix with BLSW_ERR_ARG, and write nothing."""
    import torch

    L = pkg.lib()
    P, chk = mats(pkg)
    Pi, chki = mats(pkg, pk_mode=1, sig_mode=0)
    dev = torch.device("cuda:0")
    w = torch.zeros((2, P["n_witness"], 6), dtype=torch.int64, device=dev)
    out = torch.full((2,), 7, dtype=torch.int64, device=dev)
    az = torch.full((2, 4, 6), 7, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    nw, nc = P["n_witness"], P["n_constraints"]

    def check(r, inst, ist, ws, n, form):
        return L.blsw_r1cs_check(r._r, inst, ist, w.data_ptr(), ws, n, form, out.data_ptr(), None, s)

    def evaluate(r, begin, count, form=0, ws=nw):
        return L.blsw_r1cs_evaluate(r._r, None, 0, w.data_ptr(), ws, 2, form, begin, count, az.data_ptr(), az.data_ptr(), az.data_ptr(), s)

    assert check(chk, None, 0, nw, 2, 2) == 1 and check(chk, None, 0, nw, 0, 0) == 1 and check(chk, None, 0, nw - 1, 2, 0) == 1
    assert check(chki, None, 0, Pi["n_witness"], 2, 0) == 1  # n_instance_vars = 4: instance required
    assert check(chki, w.data_ptr(), 3, Pi["n_witness"], 2, 0) == 1  # instance stride below n_instance_vars
    assert evaluate(chk, nc, 1) == 1 and evaluate(chk, nc - 2, 4) == 1 and evaluate(chk, 0, 0) == 1 and evaluate(chk, 0, 4, form=2) == 1
    assert evaluate(chk, 0, 4, ws=nw - 1) == 1
    torch.cuda.synchronize()
    assert out.tolist() == [7, 7] and bool((az == 7).all())
    with pytest.raises(pkg.BlswError):
        chki.which_is_unsatisfied(w[:, :Pi["n_witness"]])


def _engine_run(pkg, n, **options):
    """one batch through a staged engine (the shapes that need one) -> (witness, instance)"""
    import torch

    from importlib import import_module

    workload = import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    pk, msg, sig, _ = workload.make_batch(pkg, n, device=dev)
    eng = pkg.WitnessEngine(n, 32, max_steps=2, device=dev, n_buffers=2, **options)
    w = eng.new_witness_tensor()
    inst = eng.new_instance_tensor() if eng.n_instance_vars > 1 else None
    eng.submit(pk, sig, msg, witness=w, instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    return w, inst


def _corrupt_and_compare(pkg, P, chk, w, inst, i, k, in_instance=False):
    """instance i, element k of the witness (or of the instance vector) + 1: the GPU's first bad row == the host check's"""
    t = inst if in_instance else w
    h = t[i].cpu().numpy().view(np.uint64).copy()
    v = (to_int(h[k]) + 1) % P_MOD
    set_elem(t, i, k, v)
    hw = w[i].cpu().numpy().view(np.uint64)
    hi = inst[i].cpu().numpy().view(np.uint64) if inst is not None else None
    expect = hostsim_lib.r1cs_check(P, hw, hi) if hi is not None else hostsim_lib.r1cs_check(P, hw)
    got = chk.which_is_unsatisfied(w, inst).tolist()
    assert got == [expect if j == i else -1 for j in range(w.shape[0])], (k, in_instance)


def test_every_shape(pkg, oracle):
    """aggregate_verify with 2 keys, the N+1-pair product with 2 pairs, Witness parameters, and Input pk / sig with the engine's instance
    tensor: all satisfied; a corrupted witness element, and a corrupted public input, are found at the host check's row."""
    import torch

    dev = torch.device("cuda:0")
    # aggregate_verify, K = 2: bitmap (1, 0) verifies, the tampered case does not; both are satisfied assignments
    cases = [synth.make_aggregate(oracle, 2, [1, 0], start=10), synth.make_aggregate(oracle, 2, [1, 1], start=20, tamper=True)]
    eng = pkg.WitnessEngine(2, 32, max_steps=2, device=dev, n_buffers=2, n_keys=2)
    w = eng.new_witness_tensor()
    pks, bm, msg, sig = (np.stack([c[j] for c in cases]) for j in range(4))
    eng.submit_aggregate(torch.from_numpy(pks.view(np.int64)).to(dev), torch.from_numpy(bm).to(dev), torch.from_numpy(sig.view(np.int64)).to(dev),
                         torch.from_numpy(msg).to(dev), witness=w)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    P, chk = mats(pkg, n_keys=2)
    assert chk.which_is_unsatisfied(w).tolist() == [-1, -1]
    _corrupt_and_compare(pkg, P, chk, w, None, 1, pkg.layout_aggregate(32, 2)["off_agg"] + 5)
    # N+1-pair product, K = 2
    pks, msgs, sg = [], [], []
    for j, t in enumerate((None, 1)):
        a, b, c, _ = synth.make_multi(oracle, 2, tamper=t, start=4 * j)
        pks.append(a), msgs.append(b), sg.append(c)
    res, wm = pkg.verify_multi(pkg.ParametersVar(), pkg.PublicKeyVar.new_witness(torch.from_numpy(np.stack(pks).view(np.int64)).to(dev)),
                               torch.from_numpy(np.stack(msgs)).to(dev), pkg.SignatureVar.new_witness(torch.from_numpy(np.stack(sg).view(np.int64)).to(dev)))
    assert res.tolist() == [1, 0]
    P, chk = mats(pkg, n_pairs=2)
    assert chk.which_is_unsatisfied(wm).tolist() == [-1, -1]
    _corrupt_and_compare(pkg, P, chk, wm, None, 0, pkg.layout_multi(32, 2)["off_miller"] + 77)
    # Witness parameters
    wp, _ = _engine_run(pkg, 3, params_mode=1)
    P, chk = mats(pkg, params_mode=1)
    assert chk.which_is_unsatisfied(wp).tolist() == [-1] * 3
    _corrupt_and_compare(pkg, P, chk, wp, None, 2, pkg.layout(32, params_mode=1)["off_params_alloc"] + 3)
    # Input pk / sig: z = [instance | witness]
    for pk_mode, sig_mode in ((1, 1), (0, 1)):
        wi, inst = _engine_run(pkg, 3, pk_mode=pk_mode, sig_mode=sig_mode)
        P, chk = mats(pkg, pk_mode=pk_mode, sig_mode=sig_mode)
        assert chk.n_instance_vars == 1 + 3 * pk_mode + 6 * sig_mode
        assert chk.which_is_unsatisfied(wi, inst).tolist() == [-1] * 3
        assert chk.first_unreduced(wi, inst).tolist() == [-1] * 3
        _corrupt_and_compare(pkg, P, chk, wi, inst, 1, 1, in_instance=True)
        set_elem(inst, 2, 1, P_MOD + 1)
        assert chk.first_unreduced(wi, inst).tolist() == [-1, -1, 1]


def test_evaluate_matches_big_integer_rows(pkg):
    """A z, B z, C z over a window of 20 000 rows (the pairing tail: general coefficients) for two instances == a Python big-integer
    evaluation of the CSR; A z * B z == C z on every row of it; canonical input gives the same rows in canonical form."""
    P, chk = mats(pkg)
    w, _ = single_key(pkg, 2)
    wc, _ = single_key(pkg, 2, output_form=1)
    nc, count = P["n_constraints"], 20000
    begin = nc - count - 7
    az, bz, cz = (t.cpu().numpy().view(np.uint64) for t in chk.evaluate(w, rows=(begin, count)))
    azc, bzc, czc = (t.cpu().numpy().view(np.uint64) for t in chk.evaluate(wc, form=1, rows=(begin, count)))
    assert az.shape == (2, count, 6)
    for i in range(2):
        h = w[i].cpu().numpy().view(np.uint64)
        zc = {}

        def z(c):
            if c not in zc:
                zc[c] = R % P_MOD if c == 0 else to_int(h[c - 1])
            return zc[c]

        for name, got, gotc in (("A", az, azc), ("B", bz, bzc), ("C", cz, czc)):
            rp, col, val = P[name]
            lo, hi = int(rp[begin]), int(rp[begin + count])
            vals = [to_int(v) for v in val[lo:hi]]
            for j in range(count):
                s = 0
                for k in range(int(rp[begin + j]), int(rp[begin + j + 1])):
                    s += vals[k - lo] * z(int(col[k]))
                mont = s * R_INV % P_MOD  # (c R)(z R) R^-1 summed
                assert to_int(got[i, j]) == mont, (name, i, begin + j)
                assert to_int(gotc[i, j]) == mont * R_INV % P_MOD, (name, i, begin + j)
        for j in range(count):
            assert to_int(az[i, j]) * to_int(bz[i, j]) * R_INV % P_MOD == to_int(cz[i, j])


def test_bench_shape_batch_all_satisfied(pkg):
    """the engine's bench shape (1 024 instances, grouped engine) is all satisfied: the scale the kernel is for"""
    import torch

    from importlib import import_module

    workload = import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    n = 1024
    pk, msg, sig, expect = workload.make_batch(pkg, n, device=dev)
    eng = pkg.WitnessEngine(n, 32, max_steps=16, device=dev, n_buffers=3)
    w = eng.new_witness_tensor()
    r = torch.empty(n, dtype=torch.int32, device=dev)
    eng.submit(pk, sig, msg, witness=w, result=r)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    assert np.array_equal(r.cpu().numpy().astype(bool), expect) and not expect.all()
    _, chk = mats(pkg)
    assert chk.which_is_unsatisfied(w).tolist() == [-1] * n
    assert chk.first_unreduced(w).tolist() == [-1] * n
