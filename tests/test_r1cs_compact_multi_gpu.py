"""A step of the N+1-pair product checked straight from its compact form (blsw_r1cs_check_compact_multi / _evaluate_compact_multi) on the GPU: the
pair families evaluated with one pair per lane, the other rows with one instance per lane. Real matrices on real engine steps, corruptions placed
through the locator and compared with the full-vector check of the step's expansion and with the host's row check, the evaluation bit for bit,
unreduced staged elements, synthetic systems over the borders of every region and run (with and without a family), and the argument rules.
Exact comparisons, no tolerance."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import multi_inputs_lib as M
from tests import r1cs_synth as S
from tests.oracle_lib import P_MOD as P

pytestmark = pytest.mark.gpu
ERR_ARG = 1
# (n, K, mask, msg_len): three pair tiles with instance 21 on lanes 63, 64, 65 and whole instance tiles; one pair tile with half an instance tile and
# every argument a public input
CONFIGS = {"n64_k3": (64, 3, 0, 32), "n32_k2_inputs": (32, 2, 13, 50)}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bls-verify-gadget_amd")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


class Step:
    """one engine step, as its compact form and as plain vectors + instance tensor, the matrices and the checker of its circuit"""


@pytest.fixture(scope="module", params=list(CONFIGS))
def step(request, pkg, torch, oracle):
    from tests.test_multi_inputs_gpu import distinct, stack, tiled

    n, K, mask, msg_len = CONFIGS[request.param]
    s = Step()
    s.n, s.K, s.mask, s.msg_len, s.dev = n, K, mask, msg_len, torch.device("cuda:0")
    s.batch = tiled(distinct(oracle, K, msg_len), n)  # valid, tampered (false, satisfied), key 1 = (0, 0) (pk != 0 fails), valid, ...
    pks, msgs, sig = stack(torch, s.batch, s.dev)
    eng = pkg.WitnessEngine(n, msg_len, max_steps=2, n_buffers=2, device=s.dev, n_pairs=K, multi_inputs=mask)
    s.eng = eng
    s.lay = eng.compact_layout()
    assert isinstance(s.lay, pkg.blsw_compact_layout_multi_t) and s.lay.total == eng.compact_bytes()
    s.comp, s.plain, s.inst = eng.new_compact_buffer(1)[0], eng.new_witness_tensor(), eng.new_instance_tensor()
    r1, r2 = torch.empty(n, dtype=torch.int32, device=s.dev), torch.empty(n, dtype=torch.int32, device=s.dev)
    eng.submit_multi_compact(pks, msgs, sig, s.comp, result=r1)
    eng.submit_multi(pks, msgs, sig, witness=s.plain, result=r2, instance=s.inst)
    eng.flush()
    torch.cuda.synchronize()
    assert torch.equal(r1, r2) and r1.cpu().numpy().astype(bool).tolist() == [c[3] for c in s.batch]
    s.inst_arg = s.inst if mask else None
    s.mats = pkg.matrices(msg_len, n_pairs=K, multi_inputs=mask)
    s.chk = pkg.ConstraintChecker.from_matrices(s.mats, s.dev)
    assert s.chk.n_witness == s.lay.n_witness == s.plain.shape[1]
    s.fam = s.chk.pair_families(s.lay)
    # the expected verdicts: a valid and a tampered instance satisfy the system; the zero key breaks a row, the one the host's check names
    pk0, msg0, sig0, _ = s.batch[2]
    s.zero_row = M.check(pk0, msg0, sig0, mask)
    assert s.zero_row >= 0
    s.base = [s.zero_row if i % 4 == 2 else -1 for i in range(n)]
    yield s
    s.chk.close()
    eng.close()


def expansion(torch, s, comp):
    out = s.eng.new_witness_tensor()
    s.eng.expand_compact(comp, out)
    torch.cuda.synchronize()
    return out


def add_one(pkg, torch, s, comp, k, i):
    """element k of instance i of the buffer += 1 (through the locator) -> its region"""
    region, off, _ = pkg.compact_locate_multi(s.lay, k, i)
    assert region != 0 and off % 8 == 0 and off + 48 <= s.lay.total
    comp.view(torch.int64)[off // 8] += 1
    return region


def flip_bit(pkg, torch, s, comp, k, i):
    region, off, bit = pkg.compact_locate_multi(s.lay, k, i)
    assert region == 0 and bit < 31 and off % 4 == 0
    comp.view(torch.int32)[off // 4] ^= 1 << bit


def test_real_matrices(pkg, torch, step):
    s = step
    assert len(s.fam) >= 2 and sum(R for _, R in s.fam) * s.K > 0.98 * s.chk.n_constraints  # the check below runs the pair-lane kernel on nearly every row
    got = s.chk.which_is_unsatisfied_compact(s.lay, s.comp, s.inst_arg).tolist()
    plain = s.chk.which_is_unsatisfied(s.plain, s.inst_arg).tolist()
    assert got == plain == s.base
    assert s.chk.is_satisfied_compact(s.lay, s.comp, s.inst_arg).tolist() == [r < 0 for r in s.base]
    assert s.chk.first_unreduced_compact(s.lay, s.comp, s.inst_arg).tolist() == [-1] * s.n
    # the general path alone (families off: the measurement route) gives the same rows
    assert s.chk._check_compact(s.lay, s.comp, s.inst_arg, None, False, _use_families=False)[0].tolist() == s.base
    if not s.mask:  # a Witness key: the zero key's row lies in a family, in the block of pair 1 — the pair-lane kernel reported template row + 1 * R
        first, R = [(f, r) for f, r in s.fam if f <= s.zero_row < f + s.K * r][0]
        assert (s.zero_row - first) // R == 1


def test_corruptions_through_the_locator(pkg, torch, step):
    s, c, K = step, step.lay, step.K
    # satisfied instances (i % 4 != 2) in both halves of a tile and in different tiles
    who = dict(bit_first=0, bit_last=60, hash_elem=21, prep_pk=32, prep_sig=44, miller=63, two=12) if s.n == 64 else \
        dict(bit_first=0, bit_last=28, hash_elem=21, prep_pk=16, prep_sig=8, miller=31, two=12)
    assert all(s.base[i] == -1 for i in who.values()) and len(set(who.values())) == len(who)
    comp = s.comp.clone()
    b = 1000
    flip_bit(pkg, torch, s, comp, c.off_expand + b, who["bit_first"])
    flip_bit(pkg, torch, s, comp, c.off_expand + (K - 1) * c.stride_hash + b, who["bit_last"])
    assert add_one(pkg, torch, s, comp, c.pair_run_off[3] + 1 * c.stride_hash + 5000, who["hash_elem"]) == pkg.COMPACT_TILE
    assert add_one(pkg, torch, s, comp, c.pair_run_off[5] + (K - 1) * c.pair_run_stride[5] + 3, who["prep_pk"]) == pkg.COMPACT_TILE
    assert add_one(pkg, torch, s, comp, c.inst_run_off[1] + 700, who["prep_sig"]) == pkg.COMPACT_INST
    assert add_one(pkg, torch, s, comp, c.off_miller + c.pair_rows // 2, who["miller"]) == pkg.COMPACT_PAIR
    # two in one instance: an early element of the LAST pair's hash_to_g2 and a late one of the FIRST pair's — the first pair's matrix row is smaller
    assert add_one(pkg, torch, s, comp, c.pair_run_off[3] + (K - 1) * c.stride_hash + 40, who["two"]) == pkg.COMPACT_TILE
    assert add_one(pkg, torch, s, comp, c.pair_run_off[3] + 20000, who["two"]) == pkg.COMPACT_TILE
    got = s.chk.which_is_unsatisfied_compact(c, comp, s.inst_arg).tolist()
    out = expansion(torch, s, comp)
    want = s.chk.which_is_unsatisfied(out, s.inst_arg).tolist()
    assert got == want
    for i in range(s.n):
        assert (want[i] >= 0 and want[i] != s.base[i]) if i in who.values() else want[i] == s.base[i], i
    # every corruption of a pair-local witness is reported from a family, in the block of its pair
    block = {}
    for name in ("bit_first", "bit_last", "hash_elem", "two"):
        row = want[who[name]]
        first, R = [(f, r) for f, r in s.fam if f <= row < f + K * r][0]
        block[name] = (row - first) // R
    assert block == dict(bit_first=0, bit_last=K - 1, hash_elem=1, two=0)
    # the host's row check of the expanded vector of the doubly corrupted instance names the same row
    i = who["two"]
    pk_i, msg_i, sig_i, _ = s.batch[i]
    host = M.check(pk_i, msg_i, sig_i, s.mask, s.inst[i].cpu().numpy().view(np.uint64) if s.mask else None, out[i].cpu().numpy().view(np.uint64))
    assert host == want[i]
    # the general path alone agrees
    assert s.chk._check_compact(c, comp, s.inst_arg, None, False, _use_families=False)[0].tolist() == want


def test_evaluate_compact_is_evaluate_of_the_plain_vectors(pkg, torch, step):
    s = step
    first, R = max(s.fam, key=lambda f: f[1])  # the hash_to_g2 family
    windows = [(first + R + R // 2, 64), (first + s.K * R - 32, 64), (s.chk.n_constraints - 64, 64)]
    for w in windows:
        a = s.chk.evaluate_compact(s.lay, s.comp, s.inst_arg, rows=w)
        b = s.chk.evaluate(s.plain, s.inst_arg, rows=w)
        for m in range(3):
            assert a[m].shape == (s.n, 64, 6) and torch.equal(a[m], b[m]), (w, m)
        assert bool(a[0].any()) and bool(a[1].any())  # (a C row of the last rows, x * 0 = 0 style, may be all zero)


def test_unreduced_staged_elements(pkg, torch, step):
    s, c = step, step.lay
    comp = s.comp.clone()
    p_limbs = torch.from_numpy(S.limbs([P]).view(np.int64)[0]).to(s.dev)
    k_tile, k_inst = c.pair_run_off[3] + 1 * c.stride_hash + 77, c.inst_run_off[1] + c.inst_run_len[1] - 1
    i_tile, i_inst = s.n - 1, s.n // 2 + 1
    for k, i, want_region in ((k_tile, i_tile, pkg.COMPACT_TILE), (k_inst, i_inst, pkg.COMPACT_INST)):
        region, off, _ = pkg.compact_locate_multi(c, k, i)
        assert region == want_region
        comp.view(torch.int64)[off // 8:off // 8 + 6] = p_limbs
    want = [-1] * s.n
    want[i_tile], want[i_inst] = s.chk.n_instance_vars + k_tile, s.chk.n_instance_vars + k_inst
    assert s.chk.first_unreduced_compact(c, comp, s.inst_arg).tolist() == want
    # an instance-row element, and the smaller index wins within an instance
    k_row = c.off_miller + 9
    region, off, _ = pkg.compact_locate_multi(c, k_row, i_inst)
    assert region == pkg.COMPACT_PAIR
    comp.view(torch.int64)[off // 8:off // 8 + 6] = p_limbs
    assert s.chk.first_unreduced_compact(c, comp, s.inst_arg).tolist() == want
    want[0] = s.chk.n_instance_vars + k_row
    region, off, _ = pkg.compact_locate_multi(c, k_row, 0)
    comp.view(torch.int64)[off // 8:off // 8 + 6] = p_limbs
    assert s.chk.first_unreduced_compact(c, comp, s.inst_arg).tolist() == want


def test_argument_rules(pkg, torch, step):
    s, c, L = step, step.lay, pkg.lib()
    sentinel = 0x5A5A5A5A5A5A5A5A
    bad = torch.full((s.n,), sentinel, dtype=torch.int64, device=s.dev)
    unr = torch.full((s.n,), sentinel, dtype=torch.int64, device=s.dev)
    ev = [torch.full((s.n, 4, 6), sentinel, dtype=torch.int64, device=s.dev) for _ in range(3)]
    ip, ist = s.inst.data_ptr(), s.inst.stride(0) // 6

    def check(layout=c, comp=s.comp.data_ptr(), inst=ip, stride=ist):
        return L.blsw_r1cs_check_compact_multi(s.chk._r, ctypes.byref(layout), comp, inst, stride, bad.data_ptr(), unr.data_ptr(), None)

    def evaluate(layout=c, comp=s.comp.data_ptr(), inst=ip, stride=ist, begin=0, count=4):
        return L.blsw_r1cs_evaluate_compact_multi(s.chk._r, ctypes.byref(layout), comp, inst, stride, begin, count, ev[0].data_ptr(), ev[1].data_ptr(), ev[2].data_ptr(), None)

    other = pkg.compact_layout_multi(s.n, s.msg_len + 1, n_pairs=s.K, multi_inputs=s.mask)  # another circuit: n_witness differs from the handle's
    assert other.n_witness != c.n_witness
    broken = type(c).from_buffer_copy(bytes(c))
    broken.off_inst += 256
    for f in (check, evaluate):
        assert f(layout=other) == ERR_ARG and f(layout=broken) == ERR_ARG
        assert f(comp=s.comp.data_ptr() + 8) == ERR_ARG  # 16-byte alignment
        assert f(comp=None) == ERR_ARG
        assert f(stride=s.chk.n_instance_vars - 1) == ERR_ARG
        if s.mask:  # public inputs: the compact form carries witnesses only
            assert f(inst=None) == ERR_ARG
    assert evaluate(begin=s.chk.n_constraints - 3) == ERR_ARG and evaluate(count=0) == ERR_ARG
    assert L.blsw_r1cs_check_compact_multi(s.chk._r, ctypes.byref(c), s.comp.data_ptr(), ip, ist, None, None, None) == ERR_ARG
    assert L.blsw_r1cs_check_compact_multi_ex(s.chk._r, ctypes.byref(c), s.comp.data_ptr(), ip, ist, 2, bad.data_ptr(), None, None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((bad == sentinel).all()) and bool((unr == sentinel).all()) and all(bool((e == sentinel).all()) for e in ev)
    if s.mask:
        with pytest.raises(pkg.BlswError):
            s.chk.which_is_unsatisfied_compact(c, s.comp)  # no instance tensor
    # the options of the shared-keys form do not apply
    with pytest.raises(pkg.BlswError):
        s.chk.which_is_unsatisfied_compact(c, s.comp, s.inst, skip_head_rows=True)
    with pytest.raises(pkg.BlswError):
        s.chk.evaluate_compact(c, s.comp, s.inst, keyset=object())
    # and the calls work after all of it
    assert evaluate() == 0 and check() == 0
    torch.cuda.synchronize()
    assert bad.tolist() == s.base


# ---- synthetic systems over the borders of every region and run


def synthetic_system(c, break_translation):
    """[general rows | K translated blocks | general rows] over the first and last column of every run and region for pairs 0, 1 and K - 1; one
    slack per row: a pair's hash_to_g2 element in the blocks, an instance row (Miller segment) outside. -> (system, first row of the blocks, R)"""
    K, ni = c.n_pairs, 1
    coeffs = S.coefficients()
    col = lambda k: ni + k
    local = []  # pair 0's columns at the borders: the SHA bits at word and chunk borders, every non-empty run's ends
    for b in (0, 31, 32, 511, 512, c.sha_bits - 1):
        local.append(col(c.off_expand + b))
    strides = {}
    for k in local:
        strides[k] = c.stride_hash
    for r in range(6):
        if c.pair_run_len[r]:
            for k in (c.pair_run_off[r], c.pair_run_off[r] + c.pair_run_len[r] - 1):
                local.append(col(k))
                strides[col(k)] = c.pair_run_stride[r]
    shared = [col(c.inst_run_off[r] + d) for r in range(2) if c.inst_run_len[r] for d in (0, c.inst_run_len[r] - 1)] + [col(c.off_miller), col(c.n_witness - 1)]
    template = []
    for t in range(len(local)):
        a, b2, c2 = local[t], local[(t + 1) % len(local)], local[(t + 5) % len(local)]
        slack = col(c.pair_run_off[3] + 100 + t)
        strides[slack] = c.stride_hash
        template.append(([([(0, coeffs[t])] if t % 2 else []) + [(a, coeffs[t + 1])], [(b2, coeffs[t + 2])], [(c2, coeffs[t + 3])]], coeffs[t + 4], slack))
    R = len(template)

    def moved(entries, j):
        return sorted((k + j * strides[k] if k else k, v) for k, v in entries)

    blocks = []
    for j in range(K):
        for t, (row, cs, slack) in enumerate(template):
            row = [moved(m, j) for m in row]
            if break_translation and j == 1 and t == R // 2:
                row[1] = [(row[1][0][0], coeffs[40])]
            blocks.append((None, row, cs, slack + j * c.stride_hash))
    general = []
    pairs = sorted({0, 1, K - 1})
    for g, k in enumerate(shared + [k + j * strides[k] for k in local[::3] for j in pairs]):
        other = shared[g % len(shared)]
        general.append((None, [[(0, coeffs[g + 7])] + ([(k, coeffs[g + 8])] if k != other else []), [(other, coeffs[g + 9])], [(k, coeffs[g + 10])]], coeffs[g + 11],
                        col(c.off_miller + 50 + g)))
    half = len(general) // 2
    order = [(t, [list(m) for m in row], cs, s) for t, row, cs, s in general[:half] + blocks + general[half:]]
    for _, row, _, _ in order:
        for m in range(3):
            row[m] = sorted(dict(row[m]).items())
    return S.system_from_rows(order, ni, n_witness=c.n_witness), half, R


@pytest.mark.parametrize("n,K", [(4, 16), (128, 2)])
def test_synthetic_systems(pkg, torch, n, K):
    """z from a compact buffer of arbitrary contents (random bits, random elements below p) and from its expansion; slacks written into both through
    the locator. The translated system has its family (asserted) and runs the pair-lane kernel; with one coefficient of block 1 changed it has none
    (asserted) and runs the general path. Both give the reference's rows for every instance, before and after a slack is bumped in every third
    pair lane and in a general row of every fifth instance."""
    dev = torch.device("cuda:0")
    eng = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=1, device=dev, n_pairs=K)
    c = eng.compact_layout()
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    comp = torch.randint(-2**63, 2**63 - 1, (c.total // 8,), dtype=torch.int64, device=dev, generator=g)
    for base, count in ((c.off_staging, n * K * c.rows_p), (c.off_inst, n * c.rows_i), (c.off_pair, n * c.pair_rows)):
        comp[base // 8:base // 8 + 6 * count].view(-1, 6)[:, 5] &= (1 << 59) - 1  # every element of the three row regions below 2^379 < p
    comp = comp.view(torch.uint8)
    plain = eng.new_witness_tensor()
    eng.expand_compact(comp, plain)
    torch.cuda.synchronize()
    limbs64, six, one = comp.view(torch.int64), torch.arange(6, device=dev), S.encode(1, 0)
    try:
        for broken in (False, True):
            sys, first, R = synthetic_system(c, broken)
            chk = pkg.ConstraintChecker.from_matrices(sys, dev)
            assert chk.pair_families(c) == ([] if broken else [(first, R)])
            assert pkg.r1cs_pair_families(sys, c) == chk.pair_families(c)
            used = sorted({k for row in sys["rows"] for mat in row for k, _ in mat} - {0})
            vals = plain[:, torch.tensor([k - 1 for k in used], device=dev)].cpu().numpy().view(np.uint64)
            zs = []
            for i in range(n):
                z = {k: S.to_int(vals[i, j]) for j, k in enumerate(used)}
                z[0] = one
                S.solve_slacks(sys, z, 0)
                zs.append(z)
            slack_rows = [r for r, s in enumerate(sys["slack"]) if s is not None]

            def write_slacks():
                offs, rows = [], []
                for r in slack_rows:
                    k = sys["slack"][r] - 1
                    colv = S.limbs([zs[i][k + 1] for i in range(n)]).view(np.int64)
                    plain[:, k] = torch.from_numpy(colv).to(dev)
                    for i in range(n):
                        reg, off, _ = pkg.compact_locate_multi(c, k, i)
                        assert reg in (pkg.COMPACT_TILE, pkg.COMPACT_PAIR) and off % 8 == 0 and off + 48 <= c.total
                        offs.append(off // 8)
                    rows.append(colv)
                idx = torch.tensor(offs, device=dev)[:, None] + six[None, :]
                limbs64[idx] = torch.from_numpy(np.concatenate(rows)).to(dev)

            def compare():
                want = [S.first_unsatisfied(sys, z, 0) for z in zs]
                assert chk.which_is_unsatisfied_compact(c, comp).tolist() == want
                assert chk.which_is_unsatisfied(plain).tolist() == want
                a, b = chk.evaluate_compact(c, comp), chk.evaluate(plain)
                for m in range(3):
                    assert torch.equal(a[m], b[m])
                    host = a[m].cpu().numpy().view(np.uint64)
                    for i in (0, n - 1):
                        ref = S.evaluate_ref(sys, zs[i], 0)
                        assert [S.to_int(x) for x in host[i]] == [t[m] for t in ref], (i, m)
                return want

            write_slacks()
            assert compare() == [-1] * n
            for p in range(0, n * K, 3):  # pair lane p = i K + j: the slack of one template row in the block of pair j
                i, j = divmod(p, K)
                S.bump(sys, zs[i], first + j * R + (p // 3) % R, (1, P - 1, 1 << 352)[(p // 3) % 3])
            for i in range(0, n, 5):
                S.bump(sys, zs[i], slack_rows[-1 - (i // 5) % 3], 1)  # a general row behind the blocks
            write_slacks()
            want = compare()
            assert all(r >= 0 for r in want[::3]) and len(set(want)) > 2
            assert torch.equal(expansion_of(torch, eng, comp), plain)  # the buffer and the vectors still hold the same step
            chk.close()
    finally:
        eng.close()


def expansion_of(torch, eng, comp):
    out = eng.new_witness_tensor()
    eng.expand_compact(comp, out)
    torch.cuda.synchronize()
    return out


def test_cpp_mirror_checks_a_compact_step(pkg, torch, oracle, tmp_path):
    """include/blsw.hpp: ConstraintSystem::which_is_unsatisfied(blsw_compact_layout_multi_t) and ::pair_families (tests/r1cs_compact_multi/cpp_caller.cpp)
    on a step this process's engine produced, with one element corrupted: the rows and the families the Python checker gives for the same buffer"""
    import os
    import subprocess

    from tests import synth
    from tests.oracle_lib import R_MOD
    from tests.test_multi_inputs_gpu import stack

    n, K, mask, msg_len = 32, 2, 13, 50
    lines, cases = [], []
    for d in range(2):  # two distinct instances, the second with a message flipped after signing (false, still satisfied), tiled over the step
        sks = [int.from_bytes(synth._h(0x5EED, b"sk", 90 + 5 * d + j), "big") % R_MOD or 1 for j in range(K)]
        ms = [(synth._h(0x5EED, b"mm", 90 + 5 * d + j) * 2)[:msg_len] for j in range(K)]
        pk48 = [bytes(oracle.sk_to_pk(sk)) for sk in sks]
        sig96 = bytes(oracle.aggregate_g2([oracle.sign(sk, m) for sk, m in zip(sks, ms)]))
        if d == 1:
            mm = bytearray(ms[1])
            mm[9] ^= 16
            ms[1] = bytes(mm)
        lines.append(sig96.hex() + " " + " ".join("%s %s" % (p.hex(), m.hex()) for p, m in zip(pk48, ms)))
        cases.append((np.stack([oracle.g1_decompress(p)[1] for p in pk48]), np.stack([np.frombuffer(m, dtype=np.uint8) for m in ms]), oracle.g2_decompress(sig96)[1], d == 0))
    dev = torch.device("cuda:0")
    batch = [cases[i % 2] for i in range(n)]
    pks, msgs, sig = stack(torch, batch, dev)
    eng = pkg.WitnessEngine(n, msg_len, max_steps=2, n_buffers=2, device=dev, n_pairs=K, multi_inputs=mask)
    c = eng.compact_layout()
    comp, inst = eng.new_compact_buffer(1)[0], eng.new_instance_tensor()
    eng.submit_multi_compact(pks, msgs, sig, comp)
    eng.submit_multi(pks, msgs, sig, witness=eng.new_witness_tensor(), instance=inst)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()
    region, off, _ = pkg.compact_locate_multi(c, c.pair_run_off[3] + 1 * c.stride_hash + 777, 5)  # pair 1 of instance 5
    assert region == pkg.COMPACT_TILE
    comp.view(torch.int64)[off // 8] += 1
    chk = pkg.ConstraintChecker(msg_len, n_pairs=K, multi_inputs=mask, device=dev)
    want = chk.which_is_unsatisfied_compact(c, comp, inst).tolist()
    fam = chk.pair_families(c)
    chk.close()
    assert [r >= 0 for r in want] == [i == 5 for i in range(n)] and fam
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "r1cs_compact_multi", "cpp_caller")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    inputs, buf = tmp_path / "inputs.txt", tmp_path / "step.bin"
    inputs.write_text("\n".join(lines[i % 2] for i in range(n)) + "\n")
    comp.cpu().numpy().tofile(str(buf))
    out = subprocess.check_output([exe, str(inputs), str(buf)], text=True, timeout=300).split("\n")
    assert out[0].split() == ["families"] + ["%d:%d" % f for f in fam]
    assert out[1].split() == ["rows"] + [str(r) for r in want]
