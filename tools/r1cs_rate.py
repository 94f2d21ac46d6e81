#!/usr/bin/env python3
"""Rate of the device R1CS evaluator (blsw_r1cs_check / _evaluate) on the single-key shape, one JSON line:
    check_instances_per_s, check_ms_per_1024   the satisfaction check of a batch of n (default 1 024) engine-written witness vectors
    unreduced_ms_per_1024                       the separate first-unreduced pass (HBM stream of the vectors)
    evaluate_instances_per_s                    A z, B z, C z of every row for a slice of the batch (output n x 3 x 34 MB)
    products_per_instance                       product-equivalents counted from the encoded class histogram (a table coefficient = 1,
                                                a row = 3 reductions of half a product + 2 products), and the rate that implies

    python tools/r1cs_rate.py [--n 1024] [--reps 3] [--eval-n 64]

--compact: from a step in compact wire form to a verdict, two legs interleaved in one process over the same compact steps (HIP-event time per
call; median / min / max of --reps >= 5 calls each):
    expand_then_check   blsw_engine_expand_compact into n witness vectors, then blsw_r1cs_check on them (the only route before ABI 14)
    check_compact       blsw_r1cs_check_compact on the buffer itself
and the same pair for A z, B z, C z over a window of --eval-rows rows at the pairing tail (expand + evaluate / evaluate_compact).

    python tools/r1cs_rate.py --compact [--n 1024] [--reps 5] [--steps 2] [--eval-rows 20000]

--keyset: from a SHARED-KEYS step (options.shared_keys) in compact wire form to a verdict at committee size, four legs interleaved in one process over
the same steps (HIP-event time per call; median / min / max of --reps >= 5 calls each):
    expand_then_check     (a) blsw_engine_expand_compact_keyset into n witness vectors, then blsw_r1cs_check on them (the only route before ABI 16)
    check_compact         (b) blsw_r1cs_check_compact_keyset, BLSW_R1CS_HEAD_CHECK: every row for every instance, from the buffer and the set's table
    check_compact_skip    (c) the same with BLSW_R1CS_HEAD_SKIP: the rows behind the head rows only
    check_keyset          (d) blsw_r1cs_check_keyset alone: the committee's head rows, once per set
The yardstick of every leg is (a). Every GPU step runs under a time limit; when one expires or fails the process ends there and nothing follows.

    python tools/r1cs_rate.py --keyset [--n 128] [--keys 512] [--reps 5] [--steps 2] [--limit 240]

--multi: from a step of the N+1-pair product in compact wire form to a verdict, three routes interleaved call by call in one process over the same
steps (HIP-event time per call; median / min / max of --reps >= 5 calls each after one warm-up round), one JSON line per step size:
    expand_then_check     (a) blsw_engine_expand_compact into n witness vectors, then blsw_r1cs_check on them (the only route before this form was described)
    check_compact         (b) blsw_r1cs_check_compact_multi: the pair families one pair per lane, the other rows one instance per lane
    check_compact_general (c) the same call with the families switched off (blsw_r1cs_check_compact_multi_ex, use_families 0): every row one instance per lane
The yardstick of (b) and (c) is (a). The steps are satisfied systems whose Boolean is false (keys, messages and signature do not belong together).

    python tools/r1cs_rate.py --multi [--pairs 16] [--multi-n 4,64] [--reps 5] [--steps 2] [--limit 240]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def class_histogram(mats):
    """entries per class as blsw_r1cs_create encodes them: +-1, other |c| < 2^30, table (everything else); rows with non-empty A and B"""
    r_inv = pow(1 << 384, -1, P_MOD)
    h = {"one": 0, "small": 0, "table": 0}
    for name in "ABC":
        _, _, val = mats[name]
        uniq, counts = np.unique(val, axis=0, return_counts=True)
        for v, c in zip(uniq, counts):
            x = sum(int(w) << (64 * k) for k, w in enumerate(v)) * r_inv % P_MOD
            s = min(x, P_MOD - x)
            h["one" if s == 1 else ("small" if s < (1 << 30) else "table")] += int(c)
    ra, rb = (np.diff(mats[k][0].astype(np.int64)) > 0 for k in "AB")
    h["rows"] = int(mats["n_constraints"])
    h["rows_ab"] = int((ra & rb).sum())
    return h


def stats(ms, n):
    ms = sorted(ms)
    med = ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2])
    return {"median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "calls": len(ms), "instances_per_s": round(n / (med / 1e3), 1)}


def compact_legs(a):
    """--compact: the two routes from compact steps to a verdict, alternating, over the same steps of the grouped engine"""
    import torch

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    reps = max(5, a.reps)
    mats = pkg.matrices(32)
    chk = pkg.ConstraintChecker.from_matrices(mats, dev)
    eng = pkg.WitnessEngine(a.n, 32, max_steps=16, device=dev, n_buffers=3)
    lay = eng.compact_layout()
    assert lay.total == eng.compact_bytes()
    comp = eng.new_compact_buffer(a.steps)
    batches = [workload.make_batch(pkg, a.n, device=dev, start=s * a.n) for s in range(a.steps)]
    for s, (pk, msg, sig, _) in enumerate(batches):
        eng.submit_compact(pk, sig, msg, comp[s])
    eng.flush()
    torch.cuda.synchronize()
    w = eng.new_witness_tensor()  # the receiver's n vectors of 34 MB (leg a only)
    nc = int(mats["n_constraints"])
    rows = (nc - a.eval_rows, a.eval_rows)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def leg_a(s):
        eng.expand_compact(comp[s], w)
        return chk.which_is_unsatisfied(w)

    def leg_b(s):
        return chk.which_is_unsatisfied_compact(lay, comp[s])

    def eval_a(s):
        eng.expand_compact(comp[s], w)
        return chk.evaluate(w, rows=rows)

    def eval_b(s):
        return chk.evaluate_compact(lay, comp[s], rows=rows)

    legs = {"expand_then_check": leg_a, "check_compact": leg_b, "expand_then_evaluate": eval_a, "evaluate_compact": eval_b}
    ms = {k: [] for k in legs}
    same = True
    for pair in (("expand_then_check", "check_compact"), ("expand_then_evaluate", "evaluate_compact")):
        for k in pair:  # warm-up of both legs
            legs[k](0)
        torch.cuda.synchronize()
        for r in range(reps):
            s = r % a.steps
            outs = []
            for k in pair:  # alternating: a, b, a, b, ...
                t, out = timed(lambda: legs[k](s))
                ms[k].append(t)
                outs.append(out)
            if pair[0] == "expand_then_check":
                same = same and torch.equal(outs[0], outs[1]) and bool((outs[1] < 0).all())
            else:
                same = same and all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
            del outs
    eng.close()
    out = {"metric": "r1cs_check_compact_single_key", "n": a.n, "steps": a.steps, "eval_rows": a.eval_rows, "legs_agree_and_satisfied": same,
           "compact_bytes_per_instance": lay.total // a.n, "expanded_bytes_per_instance": int(mats["n_witness"]) * 48}
    out.update({k: stats(v, a.n) for k, v in ms.items()})
    out["check_compact_over_expand_then_check"] = round(out["check_compact"]["median_ms"] / out["expand_then_check"]["median_ms"], 3)
    out["check_compact_share_of_10k_per_s"] = round(out["check_compact"]["instances_per_s"] / 1e4, 3)
    print(json.dumps(out))


def keyset_legs(a):
    """--keyset: the routes from a shared-keys compact step to a verdict, alternating, over the same steps"""
    import torch

    from tools.agg_inputs_rate import StepLimit

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    reps = max(5, a.reps)
    n = a.n
    K = a.keys
    t0 = time.time()
    mats = pkg.matrices(32, n_keys=K)
    t_mats = time.time() - t0
    with StepLimit(a.limit, "set-up"):
        chk = pkg.ConstraintChecker.from_matrices(mats, dev)
        pk, msg, sig, _ = workload.make_batch(pkg, max(n * a.steps, K), device=dev, tamper_every=0)
        keyset = pkg.KeySet(pk[:K].contiguous())
        bitmap = (torch.arange(n * K, device=dev).reshape(n, K) % 3 != 0).to(torch.uint8).contiguous()  # two thirds of the committee signed
        eng = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=2, device=dev, n_keys=K, shared_keys=1)
        lay = eng.compact_layout()
        assert lay.total == eng.compact_bytes() and lay.n_witness + K * pkg.SEG_PK_ALLOC == chk.n_witness
        comp = eng.new_compact_buffer(a.steps)
        for s in range(a.steps):  # the signatures do not match the bitmaps: the gadget's Boolean is false, the assignment still satisfies the system
            eng.submit_aggregate_keyset_compact(keyset, bitmap, sig[s * n:(s + 1) * n].contiguous(), msg[s * n:(s + 1) * n].contiguous(), comp[s])
        eng.flush()
        torch.cuda.synchronize()
        w = eng.new_witness_tensor()  # the receiver's n expanded vectors (leg a only)
    head_rows = chk.head_rows(K)

    def leg_a(s):
        eng.expand_compact(comp[s], w, keyset=keyset)
        return chk.which_is_unsatisfied(w)

    legs = {"expand_then_check": leg_a,
            "check_compact": lambda s: chk.which_is_unsatisfied_compact(lay, comp[s], keyset=keyset),
            "check_compact_skip": lambda s: chk.which_is_unsatisfied_compact(lay, comp[s], keyset=keyset, skip_head_rows=True)}
    stream = torch.cuda.current_stream(dev).cuda_stream
    committee = torch.empty(2, dtype=torch.int64, device=dev)

    def leg_d(s):  # the C call: ConstraintChecker.check_keyset reads its result back, which a timed leg must not
        rc = pkg.lib().blsw_r1cs_check_keyset(chk._r, keyset._ks, committee[0:].data_ptr(), committee[1:].data_ptr(), stream)
        assert rc == 0, rc
        return committee

    legs["check_keyset"] = leg_d
    ms = {k: [] for k in legs}
    same = True
    for rep_i in range(reps + 1):  # the first repetition warms up
        s = rep_i % a.steps
        outs = {}
        for k, fn in legs.items():  # alternating: a, b, c, d, a, ...
            with StepLimit(a.limit, "repetition %d of %s" % (rep_i, k)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[k] = fn(s)
                e1.record()
                torch.cuda.synchronize()
            if rep_i:
                ms[k].append(e0.elapsed_time(e1))
        same = same and torch.equal(outs["expand_then_check"], outs["check_compact"]) and torch.equal(outs["check_compact"], outs["check_compact_skip"])
        same = same and bool((outs["check_compact"] < 0).all()) and outs["check_keyset"].tolist() == [-1, -1]
    eng.close()
    keyset.close()
    out = {"metric": "r1cs_check_compact_keyset", "n": n, "n_keys": K, "steps": a.steps, "abi": pkg.lib().blsw_version(), "legs_agree_and_satisfied": same,
           "n_constraints": int(mats["n_constraints"]), "head_rows": head_rows, "head_rows_share": round(head_rows / int(mats["n_constraints"]), 3),
           "compact_bytes_per_instance": lay.total // n, "expanded_bytes_per_instance": int(mats["n_witness"]) * 48, "host_matrices_s": round(t_mats, 2)}
    out.update({k: stats(v, n) for k, v in ms.items()})
    del out["check_keyset"]["instances_per_s"]  # once per set, not per instance
    for k in ("check_compact", "check_compact_skip"):  # every new leg against the route that existed before, never against each other
        out[k + "_over_expand_then_check"] = round(out[k]["median_ms"] / out["expand_then_check"]["median_ms"], 3)
    print(json.dumps(out))
    if not same:
        sys.exit(1)


def multi_legs(a):
    """--multi: the routes from a compact step of the N+1-pair product to a verdict, alternating, over the same steps"""
    import torch

    from tools.agg_inputs_rate import StepLimit

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    reps = max(5, a.reps)
    K = a.pairs
    t0 = time.time()
    mats = pkg.matrices(32, n_pairs=K)
    t_mats = time.time() - t0
    nc = int(mats["n_constraints"])
    with StepLimit(a.limit, "set-up"):
        chk = pkg.ConstraintChecker.from_matrices(mats, dev)
    ok = True
    for n in [int(x) for x in a.multi_n.split(",")]:
        with StepLimit(a.limit, "set-up of n = %d" % n):
            pk, msg, sig, _ = workload.make_batch(pkg, n * K * a.steps, device=dev, tamper_every=0)
            eng = pkg.WitnessEngine(n, 32, max_steps=2, n_buffers=2, device=dev, n_pairs=K)
            lay = eng.compact_layout()
            assert lay.total == eng.compact_bytes() and lay.n_witness == chk.n_witness
            comp = eng.new_compact_buffer(a.steps)
            for s in range(a.steps):
                sl = slice(s * n * K, (s + 1) * n * K)
                eng.submit_multi_compact(pk[sl].reshape(n, K, 12).contiguous(), msg[sl].reshape(n, K, 32).contiguous(), sig[s * n:(s + 1) * n].contiguous(), comp[s])
            eng.flush()
            torch.cuda.synchronize()
            w = eng.new_witness_tensor()  # the receiver's n expanded vectors (leg a only)
            t0 = time.time()
            fam = chk.pair_families(lay)  # once per (handle, layout): not part of a timed call
            t_fam = time.time() - t0

        def leg_a(s):
            eng.expand_compact(comp[s], w)
            return chk.which_is_unsatisfied(w)

        legs = {"expand_then_check": leg_a, "check_compact": lambda s: chk.which_is_unsatisfied_compact(lay, comp[s]),
                "check_compact_general": lambda s: chk._check_compact(lay, comp[s], None, None, False, _use_families=False)[0]}
        ms = {k: [] for k in legs}
        same = True
        for rep_i in range(reps + 1):  # the first repetition warms up
            s = rep_i % a.steps
            outs = {}
            for k, fn in legs.items():  # alternating: a, b, c, a, ...
                with StepLimit(a.limit, "repetition %d of %s" % (rep_i, k)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    outs[k] = fn(s)
                    e1.record()
                    torch.cuda.synchronize()
                if rep_i:
                    ms[k].append(e0.elapsed_time(e1))
            same = same and torch.equal(outs["expand_then_check"], outs["check_compact"]) and torch.equal(outs["check_compact"], outs["check_compact_general"])
            same = same and bool((outs["check_compact"] < 0).all())
        eng.close()
        del w, comp
        fam_rows = sum(R for _, R in fam) * K
        entries = {name: np.diff(mats[name][0].astype(np.int64)) for name in "ABC"}
        nnz = sum(int(e.sum()) for e in entries.values())
        nnz_template = sum(int(e[f:f + R].sum()) for e in entries.values() for f, R in fam)
        nnz_family = sum(int(e[f:f + K * R].sum()) for e in entries.values() for f, R in fam)
        out = {"metric": "r1cs_check_compact_multi", "n": n, "n_pairs": K, "steps": a.steps, "legs_agree_and_satisfied": same, "n_constraints": nc,
               "families": len(fam), "family_rows_share": round(fam_rows / nc, 4), "families_host_s": round(t_fam, 2), "host_matrices_s": round(t_mats, 2),
               "compact_bytes_per_step": int(lay.total), "expanded_bytes_per_step": int(mats["n_witness"]) * 48 * n,
               # what each route moves, ESTIMATED from the buffers' sizes (no counter is read): (a) reads the buffer, writes and reads back the vectors; (b) and (c) read the buffer
               "bytes_estimated_expand_then_check": int(lay.total) + 2 * int(mats["n_witness"]) * 48 * n, "bytes_estimated_check_compact": int(lay.total),
               # matrix entries a wave walks per group of lanes: every entry (a, c); the templates once plus the rows outside the families (b)
               "entries_general": nnz, "entries_check_compact": nnz - nnz_family + nnz_template}
        out.update({k: stats(v, n) for k, v in ms.items()})
        for k in ("check_compact", "check_compact_general"):
            out[k + "_over_expand_then_check"] = round(out[k]["median_ms"] / out["expand_then_check"]["median_ms"], 3)
        print(json.dumps(out), flush=True)
        ok = ok and same
    if not ok:
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None, help="instances per batch / step: 1024, with --keyset 128 (the step of tools/agg_shared_rate.py)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eval-n", type=int, default=64)
    ap.add_argument("--compact", action="store_true", help="expand_compact + check against check_compact, interleaved (see the module docstring)")
    ap.add_argument("--steps", type=int, default=2, help="--compact: distinct compact steps the calls rotate over")
    ap.add_argument("--eval-rows", type=int, default=20000, help="--compact: rows of the evaluate window (the pairing tail)")
    ap.add_argument("--keyset", action="store_true", help="a shared-keys compact step: expand + check against the compact-keyset checks (see the module docstring)")
    ap.add_argument("--keys", type=int, default=512, help="--keyset: keys of the committee")
    ap.add_argument("--limit", type=float, default=240.0, help="--keyset, --multi: seconds per GPU step")
    ap.add_argument("--multi", action="store_true", help="a compact step of the N+1-pair product: expand + check against the compact check with and without families")
    ap.add_argument("--pairs", type=int, default=16, help="--multi: pairs per instance")
    ap.add_argument("--multi-n", default="4,64", help="--multi: step sizes, comma separated (n * pairs a multiple of 64, n a divisor or multiple of 64)")
    a = ap.parse_args()
    a.n = a.n or (128 if a.keyset else 1024)
    if a.compact:
        return compact_legs(a)
    if a.keyset:
        return keyset_legs(a)
    if a.multi:
        return multi_legs(a)
    import torch

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    t0 = time.time()
    mats = pkg.matrices(32)
    t_mats = time.time() - t0
    t0 = time.time()
    chk = pkg.ConstraintChecker.from_matrices(mats, dev)
    t_create = time.time() - t0
    pk, msg, sig, _ = workload.make_batch(pkg, a.n, device=dev)
    eng = pkg.WitnessEngine(a.n, 32, max_steps=16, device=dev, n_buffers=3)
    w = eng.new_witness_tensor()
    eng.submit(pk, sig, msg, witness=w)
    eng.flush()
    torch.cuda.synchronize()
    eng.close()

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        best = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1))
        return min(best), out

    ms_check, bad = timed(lambda: chk.which_is_unsatisfied(w))
    ms_both, _ = timed(lambda: chk.first_unreduced(w))
    ok = int((bad < 0).sum().item())
    we = w[:a.eval_n]
    ms_eval, _ = timed(lambda: chk.evaluate(we))
    h = class_histogram(mats)
    prod = h["table"] + 1.5 * h["rows"] + 2 * h["rows_ab"]
    print(json.dumps({
        "metric": "r1cs_check_single_key", "n": a.n, "satisfied": ok,
        "check_instances_per_s": round(a.n / (ms_check / 1e3), 1), "check_ms_per_1024": round(ms_check * 1024 / a.n, 3),
        "unreduced_ms_per_1024": round((ms_both - ms_check) * 1024 / a.n, 3),
        "evaluate_instances_per_s": round(a.eval_n / (ms_eval / 1e3), 1), "eval_n": a.eval_n,
        "products_per_instance": int(prod), "implied_products_per_s": round(prod * a.n / (ms_check / 1e3) / 1e9, 2) * 1e9,
        "classes": h, "device_bytes": chk.buffer.numel(), "host_matrices_s": round(t_mats, 2), "create_s": round(t_create, 2),
    }))


if __name__ == "__main__":
    main()
