#!/usr/bin/env python3
"""blsw_verify_batch (BLS::verify as values, bls.rs:427-458): verdicts per second at three batch sizes. One JSON line each.
--groups: blsw_verify_groups_batch and verify_batch_grouped against verify_batch in the same process (groups_rates)."""
import importlib, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("bls-verify-gadget_amd")
workload = importlib.import_module("bls-verify-gadget_amd.workload")
dev = torch.device("cuda:0")


def signed_batch(n):
    sk = np.frombuffer(b"".join(workload.secret_keys(0x5EED, 16)[i % 16].to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()
    msg = torch.from_numpy(workload.messages(0x5EED, 0, n)).to(dev)
    s = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg)
    return s["pk48"], msg, s["sig96"]


def groups_rates(group=64, reps=5):
    """--groups: verify_batch, verify_groups and verify_batch_grouped ALTERNATING in one process on the same all-valid inputs with fixed seeded
    coefficients, medians of `reps` synchronised calls after a warm-up of every shape; then verify_batch_grouped on the every-16th-tampered batch
    (every group falls back: the worst case). The yardstick is this call's verify_batch, never a figure from another box."""
    sizes = (65536, 262144)
    data = {}
    for n in sizes:
        pk, msg, sig = signed_batch(n)
        bad = msg.clone()
        bad[15::16, 31] ^= 1
        sc = torch.from_numpy((np.random.default_rng(n).integers(1, 2**63, size=n, dtype=np.uint64) * 2 + 1).view(np.int64)).to(dev)
        data[n] = (pk, msg, sig, bad, sc)
    calls = {
        "verify_batch": lambda d: pkg.verify_batch(d[0], d[1], d[2]),
        "verify_groups": lambda d: pkg.verify_groups(d[0], d[1], d[2], group=group, scalars=d[4]),
        "verify_batch_grouped": lambda d: pkg.verify_batch_grouped(d[0], d[1], d[2], group=group, scalars=d[4]),
        "verify_batch_grouped_tampered": lambda d: pkg.verify_batch_grouped(d[0], d[3], d[2], group=group, scalars=d[4]),
    }
    for n in sizes:  # warm-up of every shape: code objects, workspaces in the caching allocator
        for f in calls.values():
            f(data[n])
    torch.cuda.synchronize()
    for n in sizes:
        d = data[n]
        ms = {k: [] for k in calls}
        last = {}
        for _ in range(reps):
            for k in ("verify_batch", "verify_groups", "verify_batch_grouped"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[k] = calls[k](d)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for _ in range(reps):
            k = "verify_batch_grouped_tampered"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = calls[k](d)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
        ref = float(np.median(ms["verify_batch"]))
        ref_bad = pkg.verify_batch(d[0], d[3], d[2])
        for k in calls:
            m = float(np.median(ms[k]))
            line = {"case": k, "n": n, "group": group, "chunk": pkg.VERIFY_GROUPS_CHUNK, "verdicts_per_s": n / (m * 1e-3), "ms": m, "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                    "ratio_vs_verify_batch": ref / m}
            if k == "verify_batch_grouped_tampered":
                line["matches_verify_batch"] = bool(torch.equal(last[k], ref_bad))
            else:
                line["all_true"] = bool((last[k] == 1).all().item())
            print(json.dumps(line), flush=True)


if "--groups" in sys.argv:
    # --chunk-table: the same lines from a library built with another -DBLSW_VGROUP_CHUNK (build.py --out <lib> -DBLSW_VGROUP_CHUNK=<c> and the header
    # edited to match, selected with BLSW_LIB): one process per build, the lines carry "chunk"
    groups_rates()
    sys.exit(0)
for n in (16384, 65536, 262144):
    sk = np.frombuffer(b"".join(workload.secret_keys(0x5EED, 16)[i % 16].to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()
    msg = torch.from_numpy(workload.messages(0x5EED, 0, n)).to(dev)
    s = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg)
    r = pkg.verify_batch(s["pk48"], msg, s["sig96"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        r = pkg.verify_batch(s["pk48"], msg, s["sig96"])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(json.dumps({"n": n, "verdicts_per_s": n / dt, "ms": dt * 1e3, "all_true": bool((r == 1).all().item())}))
