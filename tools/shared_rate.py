#!/usr/bin/env python3
"""blsw_verify_groups_shared_batch / blsw_registry_verify_shared_batch against the plain grouped entries on materialised messages, in ONE process: the
legs of a shape run interleaved, `--reps` repetitions each after one warm-up of every leg, every repetition printed as one JSON line, then the medians,
the spread (max - min) of the plain leg and the workspace bytes (profiles/shared_rate.txt is this output).

GROUPS shape — group = 64, 32-byte messages, n = 8 192 and 65 536 (--n a,b chooses others):
  p      verify_groups on the n materialised messages: the baseline
  sN     the shared form over n distinct messages, index i = i: one run per instance. The plain entry's work plus the scan and a one-term merge, so
         its time should lie within the spread of p; the line "groups" states both and the verdict
  s8     n / 8 messages, runs of eight
  s64    n / 64 messages: one run per group
  s1     one message
  k8 k64 s8 and s64 from a library built with -DBLSW_VS_SKIP_EMPTY (a team whose chunk is empty stores the partial 1 without walking its 63
         squarings of one): what keeping the walk costs is s64 - k64 — negative when the skip is the slower form, which is what was measured.
         --no-skip skips the legs; --build-only makes that library and exits (no device needed)
REGISTRY shape — tools/registry_rate.py's attestation shape: a registry of 2^20 keys (--keys N shrinks it), 2 048 sets, half of them with 400 .. 500
indices and half with one, 64 distinct messages sorted within the groups of 64:
  r64    registry_verify(group=64) on the materialised messages
  rs64   the shared form over the table of 64"""
import ctypes, importlib, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")
build = importlib.import_module("bls-verify-gadget_amd.build")
GROUP, N_ATT = 64, 2048
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SHARED_SYMBOLS = [s for s in pkg.EXPORTED_SYMBOLS if "_shared_" in s]


def skip_library():
    path = os.path.join(ROOT, "_ab", "libblsw_vs_skip_empty.so")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        build.build(out=path, defines=["-DBLSW_VS_SKIP_EMPTY=1"])
    return path


if "--build-only" in sys.argv:
    print(skip_library(), flush=True)
    sys.exit(0)

import torch

dev = torch.device("cuda:0")
arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
reps, n_keys = int(arg("--reps", 7)), int(arg("--keys", 1 << 20))
sizes = [int(x) for x in str(arg("--n", "8192,65536")).split(",")]
base = pkg.lib()
walk = None
if "--no-skip" not in sys.argv:
    walk = ctypes.CDLL(skip_library())
    for name in SHARED_SYMBOLS:
        getattr(walk, name).argtypes = getattr(base, name).argtypes


def under(v, f):
    """f() with the wrapper's library replaced by v"""
    pkg._lib = v
    try:
        return f()
    finally:
        pkg._lib = base


sk_of = lambda i: 0x1000003 + 7919 * i
sk_bytes = lambda xs: torch.from_numpy(np.frombuffer(b"".join(int(s).to_bytes(32, "little") for s in xs), dtype=np.uint8).reshape(len(xs), 32).copy()).to(dev)
i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)
i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def run(legs, check):
    out = {k: f() for k, f in legs.items()}  # warm-up of every leg: code objects, workspaces in the caching allocator
    torch.cuda.synchronize()
    agree = check(out)
    ms = {k: [] for k in legs}
    for rep in range(reps):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"rep": rep, "leg": k, "ms": round(ms[k][-1], 3)}), flush=True)
    return ms, {k: float(np.median(v)) for k, v in ms.items()}, agree


def ws_bytes(fn, *a):
    b = ctypes.c_uint64(0)
    assert fn(*a, ctypes.byref(b)) == 0
    return b.value


rng = np.random.default_rng(0x5A4ED)
# ---------------------------------------------------------------- the groups shape
for n in sizes:
    sks = sk_bytes([sk_of(i % 16) for i in range(n)])
    table = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).to(dev)
    scalars = i64(rng.integers(1, 2**63, size=n, dtype=np.uint64) * 2 + 1)
    legs, bytes_ = {}, {"p": ws_bytes(base.blsw_verify_groups_workspace_bytes, n, 32, GROUP)}
    pk = None
    for name, per in (("sN", 1), ("s8", 8), ("s64", 64), ("s1", n)):
        n_msgs = (n + per - 1) // per
        rows = np.arange(n) // per
        r = pkg.sign_batch(sks, table[torch.from_numpy(rows).to(dev)].contiguous())
        pk = r["pk48"].contiguous()
        sig, idx, tab = r["sig96"].contiguous(), i32(rows), table[:n_msgs].contiguous()
        if name == "sN":
            legs["p"] = (lambda sig: lambda: pkg.verify_groups(pk, table, sig, group=GROUP, scalars=scalars))(sig)
        legs[name] = (lambda sig, idx, tab: lambda: pkg.verify_groups(pk, tab, sig, group=GROUP, scalars=scalars, msg_index=idx))(sig, idx, tab)
        bytes_[name] = ws_bytes(base.blsw_verify_groups_shared_workspace_bytes, n, n_msgs, 32, GROUP)
        if name in ("s8", "s64") and walk is not None:
            legs["k" + name[1:]] = (lambda sig, idx, tab: lambda: under(walk, lambda: pkg.verify_groups(pk, tab, sig, group=GROUP, scalars=scalars, msg_index=idx)))(sig, idx, tab)
    ms, med, agree = run(legs, lambda out: all(bool((v == 1).all().item()) for v in out.values()))
    spread_p = max(ms["p"]) - min(ms["p"])
    print(json.dumps({"shape": "groups", "n": n, "group": GROUP, "reps": reps, "all_true": agree, "median_ms": {k: round(v, 3) for k, v in med.items()},
                      "min_ms": {k: round(min(v), 3) for k, v in ms.items()}, "max_ms": {k: round(max(v), 3) for k, v in ms.items()},
                      "sets_per_s": {k: round(n / (v / 1e3)) for k, v in med.items()}, "workspace_bytes": bytes_, "spread_of_p_ms": round(spread_p, 3),
                      "sN_minus_p_ms": round(med["sN"] - med["p"], 3), "sN_within_the_spread_of_p": bool(abs(med["sN"] - med["p"]) <= spread_p),
                      "walk_minus_skip_ms": {k: round(med["s" + k] - med["k" + k], 3) for k in ("8", "64") if "k" + k in med}}), flush=True)
    del legs

# ---------------------------------------------------------------- the registry shape
if "--no-registry" not in sys.argv:
    pks = torch.cat([pkg.sign_batch(sk_bytes([sk_of(i) for i in range(lo, min(n_keys, lo + (1 << 16)))]), torch.zeros((min(n_keys, lo + (1 << 16)) - lo, 32), dtype=torch.uint8, device=dev))["pk48"]
                     for lo in range(0, n_keys, 1 << 16)]).contiguous()
    reg = pkg.KeyRegistry(n_keys, device=dev)
    reg.append(pks)
    lists = [rng.integers(0, n_keys, size=int(rng.integers(400, 501)) if i % 2 == 0 else 1) for i in range(N_ATT)]
    table = torch.from_numpy(rng.integers(0, 256, size=(64, 32), dtype=np.uint8)).to(dev)
    rows = np.concatenate([np.sort(rng.integers(0, 64, size=GROUP)) for _ in range(N_ATT // GROUP)])  # 64 distinct messages, sorted within each group
    msg = table[torch.from_numpy(rows).to(dev)].contiguous()
    sig = pkg.sign_batch(sk_bytes([sum(sk_of(int(k)) for k in lst) % R_MOD for lst in lists]), msg)["sig96"].contiguous()
    scalars = i64(rng.integers(1, 2**63, size=N_ATT, dtype=np.uint64) * 2 + 1)
    off = np.zeros(N_ATT + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    idx, off, mi = i32(np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists])), i64(off), i32(rows)
    legs = {"r64": lambda: pkg.registry_verify(reg, idx, off, msg, sig, group=GROUP, scalars=scalars),
            "rs64": lambda: pkg.registry_verify(reg, idx, off, table, sig, group=GROUP, scalars=scalars, msg_index=mi)}
    ms, med, agree = run(legs, lambda out: torch.equal(out["r64"], out["rs64"]) and bool((out["r64"] == 1).all().item()))
    runs = pkg.registry_verify(reg, idx, off, table, sig, group=GROUP, scalars=scalars, msg_index=mi, want_runs=True)[1]
    print(json.dumps({"shape": "registry", "n": N_ATT, "n_keys": n_keys, "n_msgs": 64, "group": GROUP, "reps": reps, "legs_agree_all_true": agree,
                      "mean_runs_per_group": float(runs.float().mean().item()), "median_ms": {k: round(v, 3) for k, v in med.items()},
                      "min_ms": {k: round(min(v), 3) for k, v in ms.items()}, "max_ms": {k: round(max(v), 3) for k, v in ms.items()},
                      "spread_of_r64_ms": round(max(ms["r64"]) - min(ms["r64"]), 3), "rs64_over_r64": med["rs64"] / med["r64"],
                      "workspace_bytes": {"r64": ws_bytes(base.blsw_registry_verify_workspace_bytes, N_ATT, 32, GROUP),
                                          "rs64": ws_bytes(base.blsw_registry_verify_shared_workspace_bytes, N_ATT, 64, 32, GROUP)}}), flush=True)
