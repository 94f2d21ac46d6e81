#!/usr/bin/env python3
"""blsw_registry_verify_batch against what it stands beside and what it replaces, in ONE process: the legs of a shape run interleaved, `--reps`
repetitions each, every repetition printed as one JSON line, then the medians (profiles/registry_rate.txt is this output).

SYNC shape — K = 512 keys, n = 8 192, about 90 % participation, 32-byte messages (tools/committee_rate.py's):
  b   verify_batch on the n pre-aggregated keys: the floor if the sum cost nothing
  c   committee_verify, group = 0
  r   registry_verify, group = 0, over a registry of the same 512 keys, the lists the ascending indices of the bitmap rows
  fL  r again from libraries built with -DBLSW_REGISTRY_LANES=L for L in {4, 8, 16, 32, 64} (build(defines=...); kept under _ab/)
The expectation: r / b exceeds c / b by no more than the spread (max - min) of c's repetitions. The line "sync" states both and the verdict.

ATTESTATION shape — a registry of 2^20 keys, n = 2 048 sets, half of them with 400 .. 500 indices and half with one, interleaved:
  append  the 2^20 keys into a fresh registry (one blsw_registry_append), timed alone
  p0 p64  the parent's composition: gather the compressed keys, aggregate_points (one call per list length), then verify_batch / verify_groups(64)
  r0 r64  registry_verify, group 0 and 64
  s0      r0 with the same sets SORTED by length: what mixing lengths inside a wave costs is r0 - s0
  gL      r0 from the libraries of leg fL
--build-only makes the libraries of legs fL / gL and exits (no device needed); --no-lanes skips them; --keys N shrinks the registry (a quick look)."""
import ctypes, importlib, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")
build = importlib.import_module("bls-verify-gadget_amd.build")
LANES = (4, 8, 16, 32, 64)
K, N_SYNC, N_ATT, GROUP = 512, 8192, 2048, 64
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
REGISTRY_SYMBOLS = [s for s in pkg.EXPORTED_SYMBOLS if s.startswith("blsw_registry_")]


def lanes_library(L):
    path = os.path.join(ROOT, "_ab", "libblsw_registry_lanes%d.so" % L)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        build.build(out=path, defines=["-DBLSW_REGISTRY_LANES=%d" % L])
    return path


if "--build-only" in sys.argv:
    for L in LANES:
        print(lanes_library(L), flush=True)
    sys.exit(0)

import torch

dev = torch.device("cuda:0")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
reps, n_keys = arg("--reps", 5), arg("--keys", 1 << 20)
base = pkg.lib()
variants = {}
if "--no-lanes" not in sys.argv:
    for L in LANES:
        v = ctypes.CDLL(lanes_library(L))
        for name in REGISTRY_SYMBOLS:
            getattr(v, name).argtypes = getattr(base, name).argtypes
        variants[L] = v


def under(v, f):
    """f() with the wrapper's library replaced by v: the wrapper's own path, another library's registry entry points"""
    pkg._lib = v
    try:
        return f()
    finally:
        pkg._lib = base


sk_of = lambda i: 0x1000003 + 7919 * i
sk_bytes = lambda xs: torch.from_numpy(np.frombuffer(b"".join(int(s).to_bytes(32, "little") for s in xs), dtype=np.uint8).reshape(len(xs), 32).copy()).to(dev)
i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)
i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def mint(n, chunk=1 << 16):
    """the compressed keys of secret keys sk_of(0 .. n): sign_batch in chunks (its workspace is per instance)"""
    out = []
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        out.append(pkg.sign_batch(sk_bytes([sk_of(i) for i in range(lo, lo + m)]), torch.zeros((m, 32), dtype=torch.uint8, device=dev))["pk48"])
    return torch.cat(out).contiguous()


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    return i32(np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists])), i64(off)


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


def registry_of(pks48, capacity):
    reg = pkg.KeyRegistry(capacity, device=dev)
    reg.append(pks48)
    return reg


# ---------------------------------------------------------------- the sync shape
rng = np.random.default_rng(0xC0117EE)
pks_all = mint(max(n_keys, K))
pks512 = pks_all[:K].contiguous()
bitmap_h = (rng.random((N_SYNC, K)) < 0.9).astype(np.uint8)
msg = torch.from_numpy(rng.integers(0, 256, size=(N_SYNC, 32), dtype=np.uint8)).to(dev)
sks512 = [sk_of(i) for i in range(K)]
sig = pkg.sign_batch(sk_bytes([sum(sks512[j] for j in np.flatnonzero(row)) % R_MOD for row in bitmap_h]), msg)["sig96"]
bitmap = torch.from_numpy(bitmap_h).to(dev)
idx, off = csr([np.flatnonzero(row) for row in bitmap_h])
_, agg48 = pkg.committee_verify(pks512, bitmap, msg, sig, want_aggregate=True)
reg512 = registry_of(pks512, K)
legs = {"b": lambda: pkg.verify_batch(agg48, msg, sig), "c": lambda: pkg.committee_verify(pks512, bitmap, msg, sig), "r": lambda: pkg.registry_verify(reg512, idx, off, msg, sig)}
for L, v in variants.items():
    rv = under(v, lambda: registry_of(pks512, K))
    legs["f%d" % L] = (lambda v, rv: lambda: under(v, lambda: pkg.registry_verify(rv, idx, off, msg, sig)))(v, rv)
ms, med, agree = run(legs, lambda out: all(torch.equal(out[k], out["b"]) for k in out) and bool((out["b"] == 1).all().item()))
spread_c = max(ms["c"]) - min(ms["c"])
print(json.dumps({"shape": "sync", "n": N_SYNC, "n_keys": K, "lanes": pkg.REGISTRY_LANES, "participation": float(bitmap_h.mean()), "legs_agree_all_true": agree,
                  "median_ms": {k: round(v, 3) for k, v in med.items()}, "c_over_b": med["c"] / med["b"], "r_over_b": med["r"] / med["b"], "spread_of_c_ms": round(spread_c, 3),
                  "r_minus_c_ms": round(med["r"] - med["c"], 3), "r_within_the_spread_of_c": bool(med["r"] - med["c"] <= spread_c),
                  "lanes_table_ms": {str(L): round(med["f%d" % L], 3) for L in variants}}), flush=True)
del legs, reg512

# ---------------------------------------------------------------- the attestation shape
pks = pks_all[:n_keys].contiguous()
lists = [rng.integers(0, n_keys, size=int(rng.integers(400, 501)) if i % 2 == 0 else 1) for i in range(N_ATT)]
msg = torch.from_numpy(rng.integers(0, 256, size=(N_ATT, 32), dtype=np.uint8)).to(dev)
sig = pkg.sign_batch(sk_bytes([sum(sk_of(int(k)) for k in lst) % R_MOD for lst in lists]), msg)["sig96"]
scalars = i64(rng.integers(1, 2**63, size=N_ATT, dtype=np.uint64) * 2 + 1)
idx, off = csr(lists)
order = np.argsort([len(x) for x in lists], kind="stable")
idx_s, off_s = csr([lists[i] for i in order])
order_t = torch.from_numpy(order).to(dev)
msg_s, sig_s = msg[order_t].contiguous(), sig[order_t].contiguous()
append_ms = []
for rep in range(reps + 1):  # the first one warms up
    fresh = pkg.KeyRegistry(n_keys, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh.append(pks)
    torch.cuda.synchronize()
    append_ms.append((time.perf_counter() - t0) * 1e3)
    if rep:
        print(json.dumps({"rep": rep - 1, "leg": "append", "ms": round(append_ms[-1], 3)}), flush=True)
    reg = fresh
lengths = np.array([len(x) for x in lists])
by_len = []  # the parent's index tensors, made once outside the timing: per list length the sets and their key indices
for k in sorted(set(lengths.tolist())):
    sets = np.flatnonzero(lengths == k)
    by_len.append((torch.from_numpy(sets).to(dev), torch.from_numpy(np.stack([lists[i] for i in sets]).astype(np.int64)).to(dev)))


def parent(group):
    agg = torch.empty((N_ATT, 48), dtype=torch.uint8, device=dev)
    for sets, sel in by_len:
        agg[sets] = pkg.aggregate_points(1, pks[sel].contiguous())[0]
    return pkg.verify_groups(agg, msg, sig, group=group, scalars=scalars) if group else pkg.verify_batch(agg, msg, sig)


legs = {"p0": lambda: parent(0), "p64": lambda: parent(GROUP), "r0": lambda: pkg.registry_verify(reg, idx, off, msg, sig),
        "r64": lambda: pkg.registry_verify(reg, idx, off, msg, sig, group=GROUP, scalars=scalars), "s0": lambda: pkg.registry_verify(reg, idx_s, off_s, msg_s, sig_s)}
for L, v in variants.items():
    rv = under(v, lambda: registry_of(pks, n_keys))
    legs["g%d" % L] = (lambda v, rv: lambda: under(v, lambda: pkg.registry_verify(rv, idx, off, msg, sig)))(v, rv)
ms, med, agree = run(legs, lambda out: all(torch.equal(out[k], out["p0"]) for k in out if k not in ("p64", "r64", "s0")) and torch.equal(out["p64"], out["r64"]) and
                     torch.equal(out["s0"], out["p0"][order_t]) and bool((out["p0"] == 1).all().item()) and bool((out["r64"] == 1).all().item()))
print(json.dumps({"shape": "attestation", "n": N_ATT, "n_keys": n_keys, "n_indices": int(lengths.sum()), "list_lengths": len(by_len), "group": GROUP, "lanes": pkg.REGISTRY_LANES,
                  "legs_agree_all_true": agree, "append_median_ms": round(float(np.median(append_ms[1:])), 3), "append_keys_per_s": n_keys / (float(np.median(append_ms[1:])) / 1e3),
                  "median_ms": {k: round(v, 3) for k, v in med.items()}, "r0_over_p0": med["r0"] / med["p0"], "r64_over_p64": med["r64"] / med["p64"],
                  "mixed_minus_sorted_ms": round(med["r0"] - med["s0"], 3), "lanes_table_ms": {str(L): round(med["g%d" % L], 3) for L in variants}}), flush=True)
