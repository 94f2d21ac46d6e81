#!/usr/bin/env python3
"""blsw_combine_points_batch / blsw_recover_points_batch against what stands next to them, in ONE process on the same seeded inputs. Every call is
timed with HIP events on the current stream; the legs of a section run interleaved, `--reps` repetitions each after one warm-up call per leg, every
repetition printed as one JSON line, then the medians and the range of the repetitions. One section per list length k in {4, 16, 128} at
n k = 65 536 terms (n = 16 384 / 4 096 / 512):
  a  combine_points in G2
  b  sign_batch on 65 536 messages, the yardstick: the same four-digit ladder per lane plus the hash and the fixed-base key lanes
  c  combine_points in G1
  d  c from libraries built with -DBLSW_COMBINE_PLAIN_G1 (the plain 255-step double-and-add instead of the endomorphism ladder) and with
     -DBLSW_COMBINE_G1_WAVES=1 (the G1 scale kernel at one wave per SIMD, unspilled, instead of two); build(defines=...), kept under _ab/
  e  recover_points in G2 and G1 on the same terms: what the Lagrange stage adds to a and c
  f  aggregate_points in G2 and G1 on the same points: what the scaling adds over the plain sum
--build-only makes the libraries of d and exits (no device needed); --terms T uses n k = T instead of 65 536 (a rehearsal size).
--yardstick PATH: two hash_to_g2_batch and two verify_batch calls (8 192 messages / triples) on the library at PATH, timed the same way, and
nothing else — run alternately on this commit's library and its parent's, in separate processes, to see whether the untouched entries moved."""
import ctypes, importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")
build = importlib.import_module("bls-verify-gadget_amd.build")
VARIANTS = {"plain": "-DBLSW_COMBINE_PLAIN_G1", "g1w1": "-DBLSW_COMBINE_G1_WAVES=1"}
KS = (4, 16, 128)
COMBINE_ENTRIES = ("blsw_combine_points_workspace_bytes", "blsw_combine_points_batch")


def variant_library(name):
    path = os.path.join(ROOT, "_ab", "libblsw_combine_%s.so" % name)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        build.build(out=path, defines=[VARIANTS[name]])
    return path


if "--build-only" in sys.argv:
    for v in VARIANTS:
        print(variant_library(v), flush=True)
    sys.exit(0)

import torch

dev = torch.device("cuda:0")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
reps, TERMS = arg("--reps", 5), arg("--terms", 65536)


def timed(f):
    """(milliseconds between two events around the call, its result)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0.record()
    out = f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def section(name, legs, check, **info):
    out = {k: f() for k, f in legs.items()}  # warm-up of every leg: code objects, workspaces in the caching allocator
    torch.cuda.synchronize(dev)
    print(json.dumps(dict(info, section=name, results_agree=bool(check(out)))), flush=True)
    ms = {k: [] for k in legs}
    for rep in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
            print(json.dumps(dict(info, section=name, rep=rep, leg=k, ms=round(ms[k][-1], 3))), flush=True)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(info, section=name, median_ms={k: round(v, 3) for k, v in med.items()}, range_ms={k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()})), flush=True)
    return med


rng = np.random.default_rng(0xC0B1)

if "--yardstick" in sys.argv:
    path = sys.argv[sys.argv.index("--yardstick") + 1]
    base = pkg.lib()
    v = ctypes.CDLL(path)
    for name in ("blsw_hash_to_g2_workspace_bytes", "blsw_hash_to_g2_batch", "blsw_verify_workspace_bytes", "blsw_verify_batch"):
        getattr(v, name).argtypes = getattr(base, name).argtypes
    n = 8192
    sk = np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()
    msg = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).to(dev)
    signed = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg)
    pkg._lib = v  # the wrappers' own paths, the other library's entry points
    legs = {"hash_to_g2_batch": lambda: pkg.hash_to_g2_batch(msg), "verify_batch": lambda: pkg.verify_batch(signed["pk48"], msg, signed["sig96"])}
    for k, f in legs.items():
        f()
    for rep in range(2):
        for k, f in legs.items():
            ms, out = timed(f)
            ok = bool((out == 1).all().item()) if k == "verify_batch" else True
            print(json.dumps({"yardstick": os.path.basename(path), "leg": k, "rep": rep, "n": n, "ms": round(ms, 3), "ok": ok}), flush=True)
    sys.exit(0)

sk = np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(TERMS)), dtype=np.uint8).reshape(TERMS, 32).copy()
sk_t = torch.from_numpy(sk).to(dev)
msg = torch.from_numpy(rng.integers(0, 256, size=(TERMS, 32), dtype=np.uint8)).to(dev)
signed = pkg.sign_batch(sk_t, msg)
assert int(signed["status"].abs().sum().item()) == 0
pk48, sig96 = signed["pk48"], signed["sig96"]


def fr_rows(count):
    """seeded elements of Fr as 32 little-endian bytes: the top byte below r's (0x73), the lowest bit set so that none is zero"""
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] %= 0x73
    a[:, 0] |= 1
    return torch.from_numpy(a).to(dev)


scalars, ids = fr_rows(TERMS), fr_rows(TERMS)
base = pkg.lib()


def with_library(v, f):
    def call():
        pkg._lib = v
        try:
            return f()
        finally:
            pkg._lib = base
    return call


variants = {}
for name in VARIANTS:
    v = ctypes.CDLL(variant_library(name))
    for e in COMBINE_ENTRIES:
        getattr(v, e).argtypes = getattr(base, e).argtypes
    variants[name] = v

summary = {"reps": reps, "terms": TERMS}
for k in KS:
    n = TERMS // k
    p2, p1, s, x = sig96.reshape(n, k, 96), pk48.reshape(n, k, 48), scalars.reshape(n, k, 32), ids.reshape(n, k, 32)
    legs = {
        "a_combine_g2": lambda: pkg.combine_points(2, p2, s),
        "b_sign_batch": lambda: pkg.sign_batch(sk_t, msg),
        "c_combine_g1": lambda: pkg.combine_points(1, p1, s),
        "e_recover_g2": lambda: pkg.recover_points(2, x, p2),
        "e_recover_g1": lambda: pkg.recover_points(1, x, p1),
        "f_aggregate_g2": lambda: pkg.aggregate_points(2, p2),
        "f_aggregate_g1": lambda: pkg.aggregate_points(1, p1),
    }
    for name, v in variants.items():
        legs["d_combine_g1_" + name] = with_library(v, lambda: pkg.combine_points(1, p1, s))

    def check(o):
        ok = all(not o[leg][1].any().item() for leg in legs if leg != "b_sign_batch")
        return ok and all(torch.equal(o["d_combine_g1_" + name][0], o["c_combine_g1"][0]) for name in variants)

    med = section("k%d" % k, legs, check, n=n, k=k)
    summary["k%d" % k] = {"us_per_term": {leg: round(1e3 * v / TERMS, 4) for leg, v in med.items()}, "a_over_b": med["a_combine_g2"] / med["b_sign_batch"],
                          "plain_over_glv_g1": med["d_combine_g1_plain"] / med["c_combine_g1"], "one_wave_over_two_g1": med["d_combine_g1_g1w1"] / med["c_combine_g1"],
                          "recover_over_combine": {"g2": med["e_recover_g2"] / med["a_combine_g2"], "g1": med["e_recover_g1"] / med["c_combine_g1"]},
                          "combine_over_aggregate": {"g2": med["a_combine_g2"] / med["f_aggregate_g2"], "g1": med["c_combine_g1"] / med["f_aggregate_g1"]}}
print(json.dumps({"summary": summary}), flush=True)
