#!/usr/bin/env python3
"""blsw_msm_points_batch against the path that stood before it, in ONE process on the same seeded inputs, G1 and G2, ONE list of k terms. Every call
is timed with HIP events on the current stream; the legs of a section run interleaved, `--reps` repetitions each after one warm-up call per leg, every
repetition printed as one JSON line, then the medians and the range of the repetitions (as tools/combine_rate.py).
  msm       msm_points(group, [1, k], window_bits 0)
  registry  (G1) KeyRegistry.msm over a registry that holds the same keys, one list of the indices 0 .. k - 1 with the same scalars
  existing  k <= 65 535: combine_points on the one list. Above: combine_points on ceil(k / 65 535) lists of at most 65 535 terms (counts), then
            aggregate_points over the partial sums — what a caller had to write before
Sections: k = 2^e for e in --exps (default 4 .. 20: the low end finds the k below which the per-term ladder wins), then at k = 65 536 the window
widths around the default and the all-equal-scalars list (one bucket per window takes every term). The results of the legs are compared.
--max-existing E: skip the existing path above 2^E (its one-lane sums take seconds there). --widths a,b,..: the widths of the sweep."""
import importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")
import torch

dev = torch.device("cuda:0")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
reps, max_existing = arg("--reps", 5), arg("--max-existing", 20)
exps = [int(v) for v in sys.argv[sys.argv.index("--exps") + 1].split(",")] if "--exps" in sys.argv else list(range(4, 21))
TERMS = 1 << max(exps + [16])
CHUNK = 65535
rng = np.random.default_rng(0x35A)


def timed(f):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0.record()
    out = f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1), out


def section(name, legs, **info):
    out = {k: f() for k, f in legs.items()}  # warm-up of every leg
    torch.cuda.synchronize(dev)
    first = next(iter(out.values()))
    agree = all(torch.equal(o[0], first[0]) and not o[1].any().item() for o in out.values())
    print(json.dumps(dict(info, section=name, results_agree=bool(agree))), flush=True)
    ms = {k: [] for k in legs}
    for rep in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
            print(json.dumps(dict(info, section=name, rep=rep, leg=k, ms=round(ms[k][-1], 3))), flush=True)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    print(json.dumps(dict(info, section=name, median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()})), flush=True)
    return med, spread


def fr_rows(count):
    a = rng.integers(0, 256, size=(count, 32), dtype=np.uint8)
    a[:, 31] %= 0x73
    a[:, 0] |= 1
    return torch.from_numpy(a).to(dev)


# the points: keys and signatures of seeded secret keys, 65 536 per sign call
sk = np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(TERMS)), dtype=np.uint8).reshape(TERMS, 32).copy()
msg = torch.from_numpy(rng.integers(0, 256, size=(65536, 32), dtype=np.uint8)).to(dev)
parts = [pkg.sign_batch(torch.from_numpy(sk[lo:lo + 65536]).to(dev), msg) for lo in range(0, TERMS, 65536)]
assert all(int(p["status"].abs().sum().item()) == 0 for p in parts)
POINTS = {1: torch.cat([p["pk48"] for p in parts]), 2: torch.cat([p["sig96"] for p in parts])}
SCALARS = fr_rows(TERMS)
del parts


def existing(group, k, scalars):
    p, s = POINTS[group][:k], scalars[:k]
    if k <= CHUNK:
        return pkg.combine_points(group, p.reshape(1, k, -1), s.reshape(1, k, 32))
    n = -(-k // CHUNK)
    width = p.shape[1]
    pp = torch.zeros((n * CHUNK, width), dtype=torch.uint8, device=dev)
    ss = torch.zeros((n * CHUNK, 32), dtype=torch.uint8, device=dev)
    pp[:k], ss[:k] = p, s
    counts = torch.tensor([min(CHUNK, k - i * CHUNK) for i in range(n)], dtype=torch.int32, device=dev)
    part, st = pkg.combine_points(group, pp.reshape(n, CHUNK, width), ss.reshape(n, CHUNK, 32), counts)
    out, st2 = pkg.aggregate_points(group, part.reshape(1, n, width).contiguous())
    return out, torch.cat([st, st2])


REGISTRY = pkg.KeyRegistry(TERMS, device=dev)
REGISTRY.append(POINTS[1])
INDICES = torch.arange(TERMS, dtype=torch.int32, device=dev)


def registry_msm(k, scalars, c=0):
    return REGISTRY.msm(INDICES[:k], torch.tensor([0, k], dtype=torch.int64, device=dev), scalars[:k], c)


def msm(group, k, scalars, c=0):
    return pkg.msm_points(group, POINTS[group][:k].reshape(1, k, -1), scalars[:k].reshape(1, k, 32), None, c)


summary = {"reps": reps}
for e in exps:
    k = 1 << e
    legs = {}
    for g in (1, 2):
        legs["msm_g%d" % g] = lambda g=g: msm(g, k, SCALARS)
    med, spread = {}, {}
    for g in (1, 2):  # a section per group: the legs' results are compared within it
        lg = {"msm_g%d" % g: legs["msm_g%d" % g]}
        if g == 1:
            lg["registry_g1"] = lambda: registry_msm(k, SCALARS)
        if e <= max_existing:
            lg["existing_g%d" % g] = lambda g=g: existing(g, k, SCALARS)
        m, s = section("k2^%d_g%d" % (e, g), lg, k=k, group=g)
        med.update(m)
        spread.update(s)
    summary["k2^%d" % e] = {"median_ms": {a: round(b, 3) for a, b in med.items()}, "spread_ms": {a: round(b, 3) for a, b in spread.items()}}
k = 65536
for g in (1, 2):
    widths = [int(v) for v in sys.argv[sys.argv.index("--widths") + 1].split(",")] if "--widths" in sys.argv else list(range(10, 17))  # the default is 13
    m, s = section("windows_k65536_g%d" % g, {"c%d" % c: (lambda c=c: msm(g, k, SCALARS, c)) for c in widths}, k=k, group=g)
    summary["windows_g%d" % g] = {a: round(b, 3) for a, b in m.items()}
EQUAL = SCALARS[:1].repeat(k, 1).contiguous()
for g in (1, 2):
    m, s = section("equal_scalars_k65536_g%d" % g, dict({"msm": lambda: msm(g, k, EQUAL)}, **({"registry": lambda: registry_msm(k, EQUAL)} if g == 1 else {})), k=k, group=g)
    summary["equal_scalars_g%d_ms" % g] = round(m["msm"], 3)
print(json.dumps({"summary": summary}), flush=True)
