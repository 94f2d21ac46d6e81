#!/usr/bin/env python3
"""blsw_verify_pairs_batch (AggregateVerify as values) against what stands next to it, in ONE process on the same seeded inputs, 32-byte messages. Every
call is timed with HIP events on the current stream; the legs of a section run interleaved, `--reps` repetitions each after one warm-up call per leg,
every repetition printed as one JSON line, then the medians:
  a  n = 8 192, K = 1: verify_pairs against verify_batch on the same triples — the same work, so the ratio is what the one-pair-per-step fold costs
     against team_miller_values
  b  K in {8, 32, 128} with n K = 65 536 pairs: verify_pairs against (1) verify_batch on the n K single triples and (2) blsw_verify_multi_batch with
     d_witness == NULL on pre-decoded limbs, the only other route to this verdict
  c  verify_pairs at K = 128 from libraries built with -DBLSW_VPAIRS_CHUNK=c for c in {2, 4, 8, 16, 31} (build(defines=...); kept under _ab/)
--build-only makes the libraries of section c and exits (no device needed); --no-chunks skips c; --pairs P uses n K = P instead of 65 536 (a
rehearsal size; a rate wants the full one)."""
import ctypes, importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")
build = importlib.import_module("bls-verify-gadget_amd.build")
CHUNKS = (2, 4, 8, 16, 31)
KS = (8, 32, 128)


def chunk_library(c):
    path = os.path.join(ROOT, "_ab", "libblsw_vpchunk%d.so" % c)
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        build.build(out=path, defines=["-DBLSW_VPAIRS_CHUNK=%d" % c])
    return path


if "--build-only" in sys.argv:
    for c in CHUNKS:
        print(chunk_library(c), flush=True)
    sys.exit(0)

import torch

dev = torch.device("cuda:0")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
reps, PAIRS = arg("--reps", 5), arg("--pairs", 65536)
N_A = min(8192, PAIRS)

rng = np.random.default_rng(0xA66)
sk = np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(PAIRS)), dtype=np.uint8).reshape(PAIRS, 32).copy()
msg = torch.from_numpy(rng.integers(0, 256, size=(PAIRS, 32), dtype=np.uint8)).to(dev)
signed = pkg.sign_batch(torch.from_numpy(sk).to(dev), msg)
assert int(signed["status"].abs().sum().item()) == 0
pk48, sig96, pk_xy = signed["pk48"], signed["sig96"], signed["pk_xy"]


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
    print(json.dumps(dict(info, section=name, all_true_and_legs_agree=bool(check(out)))), flush=True)
    ms = {k: [] for k in legs}
    for rep in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
            print(json.dumps({"section": name, "rep": rep, "leg": k, "ms": round(ms[k][-1], 3)}), flush=True)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(info, section=name, median_ms={k: round(v, 3) for k, v in med.items()})), flush=True)
    return med


def multi_leg(n, K, sig_agg):
    """blsw_verify_multi_batch with d_witness == NULL on limbs decoded outside the timing"""
    L = pkg.lib()
    _, sig_xy, st = pkg.decode_batch(pk48[:n].contiguous(), sig_agg)
    assert not st.cpu().numpy().any()
    keys, msgs = pk_xy.reshape(n, K, 12).contiguous(), msg.reshape(n, K, 32)
    lay = pkg.layout_multi(32, K)
    wb = ctypes.c_uint64(0)
    assert L.blsw_verify_multi_workspace_bytes(n, 32, K, ctypes.byref(wb)) == 0
    pkg.check_capacity(dev, "verify_multi (n = %d, %d pairs)" % (n, K), wb.value)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    res = torch.empty(n, dtype=torch.int32, device=dev)

    def call():
        rc = L.blsw_verify_multi_batch(keys.data_ptr(), msgs.data_ptr(), 32, K, sig_xy.data_ptr(), n, None, lay["n_witness"], res.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        return res
    return call


all_one = lambda t: bool((t == 1).all().item())
summary = {"reps": reps, "pairs": PAIRS, "chunk": pkg.VERIFY_PAIRS_CHUNK}
# a: K = 1
a_pk, a_msg, a_sig = pk48[:N_A].contiguous(), msg[:N_A].contiguous(), sig96[:N_A].contiguous()
med = section("a", {"verify_batch": lambda: pkg.verify_batch(a_pk, a_msg, a_sig), "verify_pairs": lambda: pkg.verify_pairs(a_pk.reshape(N_A, 1, 48), a_msg.reshape(N_A, 1, 32), a_sig)},
              lambda o: all_one(o["verify_batch"]) and all_one(o["verify_pairs"]), n=N_A, K=1)
summary["a_pairs_over_verify_batch"] = med["verify_pairs"] / med["verify_batch"]
# b: K pairs per instance
for K in KS:
    n = PAIRS // K
    sig_agg, st = pkg.aggregate_signatures(sig96.reshape(n, K, 96))
    assert not st.cpu().numpy().any()
    pks, msgs = pk48.reshape(n, K, 48), msg.reshape(n, K, 32)
    legs = {"verify_batch_nK": lambda: pkg.verify_batch(pk48, msg, sig96), "verify_multi_null": multi_leg(n, K, sig_agg), "verify_pairs": lambda: pkg.verify_pairs(pks, msgs, sig_agg)}
    med = section("b", legs, lambda o: all(all_one(v) for v in o.values()), n=n, K=K)
    summary["b_K%d" % K] = {"pairs_ms": med["verify_pairs"], "us_per_pair": 1e3 * med["verify_pairs"] / PAIRS, "over_verify_batch_nK": med["verify_pairs"] / med["verify_batch_nK"],
                            "over_verify_multi_null": med["verify_pairs"] / med["verify_multi_null"]}
# c: the chunk table at K = 128
if "--no-chunks" not in sys.argv:
    base = pkg.lib()
    K = 128
    n = PAIRS // K
    sig_agg, _ = pkg.aggregate_signatures(sig96.reshape(n, K, 96))
    pks, msgs = pk48.reshape(n, K, 48), msg.reshape(n, K, 32)

    def with_library(v):
        def call():
            pkg._lib = v  # the wrapper's own path, another library's two entry points
            try:
                return pkg.verify_pairs(pks, msgs, sig_agg)
            finally:
                pkg._lib = base
        return call

    legs = {}
    for c in CHUNKS:
        v = ctypes.CDLL(chunk_library(c))
        for name in ("blsw_verify_pairs_workspace_bytes", "blsw_verify_pairs_batch"):
            getattr(v, name).argtypes = getattr(base, name).argtypes
        legs["chunk%d" % c] = with_library(v)
    med = section("c", legs, lambda o: all(all_one(v) for v in o.values()), n=n, K=K)
    summary["c_chunk_table_ms"] = {k: round(v, 3) for k, v in med.items()}
print(json.dumps({"summary": summary}), flush=True)
