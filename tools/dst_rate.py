#!/usr/bin/env python3
"""The caller-chosen domain separation tag (the *_dst entries, k_sha_values_dst) against the plain entries, in ONE process on the same seeded inputs.
Every call is timed with HIP events on the current stream; the legs of a section run interleaved, `--reps` repetitions each after one warm-up call per
leg, every repetition printed as one JSON line, then the medians and each leg's own spread (max - min over its repetitions) — the margin a
comparison with the plain entry is read against:
  a  hash_to_g2, n = 65 536 messages of 32 bytes: dst=None (k_sha_values) against a 43-byte tag through k_sha_values_dst (the library's own tag
     and the POP tag: the same block counts as the plain kernel)
  b  verify_batch, n = 8 192: dst=None against the 43-byte library tag through the new kernel, on signatures made under it
  c  hash_to_g2 at tag lengths 21, 85 and 255 (1, 2 and 5 blocks per b_i), and the SHA stage alone at the same lengths (hash_to_field_batch)
  d  pop_verify against verify_batch at msg_len = 48, n = 8 192, on proofs and on signatures over the same 48 bytes
--n N uses N messages in a and c and min(8 192, N) in b and d (a rehearsal size; a rate wants the full one)."""
import importlib, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("bls-verify-gadget_amd")

import torch

dev = torch.device("cuda:0")
arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
reps, N = arg("--reps", 5), arg("--n", 65536)
N_V = min(8192, N)

rng = np.random.default_rng(0xD57)
msg = torch.from_numpy(rng.integers(0, 256, size=(N, 32), dtype=np.uint8)).to(dev)
sk = torch.from_numpy(np.frombuffer(b"".join((0x3000001 + 104729 * i).to_bytes(32, "little") for i in range(N_V)), dtype=np.uint8).reshape(N_V, 32).copy()).to(dev)
tag = lambda L: bytes((0x21 + 5 * k) & 0x7F | 0x20 for k in range(L))


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
    print(json.dumps(dict(info, section=name, check=bool(check(out)))), flush=True)
    ms = {k: [] for k in legs}
    for rep in range(reps):
        for k, f in legs.items():
            ms[k].append(timed(f)[0])
            print(json.dumps({"section": name, "rep": rep, "leg": k, "ms": round(ms[k][-1], 3)}), flush=True)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
    print(json.dumps(dict(info, section=name, median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()})), flush=True)
    return med, spread


all_one = lambda t: bool((t == 1).all().item())
summary = {"reps": reps, "n": N, "n_verify": N_V}
# a: hash_to_g2, the same block counts
legs = {"plain": lambda: pkg.hash_to_g2_batch(msg), "dst_default_43": lambda: pkg.hash_to_g2_batch(msg, dst=pkg.DST_DEFAULT), "dst_pop_43": lambda: pkg.hash_to_g2_batch(msg, dst=pkg.DST_POP)}
med, spread = section("a", legs, lambda o: torch.equal(o["plain"], o["dst_default_43"]) and not torch.equal(o["plain"], o["dst_pop_43"]), n=N, msg_len=32)
summary["a_hash_to_g2"] = {"plain_ms": med["plain"], "plain_spread_ms": spread["plain"], "dst_43_ms": med["dst_default_43"], "dst_43_minus_plain_ms": med["dst_default_43"] - med["plain"],
                           "inside_plain_spread": abs(med["dst_default_43"] - med["plain"]) <= spread["plain"], "messages_per_s_plain": 1e3 * N / med["plain"],
                           "messages_per_s_dst_43": 1e3 * N / med["dst_default_43"]}
# b: verify_batch
signed = pkg.sign_batch(sk, msg[:N_V].contiguous())
v_pk, v_msg, v_sig = signed["pk48"], msg[:N_V].contiguous(), signed["sig96"]
legs = {"plain": lambda: pkg.verify_batch(v_pk, v_msg, v_sig), "dst_default_43": lambda: pkg.verify_batch(v_pk, v_msg, v_sig, dst=pkg.DST_DEFAULT)}
med, spread = section("b", legs, lambda o: all_one(o["plain"]) and all_one(o["dst_default_43"]), n=N_V, msg_len=32)
summary["b_verify_batch"] = {"plain_ms": med["plain"], "plain_spread_ms": spread["plain"], "dst_43_ms": med["dst_default_43"], "dst_43_minus_plain_ms": med["dst_default_43"] - med["plain"],
                             "inside_plain_spread": abs(med["dst_default_43"] - med["plain"]) <= spread["plain"]}
# c: the tag length
legs = {"plain": lambda: pkg.hash_to_g2_batch(msg)}
for L in (21, 85, 255):
    legs["g2_L%d" % L] = (lambda t: lambda: pkg.hash_to_g2_batch(msg, dst=t))(tag(L))
for L in (21, 43, 85, 255):
    legs["field_L%d" % L] = (lambda t: lambda: pkg.hash_to_field_batch(msg, dst=t))(tag(L))
med, spread = section("c", legs, lambda o: True, n=N, msg_len=32)
summary["c_tag_length"] = {k: {"ms": round(v, 3), "spread_ms": round(spread[k], 3)} for k, v in med.items()}
summary["c_blocks"] = {"L21": {"b_i": 1, "b_0": 3}, "L43": {"b_i": 2, "b_0": 3}, "L85": {"b_i": 2, "b_0": 4}, "L255": {"b_i": 5, "b_0": 6}}
# d: PopVerify
proved = pkg.pop_prove(sk)
over_key = pkg.sign_batch(sk, proved["pk48"])
p_pk, p_proof, p_sig = proved["pk48"], proved["proof96"], over_key["sig96"]
legs = {"verify_batch_48": lambda: pkg.verify_batch(p_pk, p_pk, p_sig), "pop_verify": lambda: pkg.pop_verify(p_pk, p_proof), "pop_prove": lambda: pkg.pop_prove(sk)["status"]}
med, spread = section("d", legs, lambda o: all_one(o["verify_batch_48"]) and all_one(o["pop_verify"]), n=N_V, msg_len=48)
summary["d_pop"] = {"verify_batch_48_ms": med["verify_batch_48"], "verify_batch_48_spread_ms": spread["verify_batch_48"], "pop_verify_ms": med["pop_verify"],
                    "pop_verify_minus_verify_ms": med["pop_verify"] - med["verify_batch_48"], "inside_plain_spread": abs(med["pop_verify"] - med["verify_batch_48"]) <= spread["verify_batch_48"],
                    "pop_prove_ms": med["pop_prove"]}
print(json.dumps({"summary": summary}), flush=True)
