#!/usr/bin/env python3
"""Rate of the aggregate_verify engine at committee size (default 512 keys, a 32-byte message, every argument Witness), full witness vectors written,
with the committee brought per instance and with the committee as ONE shared key set (options.shared_keys). One JSON line:
    legs "replicated" (blsw_engine_submit_aggregate, keys [n][K][12]: the unchanged path) and "shared" (blsw_engine_submit_aggregate_keyset): ms_per_step
    (median / min / max of the timed repetitions), instances_per_s, workspace_bytes and the median stage times of the launch groups (BLSW_TRACE_GROUP);
    keyset_create_ms (median / min / max); broadcast_GBps: bytes written / time of k_keys_broadcast alone for both grid orders
    (blsw_keyset_broadcast_rate: 0 = instance fastest, what the engine launches; 1 = chunk fastest); fill_rate_GBps: blsw_fill_rate of the same box.
Both legs run in one process, interleaved repetition by repetition, each timed with HIP events around `steps` submitted steps and the flush; the outputs
of the two legs are compared once (digests). The same "replicated" leg on an older commit is tools/agg_inputs_rate.py --masks 0 there. Every GPU step
runs under a time limit; when one expires or fails the process ends there and nothing follows.

    python tools/agg_shared_rate.py [--n 128] [--keys 512] [--steps 4] [--max-steps 2] [--buffers 2] [--reps 5] [--limit 240]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.agg_inputs_rate import StepLimit, trace_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="instances per step")
    ap.add_argument("--keys", type=int, default=512)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed repetition")
    ap.add_argument("--max-steps", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per GPU step (set-up, a repetition of a leg, a rate)")
    a = ap.parse_args()
    os.environ["BLSW_TRACE_GROUP"] = "1"  # read by the library when an engine is destroyed
    import torch

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    dev = torch.device("cuda:0")
    n, K = a.n, a.keys
    with StepLimit(a.limit, "input generation"):
        pk, msg, sig, _ = workload.make_batch(pkg, max(n, K), device=dev, tamper_every=0)
        committee = pk[:K].contiguous()  # one committee for every instance
        pks = committee.unsqueeze(0).expand(n, K, 12).contiguous()
        msg, sig = msg[:n].contiguous(), sig[:n].contiguous()
        bitmap = (torch.arange(n * K, device=dev).reshape(n, K) % 3 != 0).to(torch.uint8).contiguous()  # two thirds of the committee signed
        torch.cuda.synchronize()
    create_ms = []
    keyset = None
    with StepLimit(a.limit, "key set creation"):
        for _ in range(a.reps + 1):  # the first one warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keyset = pkg.KeySet(committee)
            e1.record()
            torch.cuda.synchronize()
            create_ms.append(e0.elapsed_time(e1))
    legs = {}
    for name in ("replicated", "shared"):
        with StepLimit(a.limit, "engine creation (%s)" % name):
            eng = pkg.WitnessEngine(n, 32, max_steps=a.max_steps, n_buffers=a.buffers, device=dev, n_keys=K, **({"shared_keys": 1} if name == "shared" else {}))
            outs = [eng.new_witness_tensor() for _ in range(min(a.steps, a.max_steps * a.buffers))]
            res = torch.empty(n, dtype=torch.int32, device=dev)
            cnt = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
        legs[name] = dict(eng=eng, outs=outs, res=res, cnt=cnt, ms=[])

    def repetition(name):
        leg = legs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(a.steps):
            out = leg["outs"][s % len(leg["outs"])]
            if name == "shared":
                leg["eng"].submit_aggregate_keyset(keyset, bitmap, sig, msg, witness=out, result=leg["res"], count=leg["cnt"])
            else:
                leg["eng"].submit_aggregate(pks, bitmap, sig, msg, witness=out, result=leg["res"], count=leg["cnt"])
        leg["eng"].flush()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for rep in range(a.reps + 1):  # the first repetition warms up: scratch growth, first touch of the output tensors
        for name in legs:
            with StepLimit(a.limit, "repetition %d of %s" % (rep, name)):
                ms = repetition(name)
            if rep:
                legs[name]["ms"].append(ms)
    with StepLimit(a.limit, "comparison"):
        d0, d1 = pkg.witness_digest(legs["replicated"]["outs"][0]), pkg.witness_digest(legs["shared"]["outs"][0])
        same = bool(torch.equal(d0, d1) and torch.equal(legs["replicated"]["res"], legs["shared"]["res"]) and torch.equal(legs["replicated"]["cnt"], legs["shared"]["cnt"]))
    out = {"metric": "aggregate_shared_keys_rate", "n": n, "n_keys": K, "msg_len": 32, "steps_per_repetition": a.steps, "max_steps": a.max_steps, "n_buffers": a.buffers,
           "repetitions": a.reps, "abi": pkg.lib().blsw_version(), "outputs_equal": same,
           "keyset_create_ms": {"median": round(statistics.median(create_ms[1:]), 3), "min": round(min(create_ms[1:]), 3), "max": round(max(create_ms[1:]), 3)},
           "keyset_bytes": pkg.keyset_bytes(K), "legs": {}}
    n_witness = legs["shared"]["eng"].n_witness
    with StepLimit(a.limit, "broadcast rate"):
        t = legs["shared"]["outs"][0]
        out["broadcast_bytes_per_step"] = n * K * pkg.SEG_PK_ALLOC * 48
        out["broadcast_GBps"] = {"instance_fastest": round(keyset.broadcast_rate(t, order=0, reps=5) / 1e9, 1), "chunk_fastest": round(keyset.broadcast_rate(t, order=1, reps=5) / 1e9, 1)}
    for name, leg in legs.items():
        eng = leg["eng"]
        with StepLimit(a.limit, "engine destruction (%s)" % name):
            stages, groups = trace_of(eng.close)
        med = statistics.median(leg["ms"])
        out["legs"][name] = {"workspace_bytes": eng.workspace.numel(), "bytes_per_step": n * n_witness * 48,
                             "ms_per_step": {"median": round(med, 3), "min": round(min(leg["ms"]), 3), "max": round(max(leg["ms"]), 3)},
                             "instances_per_s": round(n / (med / 1e3), 1), "GBps_written": round(n * n_witness * 48 / (med / 1e3) / 1e9, 1),
                             "count_of_instance_0": int(leg["cnt"][0].item()), "group_stage_ms_median": stages, "groups_traced": groups}
        leg["outs"] = None
        leg["eng"] = None
        del eng
        torch.cuda.empty_cache()
    keyset.close()
    with StepLimit(a.limit, "fill rate"):
        buf = torch.empty(8 << 30, dtype=torch.uint8, device=dev)
        out["fill_rate_GBps"] = round(pkg.fill_rate(buf, reps=3) / 1e9, 1)
    print(json.dumps(out))
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
