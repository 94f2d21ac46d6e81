#!/usr/bin/env python3
"""Rate of the aggregate_verify engine at committee size (default 512 keys, a 32-byte message), full witness vectors written, for the circuit's
allocation masks (options.agg_inputs: 0 = every argument Witness, 3 = keys and bitmap Input, 15 = every argument Input). One JSON line:
    per mask: instances_per_s, ms_per_step (median / min / max of the timed repetitions), bytes_per_step, n_witness, n_instance_vars, workspace_bytes and
    the median stage times of its launch groups (BLSW_TRACE_GROUP); fill_rate_GBps: blsw_fill_rate of the same box, the HBM yardstick beside them.
All legs run in one process, interleaved repetition by repetition, each timed with HIP events around `steps` submitted steps and the flush. A library
without options.agg_inputs (an older commit) runs mask 0 only: that leg is the yardstick between commits. Steps are sized for the all-Witness shape
(83 MB per instance at 512 keys). Every leg runs under a time limit; when one expires or fails the process ends there and nothing follows.

    python tools/agg_inputs_rate.py [--n 128] [--keys 512] [--steps 4] [--max-steps 2] [--buffers 2] [--reps 5] [--masks 0,3,15] [--limit 240]"""
import argparse
import importlib
import json
import os
import re
import statistics
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StepLimit:
    """ends the process (exit status 124) when the enclosed GPU step takes longer than `seconds`: a hung device call cannot be interrupted from Python"""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expire)
        self.t.daemon = True
        self.what = what

    def _expire(self):
        sys.stderr.write("agg_inputs_rate: time limit in %s\n" % self.what)
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def trace_of(close):
    """runs close() (blsw_engine_destroy prints the launch groups' stage times to stderr) and returns the median of every stage over the groups"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    stages = {}
    for ln in text.splitlines():
        if not ln.startswith("[blsw group]"):
            sys.stderr.write(ln + "\n")
            continue
        for name, ms in re.findall(r"([a-z_()+H ]+?) (\d+\.\d+)(?= |$)", ln.split(":", 1)[1].replace("| total", "total")):
            stages.setdefault(name.strip(), []).append(float(ms))
    return {k: round(statistics.median(v), 2) for k, v in stages.items()}, (len(next(iter(stages.values()))) if stages else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="instances per step")
    ap.add_argument("--keys", type=int, default=512)
    ap.add_argument("--steps", type=int, default=4, help="steps per timed repetition")
    ap.add_argument("--max-steps", type=int, default=2)
    ap.add_argument("--buffers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--masks", default="0,3,15")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per GPU step (set-up, a repetition of a leg, the fill)")
    a = ap.parse_args()
    os.environ["BLSW_TRACE_GROUP"] = "1"  # read by the library when an engine is destroyed
    import torch

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    has_option = any(name == "agg_inputs" for name, _ in pkg.blsw_engine_options_t._fields_)
    masks = [int(m) for m in a.masks.split(",")] if has_option else [0]
    dev = torch.device("cuda:0")
    n, K = a.n, a.keys
    with StepLimit(a.limit, "input generation"):
        pk, msg, sig, _ = workload.make_batch(pkg, n * K, device=dev, tamper_every=0)
        pks = pk.reshape(n, K, 12).contiguous()
        msg, sig = msg[:n].contiguous(), sig[:n].contiguous()
        bitmap = (torch.arange(n * K, device=dev).reshape(n, K) % 3 != 0).to(torch.uint8).contiguous()  # two thirds of the committee signed
        torch.cuda.synchronize()
    legs = {}
    for m in masks:
        with StepLimit(a.limit, "engine creation (mask %d)" % m):
            opt = {"n_keys": K}
            if m:
                opt["agg_inputs"] = m
            eng = pkg.WitnessEngine(n, 32, max_steps=a.max_steps, n_buffers=a.buffers, device=dev, **opt)
            outs = [eng.new_witness_tensor() for _ in range(min(a.steps, a.max_steps * a.buffers))]
            inst = eng.new_instance_tensor() if m else None
            res = torch.empty(n, dtype=torch.int32, device=dev)
            cnt = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
        legs[m] = dict(eng=eng, outs=outs, inst=inst, res=res, cnt=cnt, ms=[])

    def repetition(m):
        leg = legs[m]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for s in range(a.steps):
            kw = {"instance": leg["inst"]} if leg["inst"] is not None else {}
            leg["eng"].submit_aggregate(pks, bitmap, sig, msg, witness=leg["outs"][s % len(leg["outs"])], result=leg["res"], count=leg["cnt"], **kw)
        leg["eng"].flush()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for rep in range(a.reps + 1):  # the first repetition warms up: scratch growth, first touch of the output tensors
        for m in masks:
            with StepLimit(a.limit, "repetition %d of mask %d" % (rep, m)):
                ms = repetition(m)
            if rep:
                legs[m]["ms"].append(ms)
    out = {"metric": "aggregate_engine_rate", "n": n, "n_keys": K, "msg_len": 32, "steps_per_repetition": a.steps, "max_steps": a.max_steps, "n_buffers": a.buffers,
           "repetitions": a.reps, "abi": pkg.lib().blsw_version(), "masks": {}}
    for m in masks:
        leg = legs[m]
        eng = leg["eng"]
        count = int(leg["cnt"][0].item())
        with StepLimit(a.limit, "engine destruction (mask %d)" % m):
            stages, groups = trace_of(eng.close)
        med = statistics.median(leg["ms"])
        step_bytes = n * (eng.n_witness + (eng.n_instance_vars if m else 0)) * 48
        out["masks"][str(m)] = {"n_witness": eng.n_witness, "n_instance_vars": eng.n_instance_vars, "workspace_bytes": eng.workspace.numel(),
                                "bytes_per_step": step_bytes, "ms_per_step": {"median": round(med, 3), "min": round(min(leg["ms"]), 3), "max": round(max(leg["ms"]), 3)},
                                "instances_per_s": round(n / (med / 1e3), 1), "GBps_written": round(step_bytes / (med / 1e3) / 1e9, 1), "count_of_instance_0": count,
                                "group_stage_ms_median": stages, "groups_traced": groups}
        leg["outs"], leg["inst"] = None, None
        del eng
        legs[m]["eng"] = None
        torch.cuda.empty_cache()
    with StepLimit(a.limit, "fill rate"):
        buf = torch.empty(8 << 30, dtype=torch.uint8, device=dev)
        out["fill_rate_GBps"] = round(pkg.fill_rate(buf, reps=3) / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
