#!/usr/bin/env python3
"""Rate of the N+1-pair engine at the baseline's configs[3] shape (default 128 pairs, 32-byte messages), full witness vectors written, for the circuit's
allocation masks (blsw_engine_create_multi_inputs: 0 = every argument Witness, 1 = keys Input, 4 = messages Input, 8 = signature Input, 13 = all three). One JSON line:
    per mask: instances_per_s, ms_per_step (median / min / max of the timed repetitions), bytes_per_step, n_witness, n_instance_vars, workspace_bytes and
    rate_vs_mask_0 (against mask 0 of the same build and run); fill_rate_GBps: blsw_fill_rate of the same box, the HBM yardstick beside them.
A vector is 4.19 GB at 128 pairs, so the legs run one after the other in one process and share one ring of two output tensors, sized for the longest
vector (Input messages). The first engine of a process runs about 9 % faster than the ones created after it, whatever its mask (measured with the
legs in both orders), so an untimed leg of the first mask runs before the timed ones and every timed leg is a later one. Each repetition is timed
with HIP events around `steps` submitted steps and the flush. A library without blsw_engine_create_multi_inputs
(an older commit) runs mask 0 only: that leg is the yardstick between commits. The inputs are valid points and arbitrary messages, not valid signatures
of the pairs: the circuit has one shape, its chains do the same work on every input. Every leg runs under a time limit; when one expires or fails the
process ends there and nothing follows.

    python tools/multi_inputs_rate.py [--n 16] [--pairs 128] [--steps 8] [--max-steps 4] [--buffers 3] [--reps 3] [--masks 0,1,4,8,13] [--limit 240]"""
import argparse
import importlib
import json
import os
import statistics
import sys
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
        sys.stderr.write("multi_inputs_rate: time limit in %s\n" % self.what)
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16, help="instances per step")
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=8, help="steps per timed repetition")
    ap.add_argument("--max-steps", type=int, default=4)
    ap.add_argument("--buffers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--masks", default="0,1,4,8,13")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per GPU step (set-up, a repetition of a leg, the fill)")
    a = ap.parse_args()
    import torch

    pkg = importlib.import_module("bls-verify-gadget_amd")
    workload = importlib.import_module("bls-verify-gadget_amd.workload")
    has_option = "blsw_engine_create_multi_inputs" in pkg.EXPORTED_SYMBOLS
    masks = [int(m) for m in a.masks.split(",")] if has_option else [0]
    dev = torch.device("cuda:0")
    n, K = a.n, a.pairs
    with StepLimit(a.limit, "input generation"):
        pk, msg, sig, _ = workload.make_batch(pkg, n * K, device=dev, tamper_every=0)
        pks, msgs, sig = pk.reshape(n, K, 12).contiguous(), msg.reshape(n, K, 32).contiguous(), sig[:n].contiguous()
        # one ring of two output tensors for every leg, sized for the longest vector
        longest = max(pkg.layout_multi(32, K, m)["n_witness"] if m else pkg.layout_multi(32, K)["n_witness"] for m in masks)
        ring = [torch.empty(n * longest * 6, dtype=torch.int64, device=dev) for _ in range(2)]
        res = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
    out = {"metric": "multi_engine_rate", "n": n, "n_pairs": K, "msg_len": 32, "steps_per_repetition": a.steps, "max_steps": a.max_steps, "n_buffers": a.buffers,
           "repetitions": a.reps, "abi": pkg.lib().blsw_version(), "masks": {}}
    for leg, m in enumerate(masks[:1] + masks):  # leg 0: the untimed first engine of the process
        with StepLimit(a.limit, "engine creation (mask %d)" % m):
            opt = {"n_pairs": K}
            if m:
                opt["multi_inputs"] = m
            eng = pkg.WitnessEngine(n, 32, max_steps=a.max_steps, n_buffers=a.buffers, device=dev, **opt)
            outs = [r[: n * eng.n_witness * 6].view(n, eng.n_witness, 6) for r in ring]
            inst = eng.new_instance_tensor() if m else None
            torch.cuda.synchronize()
        times = []
        for rep in range(a.reps + 1 if leg else 1):  # the first repetition warms up: scratch growth, first touch of the output tensors
            with StepLimit(a.limit, "repetition %d of mask %d" % (rep, m)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for s in range(a.steps):
                    kw = {"instance": inst} if inst is not None else {}
                    eng.submit_multi(pks, msgs, sig, witness=outs[s % 2], result=res, **kw)
                eng.flush()
                e1.record()
                torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1) / a.steps)
        if not leg:
            eng.close()
            del eng, outs, inst
            torch.cuda.empty_cache()
            continue
        med = statistics.median(times)
        step_bytes = n * (eng.n_witness + (eng.n_instance_vars if m else 0)) * 48
        out["masks"][str(m)] = {"n_witness": eng.n_witness, "n_instance_vars": eng.n_instance_vars, "workspace_bytes": eng.workspace.numel(), "bytes_per_step": step_bytes,
                                "ms_per_step": {"median": round(med, 3), "min": round(min(times), 3), "max": round(max(times), 3)},
                                "instances_per_s": round(n / (med / 1e3), 1), "GBps_written": round(step_bytes / (med / 1e3) / 1e9, 1)}
        with StepLimit(a.limit, "engine destruction (mask %d)" % m):
            eng.close()
        del eng, outs, inst
        torch.cuda.empty_cache()
    if "0" in out["masks"]:
        for m in out["masks"].values():
            m["rate_vs_mask_0"] = round(m["instances_per_s"] / out["masks"]["0"]["instances_per_s"], 3)
    del ring
    torch.cuda.empty_cache()
    with StepLimit(a.limit, "fill rate"):
        buf = torch.empty(8 << 30, dtype=torch.uint8, device=dev)
        out["fill_rate_GBps"] = round(pkg.fill_rate(buf, reps=3) / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
