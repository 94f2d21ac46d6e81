"""Child process of tests/test_registry_gpu.py::test_two_calls_on_a_side_stream_agree: a KeyRegistry filled in two appends and registry_verify twice
per mode, all on one non-default stream (the stream orders the calls behind the appends).

    python -m tests.registry_stream_worker <batch.npz>      prints one JSON line

A process of its own for the reason tests/committee_stream_worker.py gives: a stream's hardware queue keeps the scratch of the verifiers' 4.5 KB-stack
kernels for as long as the process lives, and inside the suite's process that queue would stay pinned under every engine test that runs later."""
import importlib
import json
import sys

import numpy as np
import torch  # before the library: one HIP runtime in the process, torch's


def main(path):
    pkg = importlib.import_module("bls-verify-gadget_amd")
    dev = torch.device("cuda:0")
    z = np.load(path)
    pks48, indices, offsets, msg, sig, sc = (torch.from_numpy(z[k]).to(dev) for k in ("pks48", "indices", "offsets", "msg", "sig", "scalars"))
    group, capacity, cut = int(z["group"]), int(z["capacity"]), int(z["cut"])
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(dev).cuda_stream != 0
        reg = pkg.KeyRegistry(capacity, device=dev)
        reg.append(pks48[:cut].contiguous())
        reg.append(pks48[cut:].contiguous())
        a = pkg.registry_verify(reg, indices, offsets, msg, sig, want_status=True, want_aggregate=True)
        b = pkg.registry_verify(reg, indices, offsets, msg, sig, want_status=True, want_aggregate=True)
        ga = pkg.registry_verify(reg, indices, offsets, msg, sig, group=group, scalars=sc)
        gb = pkg.registry_verify(reg, indices, offsets, msg, sig, group=group, scalars=sc)
    s.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(ga, gb)
    print(json.dumps({"same": bool(same), "size": reg.size, "verdicts": a[0].tolist(), "status": a[1].tolist(), "key_status": reg.key_status().tolist(),
                      "aggregate": [bytes(r).hex() for r in a[2].cpu().numpy()], "groups": ga.tolist()}))
    reg.close()


if __name__ == "__main__":
    main(sys.argv[1])
