"""Child process of tests/test_verify_pairs_gpu.py::test_two_streams_with_their_own_workspaces: verify_pairs on two non-default streams at once, each
call with its own workspace; the parent compares with its own calls, made one after the other.

    python -m tests.verify_pairs_stream_worker <batch.npz>      prints one JSON line

It is a process of its own for the reason tests/committee_stream_worker.py gives: a stream's hardware queue keeps the scratch of the 4.5 KB-stack
kernels (k_vp_finish, k_vp_decode) for as long as the process lives."""
import importlib
import json
import sys

import numpy as np
import torch  # before the library: one HIP runtime in the process, torch's


def main(path):
    pkg = importlib.import_module("bls-verify-gadget_amd")
    dev = torch.device("cuda:0")
    z = np.load(path)
    a_in = [torch.from_numpy(z[k]).to(dev) for k in ("pks_a", "msgs_a", "sig_a")]
    b_in = [torch.from_numpy(z[k]).to(dev) for k in ("pks_b", "msgs_b", "sig_b")]
    counts_b = torch.from_numpy(z["counts_b"]).to(dev)
    torch.cuda.synchronize(dev)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.cuda.stream(sa):
        assert torch.cuda.current_stream(dev).cuda_stream != 0
        a = pkg.verify_pairs(*a_in, want_status=True)
    with torch.cuda.stream(sb):
        assert torch.cuda.current_stream(dev).cuda_stream not in (0, sa.cuda_stream)
        b = pkg.verify_pairs(*b_in, counts=counts_b, want_status=True)
    sa.synchronize()
    sb.synchronize()
    print(json.dumps({"a": a[0].tolist(), "a_status": a[1].tolist(), "b": b[0].tolist(), "b_status": b[1].tolist()}))


if __name__ == "__main__":
    main(sys.argv[1])
