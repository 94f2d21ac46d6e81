"""What the device edge tests (test_chain_edges_gpu.py, test_agg_edges_gpu.py) share: host arrays to the device and the exact comparison of two
witness vectors on the device. TEST HARNESS ONLY."""
import numpy as np


def same(torch, tag, lane, got, want):
    assert tuple(got.shape) == tuple(want.shape), (tag, lane, got.shape, want.shape)
    if not torch.equal(got, want):
        idx = int(torch.nonzero((got != want).any(dim=1))[0].item())
        raise AssertionError("%s, lane %d: first mismatching witness index %d" % (tag, lane, idx))


def to_dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
