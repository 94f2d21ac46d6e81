"""bench.py host logic without a GPU: --gpus N outside a launcher starts N ranks as a CHILD torch.distributed.run (never an
exec of a process that touched the GPU) and relays rank 0's JSON line; launch groups are balanced; the CPU share honours the
cgroup quota. On the GPU: a plain run prints the headline line and writes --dump-outputs, and leaves everything else to --full."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_spawn_ranks_builds_a_child_launcher(bench, monkeypatch, capsys):
    seen = {}

    class P:
        returncode = 0
        stdout = "NCCL banner\n" + json.dumps({"metric": "m", "n_gpus": 4}) + "\n"

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"], seen["env"] = cmd, env
        return P()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    args = bench.parse_args()
    with pytest.raises(SystemExit) as e:
        bench.spawn_ranks(args)
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert json.loads(capsys.readouterr().out.strip())["n_gpus"] == 4  # only the JSON line reaches stdout


def test_world_size_must_match_gpus(bench, monkeypatch):
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"])
    with pytest.raises(SystemExit, match="WORLD_SIZE"):
        bench.main()


def test_group_balancing_and_cpu_share(bench):
    assert bench.balanced_coalesce(20, 16) == 10 and bench.balanced_coalesce(1024, 16) == 16 and bench.balanced_coalesce(5, 16) == 5
    assert bench.balanced_coalesce(33, 16) == 11
    assert 1 <= bench.host_cores() <= (os.cpu_count() or 1)


def test_dump_outputs_files_exact_and_seeded(bench, tmp_path, monkeypatch):
    """--dump-outputs host logic on a small CPU tensor: float64 files under 64 MB, u64 words split exactly into u32 halves, the witness sample
    drawn from the whole tensor with a fixed seed (the same files twice), ranks of a multi-GPU run sharing the budget."""
    import numpy as np
    import torch

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--dump-outputs", str(tmp_path)])
    args = bench.parse_args()
    assert args.steps == 7 and args.dump_outputs == str(tmp_path)
    words = np.array([0, 1, 2**32 - 1, 2**32, 2**63 + 5, 2**64 - 1], dtype=np.uint64)
    halves = bench.u64_to_f64(words.reshape(1, 6))
    assert halves.dtype == np.float64 and halves.shape == (1, 12)
    assert [int(halves[0, 2 * i]) + (int(halves[0, 2 * i + 1]) << 32) for i in range(6)] == [int(x) for x in words]

    class Pkg:
        @staticmethod
        def witness_digest(w):
            return w.sum(dim=1)[:, :2]

    n, nw = 5, 37
    rng = np.random.default_rng(1)
    w = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, size=(n, nw, 6), dtype=np.int64))
    res = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    shapes = bench.dump_outputs(Pkg, str(tmp_path / "a"), w, res)
    bench.dump_outputs(Pkg, str(tmp_path / "b"), w, res)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["result.npy", "witness_digest.npy", "witness_sample.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert np.load(tmp_path / "a" / "result.npy").tolist() == [1, 0, 1, 1, 0]
    sample = np.load(tmp_path / "a" / "witness_sample.npy")
    assert shapes["witness_sample"] == list(sample.shape) and sample.shape[1] == 12
    limbs = (sample[:, 0::2].astype(np.uint64) | (sample[:, 1::2].astype(np.uint64) << np.uint64(32)))
    elems = {tuple(r) for r in w.numpy().view(np.uint64).reshape(-1, 6).tolist()}
    assert all(tuple(r) in elems for r in limbs.tolist())
    assert len({tuple(r) for r in limbs.tolist()}) == n * nw  # the sample reaches every element of a small tensor
    bench.dump_outputs(Pkg, str(tmp_path / "c"), w, res, rank=1, world=2)
    assert np.load(tmp_path / "c" / "witness_sample_rank1.npy").shape[0] == sample.shape[0] // 2


def test_full_is_off_by_default_and_reaches_the_ranks(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse_args().full is False
    seen = {}

    class P:
        returncode = 0
        stdout = json.dumps({"metric": "m"}) + "\n"

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"] = cmd
        return P()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--full"])
    args = bench.parse_args()
    assert args.full is True
    with pytest.raises(SystemExit):
        bench.spawn_ranks(args)
    assert seen["cmd"][-3:] == ["--gpus", "2", "--full"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    """`bench.py` without --full: one JSON line with the headline fields and right results, the dumped arrays, and none of the
    yardsticks, checks or legs that --full adds. Not a measurement."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "128",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "instances/s" and out["higher_is_better"] is True and out["value"] > 0 and "dtype" in out
    assert out["steps"] == 2 and out["warmup"] == 1 and abs(out["ms_per_step"] - 128 / out["value"] * 1e3) < 1e-6 * out["ms_per_step"]
    assert out["config"]["results_ok"] is True and out["roofline"]["launches_timed"] > 0
    assert out["witness_ok"] is None and out["roofline"]["fill_GBps"] is None
    for key in ("side", "cpu_baseline", "consumer_mode", "value_consumer_mode", "allgather", "roofline_valu", "roofline_valu_executed"):
        assert key not in out, key
    assert sorted(os.listdir(tmp_path)) == ["result.npy", "witness_digest.npy", "witness_sample.npy"]
    assert out["dump_outputs"]["arrays"]["result"] == [128]
