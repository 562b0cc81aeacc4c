"""CPU: bench.py's "cannot fail silently" contract where no GPU is needed to show it -- a run
that cannot work still ends with exactly ONE JSON line carrying n_gpus, rccl_ranks_seen and an `error` field."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert len(lines) == 1, (p.stdout[-1000:], p.stderr[-1000:])
    return p, json.loads(lines[0])


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU failure path")
def test_single_rank_without_gpu_prints_error_line():
    p, r = _run(["--steps", "20", "--warmup", "5"])
    assert p.returncode != 0 and r["value"] is None and r["n_gpus"] == 1 and "no CPU fallback" in r["error"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU failure path")
def test_two_ranks_without_gpu_print_one_error_line():
    """self-spawned torchrun with two ranks that both fail (or one fails and the launcher SIGTERMs the other, which is
    taken by the sigwait thread): still one line, n_gpus = 2."""
    p, r = _run(["--gpus", "2", "--steps", "20", "--warmup", "5", "--watchdog-s", "120"])
    assert p.returncode != 0 and r["value"] is None and r["n_gpus"] == 2 and r["rccl_ranks_seen"] == 0 and r["error"]


def test_error_line_keeps_partial_measurements():
    sys.path.insert(0, ROOT)
    import bench
    line = bench.error_line(8, "boom", stage="rollout_allgather", partial={"value": 1.0e12, "rccl_ranks_seen": 8, "steps": 20})
    assert line["value"] == 1.0e12 and line["n_gpus"] == 8 and line["rccl_ranks_seen"] == 8
    assert line["error"] == "boom" and line["failed_stage"] == "rollout_allgather" and line["metric"] == "agent_steps_per_sec"


def test_dump_outputs_writes_the_last_step_as_float32_within_the_limit(tmp_path):
    """--dump-outputs: row t of every plane of the fragment plus last_obs, float32; over the limit a seeded sample of env rows
    (the same rows every time) and their indices."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from phantom_amd.device import Trajectory
    T, B, S, D, t = 5, 1000, 9, 3, 3
    g = torch.Generator().manual_seed(0)
    tr = Trajectory(torch.randn(T, B, S, D, generator=g), torch.randn(T, B, S, generator=g), torch.randn(T, B, S, generator=g),
                    torch.zeros(T, B, S, dtype=torch.uint8), (torch.arange(T * B * S) % 3 == 0).to(torch.uint8).view(T, B, S),
                    torch.randn(B, S, D, generator=g))
    bench.dump_outputs(str(tmp_path / "full"), tr, t)
    full = {f[:-4]: np.load(str(tmp_path / "full" / f)) for f in os.listdir(str(tmp_path / "full"))}
    assert sorted(full) == ["actions", "last_obs", "observations", "rewards", "terminations", "truncations"]
    assert all(a.dtype == np.float32 for a in full.values())
    np.testing.assert_array_equal(full["observations"], tr.observations[t].numpy())
    np.testing.assert_array_equal(full["truncations"], tr.truncations[t].float().numpy())
    np.testing.assert_array_equal(full["last_obs"], tr.last_obs.numpy())
    limit = 100_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), tr, t, limit=limit)
        assert sum(os.path.getsize(str(tmp_path / d / f)) for f in os.listdir(str(tmp_path / d))) <= limit
    rows = np.load(str(tmp_path / "a" / "env_index.npy")).astype(np.int64)
    np.testing.assert_array_equal(rows, np.load(str(tmp_path / "b" / "env_index.npy")))
    assert 0 < len(rows) < B and (np.diff(rows) > 0).all()
    for name, a in full.items():
        np.testing.assert_array_equal(np.load(str(tmp_path / "a" / (name + ".npy"))), a[rows])
