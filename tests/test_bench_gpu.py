"""bench.py as the driver runs it: `python bench.py --gpus N` must start its own ranks (the reference spawns its ranks
itself, /root/reference/main/main.py:255-259).  Rehearsed on the one-GPU box with FRHIP_BENCH_BACKEND=gloo: both ranks on cuda:0, gloo
collectives on device tensors, the whole N > 1 code path (DataParallel arena all-reduce, class-sharded PartialFC at rate 0.1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_starts_its_own_ranks_and_reports_them(tmp_path):
    env = dict(os.environ, FRHIP_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-extra",
                        "--batch", "64", "--classes", "4000", "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # ONE JSON line, from rank 0
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["global_batch"] == 128 and rec["scaling"] == "weak"
    assert rec["config"]["collective_backend"] == "gloo" and "rate 0.1" in rec["config"]["workload"]
    assert rec["value"] > 0 and rec["final_loss"] == rec["final_loss"]
    # --dump-outputs writes rank 0's outputs of the last timed step: its loss is the reported one, beside the encoder and the head shard
    assert abs(float(np.load(tmp_path / "loss.npy")) - rec["final_loss"]) < 1e-4
    assert np.load(tmp_path / "head.weight.npy").dtype == np.float32
    assert os.path.exists(tmp_path / "encoder.module.conv1.weight.npy")


def test_bench_outputs_are_identical_from_run_to_run(tmp_path):
    """same arguments -> same seeded inputs -> bit-identical outputs of the timed path (no order-dependent fp32 accumulation)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-extra",
                            "--no-cpu-baseline", "--batch", "64", "--classes", "4000", "--dump-outputs", str(tmp_path / run)],
                           env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "loss.npy" in names and "head.weight.npy" in names
    for f in names:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
