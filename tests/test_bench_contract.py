"""The bench line the round ends with (profiles/r03_final_bench.json = stdout of `python bench.py` on the MI355X box) carries
every field of the driver's contract, with the metric and workload BASELINE.json names."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    line = json.load(open(os.path.join(ROOT, "profiles", "r03_final_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["unit"] == "imgs/sec" and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["vs_baseline"] is None                      # BASELINE.md publishes no number for this metric
    assert line["dtype"] == "bf16" and line["data"] == "synthetic" and line["n_gpus"] == 1
    assert "workload" in line["config"] and "model" not in line["config"]
    assert "ResNet50" in line["config"]["workload"] and "B=512" in line["config"]["workload"]
    assert abs(line["value"] - 512 * 1e3 / line["ms_per_step"]) / line["value"] < 1e-3
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "probe", "step_frac", "measured"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1
    # BASELINE cfg 4 / cfg 5 timed in the same process behind the headline: reported beside it, never as `value`
    ex = line["extra_configs"]
    assert [e["workload"].split(":")[0] for e in ex] == ["BASELINE cfg 4", "BASELINE cfg 5", "BASELINE cfg 5"]
    assert [e["dtype"] for e in ex] == ["bf16", "bf16", "fp8-weights"]
    for e in ex:
        assert "error" not in e and e["value"] > 0 and abs(e["value"] - int(e["workload"].split("B=")[1].split(",")[0]) * 1e3 / e["ms_per_step"]) / e["value"] < 1e-3


def test_bench_cli_defaults_match_the_contract():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in src
    assert 'default=1)' in src                               # --gpus defaults to one GPU


def test_dump_outputs_is_seeded_and_bounded(tmp_path):
    """--dump-outputs: one .npy per state entry plus the loss, float32 / float64 only, under 64 MB however large the model, and the
    same sampled positions from run to run"""
    import sys

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    m = torch.nn.Module()
    m.encoder = torch.nn.Sequential(torch.nn.Conv2d(512, 512, 3), torch.nn.BatchNorm2d(512)).bfloat16()
    m.loss = torch.nn.Module()
    m.loss.register_buffer("weight", torch.randn(40000, 512))       # 80 MB in fp32: must be sampled
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, torch.tensor(1.5))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["loss.npy", "head.weight.npy"] + ["encoder.%s.npy" % k for k, v in m.encoder.state_dict().items() if v.numel()])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    assert float(np.load(tmp_path / "a" / "loss.npy")) == 1.5
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "encoder.1.running_var.npy"), np.ones(512, np.float32))
    w = np.load(tmp_path / "a" / "head.weight.npy")
    assert 0 < w.size < 40000 * 512 and np.isin(w, m.loss.weight.numpy()).all()
