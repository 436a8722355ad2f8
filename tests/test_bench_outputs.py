"""bench.py's plain run and --dump-outputs: the headline line alone, and the last timed step's outputs written as a seeded
sample that two runs (or two builds) with the same arguments can compare element for element."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample(t):
    """What dump_outputs keeps of a tensor, computed independently of it."""
    flat = t.reshape(-1)
    if flat.numel() <= bench.DUMP_SAMPLE:
        return t.to(torch.float32).cpu().numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, flat.numel(), bench.DUMP_SAMPLE, dtype=np.int64))
    return flat.cpu().numpy()[idx].astype(np.float32)


def test_dump_outputs_is_a_fixed_sample_within_64_mb(tmp_path):
    big = torch.arange(bench.DUMP_SAMPLE + 12345, dtype=torch.float32)
    small = torch.linspace(0, 1, 60, dtype=torch.float64).reshape(3, 4, 5)
    for d in ("a", "b"):
        bench.dump_outputs(torch, {"stereoscope": big, "mask": small}, str(tmp_path / d))
    for name, t in (("stereoscope", big), ("mask", small)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b) and np.array_equal(a, _sample(t))
    assert np.load(tmp_path / "a" / "mask.npy").shape == (3, 4, 5)
    # the four outputs of a step, each sampled at most DUMP_SAMPLE float32 values, stay under 64 MB
    assert 4 * (bench.DUMP_SAMPLE * 4 + 128) <= 64 * 10**6


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_its_last_step_computed(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "cfg2",
           "--frames", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert line["steps"] == 3 and line["unit"] == "frames/s" and line["dtype"] == "f32"
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(2.0)   # frames per timed step
    assert not {"roofline", "diagnostics", "cpu_baseline", "value_blur_off"} & set(line)   # the extras need --full

    from comfystereo_amd import engine
    cfg = bench.CONFIGS["cfg2"]
    H, W = cfg["h"], cfg["w"]
    device = torch.device("cuda", 0)
    image, depth = bench.make_inputs(torch, cfg, 2, 0, device)
    p = engine.make_params(2, H, W, H, W, 3, cfg["fill"], cfg["mode"], cfg["div"], 0.0, 0.0, 0.5, 2.0, True, 20.0, 20.0, 2.0, 6, 12)
    want = engine.Plan(p, device).run(image, depth)
    torch.cuda.synchronize()
    files = sorted(os.listdir(out))
    assert files == sorted(f"{n}.npy" for n in ("stereoscope", "depth_left", "depth_right", "mask"))
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10**6
    for name, t in zip(("stereoscope", "depth_left", "depth_right", "mask"), want):
        assert np.array_equal(np.load(out / f"{name}.npy"), _sample(t)), name
