"""engine.py refuses what it refused before its argument checks were single-sourced, with the same exception and the same words:
the corpora of tools/engine_refusals.py, recorded from the engine as it was (tests/golden/engine_refusals_cpu.json on host tensors,
engine_refusals_gpu.json on device tensors, which reach the checks behind the device check), replayed.  The one intended difference
is in the second file already: the five former `assert`s are ValueError.  And the one intended change of behaviour: a call runs on
the device of its tensors, whichever device is current."""
import os
import sys

import pytest
import torch

from comfystereo_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import engine_refusals   # noqa: E402


def _replay(device):
    recorded_on, want = engine_refusals.load(os.path.join(ROOT, "tests", "golden", f"engine_refusals_{'cpu' if device == 'cpu' else 'gpu'}.json"))
    assert recorded_on == device and len(want) >= engine_refusals.MIN_TOTAL
    got = engine_refusals.run(device)   # (CorpusError if a case is accepted or a function has fewer than 40)
    assert [row[:2] for row in got] == [row[:2] for row in want]
    for g, w in zip(got, want):
        assert g == w
    return want


def test_host_tensors_are_refused_as_recorded(monkeypatch):
    # (on a machine that has a GPU: what the package does when torch reports none, as the corpus was recorded)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    want = _replay("cpu")
    assert not any(row[2] == "AssertionError" for row in want)


@pytest.mark.gpu
def test_device_tensors_are_refused_as_recorded():
    want = _replay("cuda")
    former = {row[0] for row in want if row[2] == "ValueError" and row[3] == engine_refusals.FORMER_ASSERTS.get(row[0])}
    assert former == set(engine_refusals.FORMER_ASSERTS) and not any(row[2] == "AssertionError" for row in want)


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_a_call_runs_on_its_tensors_device_whichever_is_current():
    """One wrapper of each family that used to launch on the current device's stream, tensors on device 1, device 0 current: bit
    for bit what the same call gives with device 1 current."""
    g = torch.Generator().manual_seed(5)
    on1 = lambda t: t.to("cuda:1")   # noqa: E731
    codes = on1(torch.randint(0, 256, (1024,), dtype=torch.uint8, generator=g))
    depth = on1(torch.rand(2, 32, 64, generator=g) * 255)
    image, warp_depth = on1(torch.rand(1, 3, 16, 64, generator=g)), on1(torch.rand(1, 16, 64, generator=g))
    flat = on1(torch.rand(16, 64, generator=g))
    frame, frame_depth = on1(torch.rand(1, 16, 64, 3, generator=g)), on1(torch.rand(1, 16, 64, 3, generator=g))
    params = engine.make_params(1, 16, 64, 16, 64, 3, "polylines_soft", "left-right", 6.0, 0.3, 0.1, 0.5, 2.0, True, 20.0, 20.0, 2.0, 6, 12)
    plan = engine.Plan(params, "cuda:1")
    calls = [lambda: engine.expand_u8(codes), lambda: engine.directional_blur(depth, 20.0, 20.0),
             lambda: engine.forward_warp(image, warp_depth, 4.0, 0.5, 1.0), lambda: engine.gaussian_blur(flat, 1.0),
             lambda: tuple(t.clone() for t in plan.run(frame, frame_depth))]
    for call in calls:
        with torch.cuda.device(1):
            want = call()
            want = [t.cpu() for t in (want if isinstance(want, tuple) else (want,))]
        with torch.cuda.device(0):
            got = call()
            assert torch.cuda.current_device() == 0
            got = [t.cpu() for t in (got if isinstance(got, tuple) else (got,))]
        assert all(t.device.type == "cpu" and torch.equal(a, t) for a, t in zip(want, got)) and len(want) == len(got)
