"""What the three depth pre-passes of stereoimage_generation share, without a GPU: stabilize_depth, clip_depth_range and
upsample_depth_guided refuse the same bad `depth` and the same bad `batch_size` before they look for a device, each with its own
wording of the shape and all with one wording of the batch size (not gpu)."""
import re

import pytest
import torch

from comfystereo_amd import stereoimage_generation as sig

IMAGE = torch.zeros((2, 8, 8, 3))
PASSES = {
    "stabilize_depth": (sig.stabilize_depth, "[N,H,W] or [N,H,W,C]"),
    "clip_depth_range": (sig.clip_depth_range, "[N,H,W] or [N,H,W,C]"),
    "upsample_depth_guided": (lambda depth, **kw: sig.upsample_depth_guided(IMAGE, depth, **kw), "[N,dh,dw] or [N,dh,dw,C]"),
}


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("a device was looked for before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("bad", [torch.zeros((4, 4)), torch.zeros((2, 4, 4, 1, 1)), torch.zeros((0, 4, 4)), torch.zeros((2, 4, 4, 1))[:0]],
                         ids=["2d", "5d", "empty3d", "empty4d"])
def test_a_bad_depth_is_refused_before_any_device_lookup(no_device, name, bad):
    call, layout = PASSES[name]
    with pytest.raises(ValueError, match=re.escape(f"depth must be a non-empty {layout}, got shape {tuple(bad.shape)}")):
        call(bad)
    with pytest.raises(ValueError, match=re.escape(f"depth must be a non-empty {layout}, got shape {tuple(bad.shape)}")):
        call(bad.numpy())


@pytest.mark.parametrize("name", list(PASSES))
@pytest.mark.parametrize("batch_size", [0, -1])
def test_a_bad_batch_size_is_refused_before_any_device_lookup(no_device, name, batch_size):
    call, _ = PASSES[name]
    with pytest.raises(ValueError, match=re.escape(f"batch_size must be at least 1, got {batch_size}")):
        call(torch.zeros((2, 4, 4)), batch_size=batch_size)


@pytest.mark.parametrize("name", list(PASSES))
def test_good_arguments_reach_the_device_lookup(monkeypatch, name):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        PASSES[name][0](torch.zeros((2, 4, 4)))
