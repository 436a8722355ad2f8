"""The branches of the depth blur's plan (cs_blur.hip blur_plan / launch_blur) that no other test names, each on one small frame
through engine.directional_blur, bit for bit against the oracle's directional blur.  -m gpu."""
import numpy as np
import pytest
import torch

import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

PRM = (20, 20, 2.0, 6)   # strength (= mask width), edge threshold, falloff, vertical smoothing: the neighbouring tests' values


@pytest.fixture(scope="module")
def engine():
    from comfystereo_amd import engine as e
    assert torch.cuda.is_available()
    return e


def frame(h, w):
    return np.round(synth.blobs(h, w, seed=3) * 255).astype(np.float32)


_WANT = {}


def want(h, w, prm=PRM):
    """the oracle's blur of frame(h, w), computed once per shape and parameters, as bits"""
    key = (h, w, prm)
    if key not in _WANT:
        _WANT[key] = tuple(a.view(np.uint32) for a in oracle.blur(frame(h, w), *prm))
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def blur_bits(engine, depth, prm=PRM):
    return tuple(t.cpu().numpy().view(np.uint32) for t in engine.directional_blur(depth, *prm))


# (40, 128): two tile rows of two tiles, the worklist fits behind the bit rows -> listed, k_blur_fused<true>
# (40, 130): w % 4 != 0 -> the one-column-per-lane edge kernel and one workgroup per tile (no worklist), three tile columns
# (5, 8):    fused, but bit rows + worklist (592 bytes) outgrow the 160-byte buffer -> float4 edge kernel, one workgroup per tile
# (100, 1):  the bit rows (800 bytes) outgrow the buffer (512 bytes) -> the two-pass kernels
@pytest.mark.parametrize("h,w", [(40, 128), (40, 130), (5, 8), (100, 1)])
def test_plan_branch_equals_oracle(engine, h, w):
    got = blur_bits(engine, torch.from_numpy(frame(h, w)).cuda())
    for g, o, eye in zip(got, want(h, w), "LR"):
        assert np.array_equal(g, o), (h, w, eye)


def test_box_narrower_than_a_tile(engine):
    """strength 5: box of 5 columns, mask radius 5"""
    prm = (5, 20, 2.0, 6)
    got = blur_bits(engine, torch.from_numpy(frame(40, 128)).cuda(), prm)
    for g, o, eye in zip(got, want(40, 128, prm), "LR"):
        assert np.array_equal(g, o), eye


def test_depth_off_the_16_byte_grid(engine):
    """the depth tensor as a view 4 bytes into a larger allocation: listed, but k_blur_fused<false> (its float4 loader needs a
    16-byte aligned map)"""
    h, w = 40, 128
    store = torch.zeros(h * w + 8, dtype=torch.float32, device="cuda")
    depth = store[1:1 + h * w].view(h, w)
    depth.copy_(torch.from_numpy(frame(h, w)))
    assert depth.data_ptr() % 16 == 4 and depth.is_contiguous()
    got = blur_bits(engine, depth)
    for g, o, eye in zip(got, want(h, w), "LR"):
        assert np.array_equal(g, o), eye


def test_scalar_edge_kernel_switch(engine, dev_switch):
    """blur_edges_scalar: k_blur_edges instead of k_blur_edges4 and k_blur_fused<false> over the worklist -- the default's bits"""
    h, w = 40, 128
    depth = torch.from_numpy(frame(h, w)).cuda()
    default = blur_bits(engine, depth)
    dev_switch("blur_edges_scalar", 1)
    scalar = blur_bits(engine, depth)
    for d, s, o, eye in zip(default, scalar, want(h, w), "LR"):
        assert np.array_equal(s, d) and np.array_equal(s, o), eye
