"""Pillow's 8-bit bicubic resize on the MI355X (cs_pilresize.hip through engine.pil_resize and
stereodiffusion_nodes.pil_resize) against the numpy restatement (tools/pil_resize_oracle.py, itself held to PIL.Image.resize in
tests/test_fastmode_surface.py): the fixture's frame sizes, a fuzz of odd sizes, every direction of scaling, skipped passes,
1 x 1 frames, saturated checkerboards, batches, views and host tensors, the float ends, and the gray of all 2^24 colours.

Contract: every comparison is byte for byte (bit for bit on the float outputs); there is no tolerance."""
import numpy as np
import pytest
import torch

import pil_resize_oracle as po
from comfystereo_amd import _native, engine
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_gpu_grid_warp import FUZZ_WIDTHS

pytestmark = pytest.mark.gpu
WORK = 512
# (H, W) of tests/golden/fast_mode.npz
FIXTURE_SIZES = [(270, 480), (600, 800), (301, 777), (768, 432), (17, 23), (512, 512), (1080, 1920), (2160, 3840)]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rand_u8(rng, shape, kind="random"):
    if kind == "random":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "checker":   # saturated, alternating every pixel: the strongest ringing, clipped on both sides
        y, x = np.mgrid[0:shape[-3], 0:shape[-2]]
        return np.broadcast_to((((y + x) & 1) * 255).astype(np.uint8)[..., None], shape).copy()
    return (rng.integers(0, 2, shape) * 255).astype(np.uint8)   # saturated noise


def check(a, oh, ow, where):
    """engine.pil_resize of uint8 [N,H,W,C] against the restatement."""
    want = po.resize_hw(a, oh, ow)
    got = engine.pil_resize(cuda(a), (ow, oh)).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, where
    bad = int((got != want).sum())
    print(where, a.shape, "->", (oh, ow), "mismatching bytes", bad)
    assert bad == 0, (where, bad)
    return want


@pytest.mark.parametrize("hw", FIXTURE_SIZES)
def test_fixture_sizes_down_to_the_working_size_and_back(hw):
    h, w = hw
    rng = np.random.default_rng(h * 10007 + w)
    for c in (3, 1):
        a = rand_u8(rng, (1, h, w, c))
        small = check(a, WORK, WORK, ("down", c))
        check(small, h, w, ("back", c))
        check(rand_u8(rng, (1, WORK, WORK, c), "saturated"), h, w, ("back saturated", c))


@pytest.mark.parametrize("w", FUZZ_WIDTHS)
def test_fuzz_of_odd_sizes(w):
    rng = np.random.default_rng(3000 + w)
    for trial in range(4):
        # the other sizes: within the factor of 64 the kernels take, both directions
        ow = int(rng.integers(max(1, (w + 63) // 64), min(4 * w + 8, 5000)))
        h = int(rng.integers(1, 40))
        oh = int(rng.integers(max(1, (h + 63) // 64), 90))
        c = (3, 1)[trial & 1]
        n = int(rng.integers(1, 3))
        kind = ("random", "saturated")[trial >> 1]
        check(rand_u8(rng, (n, h, w, c), kind), oh, ow, ("width", w, trial))
        # the same width as a height
        if w <= 4097:
            check(rand_u8(rng, (1, w, h + 3, c), kind), ow, oh, ("height", w, trial))


def test_directions_skips_and_single_samples():
    rng = np.random.default_rng(31)
    for (h, w), (oh, ow) in [((40, 50), (97, 131)),      # up, up
                             ((97, 131), (40, 50)),      # down, down
                             ((40, 131), (97, 50)),      # up rows, down columns
                             ((97, 50), (40, 131)),      # down rows, up columns
                             ((33, 70), (33, 19)),       # vertical pass skipped
                             ((33, 70), (33, 301)),
                             ((33, 70), (9, 70)),        # horizontal pass skipped
                             ((33, 70), (150, 70)),
                             ((33, 70), (33, 70)),       # both: a copy
                             ((1, 1), (1, 1)), ((1, 1), (7, 5)), ((7, 5), (1, 1)), ((1, 9), (4, 1)), ((64, 64), (1, 1)),
                             ((640, 3), (10, 3)), ((3, 641), (3, 11))]:   # close to the limit of 64
        for c in (3, 1):
            check(rand_u8(rng, (2, h, w, c)), oh, ow, "directions")


def test_saturated_checkerboards_clip_their_ringing():
    rng = np.random.default_rng(32)
    for (h, w), (oh, ow) in [((64, 96), (100, 150)), ((64, 96), (41, 61)), ((512, 512), (301, 777)), ((301, 777), (512, 512))]:
        for c in (3, 1):
            check(rand_u8(rng, (1, h, w, c), "checker"), oh, ow, "checker")
            check(rand_u8(rng, (1, h, w, c), "saturated"), oh, ow, "saturated")
    # an upscaled saturated edge overshoots on both sides before clip8
    edge = np.zeros((1, 8, 16, 1), np.uint8)
    edge[:, :, 8:] = 255
    up = check(edge, 8, 64, "edge")
    assert up.min() == 0 and up.max() == 255


def test_a_batch_equals_its_frames():
    rng = np.random.default_rng(33)
    a = rand_u8(rng, (5, 37, 53, 3))   # (odd frame size: every frame but the first starts off a dword)
    A = cuda(a)
    for oh, ow in ((64, 64), (20, 90), (37, 11)):
        batch = engine.pil_resize(A, (ow, oh))
        assert np.array_equal(batch.cpu().numpy(), po.resize_hw(a, oh, ow))
        for k in range(a.shape[0]):
            assert torch.equal(engine.pil_resize(A[k:k + 1], (ow, oh))[0], batch[k]), (k, oh, ow)


def test_noncontiguous_and_host_inputs():
    rng = np.random.default_rng(34)
    a = rand_u8(rng, (2, 45, 67, 3))
    want = po.resize_hw(a, 30, 100)
    view = cuda(a.transpose(0, 2, 1, 3)).transpose(1, 2)
    assert not view.is_contiguous()
    got = sdn.pil_resize(view, (100, 30))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    host = sdn.pil_resize(torch.from_numpy(a), (100, 30))
    assert not host.is_cuda and np.array_equal(host.numpy(), want)
    one = sdn.pil_resize(torch.from_numpy(a[1]), (100, 30))
    assert one.shape == (30, 100, 3) and np.array_equal(one.numpy(), want[1])
    g = rand_u8(rng, (3, 2, 21, 40, 1))
    gray = sdn.pil_resize(torch.from_numpy(g[..., 0]), (64, 50))
    assert gray.shape == (3, 2, 50, 64) and np.array_equal(gray.numpy(), po.resize_hw(g, 50, 64)[..., 0])
    with pytest.raises(ValueError):
        sdn.pil_resize(torch.from_numpy(a).float(), (100, 30))
    with pytest.raises(ValueError):
        sdn.pil_resize(torch.from_numpy(a), (0, 30))


def test_float_in_and_float_out():
    rng = np.random.default_rng(35)
    x = (rng.random((2, 40, 56, 3), dtype=np.float32) * np.float32(1.3) - np.float32(0.15))   # some below 0, some above 1
    x[0, 0, :8, 0] = [0.0, 1.0, -0.0, 254.999 / 255.0, 1.0 / 255.0, 0.5, 2.0, -3.0]
    codes = po.float_codes(x)
    assert codes.min() == 0 and codes.max() == 255
    for oh, ow in ((64, 64), (40, 20), (90, 56), (40, 56)):
        want = po.resize_hw(codes, oh, ow)
        for layout in ("nhwc", "planar"):
            got, flt = engine.pil_resize(cuda(x), (ow, oh), f32=layout)
            assert np.array_equal(got.cpu().numpy(), want), (oh, ow, layout)
            wf = po.code_floats(want)
            if layout == "planar":
                wf = np.ascontiguousarray(wf.transpose(0, 3, 1, 2))
            assert np.array_equal(flt.cpu().numpy().view(np.uint32), wf.view(np.uint32)), (oh, ow, layout, "floats")
        # floats alone, into one eye of a side-by-side frame
        pair = torch.full((2, oh, 2 * ow + 1, 3), -1.0, device="cuda")
        none, eye = engine.pil_resize(cuda(x), (ow, oh), f32="nhwc", codes=False, f32_out=pair[:, :, ow:2 * ow])
        assert none is None and eye.data_ptr() == pair[:, :, ow:2 * ow].data_ptr()
        p = pair.cpu().numpy()
        assert np.array_equal(p[:, :, ow:2 * ow], po.code_floats(want)) and (p[:, :, :ow] == -1).all() and (p[:, :, 2 * ow:] == -1).all()
    # one channel, [N,H,W]
    g = x[..., 1]
    got, flt = engine.pil_resize(cuda(g), (33, 21), f32="planar")
    want = po.resize_hw(po.float_codes(g)[..., None], 21, 33)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flt.cpu().numpy()[:, 0], po.code_floats(want[..., 0]))


def test_gray_of_all_colours_in_one_launch():
    v = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([v >> 16, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    want = po.gray_codes(rgb)
    got = engine.pil_resize(cuda(rgb), (4096, 4096), gray=True)
    assert got.shape == (1, 4096, 4096, 1)
    bad = int((got[..., 0].cpu().numpy() != want).sum())
    print("gray: mismatching colours of 2^24:", bad)
    assert bad == 0
    # equal channels: k - 1, and 0 for 0
    k = np.arange(256)
    assert np.array_equal(po.gray_codes(np.stack([k, k, k], -1).astype(np.uint8)), np.maximum(k - 1, 0))
    # float colours, and the gray ahead of a resize
    rng = np.random.default_rng(36)
    x = rng.random((2, 50, 70, 3), dtype=np.float32)
    g = po.gray_codes(po.float_codes(x))[..., None]
    for oh, ow in ((50, 70), (64, 64), (50, 30), (20, 70)):
        got = engine.pil_resize(cuda(x), (ow, oh), gray=True)
        assert np.array_equal(got.cpu().numpy(), po.resize_hw(g, oh, ow)), (oh, ow)
        got = engine.pil_resize(cuda(po.float_codes(x)), (ow, oh), gray=True)
        assert np.array_equal(got.cpu().numpy(), po.resize_hw(g, oh, ow)), (oh, ow, "u8")


def test_a_reduction_beyond_the_limit_is_refused():
    L = _native.lib()
    assert L.cs_pil_resize_max_taps() == 257
    x = torch.zeros(1, 2, 6500, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(_native.NativeError) as ei:
        engine.pil_resize(x, (100, 2))     # a factor of 65
    assert ei.value.code == _native.CS_ELIMIT
    a = np.random.default_rng(37).integers(0, 256, (1, 2, 6400, 3)).astype(np.uint8)
    check(a, 2, 100, "factor 64")          # the strongest accepted reduction works
