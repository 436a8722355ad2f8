"""StereoDiffusion's Fast mode at any frame size on the MI355X (stereodiffusion_nodes.generate_stereo_fast: cs_pil_resize,
cs_inpaint_prepare and the blend) against the reference's own outputs in tests/golden/fast_mode.npz, with the 255 - image
stand-in for the model the fixture was recorded with; the calls of `inpaint`, an empty mask inside a batch, batches against
single frames, and where the results live.

Contract: everything is bit-exact; there is no tolerance."""
import numpy as np
import pytest
import torch

import make_fastmode_goldens as mg
import pil_resize_oracle as po
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_fastmode_surface import check_case, load

pytestmark = pytest.mark.gpu


def codes_of(t):
    """float32 tensor of code / 255 -> its uint8 codes, asserted to be exactly that."""
    a = t.cpu().numpy()
    u8 = np.rint(a * 255).astype(np.uint8)
    assert a.dtype == np.float32 and np.array_equal(po.code_floats(u8), a)
    return u8


class Stand:
    """255 - image on device tensors, recording what it was handed."""

    def __init__(self):
        self.calls = []

    def __call__(self, filled_u8, mask, k):
        assert filled_u8.is_cuda and mask.is_cuda
        assert filled_u8.dtype == torch.uint8 and tuple(filled_u8.shape) == (512, 512, 3)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (512, 512)
        self.calls.append((k, filled_u8.cpu().numpy(), mask.cpu().numpy()))
        return 255 - filled_u8


def test_every_fixture_case():
    z, meta = load()
    for c in meta["cases"]:
        img, dep = mg.inputs(c)
        stand = Stand()
        stereo, left, right = sdn.generate_stereo_fast(torch.from_numpy(img[None]).cuda(), torch.from_numpy(dep[None]).cuda(),
                                                       c["scale_factor"], stand)
        assert stereo.is_cuda and left.is_cuda and right.is_cuda
        assert tuple(stereo.shape) == (1, c["h"], 2 * c["w"], 3) and tuple(left.shape) == (1, c["h"], c["w"], 3)
        assert len(stand.calls) == int(c["called"]), c["id"]
        mask, filled = (stand.calls[0][2], stand.calls[0][1]) if c["called"] else (None, None)
        check_case(z, c, codes_of(left)[0], codes_of(right)[0], codes_of(stereo)[0], mask, filled)
        assert torch.equal(stereo, torch.cat([left, right], dim=2))


def small_cases(meta):
    by = {c["id"]: c for c in meta["cases"]}
    return [by[k] for k in ("270x480_disc_p5", "270x480_flat_0", "270x480_disc_p5")]


def test_a_batch_with_an_empty_mask_calls_in_order_and_equals_single_calls():
    z, meta = load()
    cases = small_cases(meta)
    imgs, deps = zip(*(mg.inputs(c) for c in cases))
    imgs, deps = np.stack(imgs), np.stack(deps)
    imgs[2] = imgs[2, ::-1]     # (the third frame is not a copy of the first)
    # frame 1: a depth that falls smoothly from near on the left to far on the right -- at a positive scale factor the frame is
    # squeezed, no source x leaves [-1, 1] and no step is deep enough to disocclude: an empty mask
    w = deps.shape[2]
    deps[1] = mg.node_floats(np.broadcast_to((255 - (np.arange(w) * 255) // (w - 1)).astype(np.uint8)[None, :, None], deps[1].shape))
    I, D = torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), torch.from_numpy(deps).cuda()
    stand = Stand()
    stereo, left, right = sdn.generate_stereo_fast(I, D, 5.0, stand)
    assert [k for k, _, _ in stand.calls] == [0, 2]   # in frame order, and not for the frame whose mask is empty
    assert tuple(stereo.shape) == (3, 270, 960, 3)
    # frame 0 is the fixture's case; frame 1 is the warped frame resized back
    check_case(z, cases[0], codes_of(left)[0], codes_of(right)[0], codes_of(stereo)[0], stand.calls[0][2], stand.calls[0][1])
    want1 = po.fast_mode_frame(imgs[1], deps[1], 5.0, None)
    assert not want1["called"] and np.array_equal(codes_of(right)[1], want1["right"]) and np.array_equal(codes_of(left)[1], want1["left"])
    for k in range(3):
        one = Stand()
        s1, l1, r1 = sdn.generate_stereo_fast(I[k:k + 1], D[k:k + 1], 5.0, one)
        assert torch.equal(s1[0], stereo[k]) and torch.equal(l1[0], left[k]) and torch.equal(r1[0], right[k]), k
        assert [i for i, _, _ in one.calls] == ([] if k == 1 else [0])
        if k != 1:
            batch_call = stand.calls[0 if k == 0 else 1]
            assert np.array_equal(one.calls[0][1], batch_call[1]) and np.array_equal(one.calls[0][2], batch_call[2])


def test_depth_layouts_and_host_tensors():
    z, meta = load()
    c = {c["id"]: c for c in meta["cases"]}["17x23_disc_p5"]
    img, dep = mg.inputs(c)
    I, D = torch.from_numpy(img[None]), torch.from_numpy(dep[None])
    # host tensors: the results come back to the host
    stand = Stand()
    host = sdn.generate_stereo_fast(I, D, c["scale_factor"], stand)
    assert all(not t.is_cuda for t in host) and len(stand.calls) == 1
    check_case(z, c, codes_of(host[1])[0], codes_of(host[2])[0], codes_of(host[0])[0], stand.calls[0][2], stand.calls[0][1])
    # one channel is taken as it is (no gray rule), in both layouts; float64 inputs
    g = D[..., 0]
    want = po.fast_mode_frame(img, dep[..., 0], c["scale_factor"], lambda f, m: 255 - f)
    for d in (g.cuda(), g[..., None].cuda(), g.double().cuda()):
        s, l, r = sdn.generate_stereo_fast(I.cuda(), d, c["scale_factor"], Stand())
        assert s.is_cuda and np.array_equal(codes_of(r)[0], want["right"]) and np.array_equal(codes_of(l)[0], want["left"])
    # the coloured depth of the fixture through the gray rule
    c = {c["id"]: c for c in meta["cases"]}["17x23_rgb_m3"]
    img, dep = mg.inputs(c)
    assert not np.array_equal(dep[..., 0], dep[..., 1])
    stand = Stand()
    s, l, r = sdn.generate_stereo_fast(torch.from_numpy(img[None]).cuda(), torch.from_numpy(dep[None]), c["scale_factor"], stand)
    assert s.is_cuda   # a device image keeps the results on the device
    check_case(z, c, codes_of(l)[0], codes_of(r)[0], codes_of(s)[0], stand.calls[0][2], stand.calls[0][1])


def test_a_wrong_answer_of_inpaint_is_refused():
    img, dep = torch.rand(1, 20, 30, 3).cuda(), torch.rand(1, 20, 30).cuda()
    dep[0, :, 15:] += 1.0
    for bad in (lambda f, m, k: f.float(), lambda f, m, k: f[:100], lambda f, m, k: f.cpu().numpy()):
        with pytest.raises(ValueError):
            sdn.generate_stereo_fast(img, dep, 8.0, bad)
