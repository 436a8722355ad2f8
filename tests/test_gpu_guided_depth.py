"""The image-guided depth upsampling on the GPU (cs_guided_depth_plan / cs_guided_depth_apply through engine.guided_depth_plan,
engine.guided_depth, stereoimage_generation.upsample_depth_guided and the StereoDepthGuidedUpsample node): the plan by value and
the output bit for bit tools/guided_oracle.py, the specification, compared as uint32.  "Bit for bit": NaN where the oracle has
NaN (of any payload: IEEE 754 leaves the payload an operation hands on to the implementation), bits elsewhere.  Nothing here has
a tolerance but the edge property, whose bound is the rounding of a weighted mean of K * K equal values."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_guided, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import guided_oracle as oracle   # noqa: E402
import make_guided_goldens as goldens   # noqa: E402

pytestmark = pytest.mark.gpu
INF = float("inf")
CASES = goldens.cases()
IDS = [c["id"] for c in CASES]
_cache = {}


def case_of(cid):
    return next(c for c in CASES if c["id"] == cid)


def expected(case):
    """(image, depth, plan, out) of a case, computed once and shared; nothing changes them."""
    if case["id"] not in _cache:
        image, depth = goldens.make_input(case)
        p, out = goldens.evaluate(case, (image, depth))
        for a in (image, depth, out):
            a.setflags(write=False)
        _cache[case["id"]] = (image, depth, p, out)
    return _cache[case["id"]]


def bits(a):
    return goldens.canonical(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def on_device(a, offset=0):
    """The array on the GPU; offset: floats by which its first element is off the allocation's (16-byte aligned) start."""
    flat = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def plan_for(case):
    return engine.guided_depth_plan(case["h"], case["w"], case["dh"], case["dw"], case["radius"], case["sigma_s"], case["sigma_r"])


def apply_into(image, depth, plan, out):
    """cs_guided_depth_apply into a tensor of the caller's (engine.guided_depth allocates its own, on the 16-byte grid)."""
    n, h, w, _ = image.shape
    engine._launch(image.device, _native.lib().cs_guided_depth_apply, engine._ptr(image), engine._ptr(depth), n, h, w, depth.shape[1],
                   depth.shape[2], depth.shape[3], plan.radius, engine._ptr(plan.buffer), plan.nbytes, engine._ptr(out))
    return out


def run(case, plan=None):
    image, depth, _, _ = expected(case)
    plan = plan_for(case) if plan is None else plan
    img = on_device(image, 1 if case["off"] == "image" else 0)
    dep = on_device(depth, 1 if case["off"] == "depth" else 0)
    if case["off"] == "out":
        out = on_device(np.zeros((case["n"], case["h"], case["w"]), np.float32), 1)
        return plan, apply_into(img, dep, plan, out)
    return plan, engine.guided_depth(img, dep, plan)


def check_plan(plan, want):
    for name in ("cx", "cy", "gx", "gy"):
        got = getattr(plan, name)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), getattr(want, name)), name
    for name in ("wx", "wy", "wr"):
        got = getattr(plan, name)
        assert got.dtype == torch.float32 and tuple(got.shape) == getattr(want, name).shape and same_bits(got, getattr(want, name)), name


# ---- every case against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_specification(case):
    image, depth, p, want = expected(case)
    plan, got = run(case)
    check_plan(plan, p)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)) and same_bits(got, want)
    if case["off"]:          # the guarded path gives what the 16-byte path gives
        assert same_bits(got, expected(case_of("8x32_to_16x64_n1_c3_r2"))[3])


def test_the_oracle_here_is_the_one_the_fixture_pins():
    with np.load(os.path.join(ROOT, "tests", "golden", "guided_depth.npz")) as z:
        meta = {c["id"]: c for c in json.loads(str(z["meta"]))["cases"]}
        for case in CASES[::4]:
            _, _, p, out = expected(case)
            assert goldens.digest(goldens.canonical(out)) == meta[case["id"]]["out_sha256"]
            assert np.array_equal(z[case["id"] + "/cx"], p.cx) and np.array_equal(z[case["id"] + "/gy"], p.gy)


@pytest.mark.parametrize("sigmas", [(1e-200, 0.1), (1.0, 1e-200), (INF, INF), (0.05, 3.0)])
def test_the_plan_at_the_ends_of_the_sigmas_range(sigmas):
    """A sigma whose square underflows (weights 0, and NaN where t == 0), infinite sigmas (weights 1), a narrow spatial Gaussian."""
    for h, w, dh, dw in ((17, 23, 5, 7), (16, 64, 16, 64)):
        check_plan(engine.guided_depth_plan(h, w, dh, dw, 3, *sigmas), oracle.plan(h, w, dh, dw, 3, *sigmas))


def test_a_plan_at_4k_from_518():
    """The sizes the pass is for: every centre, weight and guide position of a 2160 x 3840 plan from 518 x 921."""
    check_plan(engine.guided_depth_plan(2160, 3840, 518, 921), oracle.plan(2160, 3840, 518, 921))


# ---- every frame alone, plan reuse, graph ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["8x33_to_33x132_n3_c3_r2_fourfold", "5x7_to_17x23_n3_c3_r3_noninteger", "8x32_to_15x63_n3_c1_r1"])
def test_every_frame_of_a_batch_gets_what_it_gets_alone(cid):
    case = case_of(cid)
    image, depth, _, want = expected(case)
    plan = plan_for(case)
    img, dep = on_device(image), on_device(depth)
    whole = engine.guided_depth(img, dep, plan)
    for t in range(case["n"]):
        alone = engine.guided_depth(img[t:t + 1], dep[t:t + 1], plan)
        assert same_bits(alone, whole[t:t + 1]) and same_bits(alone, want[t:t + 1]), t


def test_one_plan_serves_two_batches():
    case = case_of("8x33_to_33x132_n3_c3_r2_fourfold")
    image, depth, p, want = expected(case)
    plan = plan_for(case)
    before = plan.buffer.clone()
    first = engine.guided_depth(on_device(image), on_device(depth), plan)
    second = engine.guided_depth(on_device(image[::-1].copy()), on_device(depth[::-1].copy()), plan)
    again = engine.guided_depth(on_device(image), on_device(depth), plan)
    assert same_bits(first, want) and same_bits(second, want[::-1]) and same_bits(again, want)
    assert torch.equal(plan.buffer, before)          # the apply pass only reads it
    check_plan(plan, p)


def test_one_graph_capture_and_one_replay_equal_the_eager_call():
    case = case_of("8x33_to_33x132_n3_c3_r2_fourfold")
    image, depth, _, want = expected(case)
    img, dep = on_device(image), on_device(depth)
    plan = plan_for(case)
    eager = engine.guided_depth(img, dep, plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        engine.guided_depth(img, dep, plan)            # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                      # (a wait for the device inside the call would make the capture fail)
        got = engine.guided_depth(img, dep, plan)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(got, eager) and same_bits(got, want)


# ---- the layers above ------------------------------------------------------------------------------------------------------------------
def test_host_tensors_in_sub_batches_equal_the_single_device_call():
    case = case_of("5x7_to_17x23_n3_c3_r2_noninteger")
    image, depth, _, want = expected(case)
    args = (case["radius"], case["sigma_s"], case["sigma_r"])
    on_gpu = sig.upsample_depth_guided(on_device(image), on_device(depth), *args)
    assert on_gpu.is_cuda and tuple(on_gpu.shape) == (3, 17, 23, 3)
    for batch_size in (1, 2, 16):
        host = sig.upsample_depth_guided(torch.tensor(image), torch.tensor(depth), *args, batch_size=batch_size)
        assert not host.is_cuda and host.dtype == torch.float32 and same_bits(host, on_gpu), batch_size
    for ch in range(3):                                # the result in every channel
        assert same_bits(on_gpu[..., ch], want)
    gray = oracle.gray(depth)
    three = sig.upsample_depth_guided(image.copy(), gray, *args)          # numpy in, [N,dh,dw] -> [N,H,W]
    assert tuple(three.shape) == (3, 17, 23) and same_bits(three, want)
    one = sig.upsample_depth_guided(torch.tensor(image), torch.tensor(gray[..., None].copy()), *args)
    assert tuple(one.shape) == (3, 17, 23, 1) and same_bits(one[..., 0], want)


def test_the_nodes_output_is_a_depth_map_the_stereo_step_takes():
    case = case_of("8x33_to_33x132_n3_c3_r2_fourfold")
    image, depth, _, want = expected(case)
    node = depth_guided.StereoDepthGuidedUpsample()
    (up,) = node.upsample(torch.tensor(image), torch.tensor(depth), case["radius"], case["sigma_s"], case["sigma_r"], batch_size=2)
    assert tuple(up.shape) == (3, 33, 132, 3) and not up.is_cuda and same_bits(up[..., 0], want)
    img = on_device(image)
    got = engine.generate(img, up.cuda(), 4.0, 0.0, "left-right", 0.0, 0.5, 1.0, "polylines_sharp", 6.0, 7.0, False)
    same = engine.generate(img, on_device(np.repeat(want[..., None], 3, axis=3)), 4.0, 0.0, "left-right", 0.0, 0.5, 1.0, "polylines_sharp", 6.0, 7.0, False)
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (3, 33, 2 * 132, 3)              # side by side at the frame's size: nothing was resized
    assert all(torch.equal(a, b) for a, b in zip(got, same))


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_depth_edge_lands_on_the_guides_edge_on_the_device_too(radius):
    image, depth = goldens.edge_scene(radius)
    out = engine.guided_depth(on_device(image), on_device(depth), engine.guided_depth_plan(16, 64, 4, 16, radius, 1.0, 0.1)).cpu().numpy()
    goldens.check_edge_property(out, radius)
    assert same_bits(out, oracle.guided_depth(image, depth, radius, 1.0, 0.1))


# ---- refusals that need a device -------------------------------------------------------------------------------------------------------
def test_the_engine_refuses_what_it_cannot_run():
    plan = engine.guided_depth_plan(8, 8, 4, 4)
    img, d = torch.zeros((2, 8, 8, 3), device="cuda"), torch.zeros((2, 4, 4, 1), device="cuda")
    for a, b, text in ((img.cpu(), d, "device-resident"), (img, d.cpu(), "same device"), (img, torch.zeros((2, 4, 5, 1), device="cuda"), "plan is for")):
        with pytest.raises(ValueError, match=text):
            engine.guided_depth(a, b, plan)
    with pytest.raises(ValueError, match="device-resident"):
        engine.guided_depth_plan(8, 8, 4, 4, device="cpu")
    with pytest.raises(ValueError, match="same device"):
        sig.upsample_depth_guided(img, d.cpu())
    assert tuple(engine.guided_depth(img, d, plan).shape) == (2, 8, 8)
