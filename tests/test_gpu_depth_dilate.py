"""The foreground depth edge dilation on the GPU (cs_depth_dilate through engine.depth_dilate,
stereoimage_generation.dilate_depth_edges and the StereoDepthEdgeDilate node): the output bit for bit tools/dilate_oracle.py, the
specification, compared as uint32.  "Bit for bit": NaN where the oracle has NaN, bits elsewhere.  Nothing here has a tolerance: the
pass selects values, it computes none but the gate's one subtraction."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from comfystereo_amd import _native, depth_dilate, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dilate_oracle as oracle   # noqa: E402
import make_dilate_goldens as goldens   # noqa: E402

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
CASES = goldens.cases()
IDS = [c["id"] for c in CASES]
_cache = {}


def case_of(cid):
    return next(c for c in CASES if c["id"] == cid)


def expected(case):
    """(depth, out) of a case, computed once and shared; nothing changes them."""
    if case["id"] not in _cache:
        depth = goldens.make_input(case)
        out = goldens.evaluate(case, depth)
        for a in (depth, out):
            a.setflags(write=False)
        _cache[case["id"]] = (depth, out)
    return _cache[case["id"]]


def bits(a):
    return goldens.canonical(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def same_bits(a, b):
    a, b = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a), bits(b))


def on_device(a, offset=0):
    """The array on the GPU; offset: floats by which its first element is off the allocation's (16-byte aligned) start."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    flat = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def native_call(depth, out, radius=2, shape=1, near=0, threshold=0.04, n=None, h=None, w=None, c=None, depth_ptr=None, out_ptr=None):
    """cs_depth_dilate itself -> (its code, its error text); the sizes and pointers are the tensors' unless given."""
    L = _native.lib()
    dn, dh, dw, dc = depth.shape
    p = lambda given, t: ctypes.c_void_p(t.data_ptr()) if given is None else given   # noqa: E731
    with torch.cuda.device(depth.device):
        rc = L.cs_depth_dilate(p(depth_ptr, depth), dn if n is None else n, dh if h is None else h, dw if w is None else w,
                               dc if c is None else c, radius, shape, near, threshold, p(out_ptr, out), engine._stream())
    return rc, L.cs_last_error().decode()


def apply_into(depth, out, case):
    """cs_depth_dilate into a tensor of the caller's (engine.depth_dilate allocates its own, on the 16-byte grid)."""
    rc, text = native_call(depth, out, case["radius"], _native.DILATE_SHAPE[case["shape"]], _native.DILATE_NEAR[case["near"]], case["threshold"])
    assert rc == _native.CS_OK, text
    return out


def run(case):
    depth, _ = expected(case)
    dep = on_device(depth, 1 if case["off"] == "depth" else 0)
    if case["off"] == "out":
        return apply_into(dep, on_device(np.zeros((case["n"], case["h"], case["w"]), np.float32), 1), case)
    return engine.depth_dilate(dep, case["radius"], case["shape"], case["near"], case["threshold"])


# ---- every case against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_specification(case):
    depth, want = expected(case)
    got = run(case)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert same_bits(got, want)
    if case["off"]:          # the guarded path gives what the 16-byte path gives
        assert same_bits(got, expected(case_of(case["id"][:-len("_off" + case["off"])]))[1])


def test_the_oracle_here_is_the_one_the_fixture_pins():
    with np.load(os.path.join(ROOT, "tests", "golden", "depth_dilate.npz")) as z:
        meta = {c["id"]: c for c in json.loads(str(z["meta"]))["cases"]}
        assert list(meta) == IDS
        for case in CASES[::4]:
            assert goldens.digest(goldens.canonical(expected(case)[1])) == meta[case["id"]]["out_sha256"]


# ---- the impulse: the changed pixels are exactly the window ----------------------------------------------------------------------------
IMPULSE_H, IMPULSE_WIDTHS = 40, (132, 131)   # the 16-byte path and, w % 4 != 0, the guarded one; three tiles by three either way


def impulse_positions(radius, w):
    h, r = IMPULSE_H, radius
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    seams = [(15, 63), (15, 64), (16, 63), (16, 64), (31, 127), (32, 128)]
    borders = [(r - 1, 70), (r, 70), (h - r, 70), (h - 1 - r, 70), (20, r - 1), (20, r), (20, w - r), (20, w - 1 - r)]
    return corners + seams + borders


@pytest.mark.parametrize("width", IMPULSE_WIDTHS)
@pytest.mark.parametrize("shape", oracle.SHAPES)
@pytest.mark.parametrize("radius", oracle.RADII)
def test_an_impulse_becomes_exactly_the_window(radius, shape, width):
    where = impulse_positions(radius, width)
    host = np.full((len(where), IMPULSE_H, width, 1), 0.25, np.float32)
    want = np.zeros(host.shape[:3], bool)
    for t, (y, x) in enumerate(where):
        host[t, y, x, 0] = 0.75
        for dy, dx in oracle.offsets(radius, shape):
            if 0 <= y + dy < IMPULSE_H and 0 <= x + dx < width:
                want[t, y + dy, x + dx] = True
    got = engine.depth_dilate(on_device(host), radius, shape, "bright", 0.0).cpu().numpy()
    assert np.array_equal(got == np.float32(0.75), want) and np.array_equal(got == np.float32(0.25), ~want)
    # the mirror image: a dark impulse with near = dark
    dark = engine.depth_dilate(on_device(1.0 - host), radius, shape, "dark", 0.0).cpu().numpy()
    assert np.array_equal(dark == np.float32(0.25), want) and np.array_equal(dark == np.float32(0.75), ~want)


# ---- properties that do not go through the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", oracle.RADII)
@pytest.mark.parametrize("h, w", [(17, 67), (33, 132)])
def test_threshold_zero_square_is_max_pool2d(h, w, radius):
    host = np.random.RandomState(100 * h + radius).uniform(-1.0, 1.0, (3, h, w, 1)).astype(np.float32)
    host[0] = np.round(host[0] * 8) / 8                       # ties; no zero of either sign beside the other
    host[host == 0] = np.float32(0.0)
    dev = on_device(host)
    want = F.max_pool2d(dev[..., 0].unsqueeze(1), 2 * radius + 1, stride=1, padding=radius).squeeze(1)
    assert same_bits(engine.depth_dilate(dev, radius, "square", "bright", 0.0), want)
    eroded = -F.max_pool2d(-dev[..., 0].unsqueeze(1), 2 * radius + 1, stride=1, padding=radius).squeeze(1)
    assert same_bits(engine.depth_dilate(dev, radius, "square", "dark", 0.0), eroded)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["kind"] in ("specials", "tiny") and c["near"] == "bright" and not c["off"]][:12])
def test_dark_is_the_mirror_image_of_bright(cid):
    case = case_of(cid)
    depth, _ = expected(case)
    g = oracle.gray(depth)[..., None]
    args = (case["radius"], case["shape"])
    bright = engine.depth_dilate(on_device(-g), *args, "bright", case["threshold"]).cpu().numpy()
    dark = engine.depth_dilate(on_device(g), *args, "dark", case["threshold"]).cpu().numpy()
    # the sign bit apart the same words, a NaN centre's included: both calls hand its bits on
    assert np.array_equal(dark.view(np.uint32) ^ np.uint32(0x80000000), bright.view(np.uint32))
    assert same_bits(dark, oracle.dilate(g, *args, "dark", case["threshold"]))


@pytest.mark.parametrize("h, w, c, offset", [(8, 64, 1, 0), (8, 64, 3, 0), (5, 67, 3, 0), (7, 64, 2, 0), (8, 64, 3, 1), (5, 67, 1, 0)],
                         ids=["8x64_c1", "8x64_c3", "5x67_c3", "7x64_c2", "8x64_c3_off16", "5x67_c1"])
def test_an_infinite_threshold_returns_the_gray_depth_the_other_passes_read(h, w, c, offset):
    host = np.random.RandomState(h * w + c).uniform(0.5, 1.0, (2, h, w, c)).astype(np.float32)
    depth = on_device(host, offset)
    y_temporal = engine.temporal_depth(depth, None, 1.0, INF, INF)[0].cpu().numpy()
    y_range = engine.depth_range(depth, None, 0.0, 0.0, 1.0, None, False)[0].cpu().numpy()
    for radius, shape, near in ((1, "disc", "bright"), (8, "square", "dark"), (3, "square", "bright"), (5, "disc", "dark")):
        y = engine.depth_dilate(depth, radius, shape, near, INF).cpu().numpy()
        assert y.shape == (2, h, w)
        assert np.array_equal(y.view(np.uint32), y_temporal.view(np.uint32)) and np.array_equal(y.view(np.uint32), y_range.view(np.uint32))
        assert np.array_equal(y.view(np.uint32), oracle.gray(host).view(np.uint32))


@pytest.mark.parametrize("shape", oracle.SHAPES)
@pytest.mark.parametrize("radius", oracle.RADII)
def test_a_slope_below_the_threshold_comes_back_unchanged(radius, shape):
    # gradients a per column and b per row, R (a + b) = 0.9 * 0.04: no two pixels of a window differ by the threshold
    a = b = 0.45 * 0.04 / radius
    yy, xx = np.mgrid[0:33, 0:132]
    host = (0.1 + a * xx + b * yy).astype(np.float32)[None, ..., None]
    assert float(host.max() - host.min()) > 0.04              # (the frame as a whole spans far more than the threshold)
    dev = on_device(host)
    for near in oracle.NEARS:
        assert same_bits(engine.depth_dilate(dev, radius, shape, near, 0.04), host[..., 0])
    assert not same_bits(engine.depth_dilate(dev, radius, shape, "bright", 0.0), host[..., 0])


# ---- repeatability, graph ------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits_and_every_frame_what_it_gets_alone():
    case = case_of(next(i for i in IDS if i.startswith("33x132_n3") and "specials" in i))
    depth, want = expected(case)
    dep = on_device(depth)
    args = (case["radius"], case["shape"], case["near"], case["threshold"])
    first, second = engine.depth_dilate(dep, *args), engine.depth_dilate(dep, *args)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and same_bits(first, want)
    for t in range(case["n"]):
        assert same_bits(engine.depth_dilate(dep[t:t + 1], *args), want[t:t + 1]), t


def test_one_graph_capture_and_one_replay_equal_the_eager_call():
    case = case_of(next(i for i in IDS if i.startswith("33x132_n3")))
    depth, want = expected(case)
    dep = on_device(depth)
    args = (case["radius"], case["shape"], case["near"], case["threshold"])
    eager = engine.depth_dilate(dep, *args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        engine.depth_dilate(dep, *args)                        # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # (a wait for the device inside the call would make the capture fail)
        got = engine.depth_dilate(dep, *args)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(got, eager) and same_bits(got, want)


# ---- the layers above ------------------------------------------------------------------------------------------------------------------
def test_host_tensors_in_sub_batches_equal_the_single_device_call_and_layouts_are_kept():
    case = case_of(next(i for i in IDS if i.startswith("17x67_n3_c3")))
    depth, want = expected(case)
    args = (case["radius"], case["shape"], case["near"], case["threshold"])
    on_gpu = sig.dilate_depth_edges(on_device(depth), *args)
    assert on_gpu.is_cuda and tuple(on_gpu.shape) == (3, 17, 67, 3)
    for batch_size in (1, 2, 16):
        host = sig.dilate_depth_edges(torch.tensor(depth), *args, batch_size=batch_size)
        assert not host.is_cuda and host.dtype == torch.float32 and same_bits(host, on_gpu), batch_size
    for ch in range(3):                                        # the result in every channel
        assert same_bits(on_gpu[..., ch], want)
    gray = oracle.gray(depth)
    three = sig.dilate_depth_edges(gray.copy(), *args)         # numpy in, [N,H,W] stays [N,H,W]
    assert tuple(three.shape) == (3, 17, 67) and not three.is_cuda and same_bits(three, want)
    three_dev = sig.dilate_depth_edges(on_device(gray), *args, batch_size=1)
    assert tuple(three_dev.shape) == (3, 17, 67) and three_dev.is_cuda and same_bits(three_dev, want)
    one = sig.dilate_depth_edges(torch.tensor(gray[..., None].copy()), *args, batch_size=1)
    assert tuple(one.shape) == (3, 17, 67, 1) and same_bits(one[..., 0], want)
    doubles = sig.dilate_depth_edges(torch.tensor(gray).double(), *args)   # another dtype is converted
    assert doubles.dtype == torch.float32 and same_bits(doubles, want)
    four = np.ascontiguousarray(np.concatenate([gray[..., None], depth], axis=-1))
    assert same_bits(sig.dilate_depth_edges(four, *args)[..., 3], want)    # C == 4: channel 0, y in every channel


def test_the_nodes_output():
    case = case_of(next(i for i in IDS if i.startswith("33x132_n3")))
    depth, want = expected(case)
    node = depth_dilate.StereoDepthEdgeDilate()
    (y,) = node.dilate(torch.tensor(depth), case["radius"], case["shape"], case["near"], case["threshold"], batch_size=2)
    assert tuple(y.shape) == depth.shape and not y.is_cuda and all(same_bits(y[..., ch], want) for ch in range(depth.shape[3]))
    (again,) = node.dilate(torch.tensor(depth), case["radius"], case["shape"], case["near"], case["threshold"], batch_size=2)
    assert same_bits(again, y)                                 # the node keeps no state
    defaults = node.dilate(torch.tensor(depth))[0]
    assert same_bits(defaults[..., 0], oracle.dilate(depth, 2, "disc", "bright", 0.04))


def test_a_device_tensor_from_the_guided_upsampler_keeps_its_device_and_layout():
    rng = np.random.RandomState(7)
    image = on_device(rng.uniform(0, 1, (2, 33, 132, 3)))
    low = on_device(np.round(rng.uniform(0, 1, (2, 8, 33, 3)) * 4) / 4)
    up = sig.upsample_depth_guided(image, low)
    assert up.is_cuda and tuple(up.shape) == (2, 33, 132, 3)
    y = sig.dilate_depth_edges(up)
    assert y.is_cuda and y.device == up.device and tuple(y.shape) == tuple(up.shape) and y.dtype == torch.float32
    assert same_bits(y[..., 2], oracle.dilate(up.cpu().numpy()))
    (from_node,) = depth_dilate.StereoDepthEdgeDilate().dilate(up)
    assert from_node.is_cuda and same_bits(from_node, y)


# ---- every refusal of the C entry point returns its code and leaves out untouched -------------------------------------------------------
def test_every_abi_refusal_leaves_out_untouched():
    depth = on_device(np.random.RandomState(3).uniform(0, 1, (2, 16, 64, 1)))
    out = torch.full((2, 16, 64), -7.0, dtype=torch.float32, device="cuda")
    E = _native.CS_EINVAL
    refused = [
        (dict(depth_ptr=ctypes.c_void_p(None)), E, "null pointer"), (dict(out_ptr=ctypes.c_void_p(None)), E, "null pointer"),
        (dict(n=0), E, "non-positive size"), (dict(h=-1), E, "non-positive size"), (dict(w=0), E, "non-positive size"), (dict(c=0), E, "non-positive size"),
        (dict(n=65536), _native.CS_ELIMIT, "65535 frames"), (dict(h=65536, w=32768), _native.CS_ELIMIT, "2^31 pixels"),
        (dict(radius=0), E, "radius must lie in 1..8"), (dict(radius=9), E, "radius must lie in 1..8"), (dict(radius=-2), E, "radius"),
        (dict(shape=2), E, "unknown shape"), (dict(shape=-1), E, "unknown shape"), (dict(near=2), E, "unknown near"), (dict(near=-1), E, "unknown near"),
        (dict(threshold=-0.5), E, "threshold must be >= 0"), (dict(threshold=NAN), E, "threshold must be >= 0"), (dict(threshold=-INF), E, "threshold"),
        (dict(depth_ptr=ctypes.c_void_p(depth.data_ptr() + 2)), E, "4-byte alignment"), (dict(out_ptr=ctypes.c_void_p(out.data_ptr() + 1)), E, "4-byte alignment"),
        (dict(out_ptr=ctypes.c_void_p(depth.data_ptr())), E, "must not overlap"),
        (dict(out_ptr=ctypes.c_void_p(depth.data_ptr() + depth.numel() * 4 - 4)), E, "must not overlap"),
        (dict(depth_ptr=ctypes.c_void_p(out.data_ptr() + 64)), E, "must not overlap"),
    ]
    for kw, code, text in refused:
        rc, said = native_call(depth, out, **kw)
        assert rc == code and text in said, (kw, rc, said)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    rc, said = native_call(depth, out, threshold=INF)           # what is left runs
    assert rc == _native.CS_OK and same_bits(out, depth[..., 0])


def test_the_engine_refuses_what_it_cannot_run():
    d = torch.zeros((2, 8, 8, 1), device="cuda")
    with pytest.raises(ValueError, match="device-resident"):
        engine.depth_dilate(d.cpu())
    assert tuple(engine.depth_dilate(d).shape) == (2, 8, 8)
