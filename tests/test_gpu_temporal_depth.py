"""The temporal depth filter on the GPU (cs_temporal_depth through engine.temporal_depth, stereoimage_generation.stabilize_depth
and the StereoDepthStabilizer node): y and the state bit for bit tools/temporal_oracle.py, the specification; cut equal; m within
the bound its summation order implies against the float64 value.  "Bit for bit": a NaN equals a NaN of any payload, as in the
other sweeps (IEEE 754 leaves the payload an operation hands on to the implementation).

The bound for m (cs_temporal.hip): every |g_t - g_{t-1}| is one float32 subtraction (1 rounding); a lane adds 64
of them one after the other (64); the workgroup's 256 sums meet in a pairwise tree of depth 8 (8); one thread adds the frame's P
partial sums, P = ceil(h * w / 16384), in index order (P - 1); the count h * w is converted to float32 (1) and divides the sum
(1).  All terms are non-negative, so no cancellation: each term of the sum passes through at most K = 75 + P - 1 roundings of
relative size u = 2^-24, and |m - m64| <= m64 * K u / (1 - K u) (Higham, Accuracy and Stability, lemma 3.1), plus half the
smallest subnormal.  Nothing in it is taken from the kernel's output.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import GenerateStereo, depth_stabilizer, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_temporal_goldens as goldens   # noqa: E402
import temporal_oracle as oracle   # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = goldens.cases()
IDS = [c["id"] for c in CASES]
_cache = {}


def m_bound(m64, h, w):
    k = 1 + 64 + 8 + (-(-h * w // 16384) - 1) + 1 + 1
    return np.abs(m64) * (k * U / (1 - k * U)) + 2.0 ** -149


def expected(case):
    """(depth, y, m64, cut, state, still) of a case, computed once and shared; nothing changes them."""
    if case["id"] not in _cache:
        depth = goldens.make_input(case)
        _cache[case["id"]] = (depth,) + goldens.evaluate(case, depth)
        for a in _cache[case["id"]][:4]:
            a.setflags(write=False)
    return _cache[case["id"]]


def bits(a):
    """int32 view with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
    v = a.view(np.int32).copy()
    v[np.isnan(a)] = 0x7fc00000
    return v


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def on_device(depth, offset=0):
    """The clip on the GPU; offset: floats by which its first element is off the allocation's (16-byte aligned) start."""
    flat = torch.empty(depth.size + offset, dtype=torch.float32, device="cuda")
    view = flat[offset:].view(depth.shape)
    view.copy_(torch.tensor(depth))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def run(case, depth_dev, state=None):
    return engine.temporal_depth(depth_dev, state, case["alpha"], case["motion_threshold"], case["cut_threshold"])


def check_m(m, m64, case):
    m = m.cpu().numpy().astype(np.float64)
    fin = np.isfinite(m64)
    print(case["id"], "m error / bound:", np.max(np.abs(m[fin] - m64[fin]) / m_bound(m64[fin], case["h"], case["w"]), initial=0.0))
    assert np.all(np.abs(m[fin] - m64[fin]) <= m_bound(m64[fin], case["h"], case["w"])), (m, m64)
    assert np.array_equal(np.isnan(m), np.isnan(m64)) and np.array_equal(m[~fin & ~np.isnan(m64)], m64[~fin & ~np.isnan(m64)])


def check_all(got, want, case):
    y, m, cut, state = got
    _, y_w, m_w, cut_w, state_w, _ = want
    assert y.dtype == torch.float32 and m.dtype == torch.float32 and cut.dtype == torch.int32
    assert np.array_equal(cut.cpu().numpy(), cut_w)
    check_m(m, m_w, case)
    assert same_bits(y, y_w)
    assert same_bits(state.prev_raw, state_w.prev_raw) and same_bits(state.prev, state_w.prev) and state.valid.item() == 1


# ---- every case against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_specification(case):
    want = expected(case)
    dev = on_device(want[0], case["offset"])
    check_all(run(case, dev), want, case)
    partials = -(-case["h"] * case["w"] // 16384)
    if case["id"].endswith("_p257"):     # a second trip of the 256 threads that stage a frame's partial sums
        assert partials > 256 and want[3].tolist() == [1, 0] and want[5][1].any() and not want[5][1].all()
    if case["id"].endswith("_p1025"):    # a second stage of 1024 partial sums through the finalising kernel's LDS array
        assert partials > 1024 and want[3].tolist() == [1, 1] and want[2][1] > 0.4
    if partials > 2:
        del _cache[case["id"]]           # (hundreds of megabytes: not kept for the rest of the run)
    if (not case["special"] and case["n"] == 9 and case["w"] >= 32 and case["motion_threshold"] == 0.1
            and case["cut_threshold"] == 0.08):
        still = want[5]
        assert still[2].any() and not still[2].all()   # both branches of the motion test inside one frame


def test_the_oracle_here_is_the_one_the_fixture_pins():
    with np.load(os.path.join(ROOT, "tests", "golden", "temporal_depth.npz")) as z:
        meta = {c["id"]: c for c in json.loads(str(z["meta"]))["cases"]}
        for case in [c for c in CASES if c["h"] < 1000][::7]:
            _, y, m, cut, state, _ = expected(case)
            assert goldens.digest(y) == meta[case["id"]]["y_sha256"]
            assert goldens.digest(state.prev_raw, state.prev) == meta[case["id"]]["state_sha256"]
            assert np.array_equal(z[case["id"] + "/m"], m) and np.array_equal(z[case["id"] + "/cut"], cut)


# ---- carry, determinism, graph ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["33x131_n9_c1", "33x131_n9_c3", "129x128_n9_c1", "5x67_n9_c3", "7x64_n9_c2", "7x64_n9_c1_nan"])
def test_a_batch_in_pieces_is_the_batch(cid):
    case = next(c for c in CASES if c["id"] == cid)
    want = expected(case)
    dev = on_device(want[0])
    whole = run(case, dev)
    check_all(whole, want, case)
    for split in ([4, 5], [1] * 9):   # (4 + 5: the cut at frame 4 is the second call's first frame and needs prev_raw from the state)
        state, ys, ms, cuts, b0 = None, [], [], [], 0
        for k in split:
            y, m, cut, state = run(case, dev[b0:b0 + k], state)
            ys.append(y), ms.append(m), cuts.append(cut)
            b0 += k
        assert same_bits(torch.cat(ys), whole[0]) and same_bits(torch.cat(ms), whole[1]) and torch.equal(torch.cat(cuts), whole[2])
        assert same_bits(state.prev_raw, whole[3].prev_raw) and same_bits(state.prev, whole[3].prev)
    if case["cut_at"] == 4:
        assert whole[2].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0]


def test_m_is_the_same_on_the_4_byte_path():
    """The order of the sum depends on h * w alone: the same clip 4 bytes off the 16-byte grid gives the same m, y and state."""
    case = next(c for c in CASES if c["id"] == "129x128_n9_c3")
    want = expected(case)
    a, b = run(case, on_device(want[0])), run(case, on_device(want[0], 1))
    assert same_bits(a[1], b[1]) and same_bits(a[0], b[0]) and torch.equal(a[2], b[2]) and same_bits(a[3].prev, b[3].prev)


def test_the_same_call_twice_gives_the_same_m():
    case = next(c for c in CASES if c["id"] == "129x128_n9_c1")
    dev = on_device(expected(case)[0])
    a, b = run(case, dev), run(case, dev)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and same_bits(a[0], b[0])


def test_one_capture_and_one_replay_equal_the_eager_call():
    case = next(c for c in CASES if c["id"] == "33x131_n9_c3")
    want = expected(case)
    dev = on_device(want[0])
    first = run(case, dev[:4])
    eager = run(case, dev[4:], first[3].clone())
    state = first[3].clone()
    before = state.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(case, dev[4:], state)   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)

    def put_back():
        state.prev_raw.copy_(before.prev_raw), state.prev.copy_(before.prev), state.valid.copy_(before.valid)
    put_back()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a wait for the device inside the call would make the capture fail)
        y, m, cut, _ = run(case, dev[4:], state)
    put_back()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(y, eager[0]) and same_bits(m, eager[1]) and torch.equal(cut, eager[2])
    assert same_bits(state.prev, eager[3].prev) and same_bits(state.prev_raw, eager[3].prev_raw)
    assert same_bits(y, want[1][4:])


# ---- refusals of the engine ---------------------------------------------------------------------------------------------------------
def test_the_engine_refuses_what_it_cannot_run():
    d = torch.zeros((2, 4, 4, 1), device="cuda")
    for bad, text in ((d[..., 0], "N,H,W,C"), (d.double(), "float32"), (d.cpu(), "device-resident"), (d.expand(2, 4, 4, 3), "contiguous")):
        with pytest.raises(ValueError, match=text):
            engine.temporal_depth(bad)
    _, _, _, state = engine.temporal_depth(d)
    with pytest.raises(ValueError, match="state is for frames of"):
        engine.temporal_depth(torch.zeros((2, 4, 8, 1), device="cuda"), state)
    with pytest.raises(ValueError, match="TemporalState"):
        engine.temporal_depth(d, state=(1, 2))
    for kw in (dict(alpha=1.5), dict(motion_threshold=-1.0), dict(cut_threshold=float("nan"))):
        with pytest.raises(engine._native.NativeError) as e:
            engine.temporal_depth(d, **kw)
        assert e.value.code == engine._native.CS_EINVAL


# ---- through the layers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["33x131_n9_c3", "33x131_n9_c1"])
def test_stabilize_depth_on_host_tensors_in_sub_batches(cid):
    case = next(c for c in CASES if c["id"] == cid)
    want = expected(case)
    kw = dict(alpha=case["alpha"], motion_threshold=case["motion_threshold"], cut_threshold=case["cut_threshold"])
    y_dev = run(case, on_device(want[0]))[0]
    host = torch.from_numpy(want[0].copy())
    y, state = sig.stabilize_depth(host, batch_size=4, **kw)
    assert not y.is_cuda and y.shape == host.shape and state.prev.is_cuda
    for ch in range(case["c"]):
        assert same_bits(y[..., ch], y_dev)
    if case["c"] == 1:   # [N,H,W] in, [N,H,W] out; a device tensor stays on the device
        y3, _ = sig.stabilize_depth(host[..., 0], batch_size=4, **kw)
        assert y3.shape == host.shape[:3] and same_bits(y3, y_dev)
        yd, _ = sig.stabilize_depth(host.cuda(), **kw)
        assert yd.is_cuda and same_bits(yd[..., 0], y_dev)


def test_the_node_carries_its_state_between_executions_and_reset_clears_it():
    case = next(c for c in CASES if c["id"] == "33x131_n9_c3")
    want = expected(case)
    host = torch.from_numpy(want[0].copy())
    kw = dict(alpha=case["alpha"], motion_threshold=case["motion_threshold"], cut_threshold=case["cut_threshold"], batch_size=4)
    assert depth_stabilizer.NODE_CLASS_MAPPINGS == {"StereoDepthStabilizer": depth_stabilizer.StereoDepthStabilizer}
    assert depth_stabilizer.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDepthStabilizer": "Stereo Depth Stabilizer"}
    whole, mask = depth_stabilizer.StereoDepthStabilizer().stabilize(host, **kw)
    assert whole.shape == host.shape and mask.shape == host.shape[:3] and not whole.is_cuda
    assert same_bits(whole[..., 0], want[1]) and same_bits(whole[..., 2], want[1])
    assert torch.equal(mask[:, 0, 0], torch.tensor(want[3]).float()) and torch.equal(mask, mask[:, :1, :1].expand_as(mask))
    node = depth_stabilizer.StereoDepthStabilizer()
    a, ma = node.stabilize(host[:3], **kw)
    b, mb = node.stabilize(host[3:], **kw)
    assert same_bits(torch.cat([a, b]), whole) and torch.equal(torch.cat([ma, mb]), mask)
    node = depth_stabilizer.StereoDepthStabilizer()
    a, _ = node.stabilize(host[:3], **kw)
    b, mb = node.stabilize(host[3:], reset=True, **kw)
    assert not same_bits(torch.cat([a, b]), whole) and mb[0, 0, 0] == 1 and same_bits(b[0, ..., 0], oracle.gray(want[0])[3])
    # the widgets' largest threshold stands for +inf: no cut but the clip's first frame, although frame 4 is a hard cut
    _, never = depth_stabilizer.StereoDepthStabilizer().stabilize(host, **dict(kw, cut_threshold=depth_stabilizer.NEVER))
    assert never[:, 0, 0].tolist() == [1.0] + [0.0] * 8 and mask[:, 0, 0].tolist() == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 0]
    # another frame size starts a new clip too
    node.stabilize(host[:2, :16], **kw)
    assert node._state.shape == (16, 131)


def test_the_nodes_output_feeds_the_stereo_node():
    """Plumbing, not a quality claim: the filtered depth runs through StereoImageNode.generate and gives another picture than the
    flickering depth."""
    rng = np.random.RandomState(5)
    n, h, w = 4, 48, 96
    base = np.linspace(0, 1, w, dtype=np.float32)[None, None, :, None] * np.ones((n, h, 1, 3), np.float32)
    flicker = base * 0.8 + rng.uniform(0, 0.06, (n, h, w, 1)).astype(np.float32)
    image = torch.from_numpy(rng.randint(0, 256, (n, h, w, 3)).astype(np.float32) / np.float32(255.0)).cuda()
    depth = torch.from_numpy(np.ascontiguousarray(flicker)).cuda()
    steady, _ = depth_stabilizer.StereoDepthStabilizer().stabilize(depth, alpha=0.2, motion_threshold=0.1, cut_threshold=0.08)
    assert steady.is_cuda and steady.shape == depth.shape and not torch.equal(steady, depth)
    args = dict(divergence=4.5, separation=0.0, modes="left-right", stereo_balance=0.0, convergence_point=0.5, stereo_offset_exponent=2.0,
                fill_technique="Fill - Polylines Soft", depth_blur_edge_threshold=20.0, depth_blur_strength=20.0, depth_map_blur=False)
    stereo_node = GenerateStereo.StereoImageNode()
    out_steady = stereo_node.generate(image, steady, **args)[0]
    out_flicker = stereo_node.generate(image, depth, **args)[0]
    assert out_steady.shape == out_flicker.shape == (n, h, 2 * w, 3) and torch.isfinite(out_steady).all()
    assert not torch.equal(out_steady, out_flicker)
