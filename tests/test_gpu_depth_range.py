"""The depth range clipping on the GPU (cs_depth_range through engine.depth_range, stereoimage_generation.clip_depth_range and the
StereoDepthRange node): y, the four bound vectors and the state bit for bit tools/range_oracle.py, the specification, compared as
uint32.  "Bit for bit": a NaN equals a NaN of any payload, as in the other sweeps (IEEE 754 leaves the payload an operation
hands on to the implementation).  The selection is exact, so nothing here has a tolerance."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_range as depth_range_node, depth_stabilizer, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_range_goldens as goldens   # noqa: E402
import range_oracle as oracle   # noqa: E402

pytestmark = pytest.mark.gpu
CASES = goldens.cases()
IDS = [c["id"] for c in CASES]
_cache = {}


def case_of(cid):
    return next(c for c in CASES if c["id"] == cid)


def expected(case):
    """(depth, y, lo, hi, raw_lo, raw_hi, state) of a case, computed once and shared; nothing changes them."""
    if case["id"] not in _cache:
        depth = goldens.make_input(case)
        _cache[case["id"]] = (depth,) + goldens.evaluate(case, depth)
        for a in _cache[case["id"]][:6]:
            a.setflags(write=False)
    return _cache[case["id"]]


def bits(a):
    return goldens.canonical(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def on_device(depth, offset=0):
    """The clip on the GPU; offset: floats by which its first element is off the allocation's (16-byte aligned) start."""
    flat = torch.empty(depth.size + offset, dtype=torch.float32, device="cuda")
    view = flat[offset:].view(depth.shape)
    view.copy_(torch.tensor(depth))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def run_ranks(depth, rank_lo, rank_hi, beta=1.0, cut=None, normalize=False, state=None):
    """cs_depth_range with the two ranks given as integers (engine.depth_range derives them from fractions, which cannot say
    rank_lo == rank_hi or name a rank inside a run of ties) -> what engine.depth_range returns."""
    L = _native.lib()
    n, h, w, c = depth.shape
    state = engine.RangeState(h, w, depth.device) if state is None else state
    y = torch.empty((n, h, w), dtype=torch.float32, device=depth.device)
    lo, hi, raw_lo, raw_hi = (torch.empty((n,), dtype=torch.float32, device=depth.device) for _ in range(4))
    ws, nb = engine._workspace(L.cs_depth_range_workspace_bytes(n, h, w, c), depth.device)
    engine._launch(depth.device, L.cs_depth_range, engine._ptr(depth), n, h, w, c, rank_lo, rank_hi, float(beta), int(normalize),
                   engine._opt_ptr(cut), engine._ptr(state.lo), engine._ptr(state.hi), engine._ptr(state.valid), engine._ptr(y),
                   engine._ptr(lo), engine._ptr(hi), engine._ptr(raw_lo), engine._ptr(raw_hi), engine._ptr(ws), nb)
    return y, lo, hi, raw_lo, raw_hi, state


def run(case, depth_dev, state=None, frames=slice(None)):
    """The case (or the frames of it) through the Python layer where the case names fractions, else through the C entry point."""
    cut = goldens.cut_of(case)
    cut = None if cut is None else torch.tensor(cut[frames], device="cuda")
    if case["clip"] is not None:
        return engine.depth_range(depth_dev[frames], state, case["clip"][0], case["clip"][1], case["beta"], cut, case["normalize"])
    return run_ranks(depth_dev[frames], case["rank_lo"], case["rank_hi"], case["beta"], cut, case["normalize"], state)


def check_all(got, want):
    y, lo, hi, raw_lo, raw_hi, state = got
    _, y_w, lo_w, hi_w, raw_lo_w, raw_hi_w, state_w = want
    assert all(t.dtype == torch.float32 for t in (y, lo, hi, raw_lo, raw_hi))
    assert same_bits(raw_lo, raw_lo_w) and same_bits(raw_hi, raw_hi_w), (raw_lo, raw_lo_w, raw_hi, raw_hi_w)
    assert same_bits(lo, lo_w) and same_bits(hi, hi_w), (lo, lo_w, hi, hi_w)
    assert same_bits(y, y_w)
    assert same_bits(state.lo, state_w.lo) and same_bits(state.hi, state_w.hi) and state.valid.item() == 1


# ---- every case against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_specification(case):
    want = expected(case)
    check_all(run(case, on_device(want[0], case["offset"])), want)
    g = oracle.gray(want[0])
    if case["id"].endswith("clip0"):          # clip = 0 at both ends: the minimum and the maximum of the keys
        k = oracle.key(g).reshape(case["n"], -1)
        assert np.array_equal(oracle.key(want[4]), k.min(axis=1)) and np.array_equal(oracle.key(want[5]), k.max(axis=1))
    if case["kind"] == "const" and case["normalize"]:
        assert not want[1].any() and np.array_equal(want[2], want[3])
    if case["kind"] == "nan":                 # NaN pixels pass through y
        assert np.isnan(g).sum() == 8 * case["n"] and np.isnan(want[1][np.isnan(g)]).all()
        assert case["normalize"] or np.array_equal(np.isnan(want[1]), np.isnan(g))


def test_the_oracle_here_is_the_one_the_fixture_pins():
    with np.load(os.path.join(ROOT, "tests", "golden", "depth_range.npz")) as z:
        meta = {c["id"]: c for c in json.loads(str(z["meta"]))["cases"]}
        for case in CASES[::5]:
            _, y, lo, hi, raw_lo, raw_hi, state = expected(case)
            assert goldens.digest(goldens.canonical(y)) == meta[case["id"]]["y_sha256"]
            assert np.array_equal(z[case["id"] + "/lo"], goldens.canonical(lo)) and np.array_equal(z[case["id"] + "/raw_hi"], goldens.canonical(raw_hi))


# ---- every frame alone, carry, graph -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["129x256_n3_c3_noise", "7x64_n3_c1_noise", "5x7_n3_c2_noise"])
def test_every_frame_of_a_batch_gets_what_it_gets_alone(cid):
    case = case_of(cid)
    want = expected(case)
    dev = on_device(want[0])
    whole = run(case, dev)
    assert len(set(bits(whole[3]).tolist())) == case["n"]   # (the frames' distributions differ)
    for t in range(case["n"]):
        alone = run(case, dev, frames=slice(t, t + 1))
        assert same_bits(alone[0], whole[0][t:t + 1]) and all(same_bits(a, b[t:t + 1]) for a, b in zip(alone[1:5], whole[1:5]))


@pytest.mark.parametrize("cid", ["5x67_n9_c1_noise_beta0", "5x67_n9_c3_noise_beta025", "5x67_n9_c1_noise_beta1", "5x67_n9_c3_noise_nocut",
                                 "129x256_n9_c1_noise_beta025_norm", "5x7_n9_c1_huge_nonfinite"])
def test_a_batch_in_pieces_is_the_batch(cid):
    case = case_of(cid)
    want = expected(case)
    dev = on_device(want[0])
    whole = run(case, dev)
    check_all(whole, want)
    for split in ([4, 5], [1] * 9):   # (4 + 5: the cut at frame 4 is the second call's first frame)
        state, parts, b0 = None, [], 0
        for k in split:
            *five, state = run(case, dev, state, slice(b0, b0 + k))
            parts.append(five)
            b0 += k
        for i in range(5):
            assert same_bits(torch.cat([p[i] for p in parts]), whole[i]), (split, i)
        assert same_bits(state.lo, whole[5].lo) and same_bits(state.hi, whole[5].hi)
    if case["cut_at"] == [4]:   # the cut restarts the bounds; without it frame 4 is smoothed (beta < 1)
        assert same_bits(whole[1][4], whole[3][4]) and same_bits(whole[2][4], whole[4][4])
        if case["beta"] == 0.0:
            assert same_bits(whole[1][:4], whole[3][:1].expand(4)) and same_bits(whole[1][4:], whole[3][4:5].expand(5))
    if cid.endswith("nonfinite"):   # raw - prev overflowed on frames 1..5: the raw bound was taken; from frame 6 on s is finite again
        assert same_bits(whole[1][:6], whole[3][:6]) and same_bits(whole[2][:6], whole[4][:6])
        assert not (bits(whole[1][6:]) == bits(whole[3][6:])).any()


def test_the_result_is_the_same_on_the_4_byte_path():
    case = case_of("129x256_n3_c3_noise")
    want = expected(case)
    a, b = run(case, on_device(want[0])), run(case, on_device(want[0], 1))
    assert all(same_bits(x, y) for x, y in zip(a[:5], b[:5]))


def test_one_capture_and_one_replay_equal_the_eager_call():
    case = case_of("5x67_n9_c3_noise_beta025")
    want = expected(case)
    dev = on_device(want[0])
    cut = torch.tensor(goldens.cut_of(case)[4:], device="cuda")
    args = (case["clip"][0], case["clip"][1], case["beta"], cut, case["normalize"])
    first = run(case, dev, frames=slice(0, 4))
    eager = engine.depth_range(dev[4:], first[5].clone(), *args)
    state = first[5].clone()
    before = state.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        engine.depth_range(dev[4:], state, *args)   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)

    def put_back():
        state.lo.copy_(before.lo), state.hi.copy_(before.hi), state.valid.copy_(before.valid)
    put_back()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a wait for the device inside the call would make the capture fail)
        got = engine.depth_range(dev[4:], state, *args)
    put_back()
    graph.replay()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(got[:5], eager[:5]))
    assert same_bits(state.lo, eager[5].lo) and same_bits(state.hi, eager[5].hi) and same_bits(got[0], want[1][4:])


# ---- refusals of the engine that need a device tensor ----------------------------------------------------------------------------------
def test_the_engine_refuses_what_it_cannot_run():
    d = torch.zeros((2, 4, 4, 1), device="cuda")
    for bad, text in ((d[..., 0], "N,H,W,C"), (d.double(), "float32"), (d.cpu(), "device-resident"), (d.expand(2, 4, 4, 3), "contiguous")):
        with pytest.raises(ValueError, match=text):
            engine.depth_range(bad)
    *_, state = engine.depth_range(d)
    with pytest.raises(ValueError, match="state is for frames of"):
        engine.depth_range(torch.zeros((2, 4, 8, 1), device="cuda"), state)
    with pytest.raises(ValueError, match="RangeState"):
        engine.depth_range(d, state=(1, 2))
    with pytest.raises(ValueError, match="same device"):
        engine.depth_range(d, cut=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(_native.NativeError) as e:   # the C entry point's own refusal of ranks the Python layer never derives
        run_ranks(d, 3, 2)
    assert e.value.code == _native.CS_EINVAL and "rank_lo <= rank_hi" in str(e.value)


# ---- through the layers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["5x67_n9_c3_noise_beta025", "5x67_n9_c1_noise_beta025"])
def test_clip_depth_range_on_host_tensors_in_sub_batches(cid):
    case = case_of(cid)
    want = expected(case)
    kw = dict(clip_low=case["clip"][0], clip_high=case["clip"][1], beta=case["beta"], normalize=case["normalize"])
    cuts = [torch.tensor(goldens.cut_of(case)[:3]), torch.tensor(goldens.cut_of(case)[3:])]   # (as stabilize_depth hands them out)
    dev_out = run(case, on_device(want[0]))
    host = torch.from_numpy(want[0].copy())
    bounds = []
    y, state = sig.clip_depth_range(host, batch_size=4, cuts=cuts, bounds=bounds, **kw)   # (4 + 4 + 1: the cut on a sub-batch boundary)
    assert not y.is_cuda and y.shape == host.shape and state.lo.is_cuda and len(bounds) == 3
    for ch in range(case["c"]):
        assert same_bits(y[..., ch], dev_out[0])
    for i in range(4):
        assert same_bits(torch.cat([b[i] for b in bounds]), dev_out[1 + i])
    if case["c"] == 1:   # [N,H,W] in, [N,H,W] out; a device tensor stays on the device
        y3, _ = sig.clip_depth_range(host[..., 0], batch_size=4, cuts=cuts, **kw)
        assert y3.shape == host.shape[:3] and same_bits(y3, dev_out[0])
        yd, _ = sig.clip_depth_range(host.cuda(), cuts=cuts, **kw)
        assert yd.is_cuda and same_bits(yd[..., 0], dev_out[0])


def test_the_node_behind_the_stabilizer_on_a_six_frame_clip():
    """StereoDepthStabilizer -> StereoDepthRange: the stabiliser's scene-cut mask restarts the bounds; the node carries its state
    between executions; its output is the oracle's on the stabiliser's output."""
    rng = np.random.RandomState(11)
    n, h, w = 6, 20, 36
    clip = (rng.uniform(0.3, 0.58, (1, h, w, 1)) + rng.uniform(0.0, 0.02, (n, h, w, 1))).astype(np.float32)
    clip[3:] += np.float32(0.3)                       # a hard cut at frame 3
    clip[:, 0, 1] = 0.0                               # a speck and a specular hit in every frame
    clip[:, 5, 7] = 1.0
    host = torch.from_numpy(np.repeat(clip, 3, axis=3))
    steady, mask = depth_stabilizer.StereoDepthStabilizer().stabilize(host, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08)
    assert mask[:, 0, 0].tolist() == [1.0, 0, 0, 1.0, 0, 0]
    kw = dict(clip_low=0.01, clip_high=0.01, smoothing=0.25, normalize=True, batch_size=4)
    assert depth_range_node.NODE_CLASS_MAPPINGS == {"StereoDepthRange": depth_range_node.StereoDepthRange}
    whole, = depth_range_node.StereoDepthRange().clip(steady, mask, **kw)
    assert whole.shape == host.shape and not whole.is_cuda
    ranks = oracle.ranks_of(0.01, 0.01, h * w)
    y_w, lo_w, hi_w, raw_lo_w, raw_hi_w, _ = oracle.depth_range(steady.numpy(), None, *ranks, 0.25, mask[:, 0, 0].numpy().astype(np.int32), True)
    for ch in range(3):
        assert same_bits(whole[..., ch], y_w)
    assert same_bits(lo_w[3], raw_lo_w[3]) and not same_bits(lo_w[4], raw_lo_w[4])   # restarted at the cut, smoothed behind it
    assert whole.min() == 0.0 and whole.max() == 1.0 and 0.25 < float(lo_w[0]) < 0.35 and 0.55 < float(hi_w[0]) < 0.65   # the outliers do not rule
    node = depth_range_node.StereoDepthRange()
    a, = node.clip(steady[:2], mask[:2], **kw)
    b, = node.clip(steady[2:], mask[2:], **kw)
    assert same_bits(torch.cat([a, b]), whole)
    b_reset, = node.clip(steady[2:], mask[2:], reset=True, **kw)
    assert not same_bits(b_reset, b) and same_bits(b_reset[1:], b[1:])   # frame 2 restarts; the cut at frame 3 restarts either way
    node.clip(steady[:2, :16], None, **kw)   # another frame size starts a new clip too, and the mask is optional
    assert node._state.shape == (16, w)
    on_gpu, = depth_range_node.StereoDepthRange().clip(steady.cuda(), mask.cuda(), **kw)
    assert on_gpu.is_cuda and same_bits(on_gpu, whole)
