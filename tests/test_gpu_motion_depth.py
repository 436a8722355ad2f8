"""The motion-compensated temporal depth filter on the GPU (cs_motion_depth through engine.motion_depth,
stereoimage_generation.stabilize_depth_motion and the StereoDepthStabilizerMotion node): vectors, SADs, matched flags, y, cut and
the state bit for bit tools/motion_oracle.py, the specification; m within the bound tests/test_gpu_temporal_depth.py derives for
the same summation (the statistic's kernels are the same ones, cs_temporalstat.h).  "Bit for bit": a NaN equals a NaN of any payload.

The test that fails without the feature by more than a missing name is test_moving_content_is_filtered: on a translating scene
with depth noise the pass blends more pixels than engine.temporal_depth does."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_stabilizer_motion, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_motion_goldens as goldens   # noqa: E402
import motion_oracle as oracle   # noqa: E402
import temporal_oracle   # noqa: E402

_spec = importlib.util.spec_from_file_location("_temporal_gpu_tests", os.path.join(ROOT, "tests", "test_gpu_temporal_depth.py"))
_temporal_tests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_temporal_tests)
m_bound, bits, same_bits, on_device = _temporal_tests.m_bound, _temporal_tests.bits, _temporal_tests.same_bits, _temporal_tests.on_device

pytestmark = pytest.mark.gpu
CASES = goldens.cases()
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
_cache = {}


def expected(case):
    """(depth, guide, y, m64, cut, state, vec, sad, matched, blended) of a case, computed once and shared; nothing changes them."""
    if case["id"] not in _cache:
        depth, guide = goldens.make_input(case)
        _cache[case["id"]] = (depth, guide) + goldens.evaluate(case, depth, guide)
        for a in _cache[case["id"]]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[case["id"]]


def run(case, depth_dev, guide_dev, state=None):
    return engine.motion_depth_detail(depth_dev, guide_dev, state, *goldens.params(case))


def check_m(m, m64, case):
    m = m.cpu().numpy().astype(np.float64)
    fin = np.isfinite(m64)
    print(case["id"], "m error / bound:", np.max(np.abs(m[fin] - m64[fin]) / m_bound(m64[fin], case["h"], case["w"]), initial=0.0))
    assert np.all(np.abs(m[fin] - m64[fin]) <= m_bound(m64[fin], case["h"], case["w"])), (m, m64)
    assert np.array_equal(np.isnan(m), np.isnan(m64))


def check_state(state, want):
    assert same_bits(state.prev_raw, want.prev_raw) and same_bits(state.prev, want.prev) and state.valid.item() == 1
    assert state.prev_luma.dtype == torch.uint8 and np.array_equal(state.prev_luma.cpu().numpy(), want.prev_luma)


def check_all(got, want, case):
    y, m, cut, state, vec, matched, sad = got
    _, _, y_w, m_w, cut_w, state_w, vec_w, sad_w, matched_w, _ = want
    assert (y.dtype, m.dtype, cut.dtype, vec.dtype, matched.dtype, sad.dtype) == (torch.float32, torch.float32, torch.int32, torch.int8,
                                                                                 torch.uint8, torch.int32)
    assert np.array_equal(vec.cpu().numpy(), vec_w), np.argwhere(vec.cpu().numpy() != vec_w)[:4]
    assert np.array_equal(sad.cpu().numpy(), sad_w) and np.array_equal(matched.cpu().numpy(), matched_w)
    assert np.array_equal(cut.cpu().numpy(), cut_w)
    check_m(m, m_w, case)
    assert same_bits(y, y_w)
    check_state(state, state_w)


# ---- every case against the specification ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_specification(case):
    want = expected(case)
    check_all(run(case, on_device(want[0], case["offset"]), on_device(want[1])), want, case)
    if case["special"]:
        lum = oracle.luma(want[1])
        assert lum[2, 20, 9] == 0 and np.isnan(want[2]).any()               # a NaN guide pixel has code 0; NaN depth reaches y


def test_search_range_0_and_match_threshold_255_is_temporal_depth():
    for cid in ("48x80_c1_s0_degenerate", "50x70_c3_s7"):
        case = BY_ID[cid]
        depth, guide = expected(case)[:2]
        a, mt, ct = case["alpha"], case["motion_threshold"], case["cut_threshold"]
        y, m, cut, state, vec, matched = engine.motion_depth(on_device(depth), on_device(guide), None, a, mt, ct, 0, case["smoothness"], 255)
        y_t, m_t, cut_t, state_t = engine.temporal_depth(on_device(depth), None, a, mt, ct)
        assert same_bits(y, y_t) and same_bits(m, m_t) and torch.equal(cut, cut_t)
        assert same_bits(state.prev_raw, state_t.prev_raw) and same_bits(state.prev, state_t.prev)
        assert not vec.any() and matched.all()


@pytest.mark.parametrize("cid", ["48x80_c1_s7_cut", "50x70_c3_s7", "17x33_c1_s7"])
def test_two_calls_equal_one(cid):
    case = BY_ID[cid]
    want = expected(case)
    depth, guide = on_device(want[0]), on_device(want[1])
    first = run(case, depth[:2].contiguous(), guide[:2].contiguous())
    second = run(case, depth[2:].contiguous(), guide[2:].contiguous(), first[3].clone())
    joined = [torch.cat([first[i], second[i]]) for i in (0, 1, 2)] + [second[3]] + [torch.cat([first[i], second[i]]) for i in (4, 5, 6)]
    check_all(joined, want, case)
    one = run(case, depth[2:3].contiguous(), guide[2:3].contiguous(), first[3])   # a call of one frame reads the state's y through its copy
    assert same_bits(one[0][0], want[2][2]) and np.array_equal(one[4][0].cpu().numpy(), want[6][2])


def test_two_runs_are_bit_identical():
    case = BY_ID["130x258_c1_s16"]
    want = expected(case)
    depth, guide = on_device(want[0]), on_device(want[1])
    a, b = run(case, depth, guide), run(case, depth, guide)
    for i in (0, 1, 2, 4, 5, 6):
        assert torch.equal(a[i].view(torch.uint8), b[i].view(torch.uint8)), i


def test_buffers_off_the_16_byte_grid():
    """depth, guide and out one float off the grid (the entry point itself: engine.motion_depth allocates an aligned out)."""
    case = BY_ID["48x80_c1_s7_offgrid"]
    want = expected(case)
    n, h, w, c = want[0].shape
    depth, guide = on_device(want[0], 1), on_device(want[1], 1)
    out = torch.empty(n * h * w + 1, dtype=torch.float32, device="cuda")[1:].view(n, h, w)
    assert depth.data_ptr() % 16 == 4 and guide.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    state = engine.MotionState(h, w, depth.device)
    m, cut = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    hb, wb = -(-h // 16), -(-w // 16)
    vec = torch.empty((n, hb, wb, 2), dtype=torch.int8, device="cuda")
    sad = torch.empty((n, hb, wb), dtype=torch.int32, device="cuda")
    matched = torch.empty((n, hb, wb), dtype=torch.uint8, device="cuda")
    L = _native.lib()
    a, mt, ct, S, lam, thr = goldens.params(case)
    ws, nb = engine._workspace(L.cs_motion_depth_workspace_bytes(n, h, w, c, S), depth.device)
    P = engine._ptr
    engine._launch(depth.device, L.cs_motion_depth, P(depth), P(guide), n, h, w, c, a, mt, ct, S, lam, thr, P(state.prev_raw), P(state.prev),
                   P(state.prev_luma), P(state.valid), P(out), P(m), P(cut), P(vec), P(sad), P(matched), P(ws), nb)
    check_all((out, m, cut, state, vec, matched, sad), want, case)


def test_a_captured_call_replays_to_the_eager_result():
    case = BY_ID["50x70_c3_s7"]
    want = expected(case)
    depth, guide = on_device(want[0]), on_device(want[1])
    state = engine.MotionState(case["h"], case["w"], depth.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(case, depth, guide, state.clone())   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a wait for the device inside the call would make the capture fail)
        got = run(case, depth, guide, state)
    state.valid.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check_all(got, want, case)


# ---- the module function and the node, on an image at another size than the depth (the pil_resize path) ----------------------------
def test_the_module_function_and_the_node_resize_the_image():
    rng = np.random.RandomState(77)
    n, h, w = 3, 24, 40
    big = rng.randint(0, 256, (1, 2 * h + 16, 2 * w + 16, 3)).astype(np.float32) / np.float32(255.0)
    big = np.kron(big[:, ::4, ::4], np.ones((1, 4, 4, 1), np.float32))[:, :2 * h + 16, :2 * w + 16]   # 4 x 4 patches survive the resize
    image = np.ascontiguousarray(np.concatenate([big[:, 2 * t:2 * t + 2 * h, 4 * t:4 * t + 2 * w] for t in range(n)]))
    depth = (rng.randint(0, 256, (n, h, w)).astype(np.float32) / np.float32(255.0)) * np.float32(0.3)
    small = engine.pil_resize(torch.tensor(image).cuda(), (w, h), f32="nhwc", codes=True)
    assert np.array_equal(oracle.guided_oracle.code(small[1].cpu().numpy()), small[0].cpu().numpy())   # codes / 255 come back as the codes
    want = oracle.motion_depth(depth[..., None], small[1].cpu().numpy(), None, 0.5, 0.1, 0.3, 8, 0, 12)
    assert want[4][1:].any() and want[7].any()
    for d, img in ((torch.tensor(depth), torch.tensor(image)), (torch.tensor(depth).cuda(), torch.tensor(image).cuda())):
        cuts, unmatched = [], []
        y, state = sig.stabilize_depth_motion(d, img, None, 0.5, 0.1, 0.3, 8, 0, 12, batch_size=2, cuts=cuts, unmatched=unmatched)
        assert y.device == d.device and same_bits(y, want[0]) and isinstance(state, engine.MotionState)
        assert np.array_equal(torch.cat(cuts).cpu().numpy(), want[2]) and np.array_equal(torch.cat(unmatched).cpu().numpy(), 1 - want[6])
        check_state(state, want[3])
    node = depth_stabilizer_motion.StereoDepthStabilizerMotion()
    d3 = torch.tensor(np.repeat(depth[..., None], 3, axis=-1))
    g3 = temporal_oracle.gray(d3.numpy())
    want3 = oracle.motion_depth(d3.numpy(), small[1].cpu().numpy(), None, 0.5, 0.1, 0.3, 8, 0, 12)
    y1, cut1, un1 = node.stabilize(d3[:2], torch.tensor(image[:2]), 0.5, 0.1, 0.3, 8, 0, 12, batch_size=1)
    y2, cut2, un2 = node.stabilize(d3[2:], torch.tensor(image[2:]), 0.5, 0.1, 0.3, 8, 0, 12)       # the instance carries the clip on
    y = torch.cat([y1, y2])
    assert tuple(y.shape) == (n, h, w, 3) and same_bits(y[..., 0], want3[0]) and same_bits(y[..., 2], want3[0]) and g3.shape == (n, h, w)
    assert torch.cat([cut1, cut2])[:, 0, 0].tolist() == want3[2].tolist() and tuple(un1.shape) == (2, h, w)
    un = np.repeat(np.repeat(1 - want3[6], 16, axis=1), 16, axis=2)[:, :h, :w]
    assert np.array_equal(torch.cat([un1, un2]).numpy(), un.astype(np.float32))


# ---- what the pass is for -----------------------------------------------------------------------------------------------------------
def blended_pixels(depth, y, cut, vec, matched, motion_threshold):
    """The pixels that took the blend, from a pass's own outputs (numpy): not a cut, a matched block, |g - q| < motion_threshold."""
    g = temporal_oracle.gray(depth)
    out = np.zeros(g.shape, bool)
    with np.errstate(invalid="ignore"):
        for t in range(1, g.shape[0]):
            ok = np.repeat(np.repeat(matched[t] != 0, 16, axis=0), 16, axis=1)[:g.shape[1], :g.shape[2]]
            out[t] = (cut[t] == 0) & ok & (np.abs(g[t] - oracle.gather(y[t - 1], vec[t])) < np.float32(motion_threshold))
    return out


def test_moving_content_is_filtered():
    """A scene that translates by (3, -2) pixels per frame, its depth with +-0.01 of noise per frame: the plain filter sees
    most pixels as moved and passes them unfiltered; the motion-compensated one follows them and blends them."""
    case = BY_ID["96x128_c1_s8_scene"]
    depth, guide, y_w, m_w, cut_w, state_w, vec_w, sad_w, matched_w, blended_w = expected(case)
    a, mt, ct = case["alpha"], case["motion_threshold"], case["cut_threshold"]
    plain = temporal_oracle.temporal_depth(depth, None, a, mt, ct)
    assert blended_w.sum() > 2 * plain[4].sum() > 0 and not plain[2][1:].any()   # on the CPU first, with both oracles
    got = run(case, on_device(depth), on_device(guide))
    check_all(got, expected(case), case)
    y, m, cut, state, vec, matched, sad = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    mine = blended_pixels(depth, y, cut, vec, matched, mt)
    assert np.array_equal(mine, blended_w) and mine.sum() == blended_w.sum()
    y_t, m_t, cut_t, _ = engine.temporal_depth(on_device(depth), None, a, mt, ct)
    zero = np.zeros_like(vec)
    theirs = blended_pixels(depth, y_t.cpu().numpy(), cut_t.cpu().numpy(), zero, np.ones_like(matched), mt)
    assert np.array_equal(theirs, plain[4])
    print("blended pixels: motion-compensated", mine.sum(), "plain", theirs.sum(), "of", mine[1:].size)
    assert mine.sum() > theirs.sum()
