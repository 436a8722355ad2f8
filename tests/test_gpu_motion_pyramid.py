"""The coarse-to-fine motion search of the motion-compensated depth filter on the GPU (cs_motion_depth_pyramid through
engine.motion_depth_pyramid, stereoimage_generation.stabilize_depth_motion_pyramid and the StereoDepthStabilizerMotionPyramid node):
vectors, SADs, matched flags, y, cut and the state bit for bit the fixtures of tests/golden/motion_pyramid.npz, which
tools/make_motion_pyramid_goldens.py wrote from tools/motion_pyramid_oracle.py, the specification; m within the bound
tests/test_gpu_temporal_depth.py derives for the same summation (the statistic's kernels are the same ones).  y and the state are
held against their SHA-256 with every NaN mapped to one pattern.

The shapes are chosen where the kernels can go wrong, not at workload size: see tools/make_motion_pyramid_goldens.py SHAPES."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_stabilizer_pyramid, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_motion_pyramid_goldens as goldens   # noqa: E402

_spec = importlib.util.spec_from_file_location("_temporal_gpu_tests_for_pyramid", os.path.join(ROOT, "tests", "test_gpu_temporal_depth.py"))
_temporal_tests = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_temporal_tests)
m_bound, on_device = _temporal_tests.m_bound, _temporal_tests.on_device

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(ROOT, "tests", "golden", "motion_pyramid.npz"))
META = json.loads(str(FIX["meta"]))
CASES = META["cases"]
IDS = [c["id"] for c in CASES]
BY_ID = {c["id"]: c for c in CASES}
_inputs = {}


def clip(case):
    """(depth, guide) of a case on the device, made once and shared; nothing changes them."""
    if case["id"] not in _inputs:
        depth, guide = goldens.make_input(case)
        _inputs[case["id"]] = (on_device(depth), on_device(guide))
    return _inputs[case["id"]]


def run(case, depth, guide, state=None):
    return engine.motion_depth_pyramid_detail(depth, guide, state, *goldens.params(case))


def check_all(got, case):
    y, m, cut, state, vec, matched, sad = got
    cid = case["id"]
    assert (y.dtype, m.dtype, cut.dtype, vec.dtype, matched.dtype, sad.dtype) == (torch.float32, torch.float32, torch.int32, torch.int8,
                                                                                 torch.uint8, torch.int32)
    vec, vec_w = vec.cpu().numpy(), FIX[f"{cid}/vec"]
    assert vec.shape == vec_w.shape and np.array_equal(vec, vec_w), (np.argwhere(vec != vec_w)[:4], vec[vec != vec_w][:8], vec_w[vec != vec_w][:8])
    assert np.array_equal(sad.cpu().numpy(), FIX[f"{cid}/sad"]) and np.array_equal(matched.cpu().numpy(), FIX[f"{cid}/matched"])
    assert np.array_equal(cut.cpu().numpy(), FIX[f"{cid}/cut"])
    m, m64 = m.cpu().numpy().astype(np.float64), FIX[f"{cid}/m"]
    fin = np.isfinite(m64)
    assert np.all(np.abs(m[fin] - m64[fin]) <= m_bound(m64[fin], case["h"], case["w"])) and np.array_equal(np.isnan(m), np.isnan(m64)), (m, m64)
    assert goldens.digest_f32(y.cpu().numpy()) == case["y_sha256"]
    assert state.valid.item() == 1 and state.prev_luma.dtype == torch.uint8
    assert goldens.digest_f32(state.prev_raw.cpu().numpy(), state.prev.cpu().numpy(), state.prev_luma.cpu().numpy()) == case["state_sha256"]


def test_the_fixtures_cover_what_they_are_for():
    assert {(c["h"], c["w"]) for c in CASES} == set(goldens.SHAPES) and [c["id"] for c in goldens.cases()] == IDS
    for h, w in goldens.SHAPES:
        mine = [c for c in CASES if (c["h"], c["w"]) == (h, w)]
        assert {c["c"] for c in mine} == {1, 3} and {c["search_range"] for c in mine} == {4, 64, 120}
        assert {c["smoothness"] for c in mine} == {0, 32, 4096} and {c["match_threshold"] for c in mine} == {0, 12, 255}
        assert any(FIX[c["id"] + "/cut"][1:].any() for c in mine) and any(c["constant"] for c in mine) and any(c["specials"] for c in mine)
        beyond = BY_ID[f"{h}x{w}_c1_r4_beyond"]
        # a shift beyond R + 3: no block can be on the true vector; blocks of noise against other noise differ by about 85 a pixel,
        # far above the 12 of the threshold, so nothing matches but, by chance, a clipped block of a few pixels
        vec_b, matched_b = FIX[beyond["id"] + "/vec"][1:], FIX[beyond["id"] + "/matched"][1:]
        assert min(map(abs, beyond["mv"])) > beyond["search_range"] + 3 and not (vec_b == np.array(beyond["mv"])).all(axis=-1).any()
        few = goldens.motion_oracle.npix(h, w) < 16
        assert not matched_b[:, ~few].any()
        assert not FIX[f"{h}x{w}_c1_r64_constant/vec"].any()                  # every candidate ties: (0, 0) wins on the order
    assert any(c["blended"] for c in CASES) and any(c["unmatched"] for c in CASES) and any(c["moved"] for c in CASES)
    for c in goldens.cases():
        assert {k: c[k] for k in c} == {k: BY_ID[c["id"]][k] for k in c}, c["id"]   # the generator has not drifted from the file


# ---- every case against the fixtures --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_for_bit_the_fixtures(case):
    check_all(run(case, *clip(case)), case)


@pytest.mark.parametrize("shape", goldens.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_calls_of_one_frame_equal_one_call(shape):
    """n = 1: the only filter launch reads the state's y through its copy in the workspace."""
    case = BY_ID[f"{shape[0]}x{shape[1]}_c1_r64"]
    depth, guide = clip(case)
    state, parts = None, []
    for t in range(case["n"]):
        parts.append(run(case, depth[t:t + 1].contiguous(), guide[t:t + 1].contiguous(), state))
        state = parts[-1][3]
    check_all([torch.cat([p[i] for p in parts]) for i in (0, 1, 2)] + [state] + [torch.cat([p[i] for p in parts]) for i in (4, 5, 6)], case)


@pytest.mark.parametrize("cid", ["70x131_c3_r64_cut", "144x208_c1_r64", "17x33_c3_r4_l0_m0"])
def test_two_calls_equal_one(cid):
    case = BY_ID[cid]
    depth, guide = clip(case)
    first = run(case, depth[:2].contiguous(), guide[:2].contiguous())
    second = run(case, depth[2:].contiguous(), guide[2:].contiguous(), first[3].clone())
    check_all([torch.cat([first[i], second[i]]) for i in (0, 1, 2)] + [second[3]] + [torch.cat([first[i], second[i]]) for i in (4, 5, 6)], case)


def test_a_captured_call_replays_to_the_eager_result():
    case = BY_ID["70x131_c3_r64_cut"]
    depth, guide = clip(case)
    state = engine.MotionState(case["h"], case["w"], depth.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = run(case, depth, guide, state.clone())   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # (a wait for the device inside the call would make the capture fail)
        got = run(case, depth, guide, state)
    state.valid.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check_all(got, case)
    for i in (0, 1, 2, 4, 5, 6):
        assert torch.equal(got[i].view(torch.uint8), eager[i].view(torch.uint8)), i


def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    case = BY_ID["65x97_c1_r64"]
    depth, guide = clip(case)
    n, h, w, c = depth.shape
    L, P = _native.lib(), engine._ptr
    a, mt, ct, R, lam, thr = goldens.params(case)
    need = L.cs_motion_depth_pyramid_workspace_bytes(n, h, w, c, R)
    assert need > L.cs_motion_depth_workspace_bytes(n, h, w, c, 16) and need % 256 == 0
    state = engine.MotionState(h, w, depth.device)
    hb, wb = -(-h // 16), -(-w // 16)
    out = torch.full((n, h, w), -7.0, device="cuda")
    m, cut = torch.full((n,), -7.0, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    vec = torch.full((n, hb, wb, 2), -7, dtype=torch.int8, device="cuda")
    sad = torch.full((n, hb, wb), -7, dtype=torch.int32, device="cuda")
    matched = torch.full((n, hb, wb), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    args = (P(depth), P(guide), n, h, w, c, a, mt, ct, R, lam, thr, P(state.prev_raw), P(state.prev), P(state.prev_luma), P(state.valid), P(out),
            P(m), P(cut), P(vec), P(sad), P(matched), P(ws))
    assert L.cs_motion_depth_pyramid(*args, need - 1, None) == _native.CS_EWORKSPACE and L.cs_last_error() == b"workspace too small"
    torch.cuda.synchronize()
    assert (out == -7).all() and (m == -7).all() and (cut == -7).all() and (vec == -7).all() and (sad == -7).all() and (matched == 7).all()
    assert state.valid.item() == 0 and not ws.any()
    stream = torch.cuda.current_stream().cuda_stream
    assert L.cs_motion_depth_pyramid(*args, need, stream) == _native.CS_OK
    check_all((out, m, cut, state, vec, matched, sad), case)


# ---- the designed translations of tests/test_motion_pyramid_surface.py, on the device -------------------------------------------------
@pytest.mark.parametrize("mv", goldens.TRANSLATIONS, ids=lambda mv: f"{mv[0]}_{mv[1]}")
def test_the_translations_beyond_the_full_search(mv):
    depth, guide = goldens.translation_clip(mv)
    tag = f"translation_{mv[0]}_{mv[1]}"
    y, m, cut, state, vec, matched, sad = engine.motion_depth_pyramid_detail(on_device(depth), on_device(guide), None, 0.5, 0.1, 10.0,
                                                                             goldens.TRANSLATION_R, goldens.TRANSLATION_SMOOTHNESS, 12)
    assert not vec[0].any() and np.array_equal(vec[1].cpu().numpy(), FIX[tag + "/vec"])
    assert np.array_equal(sad[1].cpu().numpy(), FIX[tag + "/sad"]) and np.array_equal(matched[1].cpu().numpy(), FIX[tag + "/matched"])
    cur, ref = goldens.translation_pair(mv)
    admissible = goldens.motion_oracle.block_sads(cur, ref, *mv)[1]
    found = ((vec[1, ..., 0] == mv[0]) & (vec[1, ..., 1] == mv[1])).cpu().numpy()
    assert admissible.sum() > 250 and (admissible & ~found).sum() <= 0.01 * admissible.sum()
    found = int(found.sum())
    plain = engine.motion_depth(on_device(depth), on_device(guide), None, 0.5, 0.1, 10.0, 32, goldens.TRANSLATION_SMOOTHNESS, 12)[4]
    print(tag, "blocks on the true vector: pyramid", found, "full search at 32:", ((plain[1, ..., 0] == mv[0]) & (plain[1, ..., 1] == mv[1])).sum().item())
    assert not ((plain[1, ..., 0] == mv[0]) & (plain[1, ..., 1] == mv[1])).any()


# ---- the module function and the node, with host tensors and a guide at another size ---------------------------------------------------
def test_the_module_function_and_the_node_equal_the_engine():
    rng = np.random.RandomState(78)
    n, h, w = 3, 40, 72
    big = rng.randint(0, 256, (1, 2 * h + 48, 2 * w + 48, 3)).astype(np.float32) / np.float32(255.0)
    big = np.kron(big[:, ::4, ::4], np.ones((1, 4, 4, 1), np.float32))[:, :2 * h + 48, :2 * w + 48]   # 4 x 4 patches survive the resize
    image = np.ascontiguousarray(np.concatenate([big[:, 8 * t:8 * t + 2 * h, 20 * t:20 * t + 2 * w] for t in range(n)]))   # (10, 4) a frame
    depth = (rng.randint(0, 256, (n, h, w)).astype(np.float32) / np.float32(255.0)) * np.float32(0.3)
    small = engine.pil_resize(torch.tensor(image).cuda(), (w, h), f32="nhwc", codes=True)[1]
    prm = (0.5, 0.1, 0.3, 8, 0, 40)
    want = engine.motion_depth_pyramid(torch.tensor(depth[..., None]).cuda(), small.contiguous(), None, *prm)
    assert want[4][1:].any() and want[5][1:].any()
    for d, img in ((torch.tensor(depth), torch.tensor(image)), (torch.tensor(depth).cuda(), torch.tensor(image).cuda())):
        cuts, unmatched = [], []
        y, state = sig.stabilize_depth_motion_pyramid(d, img, None, *prm, batch_size=2, cuts=cuts, unmatched=unmatched)
        assert y.device == d.device and torch.equal(y.cpu().view(torch.int32), want[0].cpu().view(torch.int32)) and isinstance(state, engine.MotionState)
        assert torch.equal(torch.cat(cuts).cpu(), want[2].cpu()) and torch.equal(torch.cat(unmatched).cpu(), 1 - want[5].cpu())
        for a, b in zip((state.prev_raw, state.prev, state.prev_luma), (want[3].prev_raw, want[3].prev, want[3].prev_luma)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    node = depth_stabilizer_pyramid.StereoDepthStabilizerMotionPyramid()
    d3 = torch.tensor(np.repeat(depth[..., None], 3, axis=-1))
    want3 = engine.motion_depth_pyramid(d3.cuda(), small.contiguous(), None, *prm)
    y1, cut1, un1 = node.stabilize(d3[:2], torch.tensor(image[:2]), *prm, batch_size=1)
    y2, cut2, un2 = node.stabilize(d3[2:], torch.tensor(image[2:]), *prm)       # the instance carries the clip on
    y = torch.cat([y1, y2])
    assert tuple(y.shape) == (n, h, w, 3) and torch.equal(y[..., 0].view(torch.int32), want3[0].cpu().view(torch.int32)) and torch.equal(y[..., 0], y[..., 2])
    assert torch.cat([cut1, cut2])[:, 0, 0].tolist() == want3[2].tolist() and tuple(un1.shape) == (2, h, w)
    un = (1 - want3[5].cpu()).to(torch.float32).repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)[:, :h, :w]
    assert torch.equal(torch.cat([un1, un2]), un)
