"""The motion-compensated temporal depth filter without a GPU: the specification's own properties (tools/motion_oracle.py), the
fixture's conditions, the C entry point's refusals, and the surface of engine.motion_depth, stabilize_depth_motion and the node."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_stabilizer_motion as node_module, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_motion_goldens as goldens   # noqa: E402
import motion_oracle as oracle   # noqa: E402
import temporal_oracle   # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "motion_depth.npz")
CASES = goldens.cases()
BY_ID = {c["id"]: c for c in CASES}


def bits(a):
    v = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).copy()
    v[np.isnan(a)] = 0x7fc00000
    return v


# ---- the specification's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [(3, -2), (-7, 7), (0, 5), (8, 0)])
def test_a_known_translation_is_recovered_on_every_interior_block(mv):
    rng = np.random.RandomState(11)
    S, h, w = 8, 64, 96
    canvas = rng.randint(0, 256, (h + 2 * S, w + 2 * S)).astype(np.uint8)
    ref = canvas[S:S + h, S:S + w]
    cur = canvas[S + mv[1]:S + mv[1] + h, S + mv[0]:S + mv[0] + w]          # cur(p) = ref(p + mv)
    vec, sad, matched = oracle.motion_search(cur, ref, S, 0, 0)
    assert np.all(vec[1:-1, 1:-1] == np.array(mv, np.int8)) and np.all(sad[1:-1, 1:-1] == 0) and np.all(matched[1:-1, 1:-1] == 1)


def test_on_a_constant_frame_every_vector_is_zero():
    flat = np.full((40, 70), 131, np.uint8)
    for smoothness in (0, 32):
        vec, sad, matched = oracle.motion_search(flat, flat, 9, smoothness, 0)
        assert not vec.any() and not sad.any() and matched.all()


@pytest.mark.parametrize("h,w,S", [(16, 16, 32), (17, 33, 7), (50, 70, 32), (33, 40, 3)])
def test_no_vector_points_outside_the_frame(h, w, S):
    rng = np.random.RandomState(h + w)
    cur, ref = rng.randint(0, 256, (2, h, w)).astype(np.uint8)
    vec, sad, _ = oracle.motion_search(cur, ref, S, 0, 255)
    v = vec.astype(int)
    for by in range(vec.shape[0]):
        for bx in range(vec.shape[1]):
            y0, x0, y1, x1 = 16 * by, 16 * bx, min(16 * by + 16, h), min(16 * bx + 16, w)
            assert 0 <= y0 + v[by, bx, 1] and y1 + v[by, bx, 1] <= h and 0 <= x0 + v[by, bx, 0] and x1 + v[by, bx, 0] <= w
    if (h, w) == (16, 16):
        assert not vec.any()                                                # only (0, 0) is a candidate
    # the packed key and the literal order on tuples pick the same candidate, block by block
    for by, bx in ((0, 0), (vec.shape[0] - 1, vec.shape[1] - 1)):
        best, _ = oracle.best_vector(cur, ref, by, bx, S, 0)
        assert (best[4], best[3]) == tuple(v[by, bx]) and best[0] == sad[by, bx]


def test_the_packed_key_orders_like_the_tuple():
    rng = np.random.RandomState(3)
    cost = rng.randint(0, 4, 4000)                                           # few costs: most comparisons fall to the later components
    dx, dy = rng.randint(-32, 33, (2, 4000))
    keys = oracle.key(cost, dx, dy)
    tuples = list(zip(cost, np.abs(dx) + np.abs(dy), np.abs(dy), dy, dx))
    order = sorted(range(4000), key=lambda i: tuples[i])
    assert np.all(np.diff(keys[order]) >= 0)
    assert all((keys[i] == keys[j]) == (tuples[i] == tuples[j]) for i, j in zip(order, order[1:]))
    assert int(oracle.key(255 * 256 + 4096 * 64, 32, 32)) < 2 ** 46


@pytest.mark.parametrize("cid", ["48x80_c1_s0_degenerate", "50x70_c3_s7", "48x80_c1_s7_special"])
def test_search_range_0_and_match_threshold_255_is_the_plain_filter(cid):
    case = BY_ID[cid]
    depth, guide = goldens.make_input(case)
    a, mt, ct = case["alpha"], case["motion_threshold"], case["cut_threshold"]
    y, m, cut, state, vec, sad, matched, blended = oracle.motion_depth(depth, guide, None, a, mt, ct, 0, case["smoothness"], 255)
    y_t, m_t, cut_t, state_t, still = temporal_oracle.temporal_depth(depth, None, a, mt, ct)
    assert np.array_equal(bits(y), bits(y_t)) and np.array_equal(m, m_t, equal_nan=True) and np.array_equal(cut, cut_t)
    assert np.array_equal(bits(state.prev_raw), bits(state_t.prev_raw)) and np.array_equal(bits(state.prev), bits(state_t.prev))
    assert np.array_equal(blended, still) and not vec.any() and matched.all()
    assert blended.any() and not blended[1:].all()


@pytest.mark.parametrize("cid", ["48x80_c1_s7_cut", "50x70_c3_s7", "17x33_c1_s7"])
def test_a_clip_in_sub_batches_equals_one_call(cid):
    case = BY_ID[cid]
    depth, guide = goldens.make_input(case)
    whole = goldens.evaluate(case, depth, guide)
    for split in range(1, case["n"]):
        first = goldens.evaluate(case, depth[:split], guide[:split])
        second = goldens.evaluate(case, depth[split:], guide[split:], first[3])
        for i in (0, 1, 2, 4, 5, 6):
            joined = np.concatenate([first[i], second[i]])
            assert np.array_equal(bits(joined), bits(whole[i])) if i == 0 else np.array_equal(joined, whole[i], equal_nan=(i == 1)), (split, i)
        for name in ("prev_raw", "prev"):
            assert np.array_equal(bits(getattr(second[3], name)), bits(getattr(whole[3], name)))
        assert np.array_equal(second[3].prev_luma, whole[3].prev_luma)


def test_the_luma_takes_the_guided_pass_codes():
    g = np.array([[[[np.nan, -1.0, 2.0], [0.5, 0.25, 1.0], [np.inf, -np.inf, -0.0], [0.0019, 0.002, 0.998]]]], np.float32)
    assert oracle.luma(g).tolist() == [[[(150 * 0 + 29 * 255 + 128) >> 8, (77 * 128 + 150 * 64 + 29 * 255 + 128) >> 8, (77 * 255 + 128) >> 8,
                                         (77 * 0 + 150 * 1 + 29 * 254 + 128) >> 8]]]
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)               # codes / 255 come back as the codes
    assert oracle.luma(np.stack([k, k, k], -1)[None, None])[0, 0].tolist() == list(range(256))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def test_the_fixture_is_a_cpu_evaluation_and_meets_every_branch():
    with np.load(FIXTURE) as z:
        meta = json.loads(str(z["meta"]))
        assert "not a reference capture" in meta["note"] and meta["tool"] == "tools/make_motion_goldens.py"
        assert [c["id"] for c in meta["cases"]] == [c["id"] for c in CASES]
        for entry, case in zip(meta["cases"], CASES):
            assert {k: entry[k] for k in case} == case
        for name in ("cut", "unmatched", "moved", "blended", "clipped", "vector", "edge_refused"):
            assert any(c["branches"][name] for c in meta["cases"]), name
        assert {c["search_range"] for c in CASES} >= {0, 1, 7, 16, 32} and {c["smoothness"] for c in CASES} >= {0, 32, 4096}
        assert {c["match_threshold"] for c in CASES} >= {0, 12, 255} and {(c["h"], c["w"]) for c in CASES} >= {(16, 16), (17, 33), (48, 80), (50, 70), (130, 258)}
        for case in CASES[::3]:                                             # the oracle here is the one the fixture pins
            y, m, cut, state, vec, sad, matched, blended = goldens.evaluate(case)
            entry = next(c for c in meta["cases"] if c["id"] == case["id"])
            assert goldens.digest(y) == entry["y_sha256"] and goldens.digest(state.prev_raw, state.prev, state.prev_luma) == entry["state_sha256"]
            for name, a in (("m", m), ("cut", cut), ("vec", vec), ("sad", sad), ("matched", matched)):
                assert np.array_equal(z[f"{case['id']}/{name}"], a, equal_nan=(name == "m")), (case["id"], name)
            assert temporal_oracle is not None and goldens.temporal_goldens.margin_ok(m, case["cut_threshold"])
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_every_component_of_the_key_decides_a_tie_in_the_fixture():
    case = BY_ID["48x240_c1_s2_ties"]
    _, guide = goldens.make_input(case)
    lum = oracle.luma(guide)
    vec, _, _ = oracle.motion_search(lum[1], lum[0], case["search_range"], case["smoothness"], case["match_threshold"])
    want = [(None, 0), ((0, 0), 1), ((1, 0), 2), ((0, -1), 3), ((-1, 0), 4)]    # region -> (the vector, the component that decides)
    for region, (v, component) in enumerate(want):
        best, tuples = oracle.best_vector(lum[1], lum[0], 1, 3 * region + 1, case["search_range"], case["smoothness"])
        second = sorted(tuples)[1]
        decided = next(i for i in range(5) if best[i] != second[i])
        assert decided == component, (region, best, second)
        assert (best[4], best[3]) == tuple(int(k) for k in vec[1, 3 * region + 1])
        if v is not None:
            assert (best[4], best[3]) == v


# ---- the C entry point's refusals: all of them before any launch, so addresses that are never read will do ------------------------------
FAKE, FAR = 0x10000000, 0x10000000
POINTERS = ["depth", "guide", "prev_raw", "prev", "prev_luma", "valid", "out", "m", "cut_out", "vec", "sad", "matched", "ws"]


def _call(n=2, h=16, w=16, c=1, alpha=0.5, motion=0.1, cut=0.08, S=16, smooth=32, match=12, ws_bytes=0, **ptr):
    p = {name: FAKE + i * FAR for i, name in enumerate(POINTERS)}
    p.update(ptr)
    L = _native.lib()
    rc = L.cs_motion_depth(p["depth"], p["guide"], n, h, w, c, alpha, motion, cut, S, smooth, match, p["prev_raw"], p["prev"], p["prev_luma"],
                           p["valid"], p["out"], p["m"], p["cut_out"], p["vec"], p["sad"], p["matched"], p["ws"], ws_bytes, None)
    return rc, L.cs_last_error().decode()


def test_the_symbols_are_exported_with_their_signatures():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    for name, count in (("cs_motion_depth_workspace_bytes", 5), ("cs_motion_depth", 25)):
        assert re.search(rf"CS_API\s+\w+\s+{name}\(", header) and name in _native.EXPORTS and hasattr(_native.lib(), name)
        assert len(_native.SIGNATURES[name][1]) == count
    assert _native.ABI_VERSION == 4 and _native.lib().cs_version() == 4


@pytest.mark.parametrize("name", POINTERS)
def test_a_null_pointer_is_refused(name):
    assert _call(**{name: None}) == (_native.CS_EINVAL, "null pointer")


def test_sizes_limits_and_parameters_are_refused():
    for kw in (dict(n=0), dict(h=-1), dict(w=0), dict(c=0)):
        assert _call(**kw) == (_native.CS_EINVAL, "non-positive size"), kw
    rc, text = _call(n=65536)
    assert rc == _native.CS_ELIMIT and "cs_motion_depth" in text and "65535 frames" in text
    rc, text = _call(h=65536, w=32768)
    assert rc == _native.CS_ELIMIT and "2^31 pixels" in text
    for kw, said in ((dict(alpha=1.5), "alpha must lie in [0, 1]"), (dict(alpha=float("nan")), "alpha"), (dict(motion=-1.0), "motion_threshold must be >= 0"),
                     (dict(cut=float("nan")), "cut_threshold must be >= 0"), (dict(S=-1), "search_range must lie in 0..32"),
                     (dict(S=33), "search_range must lie in 0..32"), (dict(smooth=-1), "smoothness must lie in 0..4096"),
                     (dict(smooth=4097), "smoothness must lie in 0..4096"), (dict(match=-1), "match_threshold must lie in 0..255"),
                     (dict(match=256), "match_threshold must lie in 0..255")):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and said in text, kw


def test_misalignment_overlap_and_a_small_workspace_are_refused():
    for name in ("depth", "guide", "prev_raw", "prev", "valid", "out", "m", "cut_out", "sad", "ws"):
        rc, text = _call(**{name: FAKE + POINTERS.index(name) * FAR + 2})
        assert rc == _native.CS_EINVAL and "4-byte alignment" in text, name
    for name in ("prev_luma", "vec", "matched"):                            # buffers of bytes lie on every grid
        assert _call(**{name: FAKE + POINTERS.index(name) * FAR + 1})[0] == _native.CS_EWORKSPACE, name
    # n = 2, 16 x 16, c = 1: depth and out 2048 bytes, guide 6144, the float state 1024 each, prev_luma 256, vec 4, sad 8, matched 2
    for kw in (dict(out=FAKE + 2044), dict(guide=FAKE + 4), dict(prev_luma=FAKE + 2 * FAR + 1023), dict(vec=FAKE + 11 * FAR + 1),
               dict(matched=FAKE + 10 * FAR + 7), dict(prev=FAKE + 2 * FAR + 1020), dict(ws=FAKE + 5 * FAR)):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and "must not overlap" in text, kw
    L = _native.lib()
    need = L.cs_motion_depth_workspace_bytes(2, 16, 16, 1, 16)
    assert need > 0 and need % 256 == 0 and _call(ws_bytes=need - 1) == (_native.CS_EWORKSPACE, "workspace too small")
    assert L.cs_motion_depth_workspace_bytes(2, 16, 16, 1, 33) == 0 and L.cs_motion_depth_workspace_bytes(0, 16, 16, 1, 16) == 0
    # partial sums (256) + three luma frames of 16 x 16 (768) + the copy of y (1024)
    assert need == 256 + 768 + 1024


# ---- the Python layers: every refusal precedes the device check ------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("a device was looked for before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)


BAD_PARAMETERS = [(dict(search_range=33), "search_range must be an integer in 0..32, got 33"), (dict(search_range=-1), "search_range must be"),
                  (dict(search_range=2.5), "search_range must be an integer"), (dict(search_range=True), "search_range must be"),
                  (dict(smoothness=4097), "smoothness must be an integer in 0..4096, got 4097"), (dict(match_threshold=256), "match_threshold must be an integer in 0..255"),
                  (dict(match_threshold="12"), "match_threshold must be")]


def test_the_engine_refuses_bad_arguments_before_it_looks_for_a_device(no_device):
    d, g = torch.zeros((2, 16, 16, 1)), torch.zeros((2, 16, 16, 3))
    for bad, text in ((None, "depth must be a torch.Tensor"), (d[..., 0], r"depth must be \[N,H,W,C\], got shape"), (d.double(), "depth must be float32")):
        with pytest.raises(ValueError, match=text):
            engine.motion_depth(bad, g)
    for bad, text in ((None, "guide must be a torch.Tensor"), (g.double(), "guide must be float32"), (torch.zeros((2, 16, 16, 2)), r"guide must be \[N,H,W,3\]"), (g[..., :2], "guide must be contiguous"),
                      (torch.zeros((2, 16, 16, 1)), r"guide must be \[N,H,W,3\] at the depth's size"), (torch.zeros((3, 16, 16, 3)), "at the depth's size"),
                      (torch.zeros((2, 32, 16, 3)), "at the depth's size")):
        with pytest.raises(ValueError, match=text):
            engine.motion_depth(d, bad)
    for kw, text in BAD_PARAMETERS:
        with pytest.raises(ValueError, match=text):
            engine.motion_depth(d, g, **kw)
    assert str(inspect.signature(engine.motion_depth)) == ("(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, "
                                                           "search_range=16, smoothness=32, match_threshold=12)")
    assert issubclass(engine.MotionState, engine._ClipState)


def test_good_arguments_reach_the_device_lookup(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        engine.motion_depth(torch.zeros((2, 16, 16, 1)), torch.zeros((2, 16, 16, 3)), None, 0.5, 0.1, 0.08, 32, 4096, 255)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        sig.stabilize_depth_motion(np.zeros((2, 8, 8), np.float32), np.zeros((2, 16, 16, 3), np.float32))
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        node_module.StereoDepthStabilizerMotion().stabilize(torch.zeros((2, 8, 8, 3)), torch.zeros((2, 8, 8, 3)))


def test_stabilize_depth_motion_refuses_bad_arguments_before_it_looks_for_a_device(no_device):
    d, img = torch.zeros((2, 8, 8)), torch.zeros((2, 8, 8, 3))
    with pytest.raises(ValueError) as mine:
        sig.stabilize_depth_motion(torch.zeros((4, 4)), img)
    with pytest.raises(ValueError) as other:
        sig.stabilize_depth(torch.zeros((4, 4)))
    assert str(mine.value) == str(other.value)
    for image, text in ((torch.zeros((2, 8, 8)), r"image must be a non-empty \[N,H,W,3\]"), (torch.zeros((3, 8, 8, 3)), "image has 3 frames, depth has 2")):
        with pytest.raises(ValueError, match=text):
            sig.stabilize_depth_motion(d, image)
    with pytest.raises(ValueError, match="batch_size must be at least 1, got 0"):
        sig.stabilize_depth_motion(d, img, batch_size=0)
    for kw, text in BAD_PARAMETERS:
        with pytest.raises(ValueError, match=text):
            sig.stabilize_depth_motion(d, img, **kw)
    assert str(inspect.signature(sig.stabilize_depth_motion)) == (
        "(depth, image, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32, match_threshold=12, "
        "batch_size=16, cuts=None, unmatched=None)")


def test_the_nodes_inputs_defaults_and_mappings():
    node = node_module.StereoDepthStabilizerMotion
    types = node.INPUT_TYPES()
    assert list(types["required"]) == ["depth_map", "image"] and all(v[0] == "IMAGE" for v in types["required"].values())
    assert list(types["optional"]) == ["alpha", "motion_threshold", "cut_threshold", "search_range", "smoothness", "match_threshold", "batch_size", "reset"]
    for name, lo, hi, default in (("search_range", 0, 32, 16), ("smoothness", 0, 4096, 32), ("match_threshold", 0, 255, 12)):
        kind, opts = types["optional"][name]
        assert kind == "INT" and (opts["min"], opts["max"], opts["default"]) == (lo, hi, default) and "not tuned on footage" in opts["tooltip"]
        assert engine.MOTION_RANGES[name] == hi
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "MASK") and node.RETURN_NAMES == ("stabilized_depth_map", "scene_cut_mask", "unmatched_mask")
    assert node.CATEGORY == "image/stereo" and callable(getattr(node, node.FUNCTION)) and issubclass(node, node_module.ClipNode)
    assert node_module.NODE_CLASS_MAPPINGS == {"StereoDepthStabilizerMotion": node}
    assert node_module.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDepthStabilizerMotion": "Stereo Depth Stabilizer (motion compensated)"}
    params = inspect.signature(node.stabilize).parameters
    assert list(params)[1:] == list(types["required"]) + list(types["optional"])
    assert {k: params[k].default for k in types["optional"]} == {k: v[1]["default"] for k, v in types["optional"].items()}
    for limit in ("integer-pel", "one vector per 16 x 16 block", "beyond `smoothness`", "depth map's resolution", "nobody has tuned"):
        assert limit in node_module.__doc__, limit


def test_the_kernel_file_shares_its_parts_and_records_its_resources():
    csrc = os.path.join(ROOT, "comfystereo_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("cs_motiondepth.hip", "cs_temporal.hip", "cs_guideddepth.hip",
                                                                    "cs_temporalstat.h", "cs_guidecode.h", "cs_motiondepth.h")}
    for name in ("cs_motiondepth.hip", "cs_temporal.hip"):                  # the statistic is stated once, in the header both include
        assert '#include "cs_temporalstat.h"' in text[name] and "k_temporal_stat(" not in text[name].split("#include")[-1].replace("(k_temporal_stat", "")
    assert len(re.findall(r"void\s+(?:__launch_bounds__\(\w+\)\s+)?k_temporal_stat\(", text["cs_temporalstat.h"])) == 1
    for name in ("cs_motiondepth.hip", "cs_guideddepth.hip"):               # the 8-bit code likewise
        assert '#include "cs_guidecode.h"' in text[name] and "255.0f + 0.5f" not in text[name]
    assert "255.0f + 0.5f" in text["cs_guidecode.h"]
    body = text["cs_motiondepth.hip"].split("#include")[-1]
    assert "__builtin_amdgcn_sad_u8" in body and "__builtin_amdgcn_alignbyte" in body and "atomic" not in body and "0.2989" not in body
    for kernel in ("k_motion_luma<true>", "k_motion_luma<false>", "k_motion_search", "k_motion_filter<true>", "k_motion_filter<false>"):
        assert re.search(r"//\s+" + re.escape(kernel) + r"\s+\d+\s+\d+\s+\d+\s+\d+", text["cs_motiondepth.hip"]), kernel
    assert "MD_KEY_COST = 27, MD_KEY_MAG = 20, MD_KEY_ADY = 14, MD_KEY_DY = 7" in text["cs_motiondepth.h"]
    assert (oracle.KEY_COST, oracle.KEY_MAG, oracle.KEY_ADY, oracle.KEY_DY) == (27, 20, 14, 7)
