"""The coarse-to-fine motion search of the motion-compensated depth filter without a GPU: tools/motion_pyramid_oracle.py against
itself (the fast form against the literal statement, the planes, the candidates, the refusals), the designed translations that the
full search cannot follow, sub-batches and the first frame, the surfaces of the engine, the module function and the node, and the
packed key of the kernel's order in a stand-alone host program under AddressSanitizer and UBSan."""
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_stabilizer_motion, depth_stabilizer_pyramid as node_module, engine, stereoimage_generation as sig
import comfystereo_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_motion_pyramid_goldens as goldens   # noqa: E402
import motion_oracle   # noqa: E402
import motion_pyramid_oracle as oracle   # noqa: E402

FIX = np.load(os.path.join(ROOT, "tests", "golden", "motion_pyramid.npz"))


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------------
def flat_planes(rng, h, w):
    """Two planes with large constant areas, so that many candidates tie and the order decides."""
    cur = rng.randint(0, 256, (h, w)).astype(np.uint8)
    ref = rng.randint(0, 256, (h, w)).astype(np.uint8)
    cur[: h // 2] = 90
    ref[: 2 * h // 3] = 90
    cur[:, w // 2:] = np.where(np.arange(h)[:, None] % 2 == 0, 40, 200)
    ref[:, w // 2:] = np.where(np.arange(h)[:, None] % 2 == 0, 200, 40)
    return cur, ref


@pytest.mark.parametrize("h,w,smoothness", [(70, 131, 0), (65, 97, 32), (33, 40, 0), (16, 16, 7)])
def test_the_fast_form_equals_the_literal_statement_at_every_level(h, w, smoothness):
    rng = np.random.RandomState(h * w + smoothness)
    ties = 0
    for cur, ref in (flat_planes(rng, h, w), (rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h, w)).astype(np.uint8))):
        pc, pr = oracle.pyramid(cur), oracle.pyramid(ref)
        levels, matched = oracle.pyramid_search_levels(cur, ref, 16, smoothness, 12)
        want2 = motion_oracle.motion_search(pc[2], pr[2], 4, smoothness, 255)
        assert np.array_equal(levels[2][0], want2[0]) and np.array_equal(levels[2][1], want2[1])
        for k in (1, 0):
            vec, sad = levels[k]
            hb, wb = motion_oracle.block_grid(*pc[k].shape)
            assert vec.shape == (hb, wb, 2) and vec.dtype == np.int8 and sad.dtype == np.int32
            for by in range(hb):
                for bx in range(wb):
                    best, tuples = oracle.best_vector(pc[k], pr[k], by, bx, levels[k + 1][0], smoothness)
                    assert (best[4], best[3]) == tuple(vec[by, bx]) and best[0] - smoothness * best[1] == sad[by, bx], (k, by, bx)
                    assert len(tuples) == len(set(tuples)) <= 46 and (0, 0, 0, 0, 0) in [(0,) + t[1:] for t in tuples]
                    ties += sum(t[0] == best[0] for t in tuples) > 1
        assert np.array_equal(matched, (levels[0][1] <= 12 * motion_oracle.npix(h, w)).astype(np.uint8))
    assert ties > 0 or smoothness   # (without a penalty the constant areas make candidates tie on the cost: the rest of the order decides)


def test_the_planes_on_odd_sizes():
    rng = np.random.RandomState(3)
    plane = rng.randint(0, 256, (7, 13)).astype(np.uint8)
    p = oracle.pyramid(plane)
    assert [a.shape for a in p] == [(7, 13), (4, 7), (2, 4)] and all(a.dtype == np.uint8 for a in p)
    for k in (0, 1):
        h, w = p[k].shape
        for y in range(p[k + 1].shape[0]):
            for x in range(p[k + 1].shape[1]):
                cell = [int(p[k][min(2 * y + j, h - 1), min(2 * x + i, w - 1)]) for j in (0, 1) for i in (0, 1)]
                assert p[k + 1][y, x] == (sum(cell) + 2) >> 2
    assert np.array_equal(oracle.down(np.full((1, 1), 255, np.uint8)), [[255]]) and oracle.down(np.array([[1, 2]], np.uint8))[0, 0] == 2


def test_candidates_are_distinct_and_0_0_is_always_admissible():
    parent = np.zeros((2, 3, 2), np.int8)
    assert oracle.candidates(parent, 1, 2) == sorted((ex, ey) for ex in (-1, 0, 1) for ey in (-1, 0, 1))      # five equal parents: 9, not 46
    parent[0, 1] = (10, -7)
    parent[0, 0] = (-30, 30)
    got = oracle.candidates(parent, 0, 2)                                   # parent (0, 1); left (0, 0), down (1, 1), right (0, 2); no up
    assert len(got) == len(set(got)) == 27 and (19, -15) in got and (-61, 61) in got and (0, 0) in got
    corner = np.full((1, 1, 2), 30, np.int8)
    got = oracle.candidates(corner, 0, 0)
    assert len(got) == 10 and (0, 0) in got and max(max(abs(a), abs(b)) for a, b in got) == 61
    # planes smaller than a block: every candidate but (0, 0) is inadmissible, whatever the parent says
    cur, ref = np.full((16, 16), 7, np.uint8), np.full((16, 16), 9, np.uint8)
    best, tuples = oracle.best_vector(cur, ref, 0, 0, corner, 32)
    assert tuples == [(512, 0, 0, 0, 0)] and best == tuples[0]
    vec, sad = oracle.refine(cur, ref, corner, 32)
    assert not vec.any() and sad[0, 0] == 512
    # the largest vectors of the specification fit the outputs
    assert 2 * (2 * 30 + 1) + 1 == 123 <= 127 and 255 * 256 + 4096 * 246 < 1 << 21


def test_a_search_range_outside_the_set_is_refused():
    for bad in (0, 3, 5, 62, 121, 124, -4, 2.5, True, 64.5):
        with pytest.raises(ValueError, match="search_range must be a multiple of 4 in 4..120"):
            oracle.check_range(bad)
        with pytest.raises(ValueError, match="search_range must be a multiple of 4 in 4..120"):
            engine._pyramid_args(bad, 32, 12)
    assert [oracle.check_range(v) for v in (4, 64, 120, 8.0)] == [4, 64, 120, 8] and engine._pyramid_args(120, 4096, 255) == (120, 4096, 255)
    with pytest.raises(ValueError, match="smoothness must be an integer in 0..4096"):
        oracle.check_params(64, 4097, 12)


def test_the_key_orders_like_the_tuple():
    rng = np.random.RandomState(11)
    cost = np.concatenate([rng.randint(0, 5, 4000), rng.randint(0, 255 * 256 + 4096 * 246 + 1, 200), [255 * 256 + 4096 * 246]])
    dx, dy = rng.randint(-123, 124, cost.size), rng.randint(-123, 124, cost.size)
    keys = oracle.key(cost, dx, dy)
    tuples = list(zip(cost.tolist(), (np.abs(dx) + np.abs(dy)).tolist(), np.abs(dy).tolist(), dy.tolist(), dx.tolist()))
    assert [tuples[i] for i in np.argsort(keys, kind="stable")] == sorted(tuples) and keys.max() < 1 << 52
    rx, ry, sad = oracle.unkey(keys, 0)
    assert np.array_equal(rx, dx) and np.array_equal(ry, dy) and np.array_equal(sad, cost)
    assert (oracle.KEY_COST, oracle.KEY_MAG, oracle.KEY_ADY, oracle.KEY_DY) == (31, 23, 16, 8)


# ---- the designed translations: what the full search cannot follow ------------------------------------------------------------------
@pytest.mark.parametrize("mv", goldens.TRANSLATIONS, ids=lambda mv: f"{mv[0]}_{mv[1]}")
def test_translations_beyond_32_pixels_are_found_where_the_full_search_finds_none(mv):
    cur, ref = goldens.translation_pair(mv)
    assert cur.shape == (256, 384)
    vec, sad, matched = oracle.pyramid_search(cur, ref, 64, 32, 12)
    tag = f"translation_{mv[0]}_{mv[1]}"
    assert np.array_equal(vec, FIX[tag + "/vec"]) and np.array_equal(sad, FIX[tag + "/sad"]) and np.array_equal(matched, FIX[tag + "/matched"])
    admissible = motion_oracle.block_sads(cur, ref, *mv)[1]                # the blocks whose true vector is admissible at level 0
    right = (vec[..., 0] == mv[0]) & (vec[..., 1] == mv[1])
    wrong = int((admissible & ~right).sum())
    print(mv, "wrong", wrong, "of", int(admissible.sum()))
    assert admissible.sum() > 250 and wrong <= 0.01 * admissible.sum()
    assert not sad[admissible & right].any() and matched[admissible & right].all()
    plain = motion_oracle.motion_search(cur, ref, 32, 32, 12)[0]
    assert not ((plain[..., 0] == mv[0]) & (plain[..., 1] == mv[1])).any()


# ---- sub-batches and the first frame ---------------------------------------------------------------------------------------------------
def test_sub_batches_give_bit_for_bit_one_call_and_frame_0_without_a_state_is_a_cut():
    case = dict(goldens._case(40, 72, "subbatch", c=3, n=6, R=8, mv=(5, -3), change=True))
    depth, guide = goldens.make_input(case)
    prm = goldens.params(case)
    whole = oracle.motion_depth(depth, guide, None, *prm)
    state, parts = None, []
    for b0, b1 in ((0, 1), (1, 4), (4, 6)):
        parts.append(oracle.motion_depth(depth[b0:b1], guide[b0:b1], state, *prm))
        state = parts[-1][3]
    for i in (0, 1, 2, 4, 5, 6, 7):
        joined = np.concatenate([p[i] for p in parts])
        assert joined.dtype == whole[i].dtype and np.array_equal(joined.view(np.uint8), np.ascontiguousarray(whole[i]).view(np.uint8)), i
    for a, b in zip((state.prev_raw, state.prev, state.prev_luma), (whole[3].prev_raw, whole[3].prev, whole[3].prev_luma)):
        assert np.array_equal(a, b)
    y, m, cut, st, vec, sad, matched, blended = whole
    assert cut[0] == 1 and m[0] == 0 and not vec[0].any() and not sad[0].any() and matched[0].all() and not blended[0].any()
    assert np.array_equal(y[0], motion_oracle.temporal_oracle.gray(depth)[0]) and vec[1:].any() and blended.any() and (matched[1:] == 0).any()
    assert isinstance(st, motion_oracle.State) and np.array_equal(st.prev_luma, motion_oracle.luma(guide)[-1])
    # a cut frame's vectors are computed all the same
    cut_case = dict(goldens._case(40, 72, "cutvec", n=3, R=8, mv=(5, -3), cut_at=1))
    res = oracle.motion_depth(*goldens.make_input(cut_case), None, *goldens.params(cut_case))
    assert res[2].tolist() == [1, 1, 0] and res[5][1].any()
    # the plain filter's results are untouched by the factoring: its own search is the default
    small = oracle.motion_depth(depth[:2], guide[:2], None, 0.5, 0.1, 0.3, 4, 32, 12)
    plain = motion_oracle.motion_depth(depth[:2], guide[:2], None, 0.5, 0.1, 0.3, 1, 32, 12)
    assert small[0].shape == plain[0].shape and len(small) == len(plain) == 8


def test_the_fixture_file():
    meta = json.loads(str(FIX["meta"]))
    assert [c["id"] for c in meta["cases"]] == [c["id"] for c in goldens.cases()] and "not a reference capture" in meta["note"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "motion_pyramid.npz")) < 1 << 20
    case = next(c for c in meta["cases"] if c["id"] == "17x33_c3_r4_l0_m0")
    y, m, cut, state, vec, sad, matched, _ = goldens.evaluate(case)
    assert goldens.digest_f32(y) == case["y_sha256"] and np.array_equal(vec, FIX[case["id"] + "/vec"]) and np.array_equal(sad, FIX[case["id"] + "/sad"])
    assert goldens.digest_f32(state.prev_raw, state.prev, state.prev_luma) == case["state_sha256"]


# ---- the surfaces -----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_with_their_signatures():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    for name, count in (("cs_motion_depth_pyramid_workspace_bytes", 5), ("cs_motion_depth_pyramid", 25)):
        assert re.search(rf"CS_API\s+\w+\s+{name}\(", header) and name in _native.EXPORTS and hasattr(_native.lib(), name)
        assert len(_native.SIGNATURES[name][1]) == count
    assert _native.SIGNATURES["cs_motion_depth_pyramid"] == _native.SIGNATURES["cs_motion_depth"]
    L = _native.lib()
    for R in range(-4, 130):
        need = L.cs_motion_depth_pyramid_workspace_bytes(2, 16, 16, 1, R)
        assert (need > 0) == (R % 4 == 0 and 4 <= R <= 120), R
    # MotionViews' 2048 bytes, then planes 1 (3 x 8 x 8) and 2 (3 x 4 x 4) and the two coarse vector fields, a 256-byte block each
    assert L.cs_motion_depth_pyramid_workspace_bytes(2, 16, 16, 1, 64) == L.cs_motion_depth_workspace_bytes(2, 16, 16, 1, 16) + 4 * 256
    assert L.cs_motion_depth_pyramid_workspace_bytes(0, 16, 16, 1, 64) == 0


FAKE, FAR = 0x10000000, 0x1000000
POINTERS = ("depth", "guide", "prev_raw", "prev", "prev_luma", "valid", "out", "m", "cut_out", "sad", "vec", "matched", "ws")


def _call(n=2, h=16, w=16, c=1, alpha=0.5, motion=0.1, cut=0.08, R=64, smooth=32, match=12, ws_bytes=0, **ptr):
    p = {name: FAKE + i * FAR for i, name in enumerate(POINTERS)}
    p.update(ptr)
    L = _native.lib()
    rc = L.cs_motion_depth_pyramid(p["depth"], p["guide"], n, h, w, c, alpha, motion, cut, R, smooth, match, p["prev_raw"], p["prev"],
                                   p["prev_luma"], p["valid"], p["out"], p["m"], p["cut_out"], p["vec"], p["sad"], p["matched"], p["ws"], ws_bytes,
                                   None)
    return rc, L.cs_last_error().decode()


def test_the_entry_point_refuses_before_any_launch():
    """(The pointers are fake: a launch would fault; every call here must return before one.)"""
    for name in POINTERS:
        assert _call(**{name: None}) == (_native.CS_EINVAL, "null pointer"), name
    for kw in (dict(n=0), dict(h=-1), dict(w=0), dict(c=0)):
        assert _call(**kw) == (_native.CS_EINVAL, "non-positive size"), kw
    rc, text = _call(n=65536)
    assert rc == _native.CS_ELIMIT and "cs_motion_depth_pyramid" in text and "65535 frames" in text
    for kw, said in ((dict(alpha=1.5), "alpha must lie in [0, 1]"), (dict(motion=-1.0), "motion_threshold must be >= 0"),
                     (dict(cut=float("nan")), "cut_threshold must be >= 0"), (dict(R=0), "search_range must be a multiple of 4 in 4..120"),
                     (dict(R=66), "search_range must be a multiple of 4 in 4..120"), (dict(R=124), "search_range must be a multiple of 4 in 4..120"),
                     (dict(smooth=4097), "smoothness must lie in 0..4096"), (dict(match=256), "match_threshold must lie in 0..255")):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and said in text and "cs_motion_depth_pyramid" in text, kw
    rc, text = _call(out=FAKE + 2)
    assert rc == _native.CS_EINVAL and "4-byte alignment" in text
    rc, text = _call(guide=FAKE + 4)
    assert rc == _native.CS_EINVAL and "must not overlap" in text
    need = _native.lib().cs_motion_depth_pyramid_workspace_bytes(2, 16, 16, 1, 64)
    assert _call(ws_bytes=need - 1) == (_native.CS_EWORKSPACE, "workspace too small")


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("a device was looked for before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)


BAD_PARAMETERS = [(dict(search_range=124), "search_range must be a multiple of 4 in 4..120, got 124"), (dict(search_range=0), "search_range must be"),
                  (dict(search_range=33), "search_range must be a multiple of 4"), (dict(search_range=True), "search_range must be"),
                  (dict(smoothness=4097), "smoothness must be an integer in 0..4096, got 4097"),
                  (dict(match_threshold=256), "match_threshold must be an integer in 0..255"), (dict(match_threshold="12"), "match_threshold must be")]


def test_the_engine_and_the_module_function_refuse_bad_arguments_before_any_native_call(no_device, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was asked before the arguments were checked")))
    d, g = torch.zeros((2, 16, 16, 1)), torch.zeros((2, 16, 16, 3))
    for bad, text in ((None, "depth must be a torch.Tensor"), (d[..., 0], r"depth must be \[N,H,W,C\], got shape"), (d.double(), "depth must be float32")):
        with pytest.raises(ValueError, match=text):
            engine.motion_depth_pyramid(bad, g)
    for bad, text in ((None, "guide must be a torch.Tensor"), (g.double(), "guide must be float32"), (torch.zeros((3, 16, 16, 3)), "at the depth's size")):
        with pytest.raises(ValueError, match=text):
            engine.motion_depth_pyramid_detail(d, bad)
    for kw, text in BAD_PARAMETERS:
        with pytest.raises(ValueError, match=text):
            engine.motion_depth_pyramid(d, g, **kw)
        with pytest.raises(ValueError, match=text):
            sig.stabilize_depth_motion_pyramid(torch.zeros((2, 8, 8)), torch.zeros((2, 8, 8, 3)), **kw)
    with pytest.raises(ValueError, match="image has 3 frames, depth has 2"):
        sig.stabilize_depth_motion_pyramid(torch.zeros((2, 8, 8)), torch.zeros((3, 8, 8, 3)))
    for mine, plain, default in ((engine.motion_depth_pyramid, engine.motion_depth, 64), (engine.motion_depth_pyramid_detail, engine.motion_depth_detail, 64),
                                 (sig.stabilize_depth_motion_pyramid, sig.stabilize_depth_motion, 64)):
        assert str(inspect.signature(mine)) == str(inspect.signature(plain)).replace("search_range=16", f"search_range={default}")


def test_good_arguments_reach_the_device_lookup(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        engine.motion_depth_pyramid(torch.zeros((2, 16, 16, 1)), torch.zeros((2, 16, 16, 3)), None, 0.5, 0.1, 0.08, 120, 4096, 255)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        sig.stabilize_depth_motion_pyramid(np.zeros((2, 8, 8), np.float32), np.zeros((2, 16, 16, 3), np.float32))
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        node_module.StereoDepthStabilizerMotionPyramid().stabilize(torch.zeros((2, 8, 8, 3)), torch.zeros((2, 8, 8, 3)))


def test_the_nodes_inputs_defaults_and_mappings():
    node = node_module.StereoDepthStabilizerMotionPyramid
    types, plain = node.INPUT_TYPES(), depth_stabilizer_motion.StereoDepthStabilizerMotion.INPUT_TYPES()
    assert list(types["required"]) == ["depth_map", "image"] and list(types["optional"]) == list(plain["optional"])
    kind, opts = types["optional"]["search_range"]
    assert kind == "INT" and (opts["min"], opts["max"], opts["step"], opts["default"]) == (4, 120, 4, 64) and "not tuned on footage" in opts["tooltip"]
    assert (opts["min"], opts["max"], opts["step"]) == engine.PYRAMID_SEARCH
    assert {k: v for k, v in types["optional"].items() if k != "search_range"} == {k: v for k, v in plain["optional"].items() if k != "search_range"}
    assert plain["optional"]["search_range"][1]["max"] == 32                # the plain node's inputs are not touched by the copy
    assert node.RETURN_TYPES == ("IMAGE", "MASK", "MASK") and node.RETURN_NAMES == ("stabilized_depth_map", "scene_cut_mask", "unmatched_mask")
    assert node.CATEGORY == "image/stereo" and callable(getattr(node, node.FUNCTION)) and issubclass(node, node_module.ClipNode)
    assert node_module.NODE_CLASS_MAPPINGS == {"StereoDepthStabilizerMotionPyramid": node}
    assert list(node_module.NODE_DISPLAY_NAME_MAPPINGS) == ["StereoDepthStabilizerMotionPyramid"]
    assert depth_stabilizer_motion.NODE_CLASS_MAPPINGS == {"StereoDepthStabilizerMotion": depth_stabilizer_motion.StereoDepthStabilizerMotion}
    assert "StereoDepthStabilizerMotionPyramid" not in comfystereo_amd.NODE_CLASS_MAPPINGS
    assert "StereoDepthStabilizerMotionPyramid" not in comfystereo_amd.NODE_DISPLAY_NAME_MAPPINGS
    params = inspect.signature(node.stabilize).parameters
    assert list(params)[1:] == list(types["required"]) + list(types["optional"])
    assert {k: params[k].default for k in types["optional"]} == {k: v[1]["default"] for k, v in types["optional"].items()}
    for limit in ("integer-pel", "one vector per 16 x 16 block", "beyond `smoothness`", "depth map's resolution", "nobody has tuned", "can miss"):
        assert limit in node_module.__doc__, limit


# ---- the host half under the sanitizers -------------------------------------------------------------------------------------------------
SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include "cs_motionpyramid.h"
using namespace cs;

int main() {
    int bad = 0;
    for (int R = -8; R <= 130; R++) bad += (pyramid_args_error(R, 0, 0) == nullptr) != (R >= 4 && R <= 120 && R % 4 == 0);
    bad += pyramid_args_error(64, 4096, 255) != nullptr || !pyramid_args_error(64, 4097, 0) || !pyramid_args_error(64, 0, 256);
    bad += !strstr(pyramid_args_error(66, -1, 999), "search_range") || !strstr(pyramid_args_error(64, -1, 999), "smoothness");
    if (bad) { printf("parameter checks: %d failures\n", bad); return 1; }
    // the key orders like the tuple over the corners of every field: costs that tie and differ up to the largest, every magnitude's
    // extreme splits, both signs
    const uint32_t costs[] = {0u, 1u, 2u, 65280u, 65281u, (1u << 20) - 1u, 1u << 20, 255u * 256u + 4096u * 246u};
    uint64_t prev_key = 0;
    std::tuple<uint32_t, int, int, int, int> prev_tuple;
    bool first = true;
    for (uint32_t cost : costs)
        for (int mag = 0; mag <= 246; mag++)
            for (int ady = 0; ady <= 123 && ady <= mag; ady++)
                for (int sy = -1; sy <= 1; sy += 2)
                    for (int sx = -1; sx <= 1; sx += 2) {   // tuples in ascending order: (cost, mag, |dy|, dy, dx)
                        const int adx = mag - ady;
                        if (adx > 123 || (ady == 0 && sy > 0) || (adx == 0 && sx > 0)) continue;
                        const int dy = sy * ady, dx = sx * adx;
                        const uint64_t key = pyramid_key(cost, dx, dy);
                        const auto tuple = std::make_tuple(cost, mag, ady, dy, dx);
                        if (!first && !(prev_tuple < tuple && prev_key < key)) { printf("order broken at cost %u (%d, %d)\n", cost, dx, dy); bad++; }
                        int rx, ry; int32_t sad;
                        pyramid_unkey(key, 4096, &rx, &ry, &sad);
                        if (rx != dx || ry != dy || sad != (int32_t)cost - 4096 * mag) { printf("round trip broken at (%d, %d)\n", dx, dy); bad++; }
                        if (key >> 52) { printf("key wider than 52 bits\n"); bad++; }
                        prev_key = key; prev_tuple = tuple; first = false;
                    }
    if (bad) return 1;
    // the workspace: MotionViews' blocks first, every block on a 256-byte boundary, disjoint, inside the size the library asks for
    const int shapes[][3] = {{1, 1, 1}, {1, 16, 16}, {3, 17, 33}, {2, 65, 97}, {64, 130, 258}, {5, 144, 208}};
    for (const auto& s : shapes) {
        const int n = s[0], h = s[1], w = s[2];
        const PyramidViews S = pyramid_views(nullptr, n, h, w);
        uint8_t* base = (uint8_t*)aligned_alloc(256, S.bytes);
        const PyramidViews V = pyramid_views(base, n, h, w);
        const MotionViews M = motion_views(base, n, h, w);
        bad += V.bytes != S.bytes || S.plane[1] || S.vec[2] || V.m.luma != M.luma || V.m.yprev != M.yprev || V.plane[0] != M.luma || V.bytes <= M.bytes;
        bad += V.h[0] != h || V.w[0] != w || V.h[1] != (h + 1) / 2 || V.w[2] != ((w + 1) / 2 + 1) / 2 || V.hb[2] != motion_blocks(V.h[2]);
        const size_t off[4] = {(size_t)(V.plane[1] - base), (size_t)(V.plane[2] - base), (size_t)((uint8_t*)V.vec[1] - base), (size_t)((uint8_t*)V.vec[2] - base)};
        const size_t len[4] = {((size_t)n + 1) * V.h[1] * V.pitch[1], ((size_t)n + 1) * V.h[2] * V.pitch[2], (size_t)n * V.hb[1] * V.wb[1] * 2,
                               (size_t)n * V.hb[2] * V.wb[2] * 2};
        for (int i = 0; i < 4; i++) {
            bad += off[i] % 256 != 0 || off[i] < M.bytes || off[i] + len[i] > V.bytes;
            for (int j = 0; j < i; j++) bad += off[i] < off[j] + len[j] && off[j] < off[i] + len[i];
            memset(base + off[i], i, len[i]);   // (under the sanitizer: inside the allocation)
        }
        for (int k = 0; k < MP_LEVELS; k++) bad += V.pitch[k] % 4 || V.pitch[k] < V.w[k] || V.pitch[k] > V.w[k] + 3;
        // level 2's unwanted SADs and flags fit where level 0's go; a parent exists for every block
        bad += V.hb[2] * V.wb[2] > V.hb[0] * V.wb[0] || 2 * V.hb[1] < V.hb[0] || 2 * V.wb[2] < V.wb[1];
        free(base);
        if (bad) { printf("workspace of %d x %d x %d: %d failures\n", n, h, w, bad); return 1; }
    }
    bad += MP_CANDS != 46 || MP_WIN_ROWS != 18 || MP_MAX_R / 4 > MD_MAX_S || 2 * (2 * (MP_MAX_R / 4) + 1) + 1 != 123;
    bad += low_bytes(0) != 0u || low_bytes(-3) != 0u || low_bytes(1) != 0xffu || low_bytes(3) != 0xffffffu || low_bytes(4) != 0xffffffffu || low_bytes(9) != 0xffffffffu;
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
'''


def test_parameter_checks_workspace_blocks_and_key_packing_under_the_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "pyramid_host.hip"
    src.write_text(SRC)
    exe = tmp_path / "pyramid_host"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "comfystereo_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
