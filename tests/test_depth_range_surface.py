"""The depth range clipping without a GPU: its exports, every refusal of the C entry point and of the Python layers before any
device work, the workspace size, the properties of the specification (tools/range_oracle.py), the conditions its fixture has to
meet, and the node's surface and state rules (not gpu)."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_range as node_module, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_range_goldens as goldens   # noqa: E402
import range_oracle as oracle   # noqa: E402

INF, NAN = float("inf"), float("nan")
FIXTURE = os.path.join(ROOT, "tests", "golden", "depth_range.npz")


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_in_the_header_and_in_the_bindings():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    for name in ("cs_depth_range_workspace_bytes", "cs_depth_range"):
        assert re.search(r"CS_API\s+\w+\s+" + name + r"\(", header), name
        assert name in _native.EXPORTS and name in _native.SIGNATURES
        assert hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 4 and _native.lib().cs_version() == 4
    assert len(_native.SIGNATURES["cs_depth_range"][1]) == 21 and len(_native.SIGNATURES["cs_depth_range_workspace_bytes"][1]) == 4


def test_the_kernel_file_shares_the_gray_expression_and_records_its_resources():
    # the expression lives in the header the pre-passes share; no file of the family restates it or the access built on it
    csrc = os.path.join(ROOT, "comfystereo_amd", "csrc")
    texts = {}
    for name in ("cs_gray4.h", "cs_temporal.hip", "cs_depthrange.hip", "cs_guideddepth.hip"):
        with open(os.path.join(csrc, name)) as f:
            texts[name] = f.read()
        assert "0.2989" not in texts[name], name
    assert "gray_of(" in texts["cs_gray4.h"] and len(re.findall(r"struct\s+\w*Px4\b", texts["cs_gray4.h"])) == 1
    for name in ("cs_temporal.hip", "cs_depthrange.hip"):
        assert '#include "cs_gray4.h"' in texts[name], name
        assert not re.search(r"struct\s+\w*Px4\b|\bload_gray4\s*\(|range_load4|RPx4", texts[name]), name   # (a call names its <CM, VEC>)
    text = texts["cs_depthrange.hip"]
    for kernel in ("k_range_hist<1, 1, true>", "k_range_hist<3, 1, false>", "k_range_pick", "k_range_smooth", "k_range_apply<true>"):
        assert re.search(r"//\s+" + re.escape(kernel) + r"\s+\d+\s+\d+\s+\d+\s+\d+", text), kernel


# ---- refusals of the C entry point: all of them before any launch, so addresses that are never read will do ---------------------------
FAKE = 0x10000000   # a non-null, 16-byte aligned address nothing dereferences: every call below is refused first
FAR = 0x10000000    # the buffers lie this far apart: none overlaps another at any size used here
NAMES = ["depth", "cut", "state_lo", "state_hi", "valid", "out", "lo", "hi", "raw_lo", "raw_hi", "ws"]


def _call(n=2, h=4, w=4, c=1, rank_lo=1, rank_hi=14, beta=0.5, normalize=0, ws_bytes=0, **ptr):
    L = _native.lib()
    p = {name: FAKE + i * FAR for i, name in enumerate(NAMES)}
    p.update(ptr)
    rc = L.cs_depth_range(p["depth"], n, h, w, c, rank_lo, rank_hi, beta, normalize, p["cut"], p["state_lo"], p["state_hi"], p["valid"],
                          p["out"], p["lo"], p["hi"], p["raw_lo"], p["raw_hi"], p["ws"], ws_bytes, None)
    return rc, L.cs_last_error().decode()


@pytest.mark.parametrize("name", [k for k in NAMES if k != "cut"])
def test_a_null_pointer_is_refused(name):
    assert _call(**{name: None}) == (_native.CS_EINVAL, "null pointer")


def test_an_absent_cut_is_no_null_pointer():
    assert _call(cut=None) == (_native.CS_EWORKSPACE, "workspace too small")


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(w=-3), dict(c=0)])
def test_a_non_positive_size_is_refused(kw):
    assert _call(**kw) == (_native.CS_EINVAL, "non-positive size")


def test_the_limits_are_refused():
    rc, text = _call(n=65536)
    assert rc == _native.CS_ELIMIT and "65535 frames" in text
    rc, text = _call(n=1, h=65536, w=32768)
    assert rc == _native.CS_ELIMIT and "2^31 pixels" in text


@pytest.mark.parametrize("kw", [dict(rank_lo=-1), dict(rank_lo=15, rank_hi=14), dict(rank_hi=16), dict(rank_lo=16, rank_hi=16),
                                dict(rank_lo=-2, rank_hi=-1), dict(h=1, w=1, n=1, rank_hi=1)])
def test_ranks_outside_the_frame_or_out_of_order_are_refused(kw):
    rc, text = _call(**kw)
    assert rc == _native.CS_EINVAL and "0 <= rank_lo <= rank_hi < h * w" in text


@pytest.mark.parametrize("beta", [-0.01, 1.01, NAN, INF, -INF])
def test_a_beta_outside_its_range_is_refused(beta):
    rc, text = _call(beta=beta)
    assert rc == _native.CS_EINVAL and "beta must lie in [0, 1]" in text


def test_overlap_and_misalignment_are_refused():
    # depth is 128 bytes here, out 128, a bound array and cut 8, a state word 4
    at = {name: FAKE + i * FAR for i, name in enumerate(NAMES)}
    for kw in (dict(out=at["depth"] + 16), dict(out=at["depth"] + 124), dict(state_lo=at["out"] + 32), dict(state_hi=at["state_lo"]),
               dict(valid=at["depth"] + 64), dict(lo=at["out"] + 124), dict(hi=at["lo"] + 4), dict(raw_lo=at["hi"]), dict(raw_hi=at["cut"] + 4),
               dict(cut=at["depth"]), dict(ws=at["out"] + 8, ws_bytes=1 << 20), dict(ws=at["raw_hi"] - 256)):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and "must not overlap" in text, kw
    assert _call(out=at["depth"] + 128)[0] == _native.CS_EWORKSPACE and _call(hi=at["lo"] + 8)[0] == _native.CS_EWORKSPACE   # (adjacent)
    assert _call(cut=None, raw_hi=at["cut"])[0] == _native.CS_EWORKSPACE   # (an absent cut overlaps nothing)
    for name in NAMES:
        rc, text = _call(**{name: at[name] + 2})
        assert rc == _native.CS_EINVAL and "4-byte alignment" in text, name


def test_a_small_workspace_is_refused_and_the_edges_of_every_range_reach_that_check():
    L = _native.lib()
    need = L.cs_depth_range_workspace_bytes(2, 4, 4, 1)
    assert need > 0
    for kw in (dict(), dict(beta=0.0), dict(beta=1.0), dict(rank_lo=0, rank_hi=0), dict(rank_lo=15, rank_hi=15), dict(rank_lo=0, rank_hi=15),
               dict(normalize=1), dict(c=2), dict(c=3), dict(ws_bytes=need - 1), dict(h=1, w=1, rank_lo=0, rank_hi=0)):
        assert _call(**kw) == (_native.CS_EWORKSPACE, "workspace too small"), kw
    assert _call(n=65535)[0] == _native.CS_EWORKSPACE


def test_the_workspace_size_grows_with_n_alone_and_is_zero_for_no_work():
    L = _native.lib()
    for h, w in ((1, 1), (129, 128), (2160, 3840)):
        sizes = [L.cs_depth_range_workspace_bytes(n, h, w, 1) for n in range(1, 70)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (h, w)
        assert L.cs_depth_range_workspace_bytes(64, h, w, 3) == L.cs_depth_range_workspace_bytes(64, 1, 1, 1)
    # per frame: three passes of two histograms of 2048 int32 bins, and the selections
    assert L.cs_depth_range_workspace_bytes(64, 2160, 3840, 1) >= 64 * 3 * 2 * 2048 * 4
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, -1, 1), (4, 4, 4, 0)):
        assert L.cs_depth_range_workspace_bytes(*bad) == 0


# ---- refusals of the Python layers and their wording (no GPU: every one of them precedes the device check) ------------------------------
def test_the_engine_refuses_bad_arguments_before_it_looks_for_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    d = torch.zeros((2, 4, 4, 1))
    for bad, text in ((None, "depth must be a torch.Tensor"), (d[..., 0], r"depth must be \[N,H,W,C\], got shape \(2, 4, 4\)"),
                      (d.double(), "depth must be float32, got torch.float64"), (d[:0], r"empty depth \(0, 4, 4, 1\)"),
                      (d.expand(2, 4, 4, 3), "depth must be contiguous")):
        with pytest.raises(ValueError, match=text):
            engine.depth_range(bad)
    for kw, text in ((dict(clip_low=-0.01), r"clip_low and clip_high must lie in \[0, 0.5\), got -0.01 and 0.005"),
                     (dict(clip_high=0.5), r"must lie in \[0, 0.5\), got 0.005 and 0.5"), (dict(clip_low=NAN), r"must lie in \[0, 0.5\)"),
                     (dict(beta=1.5), r"beta must lie in \[0, 1\], got 1.5"), (dict(beta=NAN), r"beta must lie in \[0, 1\]"),
                     (dict(cut=torch.zeros(3, dtype=torch.int32)), r"cut must be \[2\], one flag per frame, got shape \(3,\)"),
                     (dict(cut=torch.zeros(2)), "cut must be int32, got torch.float32"), (dict(cut=[0, 1]), "cut must be a torch.Tensor")):
        with pytest.raises(ValueError, match=text):
            engine.depth_range(d, **kw)
    with pytest.raises(RuntimeError, match="needs an MI355X"):   # what is left is the missing device
        engine.depth_range(d)


def test_clip_depth_range_refuses_bad_arguments_before_it_looks_for_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    d = torch.zeros((2, 4, 4))
    for args, kw, text in (((torch.zeros((4, 4)),), {}, r"depth must be a non-empty \[N,H,W\] or \[N,H,W,C\], got shape \(4, 4\)"),
                           ((d[:0],), {}, "non-empty"), ((d,), dict(batch_size=0), "batch_size must be at least 1, got 0"),
                           ((d,), dict(clip_high=0.7), r"must lie in \[0, 0.5\)"),
                           ((d,), dict(cuts=[torch.zeros(3, dtype=torch.int32)]), "cuts hold 3 flags, depth has 2 frames"),
                           ((d,), dict(cuts=[]), "cuts hold 0 flags, depth has 2 frames")):
        with pytest.raises(ValueError, match=text):
            sig.clip_depth_range(*args, **kw)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        sig.clip_depth_range(d)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        node_module.StereoDepthRange().clip(d)


# ---- the node's surface and its state rules ------------------------------------------------------------------------------------------------
def test_the_nodes_inputs_and_outputs():
    node = node_module.StereoDepthRange
    types = node.INPUT_TYPES()
    assert list(types["required"]) == ["depth_map"] and types["required"]["depth_map"] == ("IMAGE",)
    assert list(types["optional"]) == ["scene_cut_mask", "clip_low", "clip_high", "smoothing", "normalize", "batch_size", "reset"]
    assert types["optional"]["scene_cut_mask"][0] == "MASK"
    for name, kind, default in (("clip_low", "FLOAT", 0.005), ("clip_high", "FLOAT", 0.005), ("smoothing", "FLOAT", 0.2),
                                ("normalize", "BOOLEAN", False), ("batch_size", "INT", 16), ("reset", "BOOLEAN", False)):
        assert types["optional"][name][0] == kind and types["optional"][name][1]["default"] == default, name
    for name in ("clip_low", "clip_high"):   # the widgets cannot leave the range the layers accept; the tooltip states the limit
        assert types["optional"][name][1]["min"] == 0.0 and types["optional"][name][1]["max"] < 0.5
        assert "frame's own extreme rules" in types["optional"][name][1]["tooltip"]
    assert node.RETURN_TYPES == ("IMAGE",) and node.RETURN_NAMES == ("clipped_depth_map",) and node.FUNCTION == "clip"
    assert node.CATEGORY == "image/stereo" and callable(getattr(node, node.FUNCTION))
    assert node_module.NODE_CLASS_MAPPINGS == {"StereoDepthRange": node} and node_module.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDepthRange": "Stereo Depth Range"}
    import inspect
    assert list(inspect.signature(node.clip).parameters)[1:] == ["depth_map"] + list(types["optional"])


def test_reset_another_size_or_another_device_start_a_new_clip():
    node = node_module.StereoDepthRange()
    marker = object()
    node._start_clip_if((4, 8, "cuda:0"), False)
    assert node._state is None and node._key == (4, 8, "cuda:0")
    node._state = marker
    node._start_clip_if((4, 8, "cuda:0"), False)
    assert node._state is marker                       # the same clip goes on
    for key, reset in (((4, 8, "cuda:0"), True), ((4, 9, "cuda:0"), False), ((4, 9, "cuda:1"), False)):
        node._state = marker
        node._start_clip_if(key, reset)
        assert node._state is None and node._key == key, (key, reset)


def test_a_frame_counts_as_cut_if_its_mask_is_non_zero_at_the_first_pixel():
    mask = torch.zeros((4, 3, 5))
    mask[1] = 1.0
    mask[2, 0, 0] = 0.5
    mask[3, 1, 1] = 1.0          # (not at pixel (0, 0))
    cuts = node_module.StereoDepthRange._cuts_of(mask, 4)
    assert cuts.dtype == torch.int32 and cuts.tolist() == [0, 1, 1, 0]
    assert node_module.StereoDepthRange._cuts_of(mask[..., None], 4).tolist() == [0, 1, 1, 0]
    for bad in (mask[:3], mask[0]):
        with pytest.raises(ValueError, match="one \\[H,W\\] mask per frame \\(4\\)"):
            node_module.StereoDepthRange._cuts_of(bad, 4)


def test_the_range_state_holds_two_bounds_and_a_flag():
    state = engine.RangeState(4, 8, "cpu")
    assert state.shape == (4, 8) and state.valid.dtype == torch.int32 and state.valid.item() == 0
    assert state.lo.shape == state.hi.shape == (1,) and state.lo.dtype == torch.float32
    other = state.clone()
    other.valid.fill_(1)
    assert state.valid.item() == 0 and other.shape == (4, 8)


# ---- the specification held to its own conditions ------------------------------------------------------------------------------------
def test_the_key_sort_equals_np_sort_on_finite_inputs():
    rng = np.random.RandomState(3)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.randint(-30, 30, 4000).astype(np.float32),
                        np.float32([0.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1.0, -1.0])])
    assert np.isfinite(x).all()
    assert np.array_equal(oracle.unkey(np.sort(oracle.key(x))), np.sort(x))
    assert np.array_equal(oracle.unkey(oracle.key(x)).view(np.uint32), x.view(np.uint32))
    special = np.array([0xff800001, 0xff800000, 0x80000000, 0x00000000, 0x7f800000, 0x7fc00000], np.uint32)   # -NaN -inf -0 +0 +inf +NaN
    k = oracle.key(special.view(np.float32))
    assert np.all(k[:-1] < k[1:]) and np.array_equal(oracle.unkey(k).view(np.uint32), special)
    for rank in (0, 17, 4006):
        assert oracle.select(x.reshape(1, 1, -1), rank)[0] == np.sort(x)[rank]


def test_the_ranks_derived_from_the_fractions_at_their_edges():
    for count in (1, 2, 3, 35, 448, 2160 * 3840):
        assert oracle.ranks_of(0.0, 0.0, count) == (0, count - 1) == engine.clip_ranks(0.0, 0.0, count)
        just_under = np.nextafter(0.5, 0.0)
        lo, hi = oracle.ranks_of(just_under, just_under, count)
        assert 0 <= lo <= hi <= count - 1 and (lo, hi) == engine.clip_ranks(just_under, just_under, count)
        assert hi - lo <= 2
        for a, b in ((0.005, 0.005), (0.1, 0.3), (0.49, 0.0)):
            lo, hi = engine.clip_ranks(a, b, count)
            assert (lo, hi) == oracle.ranks_of(a, b, count) and 0 <= lo <= hi <= count - 1
    assert oracle.ranks_of(0.49, 0.49, 1) == (0, 0)
    assert engine.clip_ranks(0.005, 0.005, 2160 * 3840) == (41471, 8294399 - 41471)
    for bad in ((0.5, 0.0), (0.0, 0.5), (-1e-9, 0.0), (NAN, 0.0)):
        with pytest.raises(ValueError):
            oracle.ranks_of(*bad, 100)
        with pytest.raises(ValueError):
            engine.clip_ranks(*bad, 100)


def test_beta_one_returns_the_raw_bounds_and_beta_zero_keeps_the_first():
    d = (np.random.RandomState(5).randint(0, 257, (6, 5, 7, 1)).astype(np.float32) / np.float32(256.0))   # k / 256: every difference exact
    y, lo, hi, raw_lo, raw_hi, _ = oracle.depth_range(d, None, 2, 30, 1.0)
    assert np.array_equal(lo, raw_lo) and np.array_equal(hi, raw_hi)
    for t in range(6):
        assert y[t].min() == lo[t] and y[t].max() == hi[t]     # order statistics: a pixel at or beyond each bound
    cut = np.array([0, 0, 0, 1, 0, 0], np.int32)
    y, lo, hi, raw_lo, raw_hi, _ = oracle.depth_range(d, None, 2, 30, 0.0, cut)
    assert np.array_equal(lo, raw_lo[[0, 0, 0, 3, 3, 3]]) and np.array_equal(hi, raw_hi[[0, 0, 0, 3, 3, 3]])
    # the documented limit: a smoothed bound outside the frame's own extremes does not become the stereo step's range
    assert all(y[t].min() >= lo[t] and y[t].max() <= hi[t] for t in range(6)) and any(y[t].min() > lo[t] for t in range(6))


@pytest.mark.parametrize("cid", ["5x67_n9_c1_noise_beta025", "5x67_n9_c3_noise_beta025", "5x7_n9_c1_huge_nonfinite"])
def test_splitting_a_batch_at_every_position_equals_the_whole(cid):
    case = next(c for c in goldens.cases() if c["id"] == cid)
    d, cut = goldens.make_input(case), goldens.cut_of(case)
    args = (case["rank_lo"], case["rank_hi"], case["beta"])
    whole = oracle.depth_range(d, None, *args, cut, case["normalize"])
    for k in range(1, len(d)):
        a = oracle.depth_range(d[:k], None, *args, None if cut is None else cut[:k], case["normalize"])
        b = oracle.depth_range(d[k:], a[5], *args, None if cut is None else cut[k:], case["normalize"])
        for i in range(5):
            assert np.array_equal(goldens.canonical(np.concatenate([a[i], b[i]])), goldens.canonical(whole[i])), (k, i)
        assert b[5].lo == whole[5].lo and b[5].hi == whole[5].hi


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixtures_meta_names_its_tool_and_says_what_it_is(fixture):
    meta = json.loads(str(fixture["meta"]))
    assert meta["tool"] == "tools/make_range_goldens.py" and "not a reference capture" in meta["note"]
    assert "CPU evaluation of the specification" in meta["note"]
    assert [c["id"] for c in meta["cases"]] == [c["id"] for c in goldens.cases()] and len(set(c["id"] for c in meta["cases"])) == len(meta["cases"])
    assert os.path.getsize(FIXTURE) < (1 << 20)


def test_the_fixture_is_what_its_tool_writes(fixture):
    got = goldens.build()
    assert sorted(got) == sorted(fixture)
    assert json.loads(str(got["meta"])) == json.loads(str(fixture["meta"]))
    for name in fixture:
        if name != "meta":
            assert got[name].dtype == fixture[name].dtype and np.array_equal(got[name], fixture[name]), name


def test_the_cases_cover_what_the_kernels_can_get_wrong(fixture):
    cases = goldens.cases()
    by_id = {c["id"]: c for c in cases}
    assert {(c["h"], c["w"]) for c in cases} >= {(1, 1), (1, 3), (5, 7), (7, 64), (129, 128), (129, 256)}
    assert {-(-c["h"] * c["w"] // goldens.CHUNK) for c in cases} == {1, 2}          # a second pixel range per frame
    assert {c["c"] for c in cases} >= {1, 2, 3} and {c["beta"] for c in cases} >= {0.0, 0.25, 1.0}
    assert {c["kind"] for c in cases} == set(goldens.KINDS) and {c["normalize"] for c in cases} == {False, True}
    assert any(c["offset"] and c["h"] * c["w"] % 4 == 0 for c in cases) and any(c["h"] * c["w"] % 4 for c in cases)
    assert any(c["rank_lo"] == c["rank_hi"] and c["h"] * c["w"] > 1 for c in cases)
    assert any(c["rank_lo"] == 0 and c["rank_hi"] == c["h"] * c["w"] - 1 and c["h"] * c["w"] > 1 for c in cases)
    assert by_id["1x1_n3_c1_noise"]["rank_lo"] == by_id["1x1_n3_c1_noise"]["rank_hi"] == 0

    def digits(cid, t=0):
        return [goldens.digits_of(fixture[f"{cid}/{name}"].view(np.float32)[t]) for name in ("raw_lo", "raw_hi")]
    # each digit pass decides alone; both ranks in one bin through pass 1, through passes 1 and 2, through all three
    lo, hi = digits("7x64_n2_c1_top11")
    assert lo[0] != hi[0] and len({k >> 21 for k in oracle.key(goldens.make_input(by_id["7x64_n2_c1_top11"])[0]).ravel() & ~np.uint32(0x1fffff)}) > 100
    lo, hi = digits("7x64_n2_c1_mid11")
    assert lo[0] == hi[0] and lo[1] != hi[1] and lo[2] == hi[2]
    keys = oracle.key(goldens.make_input(by_id["7x64_n2_c1_mid11"])[0]).ravel()
    assert len(set(keys >> 21)) == 1 and len(set(keys & 1023)) == 1 and len(set(keys)) > 100
    lo, hi = digits("7x64_n2_c1_low10")
    assert lo[:2] == hi[:2] and lo[2] != hi[2]
    keys = oracle.key(goldens.make_input(by_id["7x64_n2_c1_low10"])[0]).ravel()
    assert len(set(keys >> 10)) == 1 and len(set(keys)) > 100
    lo, hi = digits("5x7_n2_c1_two_inlow")
    assert lo == hi                                                                    # the same key: one bin through pass 3
    lo, hi = digits("5x7_n2_c1_two_straddle")
    g = goldens.make_input(by_id["5x7_n2_c1_two_straddle"])[0].ravel()
    assert lo != hi and sorted(set(g)) == [0.25, 0.75] and (g == 0.25).sum() == 10      # ranks 9 | 10: the last tie below, the first above
    z = fixture["5x7_n2_c1_negzero/raw_lo"], fixture["5x7_n2_c1_negzero/raw_hi"]
    assert z[0][0] == 0x80000000 and z[1][0] == 0                                       # -0 and +0 in one frame, told apart
    assert np.isinf(fixture["7x64_n2_c1_inf_clip0/raw_lo"].view(np.float32)).all() and np.isnan(fixture["7x64_n2_c1_nan_clip0/raw_hi"].view(np.float32)).all()
    assert np.isfinite(fixture["7x64_n2_c1_nan/lo"].view(np.float32)).all() and np.isfinite(fixture["7x64_n2_c1_inf/hi"].view(np.float32)).all()
    for cid in ("64x64_n2_c1_8bit", "64x64_n2_c1_8bit_smooth"):                          # 8-bit depth: at most 256 distinct values
        assert len(set(goldens.make_input(by_id[cid]).ravel())) <= 256
    # smoothing: a cut in the middle restarts the bounds; a non-finite s takes the raw bound
    c = "5x67_n9_c1_noise_beta025"
    lo, raw = fixture[c + "/lo"], fixture[c + "/raw_lo"]
    assert lo[0] == raw[0] and lo[4] == raw[4] and (lo[[1, 2, 3, 5, 6, 7, 8]] != raw[[1, 2, 3, 5, 6, 7, 8]]).all()
    c = "5x7_n9_c1_huge_nonfinite"
    lo, raw = fixture[c + "/lo"], fixture[c + "/raw_lo"]
    assert (lo[:6] == raw[:6]).all() and (lo[6:] != raw[6:]).all()
    # the feature's purpose: four outlier pixels rule the extremes, not the bounds
    g = goldens.make_input(by_id["33x64_n2_c1_outliers"])[0]
    lo, hi = fixture["33x64_n2_c1_outliers/lo"].view(np.float32)[0], fixture["33x64_n2_c1_outliers/hi"].view(np.float32)[0]
    assert g.min() == 0.0 and g.max() == 1.0 and 0.3 <= lo < 0.31 and 0.59 < hi <= 0.6
