"""The image-guided depth upsampling without a GPU: its exports, every refusal of the C entry points and of the Python layers before
any device work, the plan's size, the properties of the specification (tools/guided_oracle.py), the edge property against the
bilinear resize, the conditions its fixture has to meet, and the node's surface (not gpu)."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import _native, depth_guided as node_module, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import guided_oracle as oracle   # noqa: E402
import make_guided_goldens as goldens   # noqa: E402

INF, NAN = float("inf"), float("nan")
FIXTURE = os.path.join(ROOT, "tests", "golden", "guided_depth.npz")
NEW_EXPORTS = ("cs_guided_depth_plan_bytes", "cs_guided_depth_plan", "cs_guided_depth_apply")


# ---- exports ---------------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_in_the_header_and_in_the_bindings():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    for name in NEW_EXPORTS:
        assert re.search(r"CS_API\s+\w+\s+" + name + r"\(", header), name
        assert name in _native.EXPORTS and name in _native.SIGNATURES
        assert hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 4 and _native.lib().cs_version() == 4
    assert [len(_native.SIGNATURES[name][1]) for name in NEW_EXPORTS] == [5, 10, 13]


def test_the_kernel_file_shares_the_gray_expression_and_records_its_resources():
    with open(os.path.join(ROOT, "comfystereo_amd", "csrc", "cs_guideddepth.hip")) as f:
        text = f.read()
    assert "gray_of(" in text and "0.2989" not in text and "exp_exact(" in text and "atomic" not in text.split("#include")[1]
    kernels = ["k_guided_plan"] + [f"k_guided_apply<{r}, {cm}, {vec}>" for r in (1, 2, 3) for cm in (1, 3, 0) for vec in ("true", "false")]
    for kernel in kernels:
        assert re.search(r"//\s+" + re.escape(kernel) + r"\s+\d+\s+\d+\s+\d+\s+\d+", text), kernel
    assert (goldens.TILE_W, goldens.TILE_H) == tuple(int(v) for v in re.search(r"GD_TW = (\d+), GD_TH = (\d+)", text).groups())


# ---- refusals of the C entry points: all of them before any launch, so addresses that are never read will do ---------------------------
FAKE = 0x10000000   # a non-null, 16-byte aligned address nothing dereferences: every call below is refused first
FAR = 0x10000000    # the buffers lie this far apart: none overlaps another at any size used here
NAMES = ["image", "depth", "plan", "out"]


def _plan(h=8, w=8, dh=4, dw=4, radius=2, sigma_s=1.0, sigma_r=0.1, plan=FAKE, plan_bytes=0):
    L = _native.lib()
    rc = L.cs_guided_depth_plan(h, w, dh, dw, radius, sigma_s, sigma_r, plan, plan_bytes, None)
    return rc, L.cs_last_error().decode()


def _apply(n=2, h=8, w=8, dh=4, dw=4, c=1, radius=2, plan_bytes=0, **ptr):
    L = _native.lib()
    p = {name: FAKE + i * FAR for i, name in enumerate(NAMES)}
    p.update(ptr)
    rc = L.cs_guided_depth_apply(p["image"], p["depth"], n, h, w, dh, dw, c, radius, p["plan"], plan_bytes, p["out"], None)
    return rc, L.cs_last_error().decode()


@pytest.mark.parametrize("name", NAMES)
def test_a_null_pointer_is_refused(name):
    assert _apply(**{name: None}) == (_native.CS_EINVAL, "null pointer")
    assert _plan(plan=None) == (_native.CS_EINVAL, "null pointer")


@pytest.mark.parametrize("kw", [dict(h=0), dict(w=0), dict(w=-3), dict(dh=0), dict(dw=-1), dict(h=-8, dh=-9)])
def test_a_non_positive_size_is_refused(kw):
    assert _apply(**kw) == (_native.CS_EINVAL, "non-positive size")
    assert _plan(**kw) == (_native.CS_EINVAL, "non-positive size")
    assert _native.lib().cs_guided_depth_plan_bytes(*[dict(dict(h=8, w=8, dh=4, dw=4, radius=2), **kw)[k] for k in ("h", "w", "dh", "dw", "radius")]) == 0


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-1), dict(c=0), dict(c=-3)])
def test_a_non_positive_count_is_refused(kw):
    assert _apply(**kw) == (_native.CS_EINVAL, "non-positive size")


@pytest.mark.parametrize("radius", [0, 4, -1, 100])
def test_a_radius_outside_one_to_three_is_refused(radius):
    for rc, text in (_apply(radius=radius), _plan(radius=radius)):
        assert rc == _native.CS_EINVAL and "radius must be 1, 2 or 3" in text
    assert _native.lib().cs_guided_depth_plan_bytes(8, 8, 4, 4, radius) == 0


@pytest.mark.parametrize("kw", [dict(sigma_s=0.0), dict(sigma_s=-1.0), dict(sigma_s=NAN), dict(sigma_r=0.0), dict(sigma_r=-0.1), dict(sigma_r=NAN),
                                dict(sigma_r=-INF), dict(sigma_s=-INF)])
def test_a_sigma_that_is_not_positive_is_refused(kw):
    rc, text = _plan(**kw)
    assert rc == _native.CS_EINVAL and "sigma_s and sigma_r must be positive" in text


def test_the_limits_are_refused():
    for call in (_apply, _plan):
        for kw in (dict(dh=9), dict(dw=9), dict(dh=9, dw=9), dict(h=1, dh=2), dict(w=3, dw=4)):
            rc, text = call(**kw)
            assert rc == _native.CS_ELIMIT and "larger than the image" in text, kw
        rc, text = call(h=65536, w=32768)
        assert rc == _native.CS_ELIMIT and "2^31 pixels" in text
    rc, text = _apply(n=65536)
    assert rc == _native.CS_ELIMIT and "65535 frames" in text


def test_overlap_and_misalignment_are_refused():
    # n = 2, 8 x 8 from 4 x 4, c = 1: image is 1536 bytes, depth 128, out 512, the plan what the library says
    need = _native.lib().cs_guided_depth_plan_bytes(8, 8, 4, 4, 2)
    at = {name: FAKE + i * FAR for i, name in enumerate(NAMES)}
    for kw in (dict(out=at["image"]), dict(out=at["image"] + 1532), dict(depth=at["image"] + 64), dict(depth=at["out"] + 508),
               dict(plan=at["out"] + 256), dict(plan=at["image"] - need + 4), dict(plan=at["depth"] + 124), dict(out=at["depth"] - 508),
               dict(image=at["plan"] + need - 4)):
        rc, text = _apply(**kw)
        assert rc == _native.CS_EINVAL and "must not overlap" in text, kw
    for kw in (dict(out=at["image"] + 1536), dict(depth=at["out"] + 512), dict(plan=at["image"] - need), dict(image=at["plan"] + need)):   # adjacent
        assert _apply(**kw)[0] == _native.CS_EWORKSPACE, kw
    for name in NAMES:
        rc, text = _apply(**{name: at[name] + 2})
        assert rc == _native.CS_EINVAL and "4-byte alignment" in text, name
        assert _apply(**{name: at[name] + 4})[0] == _native.CS_EWORKSPACE, name     # (off the 16-byte grid is no refusal)
    rc, text = _plan(plan=FAKE + 1)
    assert rc == _native.CS_EINVAL and "4-byte alignment" in text


def test_a_short_plan_buffer_is_refused_and_the_edges_of_every_range_reach_that_check():
    L = _native.lib()
    need = L.cs_guided_depth_plan_bytes(8, 8, 4, 4, 2)
    assert need > 0
    for kw in (dict(), dict(plan_bytes=need - 1), dict(radius=1), dict(radius=3), dict(dh=8, dw=8), dict(dh=1, dw=1), dict(h=1, w=1, dh=1, dw=1)):
        assert _apply(**kw) == (_native.CS_EWORKSPACE, "plan buffer too small"), kw
        assert _plan(**kw) == (_native.CS_EWORKSPACE, "plan buffer too small"), kw
    for kw in (dict(c=2), dict(c=3), dict(c=7), dict(n=65535)):
        assert _apply(**kw) == (_native.CS_EWORKSPACE, "plan buffer too small"), kw
    for kw in (dict(sigma_r=INF), dict(sigma_s=INF), dict(sigma_s=1e-300), dict(sigma_r=5e-324)):
        assert _plan(**kw) == (_native.CS_EWORKSPACE, "plan buffer too small"), kw


def test_the_plans_size_holds_its_blocks_and_depends_on_the_geometry_alone():
    L = _native.lib()
    for h, w, dh, dw in ((1, 1, 1, 1), (17, 65, 9, 33), (2160, 3840, 518, 921)):
        sizes = [L.cs_guided_depth_plan_bytes(h, w, dh, dw, r) for r in (1, 2, 3)]
        assert sizes[0] <= sizes[1] <= sizes[2]
        for r, size in zip((1, 2, 3), sizes):
            k = 2 * r + 1
            assert size >= 4 * (766 + w + h + dw + dh + k * (w + h)) and size % 256 == 0
            assert size < 4 * (766 + w + h + dw + dh + k * (w + h)) + 512


# ---- refusals of the Python layers and their wording (no GPU: every one of them precedes the device check) ------------------------------
def test_the_engine_refuses_bad_arguments_before_it_looks_for_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for args, text in (((8, 8, 9, 4), r"depth map \(9, 4\) is larger than the image \(8, 8\)"), ((8, 8, 4, 9), "larger than the image"),
                       ((0, 8, 4, 4), "sizes must be positive"), ((8, 8, 4, -1), "sizes must be positive")):
        with pytest.raises(ValueError, match=text):
            engine.guided_depth_plan(*args)
    for kw, text in ((dict(radius=0), "radius must be 1, 2 or 3, got 0"), (dict(radius=4), "radius must be 1, 2 or 3, got 4"),
                     (dict(sigma_s=0.0), "sigma_s and sigma_r must be positive, got 0.0 and 0.1"), (dict(sigma_r=-1.0), "must be positive"),
                     (dict(sigma_s=NAN), "must be positive"), (dict(sigma_r=NAN), "must be positive")):
        with pytest.raises(ValueError, match=text):
            engine.guided_depth_plan(8, 8, 4, 4, **kw)
    with pytest.raises(RuntimeError, match="needs an MI355X"):   # what is left is the missing device
        engine.guided_depth_plan(8, 8, 4, 4, sigma_r=INF)
    assert str(inspect.signature(engine.guided_depth_plan)) == "(h, w, dh, dw, radius=2, sigma_s=1.0, sigma_r=0.1, device=None)"
    assert str(inspect.signature(engine.guided_depth)) == "(image, depth, plan)"

    plan = engine.GuidedPlan(8, 8, 4, 4, 2, 1.0, 0.1, torch.zeros(4096, dtype=torch.uint8), 4096)
    img, d = torch.zeros((2, 8, 8, 3)), torch.zeros((2, 4, 4, 1))
    for a, b, p, text in ((None, d, plan, "image must be a torch.Tensor"), (img[0], d, plan, r"image must be \[N,H,W,3\], got shape \(8, 8, 3\)"),
                          (img.double(), d, plan, "image must be float32, got torch.float64"), (img[:0], d, plan, "empty image"),
                          (img[..., :2], d, plan, "image must be contiguous"), (torch.zeros((2, 8, 8, 4)), d, plan, r"image must be \[N,H,W,3\]"),
                          (img, d[..., 0], plan, r"depth must be \[N,dh,dw,C\], got shape \(2, 4, 4\)"), (img, d.half(), plan, "depth must be float32"),
                          (img, d[:1], plan, "image has 2 frames, depth has 1"), (img, d, None, "plan must be a GuidedPlan"),
                          (img, torch.zeros((2, 4, 5, 1)), plan, r"plan is for depth maps of \(4, 4\) and frames of \(8, 8\), got \(4, 5\) and \(8, 8\)"),
                          (torch.zeros((2, 8, 9, 3)), d, plan, "plan is for depth maps")):
        with pytest.raises(ValueError, match=text):
            engine.guided_depth(a, b, p)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        engine.guided_depth(img, d, plan)


def test_upsample_depth_guided_and_the_node_refuse_bad_arguments_before_they_look_for_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    img, d = torch.zeros((2, 8, 8, 3)), torch.zeros((2, 4, 4))
    for args, kw, text in (((img[0], d), {}, r"image must be a non-empty \[N,H,W,3\], got shape \(8, 8, 3\)"),
                           ((img[:0], d), {}, "image must be a non-empty"), ((torch.zeros((2, 8, 8, 1)), d), {}, "image must be a non-empty"),
                           ((img, d[0]), {}, r"depth must be a non-empty \[N,dh,dw\] or \[N,dh,dw,C\], got shape \(4, 4\)"),
                           ((img, d[:1]), {}, "image has 2 frames, depth has 1"), ((img, d), dict(batch_size=0), "batch_size must be at least 1, got 0"),
                           ((img, torch.zeros((2, 9, 4))), {}, "larger than the image"), ((img, d), dict(radius=5), "radius must be 1, 2 or 3"),
                           ((img, d), dict(sigma_s=0.0), "must be positive"), ((img, d), dict(sigma_r=NAN), "must be positive")):
        with pytest.raises(ValueError, match=text):
            sig.upsample_depth_guided(*args, **kw)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        sig.upsample_depth_guided(img, d)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        sig.upsample_depth_guided(img.numpy(), d.numpy()[..., None])
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        node_module.StereoDepthGuidedUpsample().upsample(img, d[..., None])
    assert str(inspect.signature(sig.upsample_depth_guided)) == "(image, depth, radius=2, sigma_s=1.0, sigma_r=0.1, batch_size=16)"


# ---- the node's surface --------------------------------------------------------------------------------------------------------------
def test_the_nodes_inputs_and_outputs():
    node = node_module.StereoDepthGuidedUpsample
    types = node.INPUT_TYPES()
    assert list(types["required"]) == ["image", "depth_map"] and all(types["required"][k][0] == "IMAGE" for k in types["required"])
    assert list(types["optional"]) == ["radius", "sigma_spatial", "sigma_range", "batch_size"]
    for name, kind, default in (("radius", "INT", 2), ("sigma_spatial", "FLOAT", 1.0), ("sigma_range", "FLOAT", 0.1), ("batch_size", "INT", 16)):
        assert types["optional"][name][0] == kind and types["optional"][name][1]["default"] == default, name
    assert (types["optional"]["radius"][1]["min"], types["optional"]["radius"][1]["max"]) == (1, 3)      # the widgets cannot leave the accepted range
    assert types["optional"]["sigma_spatial"][1]["min"] > 0 and types["optional"]["sigma_range"][1]["min"] > 0
    assert node.RETURN_TYPES == ("IMAGE",) and node.RETURN_NAMES == ("upsampled_depth_map",) and node.FUNCTION == "upsample"
    assert node.CATEGORY == "image/stereo" and callable(getattr(node, node.FUNCTION))
    assert node_module.NODE_CLASS_MAPPINGS == {"StereoDepthGuidedUpsample": node}
    assert node_module.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDepthGuidedUpsample": "Stereo Depth Guided Upsample"}
    assert list(inspect.signature(node.upsample).parameters)[1:] == list(types["required"]) + list(types["optional"])
    doc = node_module.__doc__
    assert "behind `StereoDepthStabilizer` and `StereoDepthRange`" in doc and "in front of the Stereo Image Node" in doc


def test_the_plan_object_returns_its_blocks_by_value():
    h, w, dh, dw, r = 5, 7, 3, 4, 2
    k = 2 * r + 1
    words = 768 + w + h + dw + dh + k * (w + h)
    raw = torch.arange(words, dtype=torch.int32)
    plan = engine.GuidedPlan(h, w, dh, dw, r, 1.0, 0.1, raw.view(torch.uint8), 4 * words)
    assert plan.taps == 5 and plan.device == raw.device
    at = 768
    for name, count in (("cx", w), ("cy", h), ("gx", dw), ("gy", dh)):
        assert getattr(plan, name).tolist() == list(range(at, at + count)), name
        at += count
    assert plan.wx.shape == (w, k) and plan.wy.shape == (h, k) and plan.wr.shape == (766,)
    assert plan.wx.view(torch.int32).flatten().tolist() == list(range(at, at + w * k))
    assert plan.wy.view(torch.int32).flatten().tolist() == list(range(at + w * k, words))
    assert plan.wr.view(torch.int32).tolist() == list(range(766))


# ---- the specification held to its own conditions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(17, 23, 5, 7), (16, 64, 16, 64), (18, 70, 1, 1), (1, 1, 1, 1), (2160, 3840, 518, 921), (33, 132, 8, 33)])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_the_oracles_plan_obeys_its_conditions(geometry, radius):
    h, w, dh, dw = geometry
    p = oracle.plan(h, w, dh, dw, radius, 1.0, 0.1)
    for c, wt, size, dsize in ((p.cx, p.wx, w, dw), (p.cy, p.wy, h, dh)):
        assert c.dtype == np.int32 and wt.dtype == np.float32 and wt.shape == (size, 2 * radius + 1)
        assert c.min() >= -radius and c.max() <= dsize - 1 + radius and (np.diff(c) >= 0).all()       # within the grid +- R, monotone
        assert c.min() >= 0 and c.max() <= dsize - 1                                               # (in fact within the grid)
        assert (wt[:, radius] == wt.max(axis=1)).all() and (wt[:, radius] > 0).all() and (wt <= 1).all()  # the centre tap weighs most (|t| <= 1 / 2)
    assert p.wr.shape == (766,) and p.wr[0] == 1.0 and (np.diff(p.wr) <= 0).all() and (p.wr >= 0).all()
    for g, size, dsize in ((p.gx, w, dw), (p.gy, h, dh)):
        assert g.dtype == np.int32 and g.shape == (dsize,) and g.min() >= 0 and g.max() <= size - 1 and (np.diff(g) > 0).all()
        if dsize == size:
            assert np.array_equal(g, np.arange(size))
    assert (oracle.plan(h, w, dh, dw, radius, 1.0, INF).wr == 1.0).all()


def test_the_plan_refuses_what_the_library_refuses():
    for args in ((8, 8, 9, 4, 2, 1.0, 0.1), (8, 8, 4, 4, 0, 1.0, 0.1), (8, 8, 4, 4, 4, 1.0, 0.1), (8, 8, 4, 4, 2, 0.0, 0.1), (8, 8, 4, 4, 2, 1.0, NAN),
                 (0, 8, 4, 4, 2, 1.0, 0.1)):
        with pytest.raises(ValueError):
            oracle.plan(*args)


def test_the_codes_clamp_round_and_map_nan_to_zero():
    v = np.float32([-1.0, -0.0, 0.0, 0.5 / 255, 0.49 / 255, 1.0, 1.5, np.inf, -np.inf, np.nan, 127.5 / 255, 254.6 / 255])
    assert oracle.code(v).tolist() == [0, 0, 0, 1, 0, 255, 255, 255, 0, 0, int(np.float32(127.5 / 255) * np.float32(255) + np.float32(0.5)), 255]


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_without_a_range_term_and_at_the_same_size_a_constant_stays_that_constant(radius):
    rng = np.random.RandomState(radius)
    image = rng.uniform(0, 1, (2, 9, 13, 3)).astype(np.float32)
    for value in (0.625, 0.1, 1.0e30, -7.0):          # (num / den of one value: the products round, the quotient undoes it only to an ulp or so)
        depth = np.full((2, 9, 13, 1), value, np.float32)
        out = oracle.guided_depth(image, depth, radius, 1.0, INF)
        k2 = (2 * radius + 1) ** 2
        assert np.abs(out - np.float32(value)).max() <= (2 * k2 + 2) * 2.0 ** -24 * abs(value)
    out = oracle.guided_depth(image, np.full((2, 9, 13, 1), 0.5, np.float32), radius, 1.0, INF)      # a power of two: every product is exact
    assert np.abs(out - 0.5).max() <= 2.0 ** -24


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_depth_edge_lands_on_the_guides_edge_where_the_bilinear_resize_has_a_ramp(radius):
    image, depth = goldens.edge_scene(radius)
    out = oracle.guided_depth(image, depth, radius, 1.0, 0.1)
    bound = goldens.check_edge_property(out, radius)
    soft = oracle.bilinear(depth, 16, 64)
    between = (soft > 0.2 * (1 + bound)) & (soft < 0.8 * (1 - bound))      # on neither plateau
    assert (between.sum(axis=2) >= 3).all() and not between[:, :, :29].any() and not between[:, :, 35:].any()   # a ramp several pixels wide
    assert not ((out > 0.2 * (1 + bound)) & (out < 0.8 * (1 - bound))).any()


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixtures_meta_names_its_tool_and_says_what_it_is(fixture):
    meta = json.loads(str(fixture["meta"]))
    assert meta["tool"] == "tools/make_guided_goldens.py" and "not a reference capture" in meta["note"]
    assert "CPU evaluation of the specification" in meta["note"]
    assert [c["id"] for c in meta["cases"]] == [c["id"] for c in goldens.cases()] and len(set(c["id"] for c in meta["cases"])) == len(meta["cases"])
    assert os.path.getsize(FIXTURE) < (1 << 17)


def test_the_oracle_reproduces_the_fixture(fixture):
    got = goldens.build()
    assert sorted(got) == sorted(fixture)
    assert json.loads(str(got["meta"])) == json.loads(str(fixture["meta"]))
    for name in fixture:
        if name != "meta":
            assert got[name].dtype == fixture[name].dtype and np.array_equal(got[name], fixture[name]), name


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    cases = goldens.cases()
    tw, th = goldens.TILE_W, goldens.TILE_H
    assert {(c["h"], c["w"]) for c in cases} >= {(h, w) for h in (th - 1, th, th + 1) for w in (tw - 1, tw, tw + 1)}
    assert {(c["radius"], c["c"]) for c in cases} >= {(r, c) for r in (1, 2, 3) for c in (1, 2, 3)} and {c["n"] for c in cases} == {1, 3}
    for r in (1, 2, 3):
        mine = [c for c in cases if c["radius"] == r]
        assert any((c["h"], c["w"]) == (c["dh"], c["dw"]) and c["h"] * c["w"] > 1 for c in mine)               # identity
        assert any((c["h"], c["w"]) == (2 * c["dh"], 2 * c["dw"]) for c in mine)                              # exactly 2
        assert any((c["dw"], c["dh"], c["w"], c["h"]) == (7, 5, 23, 17) for c in mine)                         # non-integer in both axes
    assert any(c["dh"] == 1 and c["dw"] > 1 for c in cases) and any(c["dw"] == 1 and c["dh"] > 1 for c in cases)
    assert any(c["dh"] == c["dw"] == 1 and c["h"] * c["w"] > 1 for c in cases) and any(c["h"] == c["w"] == 1 for c in cases)
    assert any(c["h"] * c["w"] % 4 for c in cases) and {c["off"] for c in cases} == {None, "image", "depth", "out"}
    assert all(c["w"] % 4 == 0 for c in cases if c["off"])                                                   # (else the guarded path runs anyway)
    assert any(c["h"] > th and c["w"] > tw for c in cases)                                                   # more than one tile on either axis
    assert any(c["sigma_r"] == INF for c in cases) and {c["guide"] for c in cases} == set(goldens.GUIDES) and {c["depth"] for c in cases} == set(goldens.DEPTHS)
    assert any(c["id"].endswith("fallback") for c in cases) and any(c["id"].endswith("subnormal") for c in cases)   # (build() asserts they occur)
    # the cases off the 16-byte grid have the inputs and so the results of the one on it
    base = next(c for c in cases if c["id"] == "8x32_to_16x64_n1_c3_r2")
    for c in cases:
        if c["off"]:
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(goldens.make_input(c), goldens.make_input(base))), c["id"]
