"""The foreground depth edge dilation without a GPU: the specification (tools/dilate_oracle.py) held to a brute-force double loop
and to scipy.ndimage's maximum / minimum filters, its fixture, the window's tap counts, every refusal of the C entry point and of
the Python layers before any device work, the export, and the node's surface (not gpu)."""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import scipy.ndimage
import torch
import torch.nn.functional as F

from comfystereo_amd import _native, depth_dilate as node_module, engine, stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dilate_oracle as oracle   # noqa: E402
import make_dilate_goldens as goldens   # noqa: E402

INF, NAN = float("inf"), float("nan")
FIXTURE = os.path.join(ROOT, "tests", "golden", "depth_dilate.npz")


# ---- the oracle against a double loop written here -------------------------------------------------------------------------------------
def _key(x):
    u = int(np.float32(x).view(np.uint32))
    return u ^ 0x80000000 if u < 0x80000000 else 0xFFFFFFFF - u


def brute(g, radius, shape, near, threshold):
    """The specification pixel by pixel and tap by tap: g [n,h,w] float32 -> y."""
    n, h, w = g.shape
    thr = np.float32(threshold)
    y = g.copy()
    for t in range(n):
        for py in range(h):
            for px in range(w):
                best = None
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        inside = abs(dx) <= radius and abs(dy) <= radius if shape == "square" else dx * dx + dy * dy <= radius * radius
                        qy, qx = py + dy, px + dx
                        if not inside or not (0 <= qy < h and 0 <= qx < w) or np.isnan(g[t, qy, qx]):
                            continue
                        v = g[t, qy, qx]
                        if best is None or (_key(v) > _key(best) if near == "bright" else _key(v) < _key(best)):
                            best = v
                c = g[t, py, px]
                if best is None or np.isnan(c):
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    diff = np.float32(best - c) if near == "bright" else np.float32(c - best)
                if diff >= thr:
                    y[t, py, px] = best
    return y


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(goldens.canonical(a), goldens.canonical(b))


@pytest.mark.parametrize("kind", goldens.KINDS)
@pytest.mark.parametrize("radius, shape", [(1, "disc"), (2, "disc"), (3, "square"), (8, "disc"), (8, "square"), (5, "disc")])
def test_the_oracle_is_the_double_loop(kind, radius, shape):
    case = dict(id="loop", h=9, w=19, n=1, c=1, kind=kind, seed=77 + radius)
    g = goldens.make_gray(case)
    if kind == "specials":
        g[0, 2:7, 3:10] = np.nan                               # an all-NaN window for the small radii
    for near in oracle.NEARS:
        for threshold in (0.0, 0.04, INF):
            assert same_bits(oracle.dilate_gray(g, radius, shape, near, threshold), brute(g, radius, shape, near, threshold)), (near, threshold)


@pytest.mark.parametrize("h, w", [(1, 1), (1, 9), (9, 1), (3, 5)])
def test_the_oracle_is_the_double_loop_on_frames_smaller_than_the_window(h, w):
    g = goldens.make_gray(dict(h=h, w=w, n=2, kind="specials", seed=h + w))
    for radius, shape in ((1, "disc"), (2, "square"), (8, "disc")):
        for near in oracle.NEARS:
            assert same_bits(oracle.dilate_gray(g, radius, shape, near, 0.0), brute(g, radius, shape, near, 0.0))


@pytest.mark.parametrize("shape", oracle.SHAPES)
@pytest.mark.parametrize("radius", [1, 2, 8])
def test_the_oracle_is_scipys_maximum_and_minimum_filter(radius, shape):
    g = np.random.RandomState(radius).uniform(-1, 1, (2, 19, 41)).astype(np.float32)      # NaN-free, no zeros
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    footprint = np.ones_like(yy, bool) if shape == "square" else (xx * xx + yy * yy <= radius * radius)
    assert footprint.sum() == len(oracle.offsets(radius, shape))
    for t in range(2):
        grown = scipy.ndimage.maximum_filter(g[t], footprint=footprint, mode="constant", cval=-np.inf)
        shrunk = scipy.ndimage.minimum_filter(g[t], footprint=footprint, mode="constant", cval=np.inf)
        assert same_bits(oracle.dilate_gray(g[t:t + 1], radius, shape, "bright", 0.0)[0], grown)
        assert same_bits(oracle.dilate_gray(g[t:t + 1], radius, shape, "dark", 0.0)[0], shrunk)
    if shape == "square":
        pooled = F.max_pool2d(torch.tensor(g).unsqueeze(1), 2 * radius + 1, stride=1, padding=radius).squeeze(1).numpy()
        assert same_bits(oracle.dilate_gray(g, radius, shape, "bright", 0.0), pooled)


def test_the_windows_tap_counts_and_chords():
    assert [len(oracle.offsets(r, "disc")) for r in (1, 2, 8)] == [5, 13, 197]
    assert sorted(oracle.offsets(1, "disc")) == [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]
    for r in oracle.RADII:
        assert len(oracle.offsets(r, "square")) == (2 * r + 1) ** 2
        chords = oracle.chords(r)
        assert sorted(chords) == list(range(-r, r + 1)) and chords[0] == r and chords[r] == chords[-r] == 0
        assert sorted(oracle.offsets(r, "disc")) == sorted((dy, dx) for dy, a in chords.items() for dx in range(-a, a + 1))


def test_the_order_the_gate_and_the_mirror_property():
    specials = np.array([-INF, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, INF], np.float32)
    keys = oracle.key(specials)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and keys[0] == 0x007FFFFF            # a total order, -0 below +0; 0 is free
    assert np.array_equal(oracle.value(keys).view(np.uint32), specials.view(np.uint32))
    assert np.array_equal(oracle.key(-specials), ~keys)
    row = np.array([[[-0.0, 0.0, NAN, INF, INF, -INF, 1.0]]], np.float32)
    y = oracle.dilate_gray(row, 1, "square", "bright", 0.0)
    assert same_bits(y, np.array([[[0.0, 0.0, NAN, INF, INF, INF, 1.0]]], np.float32))     # inf - inf is NaN: the centre stays (the same value)
    g = goldens.make_gray(dict(h=17, w=67, n=3, kind="specials", seed=5))
    for threshold in (0.0, 0.04, INF):
        dark, bright = oracle.dilate_gray(g, 3, "disc", "dark", threshold), oracle.dilate_gray(-g, 3, "disc", "bright", threshold)
        assert np.array_equal(dark.view(np.uint32) ^ np.uint32(0x80000000), bright.view(np.uint32))
    flat = goldens.make_gray(dict(h=17, w=67, n=1, kind="levels", seed=6))
    assert same_bits(oracle.dilate_gray(flat, 8, "square", "bright", INF), flat)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_equals_a_fresh_evaluation():
    built = goldens.build()
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == sorted(built)
        for name in z.files:
            assert np.array_equal(z[name], built[name]), name
        meta = json.loads(str(z["meta"]))
    assert [c["id"] for c in meta["cases"]] == [c["id"] for c in goldens.cases()] and "not a reference capture" in meta["note"]
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_the_cases_cover_what_they_are_there_for():
    cases = goldens.cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for h, w in goldens.SIZES:
        assert {c["n"] for c in cases if (c["h"], c["w"]) == (h, w)} >= {1, 3}, (h, w)
        assert {c["shape"] for c in cases if (c["h"], c["w"]) == (h, w)} == set(oracle.SHAPES), (h, w)
    for h, w in ((17, 67), (33, 132)):
        got = {(c["radius"], c["shape"], c["near"]) for c in cases if (c["h"], c["w"]) == (h, w)}
        assert got >= {(r, s, m) for r in oracle.RADII for s in oracle.SHAPES for m in oracle.NEARS}, (h, w)
    assert {(c["kind"], c["threshold"], c["near"]) for c in cases} >= {(k, t, m) for k in goldens.KINDS for t in goldens.THRESHOLDS for m in oracle.NEARS}
    assert {c["c"] for c in cases} == {1, 3, 4} and {c["off"] for c in cases} == {None, "depth", "out"}
    with open(os.path.join(ROOT, "comfystereo_amd", "csrc", "cs_depthdilate.hip")) as f:
        text = f.read()
    assert (goldens.TILE_W, goldens.TILE_H) == tuple(int(v) for v in re.search(r"DD_TW = (\d+), DD_TH = (\d+)", text).groups())


# ---- the export and the kernel file ------------------------------------------------------------------------------------------------------
def test_the_export_is_in_the_header_the_bindings_and_the_library():
    with open(os.path.join(ROOT, "include", "comfystereo_amd.h")) as f:
        header = f.read()
    assert re.search(r"CS_API\s+int\s+cs_depth_dilate\(", header)
    assert "cs_depth_dilate" in _native.EXPORTS and "cs_depth_dilate" in _native.SIGNATURES and hasattr(_native.lib(), "cs_depth_dilate")
    assert _native.ABI_VERSION == 4 and _native.lib().cs_version() == 4
    assert len(_native.SIGNATURES["cs_depth_dilate"][1]) == 11
    for name, value in (("CS_DILATE_SQUARE", _native.DILATE_SHAPE["square"]), ("CS_DILATE_DISC", _native.DILATE_SHAPE["disc"]),
                        ("CS_DILATE_NEAR_BRIGHT", _native.DILATE_NEAR["bright"]), ("CS_DILATE_NEAR_DARK", _native.DILATE_NEAR["dark"])):
        assert re.search(name + r"\s*=\s*" + str(value) + r"\b", header), name


def test_the_kernel_file_shares_the_gray_access_and_records_its_resources():
    with open(os.path.join(ROOT, "comfystereo_amd", "csrc", "cs_depthdilate.hip")) as f:
        text = f.read()
    code = text.split("#include", 1)[1]
    assert '"cs_gray4.h"' in code and "load_gray4<CM, VEC>(" in code and "store4<VEC>(" in code and "vec4_path(" in code
    assert "0.2989" not in text and "gray_of" not in code and "atomic" not in code and "sqrt" not in code
    assert not re.search(r"struct\s+\w*Px4\b", code)
    for radius in oracle.RADII:
        for shape in ("square", "disc"):
            assert re.search(rf"//\s+k_depth_dilate<{radius}, {shape}, \*, \*>\s+\d+\s+\d+\s+\d+\s+\d+", text), (radius, shape)


# ---- refusals of the C entry point: all of them before any launch, so addresses that are never read will do ---------------------------
FAKE = 0x10000000   # a non-null, 16-byte aligned address nothing dereferences: every call below is refused first
FAR = 0x10000000    # the buffers lie this far apart: neither overlaps the other at any size used here


def _call(n=2, h=8, w=8, c=1, radius=2, shape=1, near=0, threshold=0.04, depth=FAKE, out=FAKE + FAR):
    L = _native.lib()
    rc = L.cs_depth_dilate(depth, n, h, w, c, radius, shape, near, threshold, out, None)
    return rc, L.cs_last_error().decode()


def test_null_pointers_and_non_positive_sizes_are_refused():
    assert _call(depth=None) == (_native.CS_EINVAL, "null pointer") and _call(out=None) == (_native.CS_EINVAL, "null pointer")
    for kw in (dict(n=0), dict(n=-1), dict(h=0), dict(w=-3), dict(c=0), dict(c=-1)):
        assert _call(**kw) == (_native.CS_EINVAL, "non-positive size"), kw
    assert _call(depth=None, n=0, radius=0)[1] == "null pointer"                            # the established order


def test_the_limits_and_the_parameters_are_refused_in_order():
    rc, text = _call(n=65536)
    assert rc == _native.CS_ELIMIT and "cs_depth_dilate" in text and "65535 frames" in text
    rc, text = _call(h=65536, w=32768, radius=0)
    assert rc == _native.CS_ELIMIT and "2^31 pixels" in text
    for radius in (0, 9, -1, 100):
        rc, text = _call(radius=radius, shape=7, threshold=-1.0)
        assert rc == _native.CS_EINVAL and "radius must lie in 1..8" in text, radius
    for kw, said in ((dict(shape=2), "unknown shape"), (dict(shape=-1), "unknown shape"), (dict(near=2), "unknown near"), (dict(near=-1), "unknown near"),
                     (dict(shape=3, near=3), "unknown shape")):
        rc, text = _call(threshold=NAN, **kw)
        assert rc == _native.CS_EINVAL and said in text, kw
    for threshold in (-1e-30, -1.0, -INF, NAN):
        rc, text = _call(threshold=threshold, depth=FAKE + 2)
        assert rc == _native.CS_EINVAL and "threshold must be >= 0 (+inf allowed)" in text, threshold


def test_misalignment_and_overlap_are_refused():
    # n = 2, 8 x 8, c = 1: depth and out are 512 bytes each; c = 3: depth is 1536
    for kw in (dict(depth=FAKE + 2), dict(out=FAKE + FAR + 1), dict(depth=FAKE + 3, out=FAKE)):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and "4-byte alignment" in text, kw
    for kw in (dict(out=FAKE), dict(out=FAKE + 508), dict(out=FAKE - 508), dict(out=FAKE + 4, threshold=INF), dict(c=3, out=FAKE + 1532),
               dict(radius=8, shape=0, near=1, threshold=0.0, out=FAKE + 256)):
        rc, text = _call(**kw)
        assert rc == _native.CS_EINVAL and "out must not overlap depth" in text, kw


# ---- refusals of the Python layers and their wording (no GPU: every one of them precedes the device check) ------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def refuse(*args, **kw):
        raise AssertionError("a device was looked for before the arguments were checked")
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)


BAD_PARAMETERS = [(dict(radius=0), "radius must be an integer in 1..8, got 0"), (dict(radius=9), "radius must be an integer in 1..8, got 9"),
                  (dict(radius=2.5), "radius must be an integer in 1..8, got 2.5"), (dict(radius=True), "radius must be an integer"),
                  (dict(shape="circle"), "shape must be 'square' or 'disc', got 'circle'"), (dict(shape=1), "shape must be"),
                  (dict(near="far"), "near must be 'bright' or 'dark', got 'far'"), (dict(threshold=-0.01), r"threshold must be >= 0 \(\+inf allowed\), got -0.01"),
                  (dict(threshold=NAN), "threshold must be >= 0")]


def test_the_engine_refuses_bad_arguments_before_it_looks_for_a_device(no_device):
    d = torch.zeros((2, 8, 8, 1))
    for bad, text in ((None, "depth must be a torch.Tensor"), (d[..., 0], r"depth must be \[N,H,W,C\], got shape \(2, 8, 8\)"),
                      (d.double(), "depth must be float32, got torch.float64"), (d[:0], "empty depth"),
                      (torch.zeros((2, 8, 8, 2))[..., :1], "depth must be contiguous")):
        with pytest.raises(ValueError, match=text):
            engine.depth_dilate(bad)
    for kw, text in BAD_PARAMETERS:
        with pytest.raises(ValueError, match=text):
            engine.depth_dilate(d, **kw)
    assert str(inspect.signature(engine.depth_dilate)) == "(depth, radius=2, shape='disc', near='bright', threshold=0.04)"


def test_good_arguments_reach_the_device_lookup(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        engine.depth_dilate(torch.zeros((2, 8, 8, 1)), 8, "square", "dark", INF)
    for depth in (torch.zeros((2, 4, 4)), np.zeros((2, 4, 4, 3), np.float32), torch.zeros((2, 4, 4, 1), dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="needs an MI355X"):
            sig.dilate_depth_edges(depth)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        node_module.StereoDepthEdgeDilate().dilate(torch.zeros((2, 4, 4, 3)))


@pytest.mark.parametrize("bad", [torch.zeros((4, 4)), torch.zeros((2, 4, 4, 1, 1)), torch.zeros((0, 4, 4)), torch.zeros((2, 4, 4, 1))[:0]],
                         ids=["2d", "5d", "empty3d", "empty4d"])
def test_dilate_depth_edges_refuses_a_bad_depth_with_the_shared_text(no_device, bad):
    text = re.escape(f"depth must be a non-empty [N,H,W] or [N,H,W,C], got shape {tuple(bad.shape)}")
    for depth in (bad, bad.numpy()):
        with pytest.raises(ValueError, match=text):
            sig.dilate_depth_edges(depth)
        with pytest.raises(ValueError) as other:               # the very text of the other pre-passes
            sig.stabilize_depth(depth)
        with pytest.raises(ValueError) as mine:
            sig.dilate_depth_edges(depth)
        assert str(mine.value) == str(other.value)


@pytest.mark.parametrize("batch_size", [0, -1])
def test_dilate_depth_edges_refuses_a_bad_batch_size_with_the_shared_text(no_device, batch_size):
    with pytest.raises(ValueError, match=re.escape(f"batch_size must be at least 1, got {batch_size}")) as mine:
        sig.dilate_depth_edges(torch.zeros((2, 4, 4)), batch_size=batch_size)
    with pytest.raises(ValueError) as other:
        sig.clip_depth_range(torch.zeros((2, 4, 4)), batch_size=batch_size)
    assert str(mine.value) == str(other.value)


def test_dilate_depth_edges_refuses_bad_parameters_before_it_looks_for_a_device(no_device):
    for kw, text in BAD_PARAMETERS:
        with pytest.raises(ValueError, match=text):
            sig.dilate_depth_edges(torch.zeros((2, 4, 4)), **kw)
    assert str(inspect.signature(sig.dilate_depth_edges)) == "(depth, radius=2, shape='disc', near='bright', threshold=0.04, batch_size=16)"


# ---- the node's surface --------------------------------------------------------------------------------------------------------------
def test_the_nodes_inputs_defaults_and_mappings():
    node = node_module.StereoDepthEdgeDilate
    types = node.INPUT_TYPES()
    assert list(types["required"]) == ["depth_map"] and types["required"]["depth_map"][0] == "IMAGE"
    assert list(types["optional"]) == ["radius", "shape", "near", "threshold", "batch_size"]
    for name, kind, default in (("radius", "INT", 2), ("threshold", "FLOAT", 0.04), ("batch_size", "INT", 16)):
        assert types["optional"][name][0] == kind and types["optional"][name][1]["default"] == default, name
    assert (types["optional"]["radius"][1]["min"], types["optional"]["radius"][1]["max"]) == (1, 8)       # the widgets cannot leave the accepted range
    assert types["optional"]["threshold"][1]["min"] == 0.0
    assert sorted(types["optional"]["shape"][0]) == sorted(_native.DILATE_SHAPE) and types["optional"]["shape"][1]["default"] == "disc"
    assert sorted(types["optional"]["near"][0]) == sorted(_native.DILATE_NEAR) and types["optional"]["near"][1]["default"] == "bright"
    assert node.RETURN_TYPES == ("IMAGE",) and node.RETURN_NAMES == ("dilated_depth_map",) and node.FUNCTION == "dilate"
    assert node.CATEGORY == "image/stereo" and callable(getattr(node, node.FUNCTION))
    assert node_module.NODE_CLASS_MAPPINGS == {"StereoDepthEdgeDilate": node}
    assert node_module.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDepthEdgeDilate": "Stereo Depth Edge Dilate"}
    params = inspect.signature(node.dilate).parameters
    assert list(params)[1:] == list(types["required"]) + list(types["optional"])
    assert {k: params[k].default for k in types["optional"]} == {k: v[1]["default"] for k, v in types["optional"].items()}
    tips = " ".join(v[1]["tooltip"] for v in list(types["required"].values()) + list(types["optional"].values()))
    assert "last step of the chain" in tips and "behind the guided upsampler" in tips and "frames' resolution" in tips
    assert "Its place in the chain is last" in node_module.__doc__ and "keeps no state" in node_module.__doc__
    assert not [k for k in vars(node()) if not k.startswith("__")]                          # stateless
    import comfystereo_amd
    assert "StereoDepthEdgeDilate" not in comfystereo_amd.NODE_CLASS_MAPPINGS               # the package-level mappings stay as they are
