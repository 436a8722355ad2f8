"""The reference's Gaussian depth blurs (blur_depth_map, edge_selective_blur_depth_map, left_direction_aware_blur_depth_map,
right_direction_aware_blur_depth_map): the public surface, the fixtures captured from the reference against the numpy
restatement the GPU tests hold the kernels to (tools/gauss_oracle.py), and the host-side refusals of cs_gaussian_blur.  No GPU."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import gauss_oracle as go
from comfystereo_amd import _native, engine
from comfystereo_amd import stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FUNCS = ["blur_depth_map", "edge_selective_blur_depth_map", "left_direction_aware_blur_depth_map",
         "right_direction_aware_blur_depth_map"]
NEW_EXPORTS = ["cs_gaussian_blur_workspace_bytes", "cs_gaussian_blur_max_taps", "cs_gaussian_blur"]


def load():
    z = np.load(os.path.join(GOLDEN, "gauss_blur.npz"))
    return z, json.loads(str(z["meta"]))


def case_args(z, c):
    d = z[f"in/{c['input']}"]
    return (d, c["sigma"]) if c["edge_threshold"] is None else (d, c["sigma"], c["edge_threshold"])


def bits_equal(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_four_functions_exist_with_the_reference_signatures():
    want = json.load(open(os.path.join(GOLDEN, "gauss_signatures.json")))
    assert sorted(want) == sorted(FUNCS)
    for name in FUNCS:
        assert str(inspect.signature(getattr(sig, name))) == want[name], name
        assert name in sig.__doc__, f"{name} missing from the module docstring's list of extras"
        assert "float32 first" in getattr(sig, name).__doc__, f"{name}: the docstring states the one deviation"
    assert str(inspect.signature(engine.gaussian_blur)) == "(depth, sigma, op='plain', edge_threshold=None)"


def test_restatement_is_bit_equal_to_every_fixture():
    z, meta = load()
    seen = dict(fn=set(), sigma=set(), thr=set(), kinds=set())
    big_radius = False
    for c in meta["cases"]:
        args = case_args(z, c)
        got, want = getattr(go, c["fn"])(*args), z[f"{c['id']}/out"]
        assert bits_equal(got, want), (c["id"], int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        seen["fn"].add(c["fn"]); seen["sigma"].add(c["sigma"]); seen["thr"].add(c["edge_threshold"])
        seen["kinds"].add(c["input"])
        h, w = args[0].shape
        big_radius = big_radius or (c["sigma"] > 0 and int(3 * c["sigma"]) > max(h, w))
    assert seen["fn"] == set(FUNCS)
    assert {0.2, 0.4, 1, 2.5, 7, 20, 70} <= seen["sigma"] and {0.5, 6, 40} <= seen["thr"]
    assert {"codes", "unit", "noise", "ellipse", "flat", "one_row", "one_col"} <= seen["kinds"]
    assert big_radius, "a case with the radius above W and above H"
    for name, spec in meta["inputs"].items():   # the inputs are what tools/gauss_oracle.depth_map generates
        assert bits_equal(go.depth_map(spec["kind"], spec["h"], spec["w"], spec["seed"]), z[f"in/{name}"]), name
    assert z["in/one_row"].shape[0] == 1 and z["in/one_col"].shape[1] == 1
    assert os.path.getsize(os.path.join(GOLDEN, "gauss_blur.npz")) <= os.path.getsize(os.path.join(GOLDEN, "grid_warp.npz"))


def test_restatement_pass_is_np_convolve_also_for_asymmetric_taps():
    """One pass of the restatement against np.convolve itself, line by line, on tap arrays without the Gaussian's symmetry
    (which would hide a reversed tap order) -- the arithmetic cs_gaussian_blur documents for any taps handed to it."""
    rng = np.random.default_rng(3)
    for n in (1, 3, 9, 41, 201):
        taps = rng.random(n) + 0.01
        taps /= taps.sum()
        x = go.depth_map("noise", 7, 50, n)
        rows = go.convolve_axis(x, taps, 1)
        cols = go.convolve_axis(x, taps, 0)
        r = n // 2
        for i in range(x.shape[0]):
            want = np.convolve(np.pad(x[i], (r, r), mode="edge"), taps, mode="valid").astype(np.float32)
            assert bits_equal(rows[i], want), (n, i)
        for j in range(x.shape[1]):
            want = np.convolve(np.pad(x[:, j], (r, r), mode="edge"), taps, mode="valid").astype(np.float32)
            assert bits_equal(np.ascontiguousarray(cols[:, j]), want), (n, j)
        if n > 1:
            assert not bits_equal(rows, go.convolve_axis(x, taps[::-1].copy(), 1)), "the tap order must matter here"


def test_gaussian_taps_is_the_reference_expression():
    for s in (0.2, 0.4, 1, 2.5, 7, 20, 70, 200):
        k = engine.gaussian_taps(s)
        assert k.dtype == np.float64 and k.shape == (2 * int(3 * s) + 1,)
        assert np.array_equal(k, go.gaussian_taps(s))
    assert engine.gaussian_taps(0.2).tolist() == [1.0]
    assert engine.gaussian_taps(200).shape[0] == 1201 <= _native.lib().cs_gaussian_blur_max_taps()
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            engine.gaussian_taps(bad)


def test_blur_depth_map_with_no_sigma_returns_its_argument():
    d = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert sig.blur_depth_map(d, 0) is d and sig.blur_depth_map(d, -2.5) is d
    lst = [[1.0, 2.0]]
    assert sig.blur_depth_map(lst, 0) is lst


def test_without_a_gpu_the_drop_ins_raise_runtime_error(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    d = np.zeros((4, 5), dtype=np.float32)
    with pytest.raises(RuntimeError):
        sig.blur_depth_map(d, 1.0)
    for fn in FUNCS[1:]:
        with pytest.raises(RuntimeError):
            getattr(sig, fn)(d, 1.0, 6.0)
        with pytest.raises(RuntimeError):
            getattr(sig, fn)(d, 0, 6.0)   # (no sigma short cut in the blending functions)


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(L, name), name
    for name, v in (("CS_GAUSS_PLAIN", 0), ("CS_GAUSS_EDGE_SELECTIVE", 1), ("CS_GAUSS_LEFT", 2), ("CS_GAUSS_RIGHT", 3)):
        assert re.search(rf"\b{name} = {v}\b", hdr), name
    assert _native.GAUSS_OP == {"plain": 0, "edge_selective": 1, "left": 2, "right": 3}
    assert L.cs_version() == 4


def test_host_side_validation_of_cs_gaussian_blur():
    L = _native.lib()
    cap = L.cs_gaussian_blur_max_taps()
    assert cap >= 1201 and cap % 2 == 1   # radius 600: sigma = 200, the node's largest blur strength
    nb = L.cs_gaussian_blur_workspace_bytes(2, 4, 8, 7)
    assert nb >= 2 * 4 * 8 * 4 and L.cs_gaussian_blur_workspace_bytes(0, 4, 8, 7) == 0
    # distinct non-null host addresses with the alignment the entry asks for: every refusal below comes before device work
    d, o, t, ws = 64, 128, 192, 256
    call = lambda **kw: L.cs_gaussian_blur(*[{**dict(op=0, depth=d, taps=t, n_taps=7, thr=6.0, n=2, h=4, w=8, out=o, ws=ws,
                                                      nb=nb, stream=None), **kw}[k]
                                             for k in ("op", "depth", "taps", "n_taps", "thr", "n", "h", "w", "out", "ws", "nb", "stream")])
    for kw in (dict(op=4), dict(op=-1), dict(depth=None), dict(taps=None), dict(out=None), dict(ws=None), dict(n_taps=0),
               dict(n_taps=-3), dict(n_taps=8), dict(n=0), dict(h=0), dict(w=-1), dict(out=d), dict(ws=o), dict(taps=196),
               dict(depth=66)):
        assert call(**kw) == _native.CS_EINVAL, kw
    assert call(nb=nb - 1) == _native.CS_EWORKSPACE
    assert call(n_taps=cap + 2) == _native.CS_ELIMIT
    assert call(n_taps=cap, nb=0) == _native.CS_EWORKSPACE   # (the cap itself passes the limit check)
