"""The reference's grid-sample warps (apply_stereo_divergence_gpu, warp_and_fill_gpu, compute_forward_mask_gpu,
detect_disocclusions_gpu, interpolate_fill_gpu, apply_stereo_divergence_gpu_with_fill): the public surface and the numpy
restatement the GPU tests check the kernels against (tools/grid_oracle.py), on the CPU (not gpu)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grid_oracle as go
from comfystereo_amd import _native
from comfystereo_amd import stereoimage_generation as sig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FUNCS = ["apply_stereo_divergence_gpu", "warp_and_fill_gpu", "compute_forward_mask_gpu", "detect_disocclusions_gpu",
         "interpolate_fill_gpu", "apply_stereo_divergence_gpu_with_fill"]
NEW_EXPORTS = ["cs_grid_warp_workspace_bytes", "cs_grid_warp_max_width", "cs_grid_warp", "cs_interpolate_fill",
               "cs_detect_disocclusions"]


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(str(z["meta"]))


def unpack(bits, shape):
    return np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)


def oracle_case(z, c):
    """The restatement's outputs for fixture case c: a dict of the fixture's output fields."""
    cid, fn = c["id"], c["fn"]
    if fn == "interpolate_fill_gpu":
        b, ch, h, w = c["shape"]
        return dict(filled=go.interpolate_fill_gpu(z[f"{cid}/image"], unpack(z[f"{cid}/mask"], (b, h, w))))
    if fn == "detect_disocclusions_gpu":
        m = go.detect_disocclusions_gpu(z[f"{cid}/depth"], z[f"{cid}/grid"], z[f"{cid}/gxw"], c["threshold"])
        return dict(mask=m)
    args = (c["divergence_px"], c["separation_px"], c["exponent"], c["convergence"])
    if fn == "compute_forward_mask_gpu":
        return dict(mask=go.compute_forward_mask_gpu(z[f"{cid}/depth"], *args))
    if fn == "apply_stereo_divergence_gpu":
        return dict(warped=go.apply_stereo_divergence_gpu(z[f"{cid}/image"], z[f"{cid}/depth"], *args))
    if fn == "warp_and_fill_gpu":
        wr, m = go.warp_and_fill_gpu(z[f"{cid}/image"], z[f"{cid}/depth"], *args)
        return dict(warped=wr, mask=m)
    img = z[f"{cid}/image"]
    if c["layout"] == "hwc":
        img = img.transpose(2, 0, 1)
    _, h, w = img.shape
    wr, v = go.apply_stereo_divergence_gpu_with_fill(img, z[f"{cid}/depth"].reshape(h, w), *args, fill_mode=c["fill_mode"])
    return dict(warped=wr, valid=v)


def expected_case(z, c):
    cid, fn = c["id"], c["fn"]
    out = {}
    for k in ("warped", "filled"):
        if f"{cid}/{k}" in z.files:
            out[k] = z[f"{cid}/{k}"]
    if f"{cid}/mask" in z.files:
        if fn == "interpolate_fill_gpu":
            pass
        elif fn == "detect_disocclusions_gpu":
            out["mask"] = unpack(z[f"{cid}/mask"], tuple(c["shape"]))
        else:
            b, _, h, w = c["shape"]
            out["mask"] = unpack(z[f"{cid}/mask"], (b, h, w))
    if f"{cid}/valid" in z.files:
        out["valid"] = unpack(z[f"{cid}/valid"], tuple(z[f"{cid}/valid_shape"]))
    return out


def test_the_six_functions_exist_with_the_reference_signatures():
    want = json.load(open(os.path.join(GOLDEN, "grid_signatures.json")))
    assert sorted(want) == sorted(FUNCS)
    for name in FUNCS:
        assert str(inspect.signature(getattr(sig, name))) == want[name], name
    doc = sig.__doc__
    for name in FUNCS:
        assert name in doc, f"{name} missing from the module docstring's list of extras"


def test_restatement_is_bit_equal_to_every_small_fixture():
    z, meta = load("grid_warp.npz")
    fns = set()
    for c in meta["cases"]:
        got, want = oracle_case(z, c), expected_case(z, c)
        assert set(want) <= set(got), c["id"]
        for k, v in want.items():
            g = got[k].reshape(v.shape)
            if v.dtype == bool:
                assert np.array_equal(g, v), (c["id"], k)
            else:
                assert np.array_equal(g.view(np.uint32), v.view(np.uint32)), (c["id"], k, float(np.abs(g - v).max()))
        fns.add(c["fn"])
    assert fns == set(FUNCS)


def test_restatement_is_bit_equal_to_the_1080p_fixture():
    import make_grid_goldens as mg
    z, meta = load("grid_warp_1080p.npz")
    img, depth = mg.inputs_1080p()
    rows, p = meta["rows"], meta["warp"]
    args = (p["divergence_px"], p["separation_px"], p["exponent"], p["convergence"])
    assert np.array_equal(go.apply_stereo_divergence_gpu(img, depth, *args)[:, :, rows], z["asd/rows"])
    wr, m = go.warp_and_fill_gpu(img, depth, *args)
    assert np.array_equal(np.packbits(m), z["waf/mask"]) and np.array_equal(wr[:, :, rows], z["waf/rows"])
    m = go.compute_forward_mask_gpu(depth, meta["mask"]["divergence_px"], meta["mask"]["separation_px"], p["exponent"], p["convergence"])
    assert np.array_equal(np.packbits(m), z["cfm/mask"])
    f = meta["fill"]
    wr, v = go.apply_stereo_divergence_gpu_with_fill(img[0], depth[0], f["divergence_px"], f["separation_px"], p["exponent"],
                                                     p["convergence"], f["fill_mode"])
    assert np.array_equal(np.packbits(v), z["wf/valid"]) and np.array_equal(wr[:, rows], z["wf/rows"])
    mi = go.block_depth_u8(1080, 1920, meta["interp_mask"]["seed"])[None] > meta["interp_mask"]["above"]
    assert np.array_equal(go.interpolate_fill_gpu(img[:1], mi)[:, :, rows], z["ifg/rows"])


def test_restatement_linspace_equals_torch_for_every_width_up_to_16384():
    for n in range(1, 16385):
        assert np.array_equal(go.linspace(n), torch.linspace(-1, 1, n).numpy()), n


@pytest.mark.parametrize("padding", ["border", "zeros", "reflection", "nearest"])
def test_restatement_sampler_equals_cpu_grid_sample(padding):
    rng = np.random.default_rng({"border": 1, "zeros": 2, "reflection": 3, "nearest": 4}[padding])
    for _ in range(150):
        b, c, h, w = rng.integers(1, 3), rng.choice([1, 3, 4]), rng.integers(1, 9), rng.integers(1, 40)
        img = (rng.random((b, c, h, w), dtype=np.float32) * np.float32(rng.choice([1, 300]))).astype(np.float32)
        g = ((rng.random((b, h, w, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(rng.choice([2.2, 6, 50, 1e4]))).astype(np.float32)
        mode, pad = ("nearest", "border") if padding == "nearest" else ("bilinear", padding)
        want = F.grid_sample(torch.from_numpy(img), torch.from_numpy(g), mode=mode, padding_mode=pad, align_corners=True).numpy()
        got = (go.sample_nearest if mode == "nearest" else go.sample_bilinear)(img, g[..., 0], g[..., 1], pad)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (b, c, h, w)


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(L, name), name
    for name, v in (("CS_GRID_WARP", 0), ("CS_GRID_FILL", 1), ("CS_GRID_MASK", 2), ("CS_GRID_STRETCH", 3),
                    ("CS_GRID_PAD_BORDER", 0), ("CS_GRID_PAD_ZEROS", 1), ("CS_GRID_PAD_REFLECTION", 2)):
        assert re.search(rf"\b{name} = {v}\b", hdr), name
    assert L.cs_version() == 4


def test_host_side_validation_of_the_new_entries():
    L = _native.lib()
    wmax = L.cs_grid_warp_max_width(_native.GRID_OP["stretch"])
    assert wmax >= 16384 and wmax == L.cs_grid_warp_max_width(_native.GRID_OP["mask"])
    assert L.cs_grid_warp_max_width(7) == 0
    ws = ctypes_buf(L.cs_grid_warp_workspace_bytes(1, 4, wmax + 1))
    p = 16   # (any non-null host address: every refusal below comes before device work)
    assert L.cs_grid_warp(p, p, 1, 3, 4, wmax + 1, 1.0, 0.0, 2.0, 0.5, 3, 0, p, p, ws, 1 << 20, None) == _native.CS_ELIMIT
    assert L.cs_grid_warp(p, p, 1, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 4, 0, p, p, ws, 1 << 20, None) == _native.CS_EINVAL
    assert L.cs_grid_warp(p, p, 1, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 0, 1, p, None, ws, 1 << 20, None) == _native.CS_EINVAL
    assert L.cs_grid_warp(p, p, 1, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 1, 3, p, p, ws, 1 << 20, None) == _native.CS_EINVAL
    assert L.cs_grid_warp(p, p, 1, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 3, 0, p, p, ws, 0, None) == _native.CS_EWORKSPACE
    assert L.cs_grid_warp(None, p, 1, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 3, 0, p, p, ws, 1 << 20, None) == _native.CS_EINVAL
    assert L.cs_grid_warp(p, p, 0, 3, 4, 8, 1.0, 0.0, 2.0, 0.5, 3, 0, p, p, ws, 1 << 20, None) == _native.CS_EINVAL
    assert L.cs_interpolate_fill(p, None, 1, 3, 4, 8, p, None) == _native.CS_EINVAL
    assert L.cs_interpolate_fill(p, p, 1, 3, 4, 8, p, None) == _native.CS_EINVAL   # (out aliases image)
    assert L.cs_detect_disocclusions(p, p, p, 4, 1, 0.02, p, None) == _native.CS_EINVAL


def ctypes_buf(n):
    import ctypes
    return ctypes.cast(ctypes.create_string_buffer(max(int(n), 16)), ctypes.c_void_p)
