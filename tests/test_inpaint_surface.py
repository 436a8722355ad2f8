"""StereoDiffusion Fast mode's warp, inpaint mask and gap pre-fill (cs_inpaint_prepare): the public surface, the host-side
argument validation and the numpy restatement the GPU tests check the kernels against (tools/inpaint_oracle.py) held to the
reference's own outputs in tests/golden/inpaint_prep.npz, on the CPU (not gpu)."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import grid_oracle as go
import inpaint_oracle as io
from comfystereo_amd import _native, engine
from comfystereo_amd import stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cs_inpaint_prepare_workspace_bytes", "cs_inpaint_prepare_max_width", "cs_inpaint_prepare"]


def load():
    z = np.load(os.path.join(ROOT, "tests", "golden", "inpaint_prep.npz"))
    return z, json.loads(str(z["meta"]))


def case_inputs(z, meta, c):
    """image float32 [3,S,S] (k / 255: the reference's img_t) and depth float32 [S,S] (the gray codes, 0..255) of a case."""
    s = meta["size"]
    img = io.image_u8(s, s, c["image_seed"]).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(img.transpose(2, 0, 1)), z[f"{c['id']}/depth"].astype(np.float32)


def expected_mask(z, meta, c):
    s = meta["size"]
    if not c["called"]:
        return np.zeros((s, s), dtype=bool)
    return np.unpackbits(z[f"{c['id']}/mask"], count=s * s).reshape(s, s).astype(bool)


def check_case(z, meta, c, mask, warped_u8, filled_u8):
    """The reference's observables of case c against a mask [S,S] bool and the two code planes [S,S,3] uint8."""
    cid, rows = c["id"], meta["rows"]
    want_mask = expected_mask(z, meta, c)
    assert np.array_equal(mask, want_mask), (cid, "mask", int((mask != want_mask).sum()))
    # the returned right eye: the recorder's constant under the mask, the warped codes elsewhere
    right = io.blend(want_mask, np.array(meta["constant"], np.uint8), warped_u8)
    assert np.array_equal(right[rows], z[f"{cid}/right_rows"]), (cid, "warped codes outside the mask")
    assert io.digest(right) == c["sha_right"], (cid, "warped codes outside the mask (digest)")
    if c["called"]:
        assert np.array_equal(filled_u8[rows], z[f"{cid}/filled_rows"]), (cid, "filled codes")
        assert io.digest(filled_u8) == c["sha_filled"], (cid, "filled codes (digest)")
    else:   # the early return: nothing to fill
        assert np.array_equal(filled_u8, warped_u8), (cid, "filled == warped")


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(L, name), name
    assert "stereodiffusion_nodes.py:425-571" in hdr
    assert L.cs_version() == 4


def test_python_signatures():
    assert str(inspect.signature(engine.inpaint_prepare)) == "(image, depth, scale_factor, threshold=0.05, codes=False)"
    assert str(inspect.signature(sdn.prepare_inpaint)) == "(image, depth, scale_factor, threshold=0.05)"
    assert str(inspect.signature(sdn.compose_stereo)) == "(left_u8, warped_u8, inpainted_u8, mask)"
    for word in ("resize", "diffusion model", "Out of scope"):
        assert word in sdn.__doc__, word


def test_host_side_validation():
    L = _native.lib()
    wmax = L.cs_inpaint_prepare_max_width()
    assert wmax >= 8192
    big = 1 << 40
    p = 16   # (any non-null host address: every refusal below comes before device work)
    call = L.cs_inpaint_prepare
    assert call(None, p, 1, 4, 8, 1.0, 0.05, p, p, p, p, p, p, big, None) == _native.CS_EINVAL
    assert call(p, None, 1, 4, 8, 1.0, 0.05, p, p, p, p, p, p, big, None) == _native.CS_EINVAL
    assert call(p, p, 1, 4, 8, 1.0, 0.05, p, p, p, p, p, None, big, None) == _native.CS_EINVAL
    for n, h, w in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8), (1, -4, 8), (1, 4, -8)):
        assert call(p, p, n, h, w, 1.0, 0.05, p, p, p, p, p, p, big, None) == _native.CS_EINVAL, (n, h, w)
        assert L.cs_inpaint_prepare_workspace_bytes(n, h, w) == 0
    assert call(p, p, 1, 4, wmax + 1, 1.0, 0.05, p, p, p, p, p, p, big, None) == _native.CS_ELIMIT
    assert b"too wide" in L.cs_last_error()
    need = L.cs_inpaint_prepare_workspace_bytes(2, 4, wmax)
    assert need >= 2 * 2 * 4 * (wmax // 32) * 4
    assert call(p, p, 2, 4, wmax, 1.0, 0.05, p, p, p, p, p, p, need - 1, None) == _native.CS_EWORKSPACE
    assert call(p, p, 1, 4, 8, 1.0, 0.05, p, p, p, p, p, p, 0, None) == _native.CS_EWORKSPACE
    # nothing asked for: nothing done
    assert call(p, p, 1, 4, 8, 1.0, 0.05, None, None, None, None, None, p, big, None) == _native.CS_OK


def test_python_argument_validation_needs_no_device():
    import pytest
    img, dep = torch.zeros(2, 3, 4, 8), torch.zeros(2, 4, 8)
    with pytest.raises(ValueError):
        engine.inpaint_prepare(img, dep, 5.0)               # host tensors: the engine takes device tensors only
    with pytest.raises(ValueError):
        sdn.prepare_inpaint(img, dep[0], 5.0)               # batched image, single depth
    with pytest.raises(ValueError):
        sdn.prepare_inpaint(img.numpy(), dep.numpy(), 5.0)
    u8 = torch.zeros(4, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        sdn.compose_stereo(u8, u8, u8.float(), torch.zeros(4, 8, dtype=torch.bool))
    with pytest.raises(ValueError):
        sdn.compose_stereo(u8, u8, u8, torch.zeros(4, 9, dtype=torch.bool))
    with pytest.raises(ValueError):
        sdn.compose_stereo(u8, u8, u8, torch.zeros(4, 8, dtype=torch.uint8))


def test_compose_stereo_on_host_tensors_equals_numpy():
    rng = np.random.default_rng(3)
    left, warped, inp = (rng.integers(0, 256, (2, 5, 7, 3)).astype(np.uint8) for _ in range(3))
    mask = rng.random((2, 5, 7)) < 0.4
    stereo, l, r = sdn.compose_stereo(*(torch.from_numpy(a) for a in (left, warped, inp, mask)))
    want = np.stack([io.blend(mask[k], inp[k], warped[k]) for k in range(2)])
    assert np.array_equal(r.numpy(), want) and np.array_equal(l.numpy(), left)
    assert np.array_equal(stereo.numpy(), np.concatenate([left, want], axis=2))   # (np.hstack of one frame, :571)


def test_restatement_reproduces_every_fixture_case():
    z, meta = load()
    ids = [c["id"] for c in meta["cases"]]
    assert len(ids) == len(set(ids)) >= 8
    by = {c["id"]: c for c in meta["cases"]}
    # the ground the fixture has to cover: both signs, an empty mask, both frame edges, fully masked rows, an RGB depth
    assert any(c["scale_factor"] > 0 and c["called"] for c in meta["cases"])
    assert any(c["scale_factor"] < 0 and c["called"] for c in meta["cases"])
    assert any(not c["called"] for c in meta["cases"])
    assert any(all(c["edge_columns"]) for c in meta["cases"])
    assert any(c["full_rows"] > 0 for c in meta["cases"]) and "rgb_m3" in by
    for c in meta["cases"]:
        img, depth = case_inputs(z, meta, c)
        wr, fl, m = io.prepare(img[None], depth[None], c["scale_factor"])
        check_case(z, meta, c, m[0], io.codes(wr[0]), io.codes(fl[0]))
        if c["full_rows"]:
            full = m[0].all(1)
            assert int(full.sum()) == c["full_rows"] and not fl[0][:, full].any()   # fully masked rows come out black


def test_restatement_batches_frame_by_frame_with_mixed_scales():
    z, meta = load()
    cases = [c for c in meta["cases"] if c["id"] in ("disc_p5", "flat", "band_p5")]
    imgs, deps = zip(*(case_inputs(z, meta, c) for c in cases))
    imgs, deps = np.stack(imgs)[:, :, :40, :96], np.stack(deps)[:, :40, :96].copy()
    deps[1] /= np.float32(255.0)   # one frame on the 0..1 scale next to two on 0..255
    wr, fl, m = io.prepare(imgs, deps, 5.0)
    for k in range(3):
        one = io.prepare(imgs[k:k + 1], deps[k:k + 1], 5.0)
        for a, b in zip((wr, fl, m), one):
            assert np.array_equal(a[k], b[0])


def test_restatement_sampler_equals_cpu_grid_sample_on_the_fixture_grids():
    z, meta = load()
    for c in meta["cases"]:
        img, depth = case_inputs(z, meta, c)
        s = meta["size"]
        d = io.depth_chain(depth)
        gxw = (go.linspace(s) - (d * np.float32(-(c["scale_factor"] / 100.0) * s)) / np.float32(s / 2)).astype(np.float32)[None]
        gy = np.ascontiguousarray(np.broadcast_to(go.linspace(s)[None, :, None], (1, s, s)))
        grid = torch.from_numpy(np.stack([gxw, gy], -1))
        want = F.grid_sample(torch.from_numpy(img[None]), grid, mode="bilinear", padding_mode="border", align_corners=True).numpy()
        got = go.sample_bilinear(img[None], gxw, gy, "border")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["id"], "bilinear")
        d2 = (d + np.float32(0.5))[None, None]
        want = F.grid_sample(torch.from_numpy(d2), grid, mode="nearest", padding_mode="border", align_corners=True).numpy()
        got = go.sample_nearest(d2, gxw, gy, "border")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["id"], "nearest")
