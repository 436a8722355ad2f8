"""StereoDiffusion's Standard mode around its models (cs_latent_shift_plan, cs_latent_shift_apply, cs_decode_to_codes;
diffusion_utils.diffusion_step and friends; stereodiffusion_nodes.text2stereoimage and generate_stereo_standard): the public
surface, the argument refusals, and the numpy restatement the GPU tests check the kernels against (tools/standard_oracle.py) held
to the reference's own values in tests/golden/standard_mode.npz, on the CPU (not gpu).  Every comparison is bit for bit."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import pil_resize_oracle as po
import standard_fake_model as fm
import standard_oracle as so
from comfystereo_amd import _native, diffusion_utils, engine
from comfystereo_amd import stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cs_latent_shift_plan_workspace_bytes", "cs_latent_shift_plan", "cs_latent_shift_apply", "cs_decode_to_codes"]


def load():
    z = np.load(os.path.join(ROOT, "tests", "golden", "standard_mode.npz"))
    return z, json.loads(str(z["meta"]))


def bits(t):
    """A float tensor's bit patterns as a numpy integer array (what a kernel that only moves values must reproduce)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def fixture_bits(a):
    """A fixture array of latents (float32, float16, or bfloat16's int16 patterns) as integer bit patterns."""
    return a if a.dtype == np.int16 else a.view(np.int32 if a.dtype == np.float32 else np.int16)


def fixture_tensor(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.bfloat16) if dtype == torch.bfloat16 else t


def test_new_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "comfystereo_amd.h")).read()
    declared = set(re.findall(r"CS_API\s+[\w\s\*]+?\b(cs_\w+)\s*\(", hdr))
    L = _native.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _native.EXPORTS, name
        assert hasattr(L, name), name
    assert L.cs_version() == 4 == _native.ABI_VERSION
    for name, value in re.findall(r"CS_LATENT_(FIRST|RESHIFT) = (\d+)", hdr):
        assert _native.LATENT_OP[name.lower()] == int(value)
    assert len(_native.LATENT_OP) == 2
    for name, key in (("F32", "float32"), ("F16", "float16"), ("BF16", "bfloat16")):
        assert int(re.search(rf"CS_LATENT_{name} = (\d+)", hdr).group(1)) == _native.LATENT_DTYPE[key]
    assert L.cs_latent_shift_plan_workspace_bytes() >= 64


def test_python_signatures_and_docs():
    assert str(inspect.signature(engine.latent_shift_plan)) == "(disp, scale_factor, stereo_offset_exponent=1.0)"
    assert str(inspect.signature(engine.latent_shift_apply)) == "(left, right, src_col, mask, op, noise=None)"
    assert str(inspect.signature(engine.decode_to_codes)) == "(image)"
    assert str(inspect.signature(diffusion_utils.diffusion_step)) == \
        "(model, controller, latents, context, t, guidance_scale, low_resource=False)"
    assert str(inspect.signature(diffusion_utils.diffusion_step_no_cfg)) == "(model, controller, latents, context, t)"
    assert str(inspect.signature(diffusion_utils.init_latent)) == "(latent, model, height, width, generator, batch_size)"
    assert str(inspect.signature(sdn.text2stereoimage)) == \
        ("(model, prompt, uncond_embeddings, latent, disparity, scale_factor, direction, deblur, num_inference_steps, "
         "guidance_scale, noise=None, generator=None)")
    assert str(inspect.signature(sdn.generate_stereo_standard)) == \
        ("(image, depth_map, scale_factor, direction, deblur, num_inference_steps, guidance_scale, model, invert, noise=None, "
         "generator=None)")
    doc = sdn.__doc__
    out_of_scope = doc[doc.index("Out of scope"):]
    assert "generate_stereo_standard" in doc and "inversion" in out_of_scope and "wrappers" in out_of_scope
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (readme, design):
        assert "generate_stereo_standard" in text and "tools/standard_bench.py" in text and "not yet measured" in text


def test_c_abi_refusals_come_before_any_launch():
    L = _native.lib()
    left, right, src, mask, noise, ws = 1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 32, 1 << 34   # host addresses: never touched
    big = 1 << 20
    plan, apply_, decode = L.cs_latent_shift_plan, L.cs_latent_shift_apply, L.cs_decode_to_codes
    assert plan(None, 1, 4, 4, 8.0, 1.0, src, ws, big, None) == _native.CS_EINVAL
    assert plan(left, 1, 4, 4, 8.0, 1.0, None, ws, big, None) == _native.CS_EINVAL
    assert plan(left, 1, 4, 4, 8.0, 1.0, src, None, big, None) == _native.CS_EINVAL
    for dims in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert plan(left, *dims, 8.0, 1.0, src, ws, big, None) == _native.CS_EINVAL, dims
    assert plan(left, 1, 4, 4, float("nan"), 1.0, src, ws, big, None) == _native.CS_EINVAL
    assert plan(left, 1, 4, 4, 8.0, float("inf"), src, ws, big, None) == _native.CS_EINVAL
    assert plan(left, 1, 4, 16385, 8.0, 1.0, src, ws, big, None) == _native.CS_ELIMIT
    assert plan(left, 1, 4, 8193, 8.0, 1.0, src, ws, big, None) == _native.CS_ELIMIT
    assert plan(left, 65536, 4, 4, 8.0, 1.0, src, ws, big, None) == _native.CS_ELIMIT
    assert plan(left, 1, 4, 4, 8.0, 1.0, src, ws, L.cs_latent_shift_plan_workspace_bytes() - 1, None) == _native.CS_EWORKSPACE
    ok = (0, 1, 4, 8, 8)
    for args in ((None, right, src, mask, None), (left, None, src, mask, None), (left, right, None, mask, None)):
        assert apply_(*args, *ok, 0, None) == _native.CS_EINVAL, args
    for op in (0, 1):
        assert apply_(left, right, src, None, None, *ok, op, None) == _native.CS_EINVAL    # a null mask, RESHIFT's included
    assert b"CS_LATENT_RESHIFT" in L.cs_last_error()
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 4, -8, 8)):
        assert apply_(left, right, src, mask, None, 0, *dims, 0, None) == _native.CS_EINVAL, dims
    for dtype in (-1, 3):
        assert apply_(left, right, src, mask, None, dtype, 1, 4, 8, 8, 0, None) == _native.CS_EINVAL
        assert decode(left, dtype, 1, 3, 8, 8, right, None) == _native.CS_EINVAL
    for op in (-1, 2):
        assert apply_(left, right, src, mask, None, *ok, op, None) == _native.CS_EINVAL
    assert apply_(left, left + 16, src, mask, None, *ok, 0, None) == _native.CS_EINVAL      # right overlaps left
    assert apply_(left, right, src, mask, right + 4, *ok, 0, None) == _native.CS_EINVAL     # right overlaps noise
    assert b"overlap" in L.cs_last_error()
    assert decode(None, 0, 1, 3, 8, 8, right, None) == _native.CS_EINVAL
    assert decode(left, 0, 1, 3, 8, 8, None, None) == _native.CS_EINVAL
    for dims in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert decode(left, 0, *dims, right, None) == _native.CS_EINVAL, dims
    assert decode(left, 0, 1, 3, 8, 8, left + 8, None) == _native.CS_EINVAL


def test_python_refusals_come_before_the_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_native, "lib", no_lib)
    d = torch.zeros(1, 4, 8)
    for bad in (d.numpy(), d.double(), d[0], torch.zeros(1, 0, 8), d.transpose(1, 2), torch.zeros(1, 2, 8193)):
        with pytest.raises(ValueError):
            engine.latent_shift_plan(bad, 8.0)
    for sf, e in ((float("nan"), 1.0), (8.0, float("inf"))):
        with pytest.raises(ValueError):
            engine.latent_shift_plan(d, sf, e)
    lat = torch.zeros(2, 4, 8, 8)
    left, right = lat[:1], lat[1:]
    src, mask = torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8, dtype=torch.uint8)
    bad_calls = [
        (left, right, src, mask, "again", None), (left.numpy(), right, src, mask, "first", None),
        (left, right.half(), src, mask, "first", None), (left.double(), right.double(), src, mask, "first", None),
        (left, right[:, :2], src, mask, "first", None), (left, right.transpose(2, 3), src, mask, "first", None),
        (left, right, src.long(), mask, "first", None), (left, right, src[:, :4], mask, "first", None),
        (left, right, src, mask.bool(), "first", None), (left, right, src, None, "reshift", None),
        (left, right, src, mask, "reshift", right.clone()), (left, right, src, mask, "first", right.half()),
        (left[0], right[0], src, mask, "first", None),
    ]
    for args in bad_calls:
        with pytest.raises(ValueError):
            engine.latent_shift_apply(*args[:5], noise=args[5])
    for bad in (lat.numpy(), lat.double(), lat[0], torch.zeros(1, 3, 0, 8), lat.transpose(2, 3)):
        with pytest.raises(ValueError):
            engine.decode_to_codes(bad)
    model = fm.FakeModel()
    disp = torch.zeros(1, 512, 512)
    ok = dict(model=model, prompt=["", ""], uncond_embeddings=None, latent=None, disparity=disp, scale_factor=8.0, direction="uni",
              deblur=False, num_inference_steps=10, guidance_scale=3.0)
    for change in (dict(prompt=[""]), dict(prompt="ab"), dict(direction="both"), dict(num_inference_steps=0), dict(disparity=disp[0]),
                   dict(disparity=disp.double()), dict(latent=torch.zeros(4, 64, 64)), dict(noise=torch.zeros(1, 4, 64, 64))):
        with pytest.raises(ValueError):
            sdn.text2stereoimage(**{**ok, **change})
    img, dep = torch.zeros(1, 40, 56, 3), torch.zeros(1, 40, 56, 3)
    inv = lambda u8: fm.fake_invert(u8)
    for args in ((img.numpy(), dep, 8.0, "uni", False, 10, 3.0, model, inv), (img, dep, 8.0, "uni", False, 10, 3.0, model, None),
                 (img[0], dep[0], 8.0, "uni", False, 10, 3.0, model, inv), (img, dep[:, :20], 8.0, "uni", False, 10, 3.0, model, inv),
                 (img, dep, 8.0, "sideways", False, 10, 3.0, model, inv), (img.to(torch.uint8), dep, 8.0, "uni", False, 10, 3.0, model, inv)):
        with pytest.raises(ValueError):
            sdn.generate_stereo_standard(*args)


def test_without_a_gpu_the_new_functions_raise_the_usual_error(monkeypatch):
    # (on a machine that has a GPU: what the package does when torch reports none; host tensors never reach the library)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    lat = torch.zeros(2, 4, 8, 8)
    src, mask = torch.zeros(1, 8, 8, dtype=torch.int32), torch.zeros(1, 8, 8, dtype=torch.uint8)
    model = fm.FakeModel()
    calls = [
        lambda: engine.latent_shift_plan(torch.zeros(1, 8, 8), 8.0),
        lambda: engine.latent_shift_apply(lat[:1], lat[1:], src, mask, "first"),
        lambda: engine.decode_to_codes(lat),
        lambda: sdn.text2stereoimage(model, ["", ""], None, None, torch.zeros(1, 512, 512), 8.0, "uni", False, 10, 3.0),
        lambda: sdn.generate_stereo_standard(torch.zeros(1, 40, 56, 3), torch.zeros(1, 40, 56, 3), 8.0, "uni", False, 10, 3.0, model,
                                             fm.fake_invert),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert "forward" not in model.unet.__dict__


def test_diffusion_steps_on_the_stand_in_model():
    """diffusion_step / diffusion_step_no_cfg / init_latent are plain torch: on the CPU they give what their definitions say."""
    model = fm.FakeModel()
    ctrl = sdn._EmptyControl()
    g = torch.Generator().manual_seed(3)
    latent, latents = diffusion_utils.init_latent(None, model, 512, 512, g, 2)
    assert tuple(latent.shape) == (1, 4, 64, 64) and tuple(latents.shape) == (2, 4, 64, 64) and torch.equal(latents[0], latents[1])
    given, expanded = diffusion_utils.init_latent(latent, model, 512, 512, None, 2)
    assert given is latent and torch.equal(expanded, latents)
    emb = model.text_encoder(torch.zeros(2, 77))[0]
    unc = fm.fake_uncond_embeddings(1, "cpu", torch.float32)[0].expand(2, -1, -1)
    ctx = torch.cat([unc, emb])
    pu = model.unet(latents, 0, encoder_hidden_states=unc)["sample"]
    pt = model.unet(latents, 0, encoder_hidden_states=emb)["sample"]
    want = latents - 0.125 * (pu + 3.0 * (pt - pu))
    assert torch.equal(diffusion_utils.diffusion_step(model, ctrl, latents, ctx, 0, 3.0), want)
    assert torch.equal(diffusion_utils.diffusion_step(model, ctrl, latents, [unc, emb], 0, 3.0, low_resource=True), want)
    assert torch.equal(diffusion_utils.diffusion_step_no_cfg(model, ctrl, latents, emb, 0), latents - 0.125 * pt)


def test_fixture_margin_and_coverage():
    z, meta = load()
    assert meta["margin"] >= 1e-3 and meta["steps"] == 10 and meta["shift_step"] == 2 and meta["reshifts"] == [4, 6, 8]
    for name, d in meta["depths"].items():
        assert d["margin"] >= 1e-3 and so.margin(z[f"disp_latent/{name}"], 8.0) == d["margin"], name
    cases = meta["cases"]
    assert {c["dtype"] for c in cases} == {"float32", "float16", "bfloat16"}
    for key, values in (("deblur", {True, False}), ("direction", {"uni", "bi"}), ("uncond", {True, False}), ("depth", {"gray", "rgb"})):
        assert {c[key] for c in cases} == values, key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "standard_mode.npz")) < 1 << 20


def run_case_on_the_cpu(z, meta, c):
    """The Standard mode of one fixture case from the restatement: numpy for the plan, the shift, the mask, the merge, the codes
    and the resizes; CPU torch for the stand-in model and the bicubic disparity resize, which the reference runs there too."""
    dtype = getattr(torch, c["dtype"])
    steps = meta["steps"]
    image, depth = z["image"], z[f"depth/{c['depth']}"]
    img512 = po.resize_hw(so.image_codes(image[0]), 512, 512)
    dep_u8 = so.image_codes(depth[0])
    d512 = po.resize_hw(po.gray_codes(dep_u8)[..., None], 512, 512)[..., 0]
    disp = so.disparity_512(d512)
    lat_disp = torch.nn.functional.interpolate(torch.from_numpy(disp).unsqueeze(1), size=[64, 64], mode="bicubic",
                                               align_corners=False).squeeze(1).numpy()
    src_col = so.plan(lat_disp, c["scale_factor"])
    model = fm.FakeModel("cpu", dtype)
    x_t, unc = fm.fake_invert(torch.from_numpy(img512), dtype, steps if c["uncond"] else None)
    emb = model.text_encoder(torch.zeros(2, 77))[0]
    _, latents = diffusion_utils.init_latent(torch.cat([x_t, x_t]), model, 512, 512, None, 2)
    model.scheduler.set_timesteps(steps)
    out = dict(disp512=disp, disp_latent=lat_disp)
    mask = None
    for i, t in enumerate(model.scheduler.timesteps[-steps:]):
        ctx = torch.cat([unc[i].expand(*emb.shape) if unc is not None else emb, emb])
        latents = diffusion_utils.diffusion_step(model, sdn._EmptyControl(), latents, ctx, t, meta["guidance_scale"])
        b = bits(latents).copy()
        if i == meta["shift_step"]:
            noise = fixture_bits(z[f"{c['id']}/noise_right"]) if c["deblur"] else None
            b[1:], mask = so.apply_first(b[:1], src_col, noise)
            out["latents_shift_right"] = b[1:].copy()
        elif i in meta["reshifts"]:
            b[1:] = so.apply_reshift(b[:1], b[1:], src_col, mask)
        latents = torch.from_numpy(b).view(dtype)
    out["mask"], out["latents_final"] = mask, bits(latents)
    decoded = model.vae.decode(1 / 0.18215 * latents)["sample"]
    out["codes"] = so.decode_to_codes(decoded.double().numpy(), c["dtype"])
    h, w = image.shape[1:3]
    eyes = [po.code_floats(po.resize(out["codes"][k], (w, h))) for k in range(2)]
    out["stereo"] = np.concatenate(eyes, 1)[None]
    return out


def test_restatement_reproduces_every_array_of_the_fixture():
    z, meta = load()
    for c in meta["cases"]:
        got = run_case_on_the_cpu(z, meta, c)
        for key in ("disp512", "disp_latent"):
            assert np.array_equal(got[key], z[f"{key}/{c['depth']}"]), (c["id"], key)
        for key in ("latents_shift_right", "latents_final"):
            assert np.array_equal(got[key], fixture_bits(z[f"{c['id']}/{key}"])), (c["id"], key)
        for key in ("mask", "codes", "stereo"):
            assert np.array_equal(got[key], z[f"{c['id']}/{key}"]), (c["id"], key)
        assert 0 < got["mask"].mean() < 1
