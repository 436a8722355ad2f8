#!/usr/bin/env python3
"""Fixture of StereoDiffusion's Standard mode around its models: tests/golden/standard_mode.npz.

Build-machine only, like tools/make_fastmode_goldens.py: loads the reference's stereodiffusion_nodes through tools/refload.py and
runs StereoDiffusionNode._generate_stereo_impl itself (CPU torch, Pillow, with _text2stereoimage and stereo_shift_torch inside)
on seeded inputs.  The models are tools/standard_fake_model.py's: load_sd_model returns the fake model, NullInversion is
replaced by fake_invert; nothing of the reference's arithmetic is replaced.  Three of its functions are wrapped to look at
what passes through them: torch.randn_like (the deblur noise), stereo_shift_torch (the first call's channel 0 gives the mask),
the fake scheduler's step (the last result is the final latents) and the fake UNet, which records the latents it is handed (the
call after the shift step sees the shifted latents).

  python tools/make_standard_goldens.py
Layout: `meta` = JSON {steps, shift_step, reshifts, guidance_scale, versions, margin (the worst over the depths), depths:
{name: {seed, coloured, margin}}, cases: [{id, depth, dtype, deblur, direction, uncond, scale_factor}]}; arrays
'image' (float32 [1,H,W,3]), 'depth/<name>' (float32 [1,H,W,3]), 'disp512/<name>' (float32 [1,512,512]), 'disp_latent/<name>'
(float32 [1,64,64]); per case 'cid/latents_shift_right' ([1,4,64,64]: the right view after the shift step; the left view is not
touched by the shift), 'cid/latents_final' ([2,4,64,64]) -- bfloat16 as its int16 bit pattern --, 'cid/mask' (uint8 [1,64,64]),
'cid/noise_right' (deblur only: the right-view half of the tensor torch.randn_like returned, the half the reference reads),
'cid/codes' (uint8 [2,512,512,3]), 'cid/stereo' (float32 [1,H,2W,3], the node's first output; its second and third are the two
halves, asserted here).  The file stays below the 1 MiB a committed file may have.

Asserted while making it: for every depth, every shift product norm(disp_latent) * scale_px is exactly 0 or at least 1e-3
away from every integer (seeds are retried until the reference's own disparity says so), so a disparity that differs from the
reference's by less than that cannot change a truncated shift.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pil_resize_oracle as po  # noqa: E402
import standard_fake_model as fm  # noqa: E402
import standard_oracle as so  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "standard_mode.npz")
H, W = 40, 56
STEPS, GUIDANCE, SCALE = 10, 3.0, 8.0
MARGIN = 1e-3

# (id, depth, dtype, deblur, direction, uncond embeddings given)
CASES = [
    ("gray_f32_uni", "gray", "float32", False, "uni", False),
    ("gray_f32_bi_deblur_uncond", "gray", "float32", True, "bi", True),
    ("gray_f16_uni_deblur_uncond", "gray", "float16", True, "uni", True),
    ("rgb_bf16_bi_deblur", "rgb", "bfloat16", True, "bi", False),
]


def node_floats(u8):
    """uint8 -> the float32 array tensor_to_numpy maps back onto exactly these codes ((k + 0.5) / 255: safe under truncation)."""
    return (u8.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)


def image_u8(seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((H, W, 3), dtype=np.int64)
    for step, weight in ((16, 2), (4, 1), (1, 1)):
        g = rng.integers(0, 256, ((H + step - 1) // step, (W + step - 1) // step, 3))
        out += weight * np.repeat(np.repeat(g, step, 0), step, 1)[:H, :W]
    return (out // 4).astype(np.uint8)


def depth_u8(seed, coloured):
    """uint8 [H,W,3]: a few flat levels in blocks (most latent pixels then sit on a handful of disparities)."""
    rng = np.random.default_rng(seed)
    levels = rng.integers(0, 256, (3, 4))
    base = np.repeat(np.repeat(levels, (H + 2) // 3, 0), W // 4, 1)[:H, :W].astype(np.int64)
    if not coloured:
        return np.repeat(base[..., None], 3, -1).astype(np.uint8)
    return np.stack([base, np.clip(base + 20, 0, 255), 255 - base // 2], -1).astype(np.uint8)


def reference_disparity(torch, Image, dep_u8):
    """The reference's own lines (:253-265, :617-622) -> (disp512, disp_latent) float32, or None when this project's gray rule
    differs from the reference's BLAS product on a pixel."""
    gray = np.dot(dep_u8[..., :3], [0.2989, 0.5870, 0.1140]).astype(np.uint8)
    if not np.array_equal(gray, po.gray_codes(dep_u8)):
        return None
    d512 = np.array(Image.fromarray(gray).resize((512, 512)))
    assert np.array_equal(d512, po.resize_hw(gray[..., None], 512, 512)[..., 0])
    disp = so.disparity_512(d512)
    lat = torch.nn.functional.interpolate(torch.from_numpy(disp).unsqueeze(1), size=[64, 64], mode="bicubic",
                                          align_corners=False).squeeze(1).numpy()
    return disp, lat


def to_np(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def main():
    import PIL
    import torch
    from PIL import Image
    import refload
    refload.quiet()
    mod = refload.load_sd_nodes()
    arrays = {"image": node_floats(image_u8(7))[None]}
    depths = {}
    for name, coloured in (("gray", False), ("rgb", True)):
        for seed in range(1000):
            dep = depth_u8(seed, coloured)
            r = reference_disparity(torch, Image, dep)
            if r is None:
                continue
            m = so.margin(r[1], SCALE)
            if m >= MARGIN:
                break
        else:
            raise SystemExit(f"no seed gives depth {name} a margin of {MARGIN}")
        arrays[f"depth/{name}"] = node_floats(dep)[None]
        arrays[f"disp512/{name}"], arrays[f"disp_latent/{name}"] = r
        depths[name] = dict(seed=seed, coloured=coloured, margin=m)
        print("depth", name, depths[name])

    cases = []
    for cid, dname, dtype_name, deblur, direction, uncond in CASES:
        dtype = getattr(torch, dtype_name)
        model = fm.FakeModel("cpu", dtype)
        model.unet.record = True
        seen = {"noise": None, "shift": [], "steps": []}
        real_step = model.scheduler.step

        def step(*a, **k):
            out = real_step(*a, **k)
            seen["steps"].append(out["prev_sample"])
            return out

        model.scheduler.step = step

        class Inversion:
            def __init__(self, ldm, steps, guidance_scale=None):
                self.steps = steps

            def invert(self, img_resized, prompt, **kwargs):
                x_t, unc = fm.fake_invert(torch.from_numpy(img_resized), dtype, self.steps if uncond else None)
                return (None, None), x_t, unc

        def randn_like(t, *a, **k):
            seen["noise"] = real_randn_like(t, *a, **k)
            return seen["noise"]

        def shift(*a, **k):
            out = real_shift(*a, **k)
            seen["shift"].append(out.clone())
            return out

        real_randn_like, real_shift = torch.randn_like, mod.stereo_shift_torch
        saved = (mod.load_sd_model, mod.NullInversion)
        mod.load_sd_model, mod.NullInversion, mod.stereo_shift_torch = (lambda mid, dev: model), Inversion, shift
        torch.randn_like = randn_like
        codes = {}
        real_t2s = mod.StereoDiffusionNode._text2stereoimage

        def t2s(self, *a, **k):
            codes["u8"] = real_t2s(self, *a, **k)
            return codes["u8"]

        mod.StereoDiffusionNode._text2stereoimage = t2s
        try:
            torch.manual_seed(1000 + len(cases))
            node = mod.StereoDiffusionNode()
            stereo, left, right = node._generate_stereo_impl(torch.from_numpy(arrays["image"]), torch.from_numpy(arrays[f"depth/{dname}"]),
                                                             SCALE, direction, deblur, STEPS, False, GUIDANCE, None, None, None, "fake", None)
        finally:
            torch.randn_like = real_randn_like
            mod.load_sd_model, mod.NullInversion = saved
            mod.stereo_shift_torch = real_shift
            mod.StereoDiffusionNode._text2stereoimage = real_t2s
        shift_step = max(1, int(STEPS * 0.2))
        reshifts = [i for i in range(STEPS) if i > shift_step and i % shift_step == 0]
        assert len(model.unet.calls) == STEPS and len(seen["shift"]) == 1 + len(reshifts)
        assert (seen["noise"] is not None) == deblur
        lat_shift = model.unet.calls[shift_step + 1][:2]
        # the last step changes nothing after the scheduler: its result is the final latents
        lat_final = seen["steps"][-1]
        again = so.decode_to_codes(to_float(model.vae.decode(1 / 0.18215 * lat_final)["sample"]), dtype_name)
        assert np.array_equal(again, codes["u8"]), (cid, "final latents do not reproduce the reference's codes")
        assert torch.equal(lat_shift[:1], seen["steps"][shift_step][:1])   # the left view is the scheduler's: only the right is kept
        arrays[f"{cid}/latents_shift_right"] = to_np(lat_shift[1:])
        arrays[f"{cid}/latents_final"] = to_np(lat_final)
        arrays[f"{cid}/mask"] = (seen["shift"][0][1:, 0] != 0).numpy().astype(np.uint8)
        if deblur:
            arrays[f"{cid}/noise_right"] = to_np(seen["noise"][1:])   # (the reference reads noise[1:] only, :659)
        arrays[f"{cid}/codes"] = codes["u8"]
        assert stereo.shape == (1, H, 2 * W, 3) and torch.equal(left, stereo[:, :, :W]) and torch.equal(right, stereo[:, :, W:])
        arrays[f"{cid}/stereo"] = stereo.numpy()   # (left and right are its two halves)
        cases.append(dict(id=cid, depth=dname, dtype=dtype_name, deblur=deblur, direction=direction, uncond=uncond, scale_factor=SCALE))
        print(cid, "mask share", float(arrays[f"{cid}/mask"].mean()))
    versions = dict(pillow=PIL.__version__, numpy=np.__version__, torch=torch.__version__)
    meta = dict(steps=STEPS, shift_step=shift_step, reshifts=reshifts, guidance_scale=GUIDANCE, versions=versions,
                margin=min(d["margin"] for d in depths.values()), depths=depths, cases=cases)
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


def to_float(t):
    """The values of a tensor of any float dtype, exactly, as float64."""
    return t.detach().double().numpy()


if __name__ == "__main__":
    main()
