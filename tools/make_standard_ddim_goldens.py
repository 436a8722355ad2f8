#!/usr/bin/env python3
"""Fixture of StereoDiffusion's Standard loop under a real DDIM step: tests/golden/standard_ddim.npz.

Build-machine only, like tools/make_standard_goldens.py: loads the reference's stereodiffusion_nodes through tools/refload.py and
runs StereoDiffusionNode._text2stereoimage itself (CPU torch, with the reference's diffusion_step and stereo_shift_torch inside)
over tools/standard_fake_model.FakeModel whose scheduler is tools/ddim_oracle.DDIMOracle, a host scheduler.  Nothing of the
reference's arithmetic is replaced.  Wrapped, to look at what passes through: torch.randn_like (the deblur noise, which is
deblur_noise below: values a test can make again), the scheduler's step (the last result is the tensor the re-shifts write into:
the final latents) and the fake UNet, which records the latents it is handed (the call after the shift step sees the shifted ones).

  python tools/make_standard_ddim_goldens.py
Layout: `meta` = JSON {guidance_scale, scale_factor, margin, versions, cases: [{id, dtype, steps, direction, deblur, uncond}]};
per case 'cid/latents_shift_right' ([1,4,64,64], the right view just after the first shift), 'cid/latents_reshift_right/<i>' (the
right view just after the re-shift of step i, for the last re-shift that another step follows -- one at the last step is the final
latents' right view --; the left view is not touched by a shift), 'cid/latents_final' ([2,4,64,64]) -- bfloat16 as its int16 bit pattern --, 'cid/mask' (uint8
[1,64,64]), 'cid/codes' (uint8 [2,512,512,3]).  Not every step and not every combination is stored: the cases cover steps 5 and
10, uni and bi, deblur on and off and the three dtypes as a set (float32 once), and storing every re-shift makes 1.1 MB,
so the file stays below the 1 MiB a committed file may have.  The inputs are functions of this module (start_latent, disparity,
deblur_noise, the fake model's tables), not arrays of the file.

restate_case is the same loop without the reference: the fake model, DDIMOracle, torch's guidance expression on the CPU and
tools/standard_oracle's plan / apply_first / apply_reshift.  The maker asserts that it equals the reference's loop on every case;
tests/test_ddim_scheduler_surface.py recomputes one case with it.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ddim_oracle as do  # noqa: E402
import standard_fake_model as fm  # noqa: E402
import standard_oracle as so  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "standard_ddim.npz")
GUIDANCE, SCALE, MARGIN = 3.0, 8.0, 1e-3

# (id, dtype, steps, direction, deblur, uncond embeddings given)
CASES = [
    ("f32_10_bi_deblur_uncond", "float32", 10, "bi", True, True),
    ("f16_10_uni_deblur", "float16", 10, "uni", True, False),
    ("f16_5_bi_uncond", "float16", 5, "bi", False, True),
    ("bf16_10_uni", "bfloat16", 10, "uni", False, False),
    ("bf16_5_bi_deblur_uncond", "bfloat16", 5, "bi", True, True),
]


def start_latent(dtype):
    """x_t [1,4,64,64]: multiples of 1/8 in [-2, 2], exact in every dtype."""
    import torch
    g = torch.Generator().manual_seed(77)
    return (torch.randint(-16, 17, (1, 4, 64, 64), generator=g).float() / 8).to(dtype)


def deblur_noise(dtype):
    """What torch.randn_like returns under the maker, [2,4,64,64]: multiples of 1/8 in [-3, 3]."""
    import torch
    g = torch.Generator().manual_seed(78)
    return (torch.randint(-24, 25, (2, 4, 64, 64), generator=g).float() / 8).to(dtype)


def disparity():
    """float32 [1,512,512]: three by four flat blocks of levels k / 255, normalised as the reference's _norm_depth does."""
    levels = np.array([[12, 200, 90, 255], [140, 0, 230, 60], [75, 180, 30, 120]], dtype=np.uint8)
    d = np.repeat(np.repeat(levels, 171, 0)[:512], 128, 1)
    return so.disparity_512(d)


def shift_steps(steps):
    k = max(1, int(steps * 0.2))
    return k, [i for i in range(steps) if i > k and i % k == 0]


def stored_reshifts(dtype_name, steps):
    """The re-shift steps whose right view the file holds: the last one that another step follows (a re-shift at the last step is
    the final latents' right view, which the file holds anyway)."""
    return [i for i in shift_steps(steps)[1] if i + 1 < steps][-1:]


def to_np(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def oracle_model(dtype):
    model = fm.FakeModel("cpu", dtype)
    model.scheduler = do.DDIMOracle()
    return model


def restate_case(dtype_name, steps, direction, deblur, uncond):
    """The loop without the reference -> dict(latents_shift_right, latents_final, mask, codes) as the file holds them.
    (direction reaches the attention editor only, and the fake UNet has no attention layer.)"""
    import torch
    dtype = getattr(torch, dtype_name)
    model = oracle_model(dtype)
    model.scheduler.set_timesteps(steps)
    disp = torch.from_numpy(disparity())
    disp_latent = torch.nn.functional.interpolate(disp.unsqueeze(1), size=[64, 64], mode="bicubic", align_corners=False).squeeze(1)
    src_col = so.plan(disp_latent.numpy(), SCALE)
    x_t = start_latent(dtype)
    latents = torch.cat([x_t, x_t])
    text = model.text_encoder(torch.zeros((2, 77), dtype=torch.int64))[0]
    unc = fm.fake_uncond_embeddings(steps, "cpu", dtype) if uncond else None
    first, reshifts = shift_steps(steps)
    out, mask = {}, None
    bits = (lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy())
    with torch.no_grad():
        for i, t in enumerate(model.scheduler.timesteps):
            context = torch.cat([unc[i].expand(*text.shape) if uncond else text, text])
            u, c = model.unet(torch.cat([latents] * 2), t, encoder_hidden_states=context)["sample"].chunk(2)
            latents = model.scheduler.step(u + GUIDANCE * (c - u), t, latents)["prev_sample"]
            if i == first:
                noise = bits(deblur_noise(dtype)[1:].contiguous()) if deblur else None
                right, mask = so.apply_first(bits(latents[:1].contiguous()), src_col, noise)
                latents = torch.cat([latents[:1], torch.from_numpy(right).view(dtype)])
                out["latents_shift_right"] = to_np(latents[1:])
            elif i in reshifts:
                right = so.apply_reshift(bits(latents[:1].contiguous()), bits(latents[1:].contiguous()), src_col, mask)
                latents = torch.cat([latents[:1], torch.from_numpy(right).view(dtype)])
                if i in stored_reshifts(dtype_name, steps):
                    out[f"latents_reshift_right/{i}"] = to_np(latents[1:])
        image = model.vae.decode(1 / 0.18215 * latents)["sample"]
    out["latents_final"], out["mask"] = to_np(latents), mask
    out["codes"] = so.decode_to_codes(image.double().numpy(), dtype_name)
    return out


def reference_case(mod, dtype_name, steps, direction, deblur, uncond):
    import torch
    dtype = getattr(torch, dtype_name)
    model = oracle_model(dtype)
    model.unet.record = True
    seen = {"steps": [], "shift": []}
    real_step, real_randn_like, real_shift = model.scheduler.step, torch.randn_like, mod.stereo_shift_torch

    def step(*a, **k):
        r = real_step(*a, **k)
        seen["steps"].append(r["prev_sample"])   # not a copy: the re-shifts write into it
        return r

    def shift(*a, **k):
        r = real_shift(*a, **k)
        seen["shift"].append(r.clone())
        return r

    model.scheduler.step = step
    torch.randn_like = lambda t, *a, **k: deblur_noise(t.dtype)
    mod.stereo_shift_torch = shift
    try:
        x_t = start_latent(dtype)
        unc = fm.fake_uncond_embeddings(steps, "cpu", dtype) if uncond else None
        codes = mod.StereoDiffusionNode()._text2stereoimage(model, [""] * 2, unc, torch.cat([x_t, x_t], 0), torch.from_numpy(disparity()),
                                                            SCALE, direction, deblur, steps, GUIDANCE, torch.device("cpu"), None)
    finally:
        torch.randn_like, mod.stereo_shift_torch = real_randn_like, real_shift
    first, reshifts = shift_steps(steps)
    assert len(model.unet.calls) == steps and len(seen["shift"]) == 1 + len(reshifts) and first + 1 < steps
    final = seen["steps"][-1]
    again = so.decode_to_codes(model.vae.decode(1 / 0.18215 * final)["sample"].double().numpy(), dtype_name)
    assert np.array_equal(again, codes), "the final latents do not reproduce the reference's codes"
    # the UNet's next call sees a step's latents; the last step's are the final ones
    after = lambda i: to_np(model.unet.calls[i + 1][1:2] if i + 1 < steps else final[1:])   # noqa: E731
    kept = {f"latents_reshift_right/{i}": after(i) for i in stored_reshifts(dtype_name, steps)}
    return dict(latents_shift_right=to_np(model.unet.calls[first + 1][1:2]), latents_final=to_np(final), **kept,
                mask=(seen["shift"][0][1:, 0] != 0).numpy().astype(np.uint8), codes=codes)


def main():
    import PIL
    import torch
    import refload
    refload.quiet()
    mod = refload.load_sd_nodes()
    disp = torch.from_numpy(disparity())
    lat = torch.nn.functional.interpolate(disp.unsqueeze(1), size=[64, 64], mode="bicubic", align_corners=False).squeeze(1).numpy()
    m = so.margin(lat, SCALE)
    assert m >= MARGIN, f"the disparity's shift products come within {m} of an integer"
    arrays, cases = {}, []
    for cid, dtype_name, steps, direction, deblur, uncond in CASES:
        ref = reference_case(mod, dtype_name, steps, direction, deblur, uncond)
        mine = restate_case(dtype_name, steps, direction, deblur, uncond)
        for k, v in ref.items():
            assert np.array_equal(v, mine[k]), (cid, k, "the restatement differs from the reference's loop")
            arrays[f"{cid}/{k}"] = v
        cases.append(dict(id=cid, dtype=dtype_name, steps=steps, direction=direction, deblur=deblur, uncond=uncond))
        print(cid, "mask share", float(ref["mask"].mean()))
    versions = dict(pillow=PIL.__version__, numpy=np.__version__, torch=torch.__version__)
    meta = dict(guidance_scale=GUIDANCE, scale_factor=SCALE, margin=m, versions=versions, cases=cases)
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
