#!/usr/bin/env python3
"""Fixtures of Fast mode's inpainting loop: tests/golden/inpaint_runner.npz.

Build-machine only, like tools/make_standard_goldens.py.  Loads the reference's model_wrappers.py as a module of its own (beside
tools/refload.py, which stays as it is) with stand-ins for what this machine lacks: `diffusers` -- its three scheduler names map
to tools/plms_oracle.PLMSOracle, a restatement of PNDMScheduler as the reference configures it, NOT diffusers' own code -- and
`comfy.model_management`.  A ComfyUIInpaintRunner is built around the stand-in models of tools/inpaint_fake_model.py without
running its __init__'s model loading, and the reference's own __call__ runs on the CPU.  Nothing of the reference's arithmetic is
replaced; the stand-in UNet, the VAE's decode and the scheduler's step are watched for what passes through them.

  python tools/make_inpaintrun_goldens.py
Arrays per case id: '<id>/filled', '<id>/mask', '<id>/unet_in' [steps,2,9,hl,wl], '<id>/unet_out' [steps,2,4,hl,wl], '<id>/latents'
(the last step's result; absent for a loop of no step), '<id>/decode_in' (what vae.decode received), '<id>/codes'.  bfloat16 arrays
are stored as their int16 bit patterns.  meta (JSON): cases[*] = id, dtype, steps, strength, guidance, mask, seed, prompt, size,
timesteps (the sliced list), kinds (the PLMS combination of every step).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import inpaint_fake_model as fm  # noqa: E402
import plms_oracle  # noqa: E402

REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = ("float32", "float16", "bfloat16")
H, W = 16, 24   # latents 2 x 3
PROMPT = "a photo"
# (steps, strength, guidance, mask): steps 1, 2, 3 and 6 (six reach all five combinations and wrap the ring of four), strength 1.0,
# 0.6 (a sliced list: the warm-up falls on its first two entries) and 0.0 (no step), guidance 0, 1 and 7.5, the three masks
CASES = ((6, 1.0, 7.5, "mixed"), (1, 1.0, 7.5, "mixed"), (2, 1.0, 1.0, "one"), (3, 1.0, 0.0, "zero"), (6, 0.6, 7.5, "mixed"),
         (3, 0.0, 7.5, "mixed"), (2, 0.6, 1.0, "zero"), (6, 1.0, 0.0, "one"))


def load_model_wrappers():
    if "ref_model_wrappers" in sys.modules:
        return sys.modules["ref_model_wrappers"]
    diffusers = types.ModuleType("diffusers")
    diffusers.DDIMScheduler = diffusers.EulerDiscreteScheduler = diffusers.PNDMScheduler = plms_oracle.PLMSOracle
    comfy, mm = types.ModuleType("comfy"), types.ModuleType("comfy.model_management")
    mm.load_models_gpu = lambda models: None
    comfy.model_management = mm
    sys.modules.setdefault("diffusers", diffusers)
    sys.modules.setdefault("comfy", comfy)
    sys.modules.setdefault("comfy.model_management", mm)
    spec = importlib.util.spec_from_file_location("ref_model_wrappers", REF + "/model_wrappers.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_model_wrappers"] = mod
    spec.loader.exec_module(mod)
    return mod


def to_np(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def reference_runner(mw, model):
    """A ComfyUIInpaintRunner around the stand-ins: what its __init__ sets (:500-520), without the model loading."""
    import torch
    runner = mw.ComfyUIInpaintRunner.__new__(mw.ComfyUIInpaintRunner)
    runner.device = torch.device("cpu")
    runner.unet, runner.vae, runner.text_encoder, runner.tokenizer = model.parts()
    runner.scheduler = mw.PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True)
    return runner


def run_case(mw, dtype_name, steps, strength, guidance, mask_kind, seed):
    import torch
    from PIL import Image
    from comfystereo_amd import inpaint_runner as ir
    dtype = getattr(torch, dtype_name)
    model = fm.FakeInpaintModel("cpu", dtype)
    model.unet.record = True
    runner = reference_runner(mw, model)
    filled, mask = fm.seeded_frame(seed, H, W, mask_kind)
    seen = {"latents": None, "decode_in": None, "steps": []}
    real_step, real_decode = runner.scheduler.step, model.vae.decode

    def step(model_output, timestep, sample):
        seen["steps"].append((runner.scheduler.counter, int(timestep)))
        out = real_step(model_output, timestep, sample)
        seen["latents"] = out.prev_sample
        return out

    def decode(z):
        seen["decode_in"] = z
        return real_decode(z)

    runner.scheduler.step, model.vae.decode = step, decode
    with torch.no_grad():
        result = runner(PROMPT, Image.fromarray(filled.numpy(), "RGB"), Image.fromarray(mask.numpy(), "L"), num_inference_steps=steps,
                        guidance_scale=guidance, strength=strength, generator=torch.Generator().manual_seed(seed))
    codes = np.array(result.images[0])
    assert codes.shape == (H, W, 3) and codes.dtype == np.uint8
    assert model.tokenizer.prompts == [[PROMPT], [""]]
    # the package's host side agrees with the scheduler restated here: the timesteps, the kinds, the coefficients as CPU torch
    # rounds them (0-dim float32 tensors)
    sch = runner.scheduler
    ts = ir.plms_timesteps(steps)
    assert ts == sch.timesteps.tolist()
    ts = ts[max(0, int(len(ts) * (1.0 - strength))):]
    assert [t for _, t in seen["steps"]] == ts and [c for c, _ in seen["steps"]] == list(range(len(ts)))
    kinds, kept = [], 0
    for counter, t in enumerate(ts):
        kind, kept = ir.plms_kind(counter, kept)
        kinds.append(kind)
        ratio, t_, p_ = 1000 // steps, t, t - 1000 // steps
        if counter == 1:
            p_, t_ = t, t + ratio
        a_t = sch.alphas_cumprod[t_]
        a_p = sch.alphas_cumprod[p_] if p_ >= 0 else sch.final_alpha_cumprod
        want = (float((a_p / a_t) ** 0.5), float(a_p - a_t), float(a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5))
        got = ir.plms_coeffs(sch.alphas_cumprod, sch.final_alpha_cumprod, counter, t, ratio, torch.float32)
        assert got == want, (steps, counter, t, got, want)
    arrays = {"filled": filled.numpy(), "mask": mask.numpy(), "codes": codes, "decode_in": to_np(seen["decode_in"])}
    if ts:
        arrays["unet_in"] = to_np(torch.stack(model.unet.inputs))
        arrays["unet_out"] = to_np(torch.stack(model.unet.outputs))
        arrays["latents"] = to_np(seen["latents"])
        assert len(model.unet.inputs) == len(ts)
    else:
        assert model.unet.count == 0
    meta = dict(dtype=dtype_name, steps=steps, strength=strength, guidance=guidance, mask=mask_kind, seed=seed, prompt=PROMPT,
                size=[H, W], timesteps=ts, kinds=kinds)
    return arrays, meta


def oracle_error(arrays, cases):
    """The float32 error of tools/plms_oracle.py against itself in float64, on the float32 cases' own inputs: per step the recorded
    sample and guided prediction go through both; max |difference| / max(1, max |float64 result|)."""
    import torch
    worst = 0.0
    for c in cases:
        if c["dtype"] != "float32" or not c["timesteps"]:
            continue
        s32, s64 = plms_oracle.PLMSOracle(), plms_oracle.PLMSOracle(alphas_dtype=torch.float64)
        s32.set_timesteps(c["steps"])
        s64.set_timesteps(c["steps"])
        for i, t in enumerate(c["timesteps"]):
            out = torch.from_numpy(arrays[f"{c['id']}/unet_out"][i])
            e = out[:1] + c["guidance"] * (out[1:] - out[:1])
            sample = torch.from_numpy(arrays[f"{c['id']}/unet_in"][i][:1, :4])
            a = s32.step(e, t, sample).prev_sample.double()
            b = s64.step(e.double(), t, sample.double()).prev_sample
            worst = max(worst, float((a - b).abs().max() / max(1.0, float(b.abs().max()))))
    return worst


def main():
    import torch
    mw = load_model_wrappers()
    arrays, cases = {}, []
    for dtype_name in DTYPES:
        for k, (steps, strength, guidance, mask_kind) in enumerate(CASES):
            cid = f"{dtype_name}_n{steps}_s{strength}_g{guidance}_{mask_kind}"
            got, meta = run_case(mw, dtype_name, steps, strength, guidance, mask_kind, seed=100 + k)
            for name, a in got.items():
                arrays[f"{cid}/{name}"] = a
            cases.append(dict(id=cid, **meta))
            print(cid, meta["timesteps"], meta["kinds"])
    # the mixed-mask frames hold a negative pixel under the mask, and the VAE stand-in keeps its zero's sign
    for c in cases:
        if c["mask"] == "mixed" and c["timesteps"]:
            x0 = arrays[f"{c['id']}/unet_in"][0, 0, 5]
            bits = x0.view({2: np.uint16, 4: np.uint32}[x0.dtype.itemsize])
            assert (bits == (1 << (8 * x0.dtype.itemsize - 1))).any(), c["id"]
    assert {k for c in cases for k in c["kinds"]} == {"first", "second", "order2", "order3", "order4"}
    path = os.path.join(GOLDEN, "inpaint_runner.npz")
    err = oracle_error(arrays, cases)
    print("oracle float32 error against float64:", err)
    np.savez_compressed(path, meta=json.dumps(dict(cases=cases, torch=torch.__version__, oracle_err=err, scheduler="tools/plms_oracle.py (restated)")), **arrays)
    print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes", len(cases), "cases")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
