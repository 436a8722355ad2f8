"""Fast mode's loop with a few-step sampler in stock torch: the whole composition around the models -- the cats that build the
UNet's input, the guidance expression, the step of tools/fewstep_oracle.py, the blend of a 4-channel model -- as
tools/inpaintrun_stock.py is for PLMS.  It is the tests' reference for comfystereo_amd.inpaint_runner.FewStepLoop (on the CPU it
gives the bits the kernels must give) and the baseline of tools/inpaintrun_bench.py --sampler.
"""
import torch

import fewstep_oracle as oracle
import inpaintrun_stock as stock


def loop_step(unet, sampler, state, x_lat, mask_latent, masked_img_latent, t, context, k, guidance, cfg, last, channels, z=None, blend=None):
    """One iteration as stock torch runs it -> the oracle's dict.  state: the Euler sampler's un-scaled sample; x_lat: channels
    0..3 of the input (Euler: the scaled sample; LCM: the sample)."""
    inp = torch.cat([x_lat, mask_latent, masked_img_latent], dim=1) if channels == 9 else x_lat
    inp = torch.cat([inp] * 2) if cfg else inp
    pred = unet(inp, t.expand(inp.shape[0]).to(device=inp.device, dtype=inp.dtype), context=context)
    return oracle.step(sampler, pred, state if sampler == "euler" else x_lat, k, guidance, cfg, last, z=z, blend=blend)


@torch.no_grad()
def run(model, sampler, prompt, filled_u8, mask_u8, num_inference_steps, guidance_scale, strength, generators):
    """n frames (filled_u8 [n,h,w,3], mask_u8 [n,h,w] of 0 / 255, one generator each) on the device of `model` (for the bits: the
    CPU) -> dict(unet_in: every UNet input, latents, decode_in, codes [n,h,w,3])."""
    dtype, device, channels = model.dtype, model.device, model.unet.in_channels
    n = filled_u8.shape[0]
    cfg = float(guidance_scale) > 1.0
    tok = model.tokenizer
    cond = model.text_encoder(tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True,
                                  return_tensors="pt").input_ids.to(device))[0]
    uncond = model.text_encoder(tok([""], padding="max_length", max_length=tok.model_max_length, truncation=True,
                                    return_tensors="pt").input_ids.to(device))[0]
    context = (torch.cat([uncond.expand(n, -1, -1), cond.expand(n, -1, -1)]) if cfg else cond.expand(n, -1, -1)).to(dtype)
    preps = [stock.image_prep(filled_u8[k].cpu(), mask_u8[k].cpu(), dtype, (1, 1)) for k in range(n)]
    img = torch.cat([p[0] for p in preps]).to(device)
    masked = torch.cat([p[1] for p in preps]).to(device)
    img_latent = model.vae.encode(img)["latent_dist"].mean * 0.18215
    masked_img_latent = (model.vae.encode(masked)["latent_dist"].mean * 0.18215).to(dtype) if channels == 9 else None
    mask_latent = torch.cat([stock.image_prep(filled_u8[k].cpu(), mask_u8[k].cpu(), dtype, img_latent.shape[2:])[2] for k in range(n)]).to(device)
    img_latent = img_latent.to(dtype)
    acp = oracle.alphas_cumprod()
    ts = oracle.timesteps(sampler, num_inference_steps, strength)
    extra = max(len(ts) - 1, 0) if sampler == "lcm" else 0
    drawn = [[torch.randn((1,) + tuple(img_latent.shape[1:]), generator=g, device="cpu", dtype=dtype) for _ in range(1 + extra)]
             for g in generators]
    noise0 = torch.cat([d[0] for d in drawn]).to(device)
    blend = (img_latent, noise0, mask_latent) if channels == 4 else None
    seen = []
    if ts:
        x_lat, state = oracle.first_latents(sampler, img_latent.cpu(), noise0.cpu(), acp, ts[0])
        x_lat, state = x_lat.to(device), None if state is None else state.to(device)
        out = None
        for i, t in enumerate(ts):
            last = i == len(ts) - 1
            z = torch.cat([d[1 + i] for d in drawn]).to(device) if sampler == "lcm" and not last else None
            inp = torch.cat([x_lat, mask_latent, masked_img_latent], dim=1) if channels == 9 else x_lat
            seen.append(torch.cat([inp] * 2) if cfg else inp)
            out = loop_step(model.unet, sampler, state, x_lat, mask_latent, masked_img_latent, torch.tensor(t), context,
                            oracle.coeffs(sampler, acp, ts, i), guidance_scale, cfg, last, channels, z=z, blend=blend)
            x_lat, state = out["x"], out["state"]
        latents, decode_in = x_lat, out["decode_in"]
    else:
        latents, decode_in = img_latent, img_latent / 0.18215
    decoded = (model.vae.decode(decode_in)["sample"] / 2 + 0.5).clamp(0, 1)
    result = torch.nan_to_num(decoded.permute(0, 2, 3, 1).cpu().float(), nan=0.0, posinf=1.0, neginf=0.0)
    return dict(unet_in=seen, latents=latents, decode_in=decode_in, codes=(result * 255).to(torch.uint8))
