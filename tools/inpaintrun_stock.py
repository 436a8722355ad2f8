"""The inpainting loop of StereoDiffusion's Fast mode in stock torch: the composition a user of the reference's
ComfyUIInpaintRunner.__call__ runs around the models (model_wrappers.py:543-634), written from its description in
comfystereo_amd/inpaint_runner.py with tools/plms_oracle.PLMSOracle as the scheduler.

It is the tests' reference at sizes the fixtures do not hold (tests/test_inpaint_runner_surface.py first checks it bit for bit
against the fixtures, which come from the reference's own code) and the baseline of tools/inpaintrun_bench.py.  On the CPU it
gives the reference's bits; on a GPU torch rounds some of these expressions differently (a division by a Python scalar goes
through the reciprocal there), which is why the package does not run them.
"""
import torch
import torch.nn.functional as F

import plms_oracle


def image_prep(filled_u8, mask_u8, dtype, latent_size):
    """filled_u8 [h,w,3], mask_u8 [h,w] (0 / 255) on the CPU -> img, masked [1,3,h,w], mask_latent [1,1,hl,wl] of `dtype`."""
    img = (filled_u8.numpy().astype("float32") / 255.0)
    img = (torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0) * 2.0 - 1.0).to(dtype)
    mask = torch.from_numpy(mask_u8.numpy().astype("float32") / 255.0).unsqueeze(0).unsqueeze(0).to(dtype)
    masked = img * (1 - mask)
    return img, masked, F.interpolate(mask, size=tuple(latent_size), mode="nearest")


def loop_step(unet, scheduler, latents, mask_latent, masked_img_latent, t, context, guidance_scale, dtype):
    """One iteration of the loop as stock torch runs it: three cats, the UNet, the guidance expression, the scheduler's step."""
    latent_model_input = torch.cat([latents, mask_latent, masked_img_latent], dim=1)
    latent_model_input = torch.cat([latent_model_input] * 2)
    noise_pred = unet(latent_model_input.to(dtype), t.expand(2).to(device=latents.device, dtype=dtype), context=context)
    noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
    noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
    return scheduler.step(noise_pred, t, latents).prev_sample


@torch.no_grad()
def run(model, prompt, filled_u8, mask_u8, num_inference_steps, guidance_scale, strength, generator):
    """One frame on the device of `model` (for the reference's bits: the CPU) -> dict(unet_in, latents, decode_in, codes)."""
    dtype, device = model.dtype, model.device
    tok = model.tokenizer
    cond = model.text_encoder(tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True,
                                  return_tensors="pt").input_ids.to(device))[0]
    uncond = model.text_encoder(tok([""], padding="max_length", max_length=tok.model_max_length, truncation=True,
                                    return_tensors="pt").input_ids.to(device))[0]
    context = torch.cat([uncond, cond]).to(dtype)
    img, masked, mask_full = image_prep(filled_u8.cpu(), mask_u8.cpu(), dtype, (1, 1))
    img, masked = img.to(device), masked.to(device)
    img_latent = model.vae.encode(img)["latent_dist"].mean * 0.18215
    masked_img_latent = model.vae.encode(masked)["latent_dist"].mean * 0.18215
    mask_latent = image_prep(filled_u8.cpu(), mask_u8.cpu(), dtype, img_latent.shape[2:])[2].to(device)
    img_latent, masked_img_latent = img_latent.to(dtype), masked_img_latent.to(dtype)
    scheduler = plms_oracle.PLMSOracle()
    scheduler.set_timesteps(num_inference_steps)
    timesteps = scheduler.timesteps
    timesteps = timesteps[max(0, int(len(timesteps) * (1.0 - strength))):]
    noise = torch.randn(img_latent.shape, generator=generator, device="cpu", dtype=dtype).to(device)
    latents = scheduler.add_noise(img_latent, noise, timesteps[0:1]) if len(timesteps) > 0 else img_latent
    seen = []
    for t in timesteps:
        seen.append(torch.cat([torch.cat([latents, mask_latent, masked_img_latent], dim=1)] * 2))
        latents = loop_step(model.unet, scheduler, latents, mask_latent, masked_img_latent, t, context, guidance_scale, dtype)
    decode_in = latents / 0.18215
    decoded = (model.vae.decode(decode_in)["sample"] / 2 + 0.5).clamp(0, 1)
    result = torch.nan_to_num(decoded[0].permute(1, 2, 0).cpu().float(), nan=0.0, posinf=1.0, neginf=0.0)
    return dict(unet_in=seen, latents=latents, decode_in=decode_in, codes=(result * 255).to(torch.uint8))
