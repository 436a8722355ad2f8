"""The DDIM step of a v-prediction model (the SD 2.x 768-v checkpoints), restated independently of comfystereo_amd: in float64, per
dtype with every rounding, as the CPU torch expression, and as host loops of Standard mode, of DDIM inversion and of null-text
optimisation on stand-in models.

The reference is epsilon-only, so there is no reference run to capture: like tools/plms_oracle.py this is a restatement of the
published algorithm, NOT a capture of anyone's output.  Sources:
  * Salimans & Ho, "Progressive Distillation for Fast Sampling of Diffusion Models", 2022: the model answers
    v = sqrt(a_t) * eps - sqrt(1 - a_t) * x0;
  * the operation order of diffusers' DDIMScheduler.step with prediction_type="v_prediction", eta 0.

With c1 = sqrt(1 - a_t), c2 = sqrt(a_t), c3 = sqrt(1 - a_other), c4 = sqrt(a_other) and v = u + g * (c - u) the guided answer:

    x0  = c2 * x - c1 * v        e = c2 * v + c1 * x        out = c4 * x0 + c3 * e

and for null-text optimisation  loss = mean((out(latent_cur) - latent_prev)^2),
d loss / d u = (2 / count) * (out - latent_prev) * (c3 * c2 - c4 * c1) * (1 - g).

All four coefficients are first operands of products: CPU torch rounds a 0-dim float32 tensor in that place to a half dtype before
it multiplies, so `coefficients` rounds all four (under epsilon prediction c2 divides and keeps its float32).

Used by the tests and tools/make_vpred_goldens.py.  Nothing in the package imports it.
"""
import math

import numpy as np
import torch

from plms_oracle import root, scaled_linear_alphas_cumprod   # noqa: F401  (the schedule, restated there)

HALVES = (torch.float16, torch.bfloat16)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def coeffs64(alpha_t, alpha_other):
    a, o = float(alpha_t), float(alpha_other)
    return math.sqrt(1 - a), math.sqrt(a), math.sqrt(1 - o), math.sqrt(o)


def guided64(u, c, guidance):
    u = np.asarray(u, np.float64)
    return u if c is None else u + float(guidance) * (np.asarray(c, np.float64) - u)


def step64(sample, v_a, v_b, guidance, coeffs):
    """The v-prediction step in float64, no intermediate rounding."""
    c1, c2, c3, c4 = (float(c) for c in coeffs)
    x, v = np.asarray(sample, np.float64), guided64(v_a, v_b, guidance)
    x0 = c2 * x - c1 * v
    e = c2 * v + c1 * x
    return c4 * x0 + c3 * e


def eps_step64(sample, eps, coeffs):
    """The epsilon step in float64: what the v step must equal on v = c2 * eps - c1 * x0."""
    c1, c2, c3, c4 = (float(c) for c in coeffs)
    x, e = np.asarray(sample, np.float64), np.asarray(eps, np.float64)
    return c4 * ((x - c1 * e) / c2) + c3 * e


def loss64(v_uncond, v_cond, latent_cur, latent_prev, guidance, coeffs):
    diff = step64(latent_cur, v_uncond, v_cond, guidance, coeffs) - np.asarray(latent_prev, np.float64)
    return float(np.mean(diff * diff))


def null_loss_grad64(v_uncond, v_cond, latent_cur, latent_prev, guidance, coeffs):
    """-> (rec, loss, d loss / d v_uncond), float64."""
    c1, c2, c3, c4 = (float(c) for c in coeffs)
    rec = step64(latent_cur, v_uncond, v_cond, guidance, coeffs)
    diff = rec - np.asarray(latent_prev, np.float64)
    return rec, float(np.mean(diff * diff)), 2.0 / diff.size * diff * (c3 * c2 - c4 * c1) * (1.0 - float(guidance))


# ---- per dtype -------------------------------------------------------------------------------------------------------------------
def coefficients(a_t, a_other, dtype, prediction="v_prediction"):
    """(c1, c2, c3, c4) as Python floats: the square roots in double, rounded to float32, and those that are first operands of a
    product -- all four under v-prediction, all but c2 under epsilon -- to a half dtype."""
    one = torch.tensor(1.0, dtype=torch.float32)
    c = [math.sqrt(float(one - a_t)), math.sqrt(float(a_t)), math.sqrt(float(one - a_other)), math.sqrt(float(a_other))]
    c = [float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in c]
    if dtype in HALVES:
        c = [v if (i == 1 and prediction == "epsilon") else float(torch.tensor(v, dtype=torch.float32).to(dtype)) for i, v in enumerate(c)]
    return tuple(c)


def step_rounded(sample, v_a, v_b, guidance, c, dtype):
    """The v step in float64 with every operation rounded to float32 and then to `dtype`, as CPU torch rounds it -> `dtype`."""
    r = lambda t: t.to(torch.float32).to(dtype).double()   # noqa: E731
    x, v = sample.double(), v_a.double()
    if v_b is not None:
        v = r(v + r(float(guidance) * r(v_b.double() - v)))
    c1, c2, c3, c4 = c
    x0 = r(r(c2 * x) - r(c1 * v))
    e = r(r(c2 * v) + r(c1 * x))
    return r(r(c4 * x0) + r(c3 * e)).to(dtype)


def torch_step(sample, out_a, out_b, guidance, c, prediction="v_prediction"):
    """The CPU torch expression on tensors of one dtype and Python-float coefficients (already rounded as `coefficients` rounds
    them): what the kernels must give bit for bit.  prediction "epsilon": the reference's expression."""
    c1, c2, c3, c4 = c
    m = out_a if out_b is None else out_a + guidance * (out_b - out_a)
    if prediction == "epsilon":
        return c4 * ((sample - c1 * m) / c2) + c3 * m
    x0 = c2 * sample - c1 * m
    e = c2 * m + c1 * sample
    return c4 * x0 + c3 * e


def torch_null_loss(v_uncond, v_cond, latent_cur, latent_prev, guidance, c):
    """The CPU torch-autograd composition -> (rec, loss, d loss / d v_uncond) in the tensors' dtype: the project's yardstick for
    how far a correct implementation may be from the float64 restatement."""
    u = v_uncond.detach().clone().requires_grad_(True)
    rec = torch_step(latent_cur, u, v_cond, guidance, c)
    loss = torch.nn.functional.mse_loss(rec, latent_prev)
    (grad,) = torch.autograd.grad(loss, [u])
    return rec.detach(), loss.detach(), grad


# ---- host loops on the stand-in models (CPU torch; tools/standard_fake_model.py, tools/null_fake_model.py) ---------------------------
def timesteps(steps, offset=0, train=1000):
    return [i * (train // steps) + offset for i in range(steps)][::-1]


def shift_steps(steps):
    k = max(1, int(steps * 0.2))
    return k, k


def host_shift(left, right, src_col, mask, op, noise):
    """The latent shift on host tensors: right takes left at column src_col of its row (0 where src_col is -1); "first" makes the
    mask from channel 0 of that (non-zero, a NaN included) and puts `noise` where it is 0; "reshift" writes under the stored mask."""
    b, ch, h, w = left.shape
    landed = (src_col >= 0) & (src_col < w)
    idx = src_col.clamp(0, w - 1).long()[:, None].expand(b, ch, h, w)
    moved = torch.where(landed[:, None], torch.gather(left, 3, idx), torch.zeros_like(left))
    if op == "first":
        mask = (moved[:, 0] != 0).to(torch.uint8)
        right = moved if noise is None else torch.where(mask[:, None].bool(), moved, noise)
    else:
        right = torch.where(mask[:, None].bool(), moved, right)
    return right, mask


def standard_loop(model, alphas_cumprod, latent2, src_col, steps, guidance, uncond_embeddings=None, noise=None,
                  prediction="v_prediction"):
    """StereoDiffusion's Standard loop on a host model: latent2 [2,C,h,w] (left, right), src_col int32 [1,h,w] (the plan's table),
    noise [1,C,h,w] (deblur) or None -> (latents [2,C,h,w], mask uint8 [1,h,w])."""
    dtype = latent2.dtype
    tok = model.tokenizer
    text = model.text_encoder(tok(["", ""]).input_ids)[0]
    latents, mask, shifted = latent2.clone(), torch.zeros(src_col.shape, dtype=torch.uint8), False
    first, interval = shift_steps(steps)
    ts = timesteps(steps)
    with torch.no_grad():
        for i, t in enumerate(ts):
            uncond = text if uncond_embeddings is None else uncond_embeddings[i].expand(*text.shape)
            pred = model.unet(torch.cat([latents] * 2), torch.tensor(t), encoder_hidden_states=torch.cat([uncond, text]))["sample"]
            u, c = pred.chunk(2)
            prev_t = t - 1000 // steps
            cf = coefficients(alphas_cumprod[t], alphas_cumprod[prev_t] if prev_t >= 0 else alphas_cumprod[0], dtype, prediction)
            latents = torch_step(latents, u, c, guidance, cf, prediction)
            op = "first" if i == first else ("reshift" if shifted and i > first and i % interval == 0 else "none")
            if op != "none":
                right, mask = host_shift(latents[:1], latents[1:], src_col, mask, op, noise if op == "first" else None)
                latents = torch.cat([latents[:1], right])
                shifted = True
    return latents, mask


def ddim_inversion_loop(model, latent, steps, prediction="v_prediction"):
    """NullInversion.ddim_loop on a host model whose scheduler has alphas_cumprod, timesteps and final_alpha_cumprod: the step with
    the two alphas exchanged (next_step) -> the list of latents."""
    sch = model.scheduler
    sch.set_timesteps(steps)
    tok = model.tokenizer
    cond = model.text_encoder(tok([""]).input_ids)[0]
    out = [latent]
    with torch.no_grad():
        for i in range(steps):
            t = int(sch.timesteps[len(sch.timesteps) - i - 1])
            pred = model.unet(latent, t, encoder_hidden_states=cond)["sample"]
            cur = min(t - 1000 // steps, 999)
            a_t = sch.alphas_cumprod[cur] if cur >= 0 else sch.final_alpha_cumprod
            if latent.dtype == torch.float64:
                cf = coeffs64(a_t, sch.alphas_cumprod[t])
            else:
                cf = coefficients(a_t, sch.alphas_cumprod[t], latent.dtype, prediction)
            latent = torch_step(latent, pred, None, 1.0, cf, prediction)
            out.append(latent)
    return out


def null_optimization(model, latents, context, steps, guidance, num_inner_steps, epsilon, prediction="v_prediction"):
    """NullInversion.null_optimization on a host model in the model's own dtype -- float64: the restatement without intermediate
    rounding; float32: the CPU torch-autograd composition, the yardstick of how far a correct run may be from it -- with torch
    autograd through the model and the step, and Adam written out (fresh moments per outer step, lr = 0.01 * (1 - i / 100)).
    latents: the list ddim_inversion_loop returns; context [2,77,W]: the empty prompt's embedding twice.
    -> (embeddings [steps] of [1,77,W], losses [steps][inner steps taken])."""
    sch = model.scheduler
    uncond, cond = context.chunk(2)
    latent_cur = latents[-1]
    embeddings, losses = [], []
    for i in range(steps):
        uncond = uncond.clone().detach().requires_grad_(True)
        lr = 1e-2 * (1. - i / 100.)
        m, v = torch.zeros_like(uncond), torch.zeros_like(uncond)
        latent_prev = latents[len(latents) - i - 2]
        t = int(sch.timesteps[i])
        prev_t = t - 1000 // steps
        a_prev = sch.alphas_cumprod[prev_t] if prev_t >= 0 else sch.final_alpha_cumprod
        if latent_cur.dtype == torch.float64:
            cf = coeffs64(sch.alphas_cumprod[t], a_prev)
        else:
            cf = coefficients(sch.alphas_cumprod[t], a_prev, latent_cur.dtype, prediction)
        with torch.no_grad():
            out_cond = model.unet(latent_cur, t, encoder_hidden_states=cond)["sample"]
        taken = []
        for j in range(1, num_inner_steps + 1):
            out_unc = model.unet(latent_cur, t, encoder_hidden_states=uncond)["sample"]
            loss = ((torch_step(latent_cur, out_unc, out_cond, guidance, cf, prediction) - latent_prev) ** 2).mean()
            (g,) = torch.autograd.grad(loss, [uncond])
            with torch.no_grad():
                m = m + (1 - 0.9) * (g - m)
                v = 0.999 * v + (1 - 0.999) * g * g
                uncond -= lr / (1 - 0.9 ** j) * m / (v.sqrt() / (1 - 0.999 ** j) ** 0.5 + 1e-8)
            taken.append(float(loss.detach()))
            if taken[-1] < epsilon + i * 2e-5:
                break
        losses.append(taken)
        embeddings.append(uncond[:1].detach().clone())
        with torch.no_grad():
            both = model.unet(torch.cat([latent_cur] * 2), t, encoder_hidden_states=torch.cat([uncond.detach(), cond]))["sample"]
            out_unc, out_cond = both.chunk(2)
            latent_cur = torch_step(latent_cur, out_unc, out_cond, guidance, cf, prediction)
    return embeddings, losses
