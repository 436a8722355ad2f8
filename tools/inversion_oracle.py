"""A float64 restatement of null-text inversion outside the UNet (cs_ddim_step, cs_null_loss_grad, cs_adam_step) and of
NullInversion.ddim_loop / null_optimization on a given model, with no intermediate rounding: the yardstick the tests measure
both this package's results and the reference's own (tests/golden/inversion*.npz, `meta` -> ref_err) against.  Line numbers are
the reference's inversion.py.

The bound a test applies: error(ours, oracle) <= max(4 * error(reference, oracle), one ulp of the dtype at the tensor's largest
magnitude) -- `bound()`; errors are largest absolute differences.
"""
import numpy as np

MANTISSA_BITS = {"float32": 23, "float16": 10, "bfloat16": 7}


def ulp(dtype_name, magnitude):
    """The spacing of `dtype_name` at |magnitude| (the smallest normal's below it)."""
    m = max(float(abs(magnitude)), {"float32": 2.0 ** -126, "float16": 2.0 ** -14, "bfloat16": 2.0 ** -126}[dtype_name])
    return 2.0 ** (np.floor(np.log2(m)) - MANTISSA_BITS[dtype_name])


def err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def bound(ref_err, dtype_name, want):
    return max(4.0 * float(ref_err), ulp(dtype_name, np.max(np.abs(np.asarray(want, dtype=np.float64)))))


def step_coeffs(alpha_t, alpha_other):
    """(c1, c2, c3, c4) in float64 from the two alphas (:59-64, :69-74)."""
    a, o = float(alpha_t), float(alpha_other)
    return (1 - a) ** 0.5, a ** 0.5, (1 - o) ** 0.5, o ** 0.5


def ddim_step(sample, eps_a, eps_b, guidance, coeffs):
    """prev_step (:57-65) / next_step (:67-75) after the guidance (:88)."""
    c1, c2, c3, c4 = (float(c) for c in coeffs)
    s, a = np.asarray(sample, np.float64), np.asarray(eps_a, np.float64)
    e = a if eps_b is None else a + float(guidance) * (np.asarray(eps_b, np.float64) - a)
    return c4 * ((s - c1 * e) / c2) + c3 * e


def null_loss_grad(eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs):
    """(:199-201) -> (rec, loss, d loss / d eps_uncond)."""
    c1, c2, c3, c4 = (float(c) for c in coeffs)
    rec = ddim_step(latent_cur, eps_uncond, eps_cond, guidance, coeffs)
    diff = rec - np.asarray(latent_prev, np.float64)
    loss = float(np.mean(diff * diff))
    grad = 2.0 / diff.size * diff * (c3 - c4 * c1 / c2) * (1.0 - float(guidance))
    return rec, loss, grad


def adam(param, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) from zero moments over the gradients given, one step each ->
    [(param, exp_avg, exp_avg_sq) after every step]."""
    p = np.asarray(param, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for k, g in enumerate(grads, 1):
        g = np.asarray(g, np.float64)
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        denom = np.sqrt(v) / (1 - beta2 ** k) ** 0.5 + eps
        p = p - lr / (1 - beta1 ** k) * m / denom
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def _alphas(scheduler, timestep, kind):
    ratio = scheduler.config.num_train_timesteps // scheduler.num_inference_steps
    if kind == "prev":
        other = timestep - ratio
        return scheduler.alphas_cumprod[timestep], scheduler.alphas_cumprod[other] if other >= 0 else scheduler.final_alpha_cumprod
    cur = min(timestep - ratio, 999)
    return (scheduler.alphas_cumprod[cur] if cur >= 0 else scheduler.final_alpha_cumprod), scheduler.alphas_cumprod[timestep]


def ddim_loop(model64, latent, cond, steps):
    """ddim_loop (:161-171) on a float64 model -> the list of latents (torch float64)."""
    import torch
    out = [latent]
    with torch.no_grad():
        for i in range(steps):
            t = int(model64.scheduler.timesteps[len(model64.scheduler.timesteps) - i - 1])
            e = model64.unet(latent, t, encoder_hidden_states=cond)["sample"]
            c1, c2, c3, c4 = step_coeffs(*_alphas(model64.scheduler, t, "next"))
            latent = c4 * ((latent - c1 * e) / c2) + c3 * e
            out.append(latent)
    return out


def null_optimization(model64, latents, context, steps, guidance, num_inner_steps, epsilon):
    """null_optimization (:184-212) on a float64 model, torch autograd and this file's Adam ->
    (embeddings [steps] of [1,77,W], losses [steps][inner steps taken])."""
    import torch
    uncond, cond = context.chunk(2)
    latent_cur = latents[-1]
    embeddings, losses = [], []
    for i in range(steps):
        uncond = uncond.clone().detach().requires_grad_(True)
        lr = 1e-2 * (1. - i / 100.)
        m, v = torch.zeros_like(uncond), torch.zeros_like(uncond)
        latent_prev = latents[len(latents) - i - 2]
        t = int(model64.scheduler.timesteps[i])
        c1, c2, c3, c4 = step_coeffs(*_alphas(model64.scheduler, t, "prev"))

        def step(e, x):
            return c4 * ((x - c1 * e) / c2) + c3 * e

        with torch.no_grad():
            e_cond = model64.unet(latent_cur, t, encoder_hidden_states=cond)["sample"]
        taken = []
        for j in range(1, num_inner_steps + 1):
            e_unc = model64.unet(latent_cur, t, encoder_hidden_states=uncond)["sample"]
            loss = ((step(e_unc + guidance * (e_cond - e_unc), latent_cur) - latent_prev) ** 2).mean()
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
            e2 = model64.unet(torch.cat([latent_cur] * 2), t, encoder_hidden_states=torch.cat([uncond.detach(), cond]))["sample"]
            e_unc, e_cond = e2.chunk(2)
            latent_cur = step(e_unc + guidance * (e_cond - e_unc), latent_cur)
    return embeddings, losses


def margins(losses, epsilon):
    """The smallest |loss - threshold| / threshold over every loss the loop compares (:206)."""
    worst = np.inf
    for i, row in enumerate(losses):
        thr = epsilon + i * 2e-5
        for x in row:
            worst = min(worst, abs(float(x) - thr) / thr)
    return float(worst)
