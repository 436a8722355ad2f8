"""The specification of Fast mode's few-step samplers (cs_inpaint_fewstep_init, cs_inpaint_fewstep_step,
comfystereo_amd.inpaint_runner.FewStepLoop): both algorithms restated from their papers as CPU torch tensor expressions.  The
kernels equal the CPU evaluation of this file bit for bit in float32, float16 and bfloat16.

  Euler  Karras et al. 2022, "Elucidating the Design Space of Diffusion-Based Generative Models", Alg. 1 without churn (first
         order): x_next = x + (sigma_next - sigma) * d with d = (x - D(x)) / sigma, which for an epsilon model run on the input
         x / sqrt(sigma^2 + 1) is the prediction e itself.  sigma_t = sqrt((1 - a_t) / a_t).
  LCM    Luo et al. 2023, "Latent Consistency Models", multistep consistency sampling: the consistency function
         f(x, t) = c_skip(t) x + c_out(t) x0(x, e, t) with the boundary condition of sigma_data = 0.5 and timestep scaling 10,
         then fresh noise to the next timestep's level.

The rounding rule: the guided prediction e = u + guidance * (t - u) is formed in the tensors' dtype, as the PLMS path forms it.
Everything after it is float32 arithmetic on the dtype's values with float32 coefficients computed on the host (numpy float32
scalars: every operation correctly rounded), one operation at a time, and ONE rounding to the dtype per stored tensor.

On the CPU every expression below is a chain of single IEEE operations (a 0-dim float32 tensor meets a float32 tensor: no
conversion, no reciprocal, no fused multiply-add).  On a GPU torch rounds some of them differently, which is why the package does
not run them.
"""
import numpy as np
import torch

import plms_oracle

F32 = np.float32
TRAIN_STEPS, LCM_ORIGIN_STEPS = 1000, 50
SAMPLERS = ("euler", "lcm")


def alphas_cumprod():
    return plms_oracle.PLMSOracle().alphas_cumprod


# ---- timesteps ---------------------------------------------------------------------------------------------------------------------
def euler_timesteps(n, train=TRAIN_STEPS):
    """Trailing spacing: round(T - i * T / N) - 1, numpy's round on float64."""
    return [int(v) for v in np.round(train - np.arange(n, dtype=np.float64) * (train / n)) - 1]


def lcm_timesteps(n, train=TRAIN_STEPS, origin=LCM_ORIGIN_STEPS):
    """The origin grid t = c j - 1 (j = 1..origin, c = T // origin), descending, at the indices floor(linspace(0, origin, N))."""
    if n > origin:
        raise ValueError(f"sampler 'lcm' takes at most {origin} steps, got {n}")
    c = train // origin
    grid = [c * j - 1 for j in range(origin, 0, -1)]
    return [grid[int(k)] for k in np.floor(np.linspace(0, origin, n, endpoint=False))]


def timesteps(sampler, n, strength=1.0, train=TRAIN_STEPS):
    ts = euler_timesteps(n, train) if sampler == "euler" else lcm_timesteps(n, train)
    return ts[max(0, int(len(ts) * (1.0 - strength))):]   # the runner's rule (reference model_wrappers.py:592-593)


# ---- coefficients: float32 on the host -----------------------------------------------------------------------------------------------
def _a(acp, t):
    """a_t; past the last timestep a = 1 (sigma = 0)."""
    return F32(1.0) if t is None else F32(float(acp[t]))


def sigma(acp, t):
    a = _a(acp, t)
    return np.sqrt((F32(1.0) - a) / a)


def euler_init_coeffs(acp, t0):
    s0 = sigma(acp, t0)
    return float(s0), float(np.sqrt(s0 * s0 + F32(1.0)))


def euler_coeffs(acp, t, t_next):
    """(sigma_next - sigma_t, sqrt(sigma_next^2 + 1), sigma_next); t_next None: the last step."""
    sn = sigma(acp, t_next)
    return float(sn - sigma(acp, t)), float(np.sqrt(sn * sn + F32(1.0))), float(sn)


def lcm_coeffs(acp, t, t_next):
    """(sqrt(1 - a_t), sqrt(a_t), c_out, c_skip, sqrt(a_next), sqrt(1 - a_next)); c_skip = 0.25 / ((10 t)^2 + 0.25),
    c_out = 10 t / sqrt((10 t)^2 + 0.25)."""
    a, an = _a(acp, t), _a(acp, t_next)
    s = F32(10 * t)
    q = s * s + F32(0.25)
    return (float(np.sqrt(F32(1.0) - a)), float(np.sqrt(a)), float(s / np.sqrt(q)), float(F32(0.25) / q), float(np.sqrt(an)),
            float(np.sqrt(F32(1.0) - an)))


def coeffs(sampler, acp, ts, i):
    t_next = ts[i + 1] if i + 1 < len(ts) else None
    return euler_coeffs(acp, ts[i], t_next) if sampler == "euler" else lcm_coeffs(acp, ts[i], t_next)


def k32(v):
    """A host coefficient as the 0-dim float32 tensor the expressions take."""
    return torch.tensor(float(v), dtype=torch.float32)


VAE_SCALE = k32(0.18215)


# ---- the first latents ---------------------------------------------------------------------------------------------------------------
def first_latents(sampler, img_latent, noise, acp, t0):
    """-> (channels 0..3 of the UNet's first input, the Euler state or None).  Euler: the sample img_latent + sigma_0 * noise in
    float32, stored once as the state and once divided by sqrt(sigma_0^2 + 1) as the input; LCM: scheduler.add_noise as the PLMS
    path has it (every operation in the dtype)."""
    if sampler == "lcm":
        return plms_oracle.PLMSOracle().add_noise(img_latent, noise, torch.tensor([t0])), None
    s0, scale = (k32(v) for v in euler_init_coeffs(acp, t0))
    lat = img_latent.float() + s0 * noise.float()            # 2 roundings
    return (lat / scale).to(img_latent.dtype), lat.to(img_latent.dtype)


# ---- one step ------------------------------------------------------------------------------------------------------------------------
def guided(pred, guidance, cfg):
    """e, in the dtype: u + guidance * (t - u) of the two halves of pred, or pred itself without guidance."""
    if not cfg:
        return pred
    u, t = pred.chunk(2)
    return u + guidance * (t - u)


def prev_f32(sampler, s, e, k, last, z=None):
    """The sample after the step, float32, from the sample s and the prediction e (both of the dtype)."""
    s, e = s.float(), e.float()
    k = [k32(v) for v in k]
    if sampler == "euler":
        return s + e * k[0]                                  # 2 roundings
    x0 = (s - k[0] * e) / k[1]                               # 3 roundings
    den = k[2] * x0 + k[3] * s                               # 6 on the path of x0
    return den if last else k[4] * den + k[5] * z.float()    # 9


def keep_f32(sampler, img_latent, noise0, k, last):
    """The image's latents at the next noise level, float32 (a 4-channel model, outside the mask)."""
    if last:
        return img_latent.float()
    k = [k32(v) for v in k]
    if sampler == "euler":
        return img_latent.float() + k[2] * noise0.float()    # 2 roundings
    return k[4] * img_latent.float() + k[5] * noise0.float()  # 3 roundings


def step(sampler, pred, s, k, guidance, cfg, last, z=None, blend=None):
    """One step.  pred [2n or n,4,h,w], s [n,4,h,w] (Euler: the state; LCM: channels 0..3 of the input), z: this step's noise
    (LCM, not the last step), blend = (img_latent, noise0, mask_l [n,1,h,w]) for a 4-channel model or None.
    -> dict(x: channels 0..3 of the next input, state: the Euler state (LCM: None), decode_in: lat / 0.18215), of the dtype.
    The blend is a select: where(mask_l != 0, prev, keep) moves values, nothing is multiplied by the mask."""
    dtype = s.dtype
    lat = prev_f32(sampler, s, guided(pred, guidance, cfg), k, last, z)
    if blend is not None:
        img_latent, noise0, mask_l = blend
        lat = torch.where(mask_l != 0, lat, keep_f32(sampler, img_latent, noise0, k, last))
    x = (lat / k32(k[1])).to(dtype) if sampler == "euler" else lat.to(dtype)
    return dict(x=x, state=lat.to(dtype) if sampler == "euler" else None, decode_in=(lat / VAE_SCALE).to(dtype))
