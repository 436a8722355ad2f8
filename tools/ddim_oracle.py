"""DDIM as StereoDiffusion's Standard mode configures it, restated independently of comfystereo_amd/schedulers.py:
DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
(reference model_wrappers.py:429-435), eta 0, epsilon prediction, leading spacing with offset 0.

diffusers is not available where the fixtures are made, so this is a restatement of the published algorithm (Song et al.,
"Denoising Diffusion Implicit Models", eq. 12 with sigma = 0), NOT a capture of diffusers' output.  Square roots are taken in
double and rounded once, as tools/plms_oracle.py does and for its reason.

  DDIMOracle.step        the torch expression on 0-dim float32 coefficients, as a host scheduler under the reference's own loop
  step_rounded           the same step in float64, every operation rounded as CPU torch rounds it on a tensor of `dtype`: to
                         float32, then to the dtype; a coefficient that is the first operand of a product is rounded to a half
                         dtype before it multiplies, the divisor keeps its float32

Used by the tests and the fixture makers.  Nothing in the package imports it.
"""
import math
import types

import torch

from plms_oracle import BETA_END, BETA_START, TRAIN_STEPS, root, scaled_linear_alphas_cumprod


def ddim_timesteps(num_inference_steps, num_train_timesteps=TRAIN_STEPS):
    """Leading spacing, offset 0: (0, r, 2 r, ...) with r = T // N, descending, int64."""
    ratio = num_train_timesteps // num_inference_steps
    return [i * ratio for i in range(num_inference_steps)][::-1]


def alphas_of_step(alphas_cumprod, final_alpha_cumprod, t, num_inference_steps, num_train_timesteps=TRAIN_STEPS):
    prev_t = t - num_train_timesteps // num_inference_steps
    return alphas_cumprod[t], (alphas_cumprod[prev_t] if prev_t >= 0 else final_alpha_cumprod)


def coefficients(a_t, a_prev, dtype):
    """(c1, c2, c3, c4) as float32 values in Python floats: sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev), sqrt(a_prev)."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))   # noqa: E731
    one = torch.tensor(1.0, dtype=torch.float32)
    c = [f32(math.sqrt(float(one - a_t))), f32(math.sqrt(float(a_t))), f32(math.sqrt(float(one - a_prev))), f32(math.sqrt(float(a_prev)))]
    if dtype in (torch.float16, torch.bfloat16):
        c = [float(torch.tensor(v, dtype=torch.float32).to(dtype)) if i != 1 else v for i, v in enumerate(c)]
    return tuple(c)


def step_rounded(model_output, sample, c, dtype):
    """c4 * ((sample - c1 * e) / c2) + c3 * e in float64, each operation rounded to float32 and then to `dtype` -> a tensor of
    `dtype`."""
    r = lambda v: v.to(torch.float32).to(dtype).double()   # noqa: E731
    e, s = model_output.double(), sample.double()
    c1, c2, c3, c4 = c
    x0 = r(r(s - r(c1 * e)) / c2)
    return r(r(c4 * x0) + r(c3 * e)).to(dtype)


class DDIMOracle:
    def __init__(self, beta_start=BETA_START, beta_end=BETA_END, num_train_timesteps=TRAIN_STEPS):
        self.config = types.SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end)
        self.alphas_cumprod = scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps)
        self.final_alpha_cumprod = self.alphas_cumprod[0]   # set_alpha_to_one=False
        self.num_inference_steps = None
        self.timesteps = torch.zeros(0, dtype=torch.int64)

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.tensor(ddim_timesteps(num_inference_steps, self.config.num_train_timesteps), dtype=torch.int64).to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample):
        a_t, a_prev = alphas_of_step(self.alphas_cumprod, self.final_alpha_cumprod, int(timestep), self.num_inference_steps,
                                     self.config.num_train_timesteps)
        pred_original_sample = (sample - root(1 - a_t) * model_output) / root(a_t)
        pred_sample_direction = root(1 - a_prev) * model_output
        prev_sample = root(a_prev) * pred_original_sample + pred_sample_direction
        return {"prev_sample": prev_sample}
