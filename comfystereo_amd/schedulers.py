"""The DDIM scheduler of StereoDiffusion's Standard mode, restated from the published algorithm (Song et al., "Denoising Diffusion
Implicit Models") with the arguments the reference gives diffusers' class (reference model_wrappers.py:429-435): scaled_linear
betas 0.00085 .. 0.012 over 1000 training steps, set_alpha_to_one=False (the last step goes to alphas_cumprod[0]),
clip_sample=False, eta 0, epsilon prediction, leading timestep spacing with offset 0.  diffusers is not a dependency.

The surface is what inversion.NullInversion, inpaint_runner.InpaintRunner and the Standard loop read: config.num_train_timesteps,
num_inference_steps, alphas_cumprod, final_alpha_cumprod, set_timesteps, timesteps, scale_model_input, step -- and coeffs(t, dtype),
the four float32 coefficients of

    prev = c4 * ((sample - c1 * e) / c2) + c3 * e,    c1 = sqrt(1 - a_t), c2 = sqrt(a_t), c3 = sqrt(1 - a_prev), c4 = sqrt(a_prev)

which engine.ddim_step and engine.standard_step take.  step() on device tensors is engine.ddim_step, one launch; on host tensors it
is the torch expression.  tools/ddim_oracle.py states the same independently, for the tests.

_sqrt and _operand, the two rules that turn an alpha into the float a kernel takes, live here; inversion.py and inpaint_runner.py
import them.
"""
import math
import types

import torch


def _sqrt(x):
    """x ** 0.5 (reference inversion.py:62-64, :72-74), correctly rounded.  torch evaluates the power -- and torch.sqrt -- of a 0-dim
    float32 tensor with whatever its CPU dispatch picks on the host, and not every pick is correctly rounded (an ulp on some
    alphas).  The square root in double, rounded to the tensor's dtype, is the correctly rounded result everywhere (a double holds
    more than twice a float32's bits plus two), which is also what the reference's expression gives wherever it is right."""
    if isinstance(x, torch.Tensor):
        return torch.tensor(math.sqrt(float(x)), dtype=x.dtype if x.is_floating_point() else torch.float32)
    return x ** 0.5


def _operand(c, dtype, first):
    """The float the kernels take for a coefficient `c` that multiplies (first=True) or divides a tensor of `dtype`: CPU torch
    converts a 0-dim float32 tensor that is the first operand of a product with a half tensor to the half dtype before it
    multiplies, and keeps a divisor's float32."""
    if first and isinstance(c, torch.Tensor) and dtype in (torch.float16, torch.bfloat16):
        c = c.to(dtype)
    return float(c)


class StepOutput(dict):
    """What step() returns: it answers both ["prev_sample"] and .prev_sample."""

    @property
    def prev_sample(self):
        return self["prev_sample"]


class DDIMScheduler:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                 num_train_timesteps=1000):
        if beta_schedule != "scaled_linear" or clip_sample:
            raise ValueError("DDIMScheduler restates the scaled_linear schedule without sample clipping only")
        from .inpaint_runner import scaled_linear_alphas_cumprod   # (inpaint_runner imports this module's helpers)
        self.config = types.SimpleNamespace(num_train_timesteps=int(num_train_timesteps), beta_start=beta_start, beta_end=beta_end,
                                            beta_schedule=beta_schedule, clip_sample=False, set_alpha_to_one=bool(set_alpha_to_one),
                                            prediction_type="epsilon", timestep_spacing="leading", steps_offset=0)
        self.alphas_cumprod = scaled_linear_alphas_cumprod(beta_start, beta_end, int(num_train_timesteps))
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.arange(int(num_train_timesteps) - 1, -1, -1, dtype=torch.int64)
        self._coeffs = {}

    def set_timesteps(self, num_inference_steps, device=None):
        n = int(num_inference_steps)
        if n < 1 or n > self.config.num_train_timesteps:
            raise ValueError(f"num_inference_steps must be in 1..{self.config.num_train_timesteps}, got {num_inference_steps}")
        self.num_inference_steps = n
        ratio = self.config.num_train_timesteps // n
        self.timesteps = (torch.arange(n - 1, -1, -1, dtype=torch.int64) * ratio).to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def coeffs(self, timestep, dtype):
        """(c1, c2, c3, c4) of the step from `timestep` to the one before it, as Python floats holding float32 values: c1, c3 and c4
        multiply (rounded to a half dtype first), c2 divides (it keeps its float32)."""
        if self.num_inference_steps is None:
            raise ValueError("set_timesteps has not been called")
        t = int(timestep)
        key = (t, dtype, self.num_inference_steps)
        if key not in self._coeffs:
            prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
            self._coeffs[key] = (_operand(_sqrt(1 - a_t), dtype, True), _operand(_sqrt(a_t), dtype, False),
                                 _operand(_sqrt(1 - a_prev), dtype, True), _operand(_sqrt(a_prev), dtype, True))
        return self._coeffs[key]

    def step(self, model_output, timestep, sample):
        """One DDIM step (eta 0): the previous sample from the noise prediction `model_output` at `timestep`."""
        if sample.is_cuda:
            from . import engine
            prev = engine.ddim_step(sample.detach().contiguous(), model_output.detach().contiguous(), None, 1.0,
                                    self.coeffs(timestep, sample.dtype))
            return StepOutput(prev_sample=prev)
        if self.num_inference_steps is None:
            raise ValueError("set_timesteps has not been called")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        pred_original = (sample - _sqrt(1 - a_t) * model_output) / _sqrt(a_t)
        direction = _sqrt(1 - a_prev) * model_output
        return StepOutput(prev_sample=_sqrt(a_prev) * pred_original + direction)
