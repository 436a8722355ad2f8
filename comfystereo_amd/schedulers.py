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

prediction_type="v_prediction" (the SD 2.x 768-v checkpoints; Salimans & Ho, "Progressive Distillation for Fast Sampling of
Diffusion Models", 2022): the model answers v = c2 * eps - c1 * x0, and the step, in the operation order of diffusers'
DDIMScheduler.step, is

    x0 = c2 * sample - c1 * v;    e = c2 * v + c1 * sample;    prev = c4 * x0 + c3 * e

c2 is then the first operand of a product like the other three and coeffs() rounds it to a half dtype too.
tools/vpred_oracle.py states this independently.

_sqrt and _operand, the two rules that turn an alpha into the float a kernel takes, live here; inversion.py and inpaint_runner.py
import them.
"""
import math
import types

import torch


PREDICTION_TYPES = ("epsilon", "v_prediction")


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


def check_work_size(work_size):
    """The side of the square frame Standard mode works on (512; 768 for the SD 2.x 768-v checkpoints): a positive multiple of 8,
    the VAE's factor, or ValueError.  -> work_size"""
    if isinstance(work_size, bool) or not isinstance(work_size, int) or work_size < 8 or work_size % 8:
        raise ValueError(f"work_size must be a positive multiple of 8, got {work_size!r}")
    return work_size


def prediction_of(scheduler):
    """What the scheduler's model predicts: scheduler.config.prediction_type, "epsilon" where a scheduler does not say."""
    prediction = getattr(getattr(scheduler, "config", None), "prediction_type", "epsilon")
    if prediction not in PREDICTION_TYPES:
        raise ValueError(f"prediction_type must be one of {', '.join(PREDICTION_TYPES)}, got {prediction!r}")
    return prediction


class StepOutput(dict):
    """What step() returns: it answers both ["prev_sample"] and .prev_sample."""

    @property
    def prev_sample(self):
        return self["prev_sample"]


def step_coeffs(alpha_t, alpha_other, dtype, prediction_type="epsilon"):
    """The four floats of the step between two alphas: c1, c3 and c4 multiply (rounded to a half dtype first); c2 divides under
    "epsilon" (it keeps its float32) and multiplies under "v_prediction" (rounded like the others)."""
    return (_operand(_sqrt(1 - alpha_t), dtype, True), _operand(_sqrt(alpha_t), dtype, prediction_type == "v_prediction"),
            _operand(_sqrt(1 - alpha_other), dtype, True), _operand(_sqrt(alpha_other), dtype, True))


class DDIMScheduler:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                 num_train_timesteps=1000, prediction_type="epsilon"):
        if beta_schedule != "scaled_linear" or clip_sample:
            raise ValueError("DDIMScheduler restates the scaled_linear schedule without sample clipping only")
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type must be one of {', '.join(PREDICTION_TYPES)}, got {prediction_type!r}")
        from .inpaint_runner import scaled_linear_alphas_cumprod   # (inpaint_runner imports this module's helpers)
        self.config = types.SimpleNamespace(num_train_timesteps=int(num_train_timesteps), beta_start=beta_start, beta_end=beta_end,
                                            beta_schedule=beta_schedule, clip_sample=False, set_alpha_to_one=bool(set_alpha_to_one),
                                            prediction_type=prediction_type, timestep_spacing="leading", steps_offset=0)
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
        multiply (rounded to a half dtype first), c2 divides (it keeps its float32) -- or, for a v-prediction model, multiplies and is
        rounded like the others (step_coeffs)."""
        if self.num_inference_steps is None:
            raise ValueError("set_timesteps has not been called")
        t = int(timestep)
        key = (t, dtype, self.num_inference_steps, self.config.prediction_type)
        if key not in self._coeffs:
            prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
            self._coeffs[key] = step_coeffs(a_t, a_prev, dtype, self.config.prediction_type)
        return self._coeffs[key]

    def step(self, model_output, timestep, sample):
        """One DDIM step (eta 0): the previous sample from the model's answer `model_output` (the noise, or v) at `timestep`."""
        prediction = self.config.prediction_type
        if prediction not in PREDICTION_TYPES:   # (config is a plain namespace: someone may have written to it)
            raise ValueError(f"prediction_type must be one of {', '.join(PREDICTION_TYPES)}, got {prediction!r}")
        if sample.is_cuda:
            from . import engine
            prev = engine.ddim_step_pred(sample.detach().contiguous(), model_output.detach().contiguous(), None, 1.0,
                                         self.coeffs(timestep, sample.dtype), prediction=prediction)
            return StepOutput(prev_sample=prev)
        if self.num_inference_steps is None:
            raise ValueError("set_timesteps has not been called")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        if prediction == "v_prediction":
            pred_original = _sqrt(a_t) * sample - _sqrt(1 - a_t) * model_output
            pred_epsilon = _sqrt(a_t) * model_output + _sqrt(1 - a_t) * sample
            return StepOutput(prev_sample=_sqrt(a_prev) * pred_original + _sqrt(1 - a_prev) * pred_epsilon)
        pred_original = (sample - _sqrt(1 - a_t) * model_output) / _sqrt(a_t)
        direction = _sqrt(1 - a_prev) * model_output
        return StepOutput(prev_sample=_sqrt(a_prev) * pred_original + direction)
