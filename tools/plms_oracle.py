"""PLMS as StereoDiffusion's Fast mode configures it, restated in torch: PNDMScheduler(beta_start=0.00085, beta_end=0.012,
beta_schedule="scaled_linear", skip_prk_steps=True) (reference model_wrappers.py:515-520).

diffusers is not available where the fixtures are made, so this is a restatement of the published algorithm (Liu et al., "Pseudo
Numerical Methods for Diffusion Models on Manifolds", in the form diffusers' PNDMScheduler runs it without its Runge-Kutta
warm-up), NOT a capture of diffusers' own output.  Operation for operation: the coefficients are 0-dim float32 tensors that meet
the sample's dtype exactly where the published step does, which decides how CPU torch rounds each one.

Used by tools/make_inpaintrun_goldens.py (as the scheduler under the reference's own loop), by tools/inpaintrun_bench.py (as the
stock-torch baseline) and by the tests.  Nothing in the package imports it.
"""
import math
import types

import torch

BETA_START, BETA_END, TRAIN_STEPS = 0.00085, 0.012, 1000


def scaled_linear_alphas_cumprod(beta_start=BETA_START, beta_end=BETA_END, num_train_timesteps=TRAIN_STEPS, dtype=torch.float32):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=dtype) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def root(x):
    """x ** 0.5 of a tensor, correctly rounded to its dtype: the square root in double, rounded once.  torch evaluates `** 0.5` of
    a 0-dim tensor with whatever its CPU dispatch picks on the host, and not every pick is correctly rounded (an ulp on a few
    alphas): a restatement that fixtures and tests on other machines share has to say which.  Where torch is right, this is it."""
    flat = [math.sqrt(float(v)) for v in x.reshape(-1)]
    return torch.tensor(flat, dtype=torch.float64).to(x.dtype).reshape(x.shape).to(x.device)


def plms_timesteps(num_inference_steps, num_train_timesteps=TRAIN_STEPS):
    """N + 1 entries with the second duplicated (one entry for N = 1), descending, int64."""
    ratio = num_train_timesteps // num_inference_steps
    ts = torch.arange(0, num_inference_steps, dtype=torch.int64) * ratio
    return torch.cat([ts[:-1], ts[-2:-1], ts[-1:]]).flip(0).contiguous()


class PLMSOracle:
    def __init__(self, beta_start=BETA_START, beta_end=BETA_END, beta_schedule="scaled_linear", skip_prk_steps=True,
                 num_train_timesteps=TRAIN_STEPS, alphas_dtype=torch.float32):
        """alphas_dtype: float32, the scheduler's own; float64 only to measure this restatement's float32 error."""
        if beta_schedule != "scaled_linear" or not skip_prk_steps:
            raise ValueError("PLMSOracle restates the scaled_linear schedule without the Runge-Kutta warm-up only")
        self.config = types.SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end)
        self.alphas_cumprod = scaled_linear_alphas_cumprod(beta_start, beta_end, num_train_timesteps, alphas_dtype)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.zeros(0, dtype=torch.int64)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        self.timesteps = plms_timesteps(num_inference_steps, self.config.num_train_timesteps).to(device)
        self.ets, self.counter, self.cur_sample = [], 0, None

    def add_noise(self, original_samples, noise, timesteps):
        acp = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        timesteps = timesteps.to(original_samples.device)
        sqrt_alpha_prod = root(acp[timesteps]).flatten()
        sqrt_one_minus_alpha_prod = root(1 - acp[timesteps]).flatten()
        while sqrt_alpha_prod.dim() < original_samples.dim():
            sqrt_alpha_prod = sqrt_alpha_prod.unsqueeze(-1)
            sqrt_one_minus_alpha_prod = sqrt_one_minus_alpha_prod.unsqueeze(-1)
        return sqrt_alpha_prod * original_samples + sqrt_one_minus_alpha_prod * noise

    def step(self, model_output, timestep, sample):
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev_timestep = timestep - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + ratio
        ets = self.ets
        if len(ets) == 1 and self.counter == 0:
            self.cur_sample = sample
        elif len(ets) == 1 and self.counter == 1:
            model_output = (model_output + ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(ets) == 2:
            model_output = (3 * ets[-1] - ets[-2]) / 2
        elif len(ets) == 3:
            model_output = (23 * ets[-1] - 16 * ets[-2] + 5 * ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4])
        prev_sample = self._get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return types.SimpleNamespace(prev_sample=prev_sample)

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        sample_coeff = root(alpha_prod_t_prev / alpha_prod_t)
        model_output_denom_coeff = alpha_prod_t * root(beta_prod_t_prev) + root(alpha_prod_t * beta_prod_t * alpha_prod_t_prev)
        return sample_coeff * sample - (alpha_prod_t_prev - alpha_prod_t) * model_output / model_output_denom_coeff
