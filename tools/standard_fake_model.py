"""A deterministic stand-in for the models of StereoDiffusion's Standard mode, for the fixture maker (on the CPU, under the
reference's own loop) and the tests (on the GPU, under comfystereo_amd.stereodiffusion_nodes) alike.

It has the reference's `ldm_stable` surface -- tokenizer, text_encoder, unet, vae, scheduler, device -- and nothing in it
rounds differently on the two devices: the UNet and the VAE are built from roll, flip, additions and multiplications by powers
of two (every operation a single IEEE rounding; no matrix product, no transcendental function), the scheduler's step is
latents - 0.125 * noise_pred, the text encoder returns a fixed seeded table.  The VAE forces a few pixels to NaN, +-inf and
values outside [-1, 1].  The UNet multiplies its answer by a parameter that is 1 and requires grad, as a real UNet's
weights do: a caller that leaves autograd on gets tensors that require grad unless the loop switches it off.  No module's
class name contains `Attention`: the attention hooks find no layer, which is legal.

fake_invert stands where the reference runs NullInversion.invert: x_t is a fixed function of the 512 x 512 image codes.
"""
import types

import torch
import torch.nn as nn

TOKENS, WIDTH = 77, 8


class FakeTokenizer:
    model_max_length = TOKENS

    def __call__(self, prompts, **kwargs):
        return types.SimpleNamespace(input_ids=torch.arange(TOKENS, dtype=torch.int64).repeat(len(prompts), 1))


def _table(seed, device, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (1, TOKENS, WIDTH), generator=g).float() / 8).to(device, dtype)   # multiples of 1/8: exact in every dtype


class FakeTextEncoder:
    def __init__(self, device, dtype):
        self.table = _table(1234, device, dtype)

    def __call__(self, input_ids):
        return (self.table.expand(input_ids.shape[0], TOKENS, WIDTH),)


class FakeScheduler:
    def __init__(self):
        self.timesteps = torch.zeros(0, dtype=torch.int64)

    def set_timesteps(self, n):
        self.timesteps = torch.arange(n - 1, -1, -1, dtype=torch.int64) * (1000 // n)

    def scale_model_input(self, latents, t):
        return latents

    def step(self, noise_pred, t, latents):
        return {"prev_sample": latents - 0.125 * noise_pred}


class FakeUNet(nn.Module):
    in_channels = 4

    def __init__(self, device="cpu"):
        super().__init__()
        self.gain = nn.Parameter(torch.ones((), device=device))   # times 1: exact in every dtype
        self.calls = []        # the latents handed to every call (references, not copies), when `record` is set
        self.record = False
        self.fail_at = None    # the call that raises instead of answering (the hook-restoring test)
        self.count = 0

    def forward(self, x, t, encoder_hidden_states=None):
        if self.fail_at is not None and self.count == self.fail_at:
            raise RuntimeError("FakeUNet: told to fail")
        self.count += 1
        if self.record:
            self.calls.append(x)
        ctx = encoder_hidden_states[:, 0, 0].reshape(-1, 1, 1, 1)
        sample = 0.5 * torch.roll(x, 1, dims=-1) - 0.25 * torch.flip(x, dims=[-2])
        sample = sample + 0.125 * torch.roll(x, 1, dims=1)
        return {"sample": (sample + 0.0625 * ctx) * self.gain}


class FakeVAE:
    def decode(self, z):
        z = 0.25 * z
        rgb = torch.stack([z[:, 0] + 0.5 * z[:, 1], z[:, 1] - 0.25 * z[:, 2], 0.5 * z[:, 2] + z[:, 3]], 1)
        img = rgb.repeat_interleave(8, -2).repeat_interleave(8, -1).contiguous()
        img[:, 0, 0, 0] = float("nan")
        img[:, 1, 0, 1] = float("inf")
        img[:, 2, 0, 2] = float("-inf")
        img[:, 0, 1, 0] = 3.0
        img[:, 1, 1, 1] = -3.0
        img[:, 2, 1, 2] = 1.0
        img[:, 0, 1, 3] = -1.0
        return {"sample": img}


class FakeModel:
    def __init__(self, device="cpu", dtype=torch.float32):
        self.device = torch.device(device)
        self.dtype = dtype
        self.tokenizer = FakeTokenizer()
        self.text_encoder = FakeTextEncoder(self.device, dtype)
        self.unet = FakeUNet(self.device)
        self.vae = FakeVAE()
        self.scheduler = FakeScheduler()


def fake_uncond_embeddings(steps, device, dtype):
    """One [1,77,8] embedding per step, as null-text optimisation returns them."""
    return [_table(100 + i, device, dtype) for i in range(steps)]


def fake_invert(image_u8, dtype=torch.float32, steps=None):
    """image_u8 uint8 [512,512,3] (torch, any device) -> (x_t [1,4,64,64] of `dtype` on that device, uncond_embeddings: `steps`
    of them, or None).  x_t[c] = (image[::8, ::8, c % 3] - 128) / 64, exact in every dtype."""
    sub = image_u8[::8, ::8].permute(2, 0, 1).float()
    x_t = ((torch.stack([sub[0], sub[1], sub[2], sub[0].flip(-1)]) - 128) / 64)[None].to(dtype)
    return x_t, (fake_uncond_embeddings(steps, image_u8.device, dtype) if steps else None)
