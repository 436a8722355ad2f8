"""Deterministic stand-ins for the model of null-text inversion, for the fixture maker (on the CPU, under the reference's own
NullInversion) and the tests (on the GPU, under comfystereo_amd.inversion) alike.  Both have the reference's `ldm_stable`
surface -- tokenizer, text_encoder, unet, vae, scheduler, device.

Shared: a DDIM-like scheduler of our own (`alphas_cumprod`: Stable Diffusion's scaled-linear schedule, computed in Python floats and
kept as 1000 float32 entries on the host; `final_alpha_cumprod` = its first entry; `timesteps` spaced from the top down with an
offset of 1, so the last step's neighbour lies below 0 and both `final_alpha_cumprod` branches are taken); a VAE that is
sub-sampling and sums of two terms; a tokenizer whose ids depend on the prompt's length and a text encoder that rolls a seeded
table of multiples of 1/8 by them.

form "exact": the UNet is roll, flip, additions and multiplications by powers of two -- every operation one IEEE rounding, the
same on every device, no matrix product -- and adds a [64,64] plane of `encoder_hidden_states` to every channel: linear in the
embedding and differentiable.  No module is named CrossAttention: the attention hook finds nothing, which is legal.

form "attn": the same plus one module whose class IS named CrossAttention (to_q / to_k / to_v / to_out, heads = 2, head
dimension 4, scale 0.5; 4096 queries from the latent's pixels, 77 keys from the embedding) under the child `down_blocks`: the
hook of register_attention_control installs on it and the fused forward and backward run inside the optimisation loop.
"""
import math
import types

import numpy as np
import torch
import torch.nn as nn

TOKENS, WIDTH = 77, 64
HEADS, HEAD_DIM = 2, 4
PROMPT_SHIFT = 2.0 ** -7    # text encoder: embedding = table + PROMPT_SHIFT * (the table rolled by the prompt's length)
CONTEXT_GAIN = 1.0          # UNet: what a unit of the embedding adds to the prediction


class NullTokenizer:
    model_max_length = TOKENS

    def __call__(self, prompts, **kwargs):
        ids = torch.stack([torch.arange(TOKENS, dtype=torch.int64) + len(p) for p in prompts])
        return types.SimpleNamespace(input_ids=ids)


class NullTextEncoder:
    def __init__(self, device, dtype):
        g = torch.Generator().manual_seed(4321)
        table = torch.randint(-8, 9, (TOKENS, WIDTH), generator=g).double() / 8
        # the prompt moves the embedding a little, as far as a few Adam steps of null-text optimisation reach
        self.tables = [(table + PROMPT_SHIFT * torch.roll(table, k, 1)).to(device, dtype) for k in range(TOKENS)]

    def __call__(self, input_ids):
        return (torch.stack([self.tables[int(row[0]) % TOKENS] for row in input_ids.cpu()]),)


class NullScheduler:
    def __init__(self):
        # one Python float operation at a time: IEEE double, the same on every host (array code may fuse or reorder)
        lo, hi, prod, alphas = math.sqrt(0.00085), math.sqrt(0.012), 1.0, []
        for i in range(1000):
            root = lo + (hi - lo) * i / 999
            prod = prod * (1.0 - root * root)
            alphas.append(prod)
        self.alphas_cumprod = torch.from_numpy(np.array(alphas, dtype=np.float64).astype(np.float32))
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.config = types.SimpleNamespace(num_train_timesteps=1000, steps_offset=1)
        self.num_inference_steps = None
        self.timesteps = torch.zeros(0, dtype=torch.int64)

    def set_timesteps(self, n):
        self.num_inference_steps = n
        self.timesteps = torch.arange(n - 1, -1, -1, dtype=torch.int64) * (1000 // n) + 1

    # the Standard loop's use of a scheduler (stereodiffusion_nodes.text2stereoimage)
    def scale_model_input(self, latents, t):
        return latents

    def step(self, noise_pred, t, latents):
        return {"prev_sample": latents - 0.125 * noise_pred}


class CrossAttention(nn.Module):
    """The surface the attention hooks look for (the class name, to_q / to_k / to_v / to_out, heads, scale)."""

    def __init__(self, query_dim, context_dim, generator):
        super().__init__()
        inner = HEADS * HEAD_DIM
        self.heads, self.scale = HEADS, HEAD_DIM ** -0.5
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim)])
        with torch.no_grad():
            for p, spread in ((self.to_q.weight, 1.0), (self.to_k.weight, 0.25), (self.to_v.weight, 0.25), (self.to_out[0].weight, 0.5),
                              (self.to_out[0].bias, 0.1)):
                p.copy_((torch.rand(p.shape, generator=generator, dtype=torch.float64) * 2 - 1) * spread)

    def reshape_heads_to_batch_dim(self, t):
        b, n, hd = t.shape
        return t.reshape(b, n, self.heads, hd // self.heads).permute(0, 2, 1, 3).reshape(b * self.heads, n, hd // self.heads)

    def reshape_batch_dim_to_heads(self, t):
        bh, n, d = t.shape
        return t.reshape(bh // self.heads, self.heads, n, d).permute(0, 2, 1, 3).reshape(bh // self.heads, n, self.heads * d)

    def forward(self, x, context=None, mask=None):
        context = x if context is None else context
        q, k, v = (self.reshape_heads_to_batch_dim(t) for t in (self.to_q(x), self.to_k(context), self.to_v(context)))
        attn = (torch.einsum("b i d, b j d -> b i j", q, k) * self.scale).softmax(dim=-1)
        return self.to_out[0](self.reshape_batch_dim_to_heads(torch.einsum("b i j, b j d -> b i d", attn, v)))


class NullUNet(nn.Module):
    in_channels = 4

    def __init__(self, form):
        super().__init__()
        self.gain = nn.Parameter(torch.ones(()))   # times 1: exact, and the output requires grad as a real UNet's does
        if form == "attn":
            self.down_blocks = nn.ModuleList([CrossAttention(4, WIDTH, torch.Generator().manual_seed(99))])
        self.form = form

    def forward(self, x, t, encoder_hidden_states=None):
        ctx = encoder_hidden_states
        late = 0.5 if int(t) >= 500 else 0.25
        sample = late * torch.roll(x, 1, dims=-1) - 0.25 * torch.flip(x, dims=[-2])
        sample = sample + 0.125 * torch.roll(x, 1, dims=1)
        plane = ctx[:, :x.shape[-2], :x.shape[-1]]   # [64,64] at the reference's latents; smaller work frames take their corner
        planes = torch.stack([plane, torch.roll(plane, 1, -1), torch.flip(plane, [-2]), torch.roll(plane, 3, -2)], 1)
        sample = sample + CONTEXT_GAIN * planes
        if self.form == "attn":
            b, c, h, w = x.shape
            tokens = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
            mixed = self.down_blocks[0](tokens, context=ctx)
            sample = sample + 0.25 * mixed.reshape(b, h, w, c).permute(0, 3, 1, 2)
        return {"sample": sample * self.gain}


class NullVAE(nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = nn.Parameter(torch.zeros(()))   # gives the VAE a dtype (reference inversion.py:117)

    def encode(self, image):
        r, g, b = (image[:, i, ::8, ::8] for i in range(3))
        mean = torch.stack([r, g, b, 0.5 * r - 0.5 * g], 1)
        return {"latent_dist": types.SimpleNamespace(mean=mean)}

    def decode(self, z):
        z = 0.25 * z
        rgb = torch.stack([z[:, 0] + 0.5 * z[:, 1], z[:, 1] - 0.25 * z[:, 2], 0.5 * z[:, 2] + z[:, 3]], 1)
        return {"sample": rgb.repeat_interleave(8, -2).repeat_interleave(8, -1).contiguous()}


class NullModel:
    def __init__(self, form="exact", device="cpu", dtype=torch.float32):
        if form not in ("exact", "attn"):
            raise ValueError(form)
        self.device = torch.device(device)
        self.dtype = dtype
        self.tokenizer = NullTokenizer()
        self.text_encoder = NullTextEncoder(self.device, dtype)
        self.unet = NullUNet(form).to(self.device, dtype)
        self.vae = NullVAE().to(self.device, dtype)
        self.scheduler = NullScheduler()


def seeded_image(seed, size=512):
    """uint8 [size,size,3]: blocks of three scales, as the other fixtures' images."""
    rng = np.random.default_rng(seed)
    out = np.zeros((size, size, 3), dtype=np.int64)
    for step, weight in ((64, 2), (16, 1), (8, 1)):
        g = rng.integers(0, 256, (size // step, size // step, 3))
        out += weight * np.repeat(np.repeat(g, step, 0), step, 1)
    return (out // 4).astype(np.uint8)
