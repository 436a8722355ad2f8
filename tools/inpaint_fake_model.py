"""A deterministic stand-in for the models of StereoDiffusion's Fast mode, for the fixture maker (on the CPU, under the
reference's own ComfyUIInpaintRunner.__call__) and the tests (on the GPU, under comfystereo_amd.inpaint_runner) alike.

It has the surface the reference's runner uses -- unet(x, t, context=...), vae.encode(img)['latent_dist'].mean,
vae.decode(z)['sample'], text_encoder(ids)[0], tokenizer(prompts, ...).input_ids -- and, like tools/standard_fake_model.py,
nothing in it rounds differently on the two devices: roll, flip, slices, additions and multiplications by powers of two (every
operation elementwise and a single IEEE rounding; no reduction, no matrix product, no transcendental function).

  FakeUNet   9 input channels; its answer depends on all nine, on the timestep and on the context, so cond != uncond
  FakeVAE    encode: every 8th pixel of the image and of a shifted copy (the sign of a zero survives in channel 0);
             decode: 8 x 8 blocks, cropped to the last encoded size, a few pixels forced to NaN, +-inf and values outside [-1, 1]
  tokenizer / text encoder: the embedding is one of four fixed tables, chosen by the prompt's length
"""
import types

import torch
import torch.nn as nn

TOKENS, WIDTH = 77, 8


class FakeTokenizer:
    model_max_length = TOKENS

    def __init__(self):
        self.prompts = []

    def __call__(self, prompts, **kwargs):
        self.prompts.append(list(prompts))
        return types.SimpleNamespace(input_ids=torch.stack([torch.arange(TOKENS, dtype=torch.int64) + len(p) for p in prompts]))


def _table(seed, device, dtype):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-8, 9, (TOKENS, WIDTH), generator=g).float() / 8   # multiples of 1/8: exact in every dtype
    t[0, 0] = (seed % 4 + 1) / 8
    return t.to(device, dtype)


class FakeTextEncoder:
    def __init__(self, device, dtype):
        self.tables = torch.stack([_table(4000 + k, device, dtype) for k in range(4)])

    def __call__(self, input_ids):
        return (self.tables[(input_ids[:, 0] % 4).to(self.tables.device)],)


class FakeUNet(nn.Module):
    in_channels = 9

    def __init__(self, device="cpu", dtype=torch.float32, in_channels=9):
        super().__init__()
        self.in_channels = in_channels
        self.gain = nn.Parameter(torch.ones((), device=device, dtype=dtype))   # times 1: exact in every dtype
        self.record = False
        self.inputs, self.outputs, self.pointers, self.count = [], [], [], 0

    def forward(self, x, t, context=None):
        self.count += 1
        lat, m, ml = x[:, :4], x[:, 4:5], x[:, 5:9]
        ctx = context[:, 0, 0].reshape(-1, 1, 1, 1)
        out = 0.5 * torch.roll(lat, 1, dims=-1) - 0.25 * torch.flip(lat, dims=[-2])
        out = out + 0.125 * torch.roll(lat, 1, dims=1)
        out = out + 0.25 * (m * ml) + 0.125 * torch.roll(ml, 1, dims=1)
        out = out + 0.0625 * ctx + 2.0 ** -12 * t.reshape(-1, 1, 1, 1)
        out = out * self.gain
        if self.record:
            self.inputs.append(x.detach().clone())
            self.outputs.append(out.detach().clone())
            self.pointers.append(x.data_ptr())
        return out


class FakeVAE:
    def __init__(self, mean_dtype=None):
        self.mean_dtype = mean_dtype   # None: the image's
        self.size = None
        self.encoded, self.decoded = 0, 0

    def encode(self, img):
        self.encoded += 1
        self.size = tuple(img.shape[-2:])
        s = img[:, :, ::8, ::8]
        s2 = torch.roll(img, (3, 5), dims=(-2, -1))[:, :, ::8, ::8]
        # channel 0 is a copy: a -0.0 of the masked image stays one.  The others start from a constant: torch's float16 kernels do
        # not agree between devices on the sign of a zero product or of a sum of zeros, and a zero added to something else is gone
        mean = torch.stack([s[:, 0], (s[:, 1] + 0.25) + 0.5 * s2[:, 2], (s[:, 2] - 0.5) - 0.25 * s2[:, 0],
                            (0.5 * s[:, 0] + 0.125) + 0.5 * s2[:, 1]], 1)
        return {"latent_dist": types.SimpleNamespace(mean=mean.to(self.mean_dtype or mean.dtype).contiguous())}

    def decode(self, z):
        self.decoded += 1
        z = 0.25 * z
        rgb = torch.stack([z[:, 0] + 0.5 * z[:, 1], z[:, 1] - 0.25 * z[:, 2], 0.5 * z[:, 2] + z[:, 3]], 1)
        img = rgb.repeat_interleave(8, -2).repeat_interleave(8, -1)
        if self.size is not None:
            img = img[:, :, :self.size[0], :self.size[1]]
        img = img.contiguous()
        img[:, 0, 0, 0] = float("nan")
        img[:, 1, 0, 1] = float("inf")
        img[:, 2, 0, 2] = float("-inf")
        img[:, 0, 1, 0] = 3.0
        img[:, 1, 1, 1] = -3.0
        img[:, 2, 1, 2] = 1.0
        img[:, 0, 1, 3] = -1.0
        return {"sample": img}


class FakeInpaintModel:
    def __init__(self, device="cpu", dtype=torch.float32, mean_dtype=None, in_channels=9):
        self.device, self.dtype = torch.device(device), dtype
        self.tokenizer = FakeTokenizer()
        self.text_encoder = FakeTextEncoder(self.device, dtype)
        self.unet = FakeUNet(self.device, dtype, in_channels)
        self.vae = FakeVAE(mean_dtype)

    def parts(self):
        return self.unet, self.vae, self.text_encoder, self.tokenizer


def seeded_frame(seed, h, w, mask_kind="mixed"):
    """-> (filled uint8 [h,w,3], mask uint8 [h,w] of 0 / 255).  Every pixel below code 128 somewhere under a mixed mask: negative
    pixels under the mask, whose product with (1 - mask) is -0.0."""
    g = torch.Generator().manual_seed(seed)
    filled = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    if mask_kind == "zero":
        mask = torch.zeros((h, w), dtype=torch.uint8)
    elif mask_kind == "one":
        mask = torch.full((h, w), 255, dtype=torch.uint8)
    else:
        mask = (torch.rand((h, w), generator=g) < 0.5).to(torch.uint8) * 255
        mask[0, 0], mask[-1, -1] = 255, 0
        filled[0, 0] = torch.tensor([3, 100, 127], dtype=torch.uint8)   # negative under the mask, at a pixel the VAE keeps
    return filled, mask
