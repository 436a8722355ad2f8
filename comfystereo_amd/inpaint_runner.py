"""StereoDiffusion's Fast mode around its inpainting model: the loop of the reference's ComfyUIInpaintRunner.__call__
(model_wrappers.py:522-641) on fused HIP kernels.

The UNet, VAE, text encoder and tokenizer are the caller's, duck-typed exactly as the reference's self.unet / vae / text_encoder /
tokenizer; everything between two model calls runs in one HIP launch each:

  image and mask -> img, img * (1 - mask), the mask at the latents' size (:562-572, :580)   engine.inpaint_image_prep
  mean * 0.18215 twice, scheduler.add_noise (:575-602)                                       engine.inpaint_latent_init
  guidance + PNDMScheduler.step (:621-625), latents / 0.18215 on the last step (:628)        engine.plms_step
  (decoded / 2 + 0.5).clamp(0, 1), nan_to_num, * 255 -> uint8 (:629-634)                     engine.decode_to_codes

The UNet reads ONE persistent input x [2n, 9, hl, wl] (uncond half, cond half; per frame latents, mask, masked-image latents): the
step kernel writes the new latents straight into channels 0..3 of both halves, so between two UNet calls there is no `cat`, no
torch elementwise kernel and no allocation -- one launch.  Channels 4..8 are written once before the loop.

PLMS is the reference's PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True)
(:515-520), restated here from the published algorithm (diffusers is not a dependency): the timestep list with its second entry
duplicated, the two warm-up combinations, the linear multistep ones up to order 4.  A step's coefficients are a function of
(counter, t) -- the runner slices the timestep list for strength < 1 while the counter still starts at 0 (:592-593), so the warm-up
falls on whatever the first two sliced timesteps are -- evaluated on the host with the roundings CPU torch gives 0-dim float32
coefficients that meet tensors of the model's dtype (inversion._operand, inversion._sqrt).

No CPU fallback: without a GPU the first kernel raises RuntimeError.
"""
import torch

from . import _native, engine
from .inversion import _operand, _sqrt

BETA_START, BETA_END, TRAIN_STEPS = 0.00085, 0.012, 1000   # (:515-520)
VAE_FACTOR = 8             # the first guess of the latents' size; the VAE's answer decides
DEFAULT_PROMPT = "high quality, detailed"   # reference stereodiffusion_nodes.py:368


def scaled_linear_alphas_cumprod(beta_start=BETA_START, beta_end=BETA_END, num_train_timesteps=TRAIN_STEPS):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def plms_timesteps(num_inference_steps, num_train_timesteps=TRAIN_STEPS):
    """The N + 1 timesteps of PLMS without its Runge-Kutta warm-up, descending, the second duplicated (N = 1: one entry)."""
    ratio = num_train_timesteps // num_inference_steps
    ts = [i * ratio for i in range(num_inference_steps)]
    return (ts[:-1] + ts[-2:-1] + ts[-1:])[::-1]


def plms_kind(counter, kept):
    """-> (kind, kept'): the combination of step `counter` when `kept` predictions are in the history (at most 4 are kept)."""
    if counter == 0:
        return "first", 1
    if counter == 1:
        return "second", kept
    kept = min(kept + 1, 4)
    return ("order2", "order3", "order4")[kept - 2], kept


def plms_coeffs(alphas_cumprod, final_alpha_cumprod, counter, t, ratio, dtype):
    """(sc, da, denom) of prev = sc * sample - da * m / denom for step `counter` at timestep `t`: sc and da meet the tensors as the
    first operand of a product (rounded to a half dtype first), denom divides (it keeps its float32)."""
    prev_t = t - ratio
    if counter == 1:   # the second warm-up step goes over the first one's interval again
        prev_t, t = t, t + ratio
    a_t = alphas_cumprod[t]
    a_p = alphas_cumprod[prev_t] if prev_t >= 0 else final_alpha_cumprod
    sc = _sqrt(a_p / a_t)
    denom = a_t * _sqrt(1 - a_p) + _sqrt(a_t * (1 - a_t) * a_p)
    return _operand(sc, dtype, True), _operand(a_p - a_t, dtype, True), _operand(denom, dtype, False)


def add_noise_coeffs(alphas_cumprod, t, dtype):
    """(sa, sb) of scheduler.add_noise: the square roots of alphas_cumprod.to(dtype)[t] and of one minus it, in the dtype."""
    a = alphas_cumprod[t].to(dtype)
    return float(_sqrt(a)), float(_sqrt(1 - a))


class InpaintLoop:
    """The denoising loop's state on the device: x, the ring of four predictions, cur_sample, the VAE's input.  step(i) is one UNet
    call and one launch; it does not wait for the device or allocate, so it can be captured in a graph."""

    def __init__(self, runner, x, context, timesteps, guidance_scale):
        self.runner, self.x, self.context, self.timesteps, self.guidance = runner, x, context, list(timesteps), float(guidance_scale)
        n2, _, hl, wl = x.shape
        self.n = n2 // 2
        shape = (self.n, 4, hl, wl)
        self.history = torch.empty((4,) + shape, dtype=x.dtype, device=x.device)
        self.cur_sample = torch.empty(shape, dtype=x.dtype, device=x.device)
        self.decode_in = torch.empty(shape, dtype=x.dtype, device=x.device)
        # the timesteps as the UNet takes them (:611, :616): one conversion before the loop, a view per step
        self.t_model = torch.tensor(self.timesteps, dtype=torch.int64).to(x.device).to(x.dtype)
        self.ratio = runner.num_train_timesteps // runner.num_inference_steps
        # per step: the kind, the ring slots it reads (the latest first) and the one it writes, the coefficients
        self.plan, kept, head = [], 0, -1
        for counter, t in enumerate(self.timesteps):
            kind, kept = plms_kind(counter, kept)
            reads = [(head - j) % 4 for j in range((0, 1, 1, 2, 3)[_native.PLMS_KIND[kind]])]
            write = None if kind == "second" else (head + 1) % 4
            head = head if write is None else write
            coeffs = plms_coeffs(runner.alphas_cumprod, runner.final_alpha_cumprod, counter, t, self.ratio, x.dtype)
            self.plan.append((kind, reads, write, coeffs))

    def step(self, i):
        kind, reads, write, coeffs = self.plan[i]
        noise_pred = self.runner.unet(self.x, self.t_model[i].expand(2 * self.n), context=self.context)
        if not noise_pred.is_contiguous():
            noise_pred = noise_pred.contiguous()
        engine.plms_step(noise_pred.detach(), self.x, kind, self.guidance, coeffs, e_out=None if write is None else self.history[write],
                         history=[self.history[r] for r in reads], cur_sample=self.cur_sample if kind in ("first", "second") else None,
                         decode_in=self.decode_in if i == len(self.plan) - 1 else None)
        return self.x


class InpaintRunner:
    """ComfyUIInpaintRunner (reference model_wrappers.py:488-641) around the caller's models.  unet(x, t, context=...) -> the noise
    prediction; vae.encode(img)['latent_dist'].mean, vae.decode(z)['sample']; text_encoder(ids)[0]; tokenizer(prompts, ...).input_ids.
    scheduler: only its alphas_cumprod, final_alpha_cumprod and config.num_train_timesteps are read; None: the reference's constants."""

    def __init__(self, unet, vae, text_encoder, tokenizer, scheduler=None):
        in_ch = unet.in_channels if hasattr(unet, 'in_channels') else 4
        if in_ch != 9:
            raise ValueError(
                f"Connected model has {in_ch} UNet input channels, but inpainting "
                f"requires 9 channels. Please use an inpainting checkpoint "
                f"(e.g., sd-v1-5-inpainting)."
            )
        self.unet, self.vae, self.text_encoder, self.tokenizer = unet, vae, text_encoder, tokenizer
        if scheduler is None:
            self.alphas_cumprod = scaled_linear_alphas_cumprod()
            self.num_train_timesteps = TRAIN_STEPS
            self.final_alpha_cumprod = self.alphas_cumprod[0]
        else:
            self.alphas_cumprod = scheduler.alphas_cumprod.detach().to("cpu", torch.float32)
            self.num_train_timesteps = int(scheduler.config.num_train_timesteps)
            final = getattr(scheduler, "final_alpha_cumprod", None)
            self.final_alpha_cumprod = self.alphas_cumprod[0] if final is None else torch.as_tensor(final).detach().to("cpu", torch.float32)
        self.num_inference_steps = None
        self.loop = None   # the last run's InpaintLoop (its x holds the final latents in channels 0..3)

    def _embeddings(self, prompt, device):
        tok = self.tokenizer
        text_input = tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        text_embeddings = self.text_encoder(text_input.input_ids.to(device))[0]
        uncond_input = tok([""], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        uncond_embeddings = self.text_encoder(uncond_input.input_ids.to(device))[0]
        return uncond_embeddings, text_embeddings

    @torch.no_grad()
    def prepare(self, prompt, filled_u8, mask, generators, num_inference_steps=30, guidance_scale=7.5, strength=1.0):
        """Everything before the loop (:539-602) -> the InpaintLoop, ready for step(0)."""
        param = next(self.unet.parameters())
        device, dtype = param.device, param.dtype
        if not isinstance(filled_u8, torch.Tensor) or filled_u8.dim() != 4 or filled_u8.shape[-1] != 3 or filled_u8.dtype != torch.uint8:
            raise ValueError("filled_u8 must be a uint8 tensor [N,H,W,3]")
        n, h, w, _ = filled_u8.shape
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (n, h, w) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"mask must be a uint8 or bool tensor {(n, h, w)}")
        generators = list(generators) if isinstance(generators, (list, tuple)) else [generators]
        if len(generators) != n:
            raise ValueError(f"{n} frame(s) take {n} generator(s), got {len(generators)}")
        if int(num_inference_steps) < 1:
            raise ValueError(f"num_inference_steps must be at least 1, got {num_inference_steps}")
        filled_u8, mask = filled_u8.to(device).contiguous(), mask.to(device).contiguous()
        self.num_inference_steps = int(num_inference_steps)

        uncond, cond = self._embeddings(prompt, device)
        context = torch.cat([uncond.expand(n, -1, -1), cond.expand(n, -1, -1)]).to(dtype).contiguous()   # [uncond, cond] (:558)

        hl, wl = max(h // VAE_FACTOR, 1), max(w // VAE_FACTOR, 1)
        x = torch.empty((2 * n, 9, hl, wl), dtype=dtype, device=device)
        img, masked = engine.inpaint_image_prep(filled_u8, mask, x, (hl, wl))
        mean_img = self.vae.encode(img)['latent_dist'].mean
        mean_masked = self.vae.encode(masked)['latent_dist'].mean
        if tuple(mean_img.shape[2:]) != (hl, wl):   # a VAE of another factor: the mask again, at its size
            hl, wl = mean_img.shape[2], mean_img.shape[3]
            x = torch.empty((2 * n, 9, hl, wl), dtype=dtype, device=device)
            engine.inpaint_image_prep(filled_u8, mask, x, (hl, wl))

        timesteps = plms_timesteps(self.num_inference_steps, self.num_train_timesteps)
        timesteps = timesteps[max(0, int(len(timesteps) * (1.0 - strength))):]   # (:592-593)
        # drawn on the host in the model's dtype, frame by frame, as the reference draws it (:596-597)
        noise = torch.cat([torch.randn((1, 4, hl, wl), generator=g, device="cpu", dtype=dtype) for g in generators]).to(device)
        loop = InpaintLoop(self, x, context, timesteps, guidance_scale)
        mean_img, mean_masked = mean_img.detach().to(device).contiguous(), mean_masked.detach().to(device).contiguous()
        if timesteps:
            coeffs = add_noise_coeffs(self.alphas_cumprod, timesteps[0], dtype)
            loop.img_latent = engine.inpaint_latent_init(mean_img, mean_masked, noise, coeffs, x)
        else:   # the latents are the image's, and the VAE's input comes from here
            loop.img_latent = engine.inpaint_latent_init(mean_img, mean_masked, None, None, x, decode_in=loop.decode_in)
        self.loop = loop
        return loop

    @torch.no_grad()
    def run(self, prompt, filled_u8, mask, generators, num_inference_steps=30, guidance_scale=7.5, strength=1.0):
        """n frames in one UNet batch of 2n: filled_u8 uint8 [n,h,w,3], mask uint8 or bool [n,h,w] (non-zero: inpaint), device
        tensors; frame k draws its noise from generators[k].  -> uint8 [n,h,w,3]"""
        loop = self.prepare(prompt, filled_u8, mask, generators, num_inference_steps, guidance_scale, strength)
        for i in range(len(loop.timesteps)):
            loop.step(i)
        decoded = self.vae.decode(loop.decode_in)['sample']
        return engine.decode_to_codes(decoded.detach().to(loop.x.device).contiguous())

    def __call__(self, prompt, filled_u8, mask, num_inference_steps=30, guidance_scale=7.5, strength=1.0, generator=None):
        """One frame: filled_u8 uint8 [h,w,3], mask [h,w] -> uint8 [h,w,3]."""
        return self.run(prompt, filled_u8[None], mask[None], [generator], num_inference_steps, guidance_scale, strength)[0]


def make_inpaint(runner, prompt, num_inference_steps=30, guidance_scale=7.5, strength=1.0, seed=0):
    """-> inpaint(filled_u8, mask, frame_index): the callable stereodiffusion_nodes.generate_stereo_fast takes where the reference
    calls its inpainting pipeline, with a fresh CPU generator seeded seed + frame_index per frame (reference
    stereodiffusion_nodes.py:378-387) and the reference's prompt for an empty one (:368)."""
    prompt = prompt if prompt else DEFAULT_PROMPT

    def inpaint(filled_u8, mask, frame_index):
        generator = torch.Generator(device="cpu")
        generator.manual_seed(seed + frame_index)
        return runner(prompt, filled_u8, mask, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                      strength=strength, generator=generator)

    return inpaint
