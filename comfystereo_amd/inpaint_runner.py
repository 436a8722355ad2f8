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

Few-step models (SD-Turbo, the LCM checkpoints) take another family of steps, chosen by InpaintRunner's `sampler`: "euler" (Karras
et al. 2022, Alg. 1 without churn, trailing timestep spacing) and "lcm" (Luo et al. 2023, multistep consistency sampling), restated
from the papers in tools/fewstep_oracle.py, the specification of their bits, and run by FewStepLoop on engine.fewstep_step -- again
one launch between two UNet calls.  With guidance_scale <= 1 they run the UNet on the conditional batch alone (the reference's
diffusion_step_no_cfg, diffusion_utils.py:69-98: "Turbo models: 0.0"), and they accept an ordinary 4-channel UNet, used
RePaint-style as the reference's Fast-mode docstring describes (:328-336): after every step the latents outside the mask are
replaced by the image's latents at the next noise level.  "plms", the default, is everything described above, unchanged.

No CPU fallback: without a GPU the first kernel raises RuntimeError.
"""
import numpy as np
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


SAMPLERS = ("plms", "euler", "lcm")
LCM_ORIGIN_STEPS = 50      # the grid the LCM checkpoints were distilled on
_F32 = np.float32


def fewstep_timesteps(sampler, num_inference_steps, num_train_timesteps=TRAIN_STEPS):
    """The N timesteps of a few-step sampler, descending.  "euler": trailing spacing, round(T - i T / N) - 1 (numpy's round on
    float64); "lcm": the origin grid t = c j - 1 (j = 1..50, c = T // 50), descending, at the indices
    floor(linspace(0, 50, N, endpoint=False))."""
    n, train = int(num_inference_steps), int(num_train_timesteps)
    if sampler == "euler":
        return [int(v) for v in np.round(train - np.arange(n, dtype=np.float64) * (train / n)) - 1]
    if n > LCM_ORIGIN_STEPS:
        raise ValueError(f"sampler 'lcm' takes at most {LCM_ORIGIN_STEPS} steps, got {n}")
    c = train // LCM_ORIGIN_STEPS
    grid = [c * j - 1 for j in range(LCM_ORIGIN_STEPS, 0, -1)]
    return [grid[int(k)] for k in np.floor(np.linspace(0, LCM_ORIGIN_STEPS, n, endpoint=False))]


def _alpha(alphas_cumprod, t):
    """a_t as a numpy float32 scalar (every operation on it is one correctly rounded float32 operation); past the last timestep 1."""
    return _F32(1.0) if t is None else _F32(float(alphas_cumprod[t]))


def _sigma(alphas_cumprod, t):
    a = _alpha(alphas_cumprod, t)
    return np.sqrt((_F32(1.0) - a) / a)


def euler_init_coeffs(alphas_cumprod, t0):
    """(sigma_0, sqrt(sigma_0^2 + 1)): the first sample is img_latent + sigma_0 * noise, the first UNet input that over the root."""
    s0 = _sigma(alphas_cumprod, t0)
    return float(s0), float(np.sqrt(s0 * s0 + _F32(1.0)))


def fewstep_coeffs(sampler, alphas_cumprod, t, t_next):
    """engine.FEWSTEP_COEFFS[sampler] for the step from t to t_next (None: the last step, sigma_next = 0, a_next = 1), in float32
    on the host."""
    if sampler == "euler":
        sn = _sigma(alphas_cumprod, t_next)
        return float(sn - _sigma(alphas_cumprod, t)), float(np.sqrt(sn * sn + _F32(1.0))), float(sn)
    a, an = _alpha(alphas_cumprod, t), _alpha(alphas_cumprod, t_next)
    s = _F32(10 * t)   # timestep scaling 10, sigma_data 0.5: c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25)
    q = s * s + _F32(0.25)
    return (float(np.sqrt(_F32(1.0) - a)), float(np.sqrt(a)), float(s / np.sqrt(q)), float(_F32(0.25) / q), float(np.sqrt(an)),
            float(np.sqrt(_F32(1.0) - an)))


class FewStepLoop:
    """InpaintLoop's contract for the samplers "euler" and "lcm": step(i) is one UNet call and one launch (engine.fewstep_step); it
    does not wait for the device, allocate or draw noise, so it can be captured in a graph.  x is [2n, C, hl, wl] under
    classifier-free guidance (cfg) and [n, C, hl, wl] without; state: the Euler sampler's un-scaled sample; step_noise
    [steps - 1, n, 4, hl, wl]: the LCM sampler's fresh noise, drawn before the loop; C = 4: img_latent, noise0 and mask_l feed the
    blend that keeps the image outside the mask."""

    def __init__(self, runner, x, context, timesteps, guidance_scale, sampler, cfg, noise0=None, step_noise=None):
        self.runner, self.x, self.context, self.timesteps, self.guidance = runner, x, context, list(timesteps), float(guidance_scale)
        self.sampler, self.cfg, self.noise0, self.step_noise = sampler, bool(cfg), noise0, step_noise
        rows, self.channels, hl, wl = x.shape
        self.n = rows // 2 if self.cfg else rows
        shape = (self.n, 4, hl, wl)
        self.state = torch.empty(shape, dtype=x.dtype, device=x.device) if sampler == "euler" else None
        self.mask_l = torch.empty((self.n, 1, hl, wl), dtype=x.dtype, device=x.device) if self.channels == 4 else None
        self.decode_in = torch.empty(shape, dtype=x.dtype, device=x.device)
        self.img_latent = None
        self.t_model = torch.tensor(self.timesteps, dtype=torch.int64).to(x.device).to(x.dtype)
        ts = self.timesteps
        self.plan = [fewstep_coeffs(sampler, runner.alphas_cumprod, t, ts[i + 1] if i + 1 < len(ts) else None) for i, t in enumerate(ts)]

    def step(self, i):
        last = i == len(self.plan) - 1
        noise_pred = self.runner.unet(self.x, self.t_model[i].expand(self.x.shape[0]), context=self.context)
        if not noise_pred.is_contiguous():
            noise_pred = noise_pred.contiguous()
        engine.fewstep_step(noise_pred.detach(), self.x, self.sampler, self.guidance, self.plan[i], self.cfg, last=last, state=self.state,
                            step_noise=None if self.sampler != "lcm" or last else self.step_noise[i], img_latent=self.img_latent,
                            noise0=self.noise0, mask_l=self.mask_l, decode_in=self.decode_in if last else None)
        return self.x


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
    scheduler: only its alphas_cumprod, final_alpha_cumprod and config.num_train_timesteps are read; None: the reference's constants.
    sampler: "plms" (the reference's loop), or for few-step models "euler" / "lcm", which also take a 4-channel UNet and run
    without classifier-free guidance when guidance_scale <= 1."""

    def __init__(self, unet, vae, text_encoder, tokenizer, scheduler=None, sampler="plms"):
        if sampler not in SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r} ({', '.join(SAMPLERS)})")
        self.sampler = sampler
        in_ch = unet.in_channels if hasattr(unet, 'in_channels') else 4
        self.in_channels = in_ch
        if in_ch != 9 and not (in_ch == 4 and sampler != "plms"):
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
        if self.sampler != "plms":
            return self._prepare_fewstep(prompt, filled_u8, mask, generators, guidance_scale, strength, device, dtype)

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

    def _prepare_fewstep(self, prompt, filled_u8, mask, generators, guidance_scale, strength, device, dtype):
        """prepare() for the samplers "euler" and "lcm" -> the FewStepLoop.  The image work is the PLMS path's, into a 9-channel
        buffer `prep`: a 9-channel model's input is that buffer (its first half without guidance), a 4-channel model's input is a
        tensor of its own and the mask at the latents' size is copied out of prep once."""
        n, h, w, _ = filled_u8.shape
        channels, sampler = self.in_channels, self.sampler
        cfg = float(guidance_scale) > 1.0   # (the reference's diffusion_step_no_cfg rule: no guidance, no unconditional batch)
        timesteps = fewstep_timesteps(sampler, self.num_inference_steps, self.num_train_timesteps)
        timesteps = timesteps[max(0, int(len(timesteps) * (1.0 - strength))):]   # (:592-593)
        uncond, cond = self._embeddings(prompt, device)
        context = torch.cat([uncond.expand(n, -1, -1), cond.expand(n, -1, -1)]) if cfg else cond.expand(n, -1, -1)
        context = context.to(dtype).contiguous()

        hl, wl = max(h // VAE_FACTOR, 1), max(w // VAE_FACTOR, 1)
        prep = torch.empty((2 * n, 9, hl, wl), dtype=dtype, device=device)
        img, masked = engine.inpaint_image_prep(filled_u8, mask, prep, (hl, wl))
        mean_img = self.vae.encode(img)['latent_dist'].mean
        mean_masked = self.vae.encode(masked)['latent_dist'].mean if channels == 9 else mean_img   # (4 channels: 5..8 are not read)
        if tuple(mean_img.shape[2:]) != (hl, wl):   # a VAE of another factor: the mask again, at its size
            hl, wl = mean_img.shape[2], mean_img.shape[3]
            prep = torch.empty((2 * n, 9, hl, wl), dtype=dtype, device=device)
            engine.inpaint_image_prep(filled_u8, mask, prep, (hl, wl))
        rows = 2 * n if cfg else n
        x = prep[:rows] if channels == 9 else torch.empty((rows, 4, hl, wl), dtype=dtype, device=device)

        # drawn on the host in the model's dtype, frame by frame: the initial noise (:596-597), then the LCM sampler's fresh noise
        # of every step but the last, in step order
        extra = max(len(timesteps) - 1, 0) if sampler == "lcm" else 0
        drawn = [[torch.randn((1, 4, hl, wl), generator=g, device="cpu", dtype=dtype) for _ in range(1 + extra)] for g in generators]
        noise0 = torch.cat([d[0] for d in drawn]).to(device)
        step_noise = torch.stack([torch.cat([d[1 + i] for d in drawn]) for i in range(extra)]).to(device) if extra else None
        loop = FewStepLoop(self, x, context, timesteps, guidance_scale, sampler, cfg, noise0=noise0, step_noise=step_noise)
        mean_img, mean_masked = mean_img.detach().to(device).contiguous(), mean_masked.detach().to(device).contiguous()
        loop.img_latent = engine.inpaint_latent_init(mean_img, mean_masked, None, None, prep, decode_in=None if timesteps else loop.decode_in)
        if not timesteps:
            coeffs = None
        elif sampler == "euler":
            coeffs = euler_init_coeffs(self.alphas_cumprod, timesteps[0])
        else:
            coeffs = add_noise_coeffs(self.alphas_cumprod, timesteps[0], dtype)
        engine.fewstep_latent_init(loop.img_latent, noise0 if timesteps else None, coeffs, x, sampler, cfg, state=loop.state,
                                   prep=prep if channels == 4 else None, mask_l=loop.mask_l)
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


def make_inpaint(runner, prompt, num_inference_steps=30, guidance_scale=7.5, strength=1.0, seed=0, sampler=None):
    """-> inpaint(filled_u8, mask, frame_index): the callable stereodiffusion_nodes.generate_stereo_fast takes where the reference
    calls its inpainting pipeline, with a fresh CPU generator seeded seed + frame_index per frame (reference
    stereodiffusion_nodes.py:378-387) and the reference's prompt for an empty one (:368).  sampler, when given, is the one the
    runner must have been built for (ValueError otherwise): the node passes its switch to both."""
    prompt = prompt if prompt else DEFAULT_PROMPT
    if sampler is not None:
        if sampler not in SAMPLERS:
            raise ValueError(f"unknown sampler {sampler!r} ({', '.join(SAMPLERS)})")
        if sampler != getattr(runner, "sampler", "plms"):
            raise ValueError(f"the runner was built for sampler {getattr(runner, 'sampler', 'plms')!r}, not {sampler!r}")

    def inpaint(filled_u8, mask, frame_index):
        generator = torch.Generator(device="cpu")
        generator.manual_seed(seed + frame_index)
        return runner(prompt, filled_u8, mask, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                      strength=strength, generator=generator)

    return inpaint
