"""StereoDiffusion's two modes around their models (reference stereodiffusion_nodes.py).

Fast mode, around its inpainting model (StereoDiffusionNode._generate_stereo_fast and _generate_stereo_fast_single):

    generate_stereo_fast  the whole per-frame work of the mode at any frame size, batched, with the model as a callback (:378-573)
    pil_resize            PIL.Image.resize(size) with Pillow's defaults (8-bit bicubic), byte for byte (:422-423, :481-482, :569-570)
    prepare_inpaint       the backward warp, the inpaint mask and the gap pre-fill handed to the model (:425-542)
    compose_stereo        the model's pixels pasted back under the mask and the side-by-side pair (:563-571)

Standard mode, around its UNet, VAE and scheduler (_generate_stereo_impl and _text2stereoimage):

    generate_stereo_standard  the tensor work of the mode: codes, gray, the resizes to 512 x 512, the disparity, the loop, the
                              resizes back into the side-by-side float frame (:249-307), with the inversion as a callback
    generate_stereo_standard_frames  the same on every frame, groups of frames as one batch through the inversion, the loop and the
                              VAE (not in the reference, which stops after the first frame; the node takes it under STANDARD_ALL_FRAMES)
    text2stereoimage          the denoising loop with BNAttention installed, the latent shift at 20 % of the steps and its
                              re-application every 20 %, the VAE decode and the uint8 codes (:576-682)

The arithmetic of pil_resize and prepare_inpaint runs in the HIP kernels behind cs_pil_resize and cs_inpaint_prepare, the latent
shift, its mask and merge and the codes of the decoded images in those behind cs_latent_shift_plan, cs_latent_shift_apply and
cs_decode_to_codes (there is no CPU fallback: without a GPU they raise); compose_stereo is a `where` and a concatenation, plain
torch plumbing on whatever device its tensors are on.  The Standard loop makes the shift table once, applies it with one launch
per shift step and never indexes with a boolean mask, so it does not wait for the device and a step can be captured in a graph.

A coloured depth is made gray as trunc((r * 0.2989 + g * 0.5870) + b * 0.1140) in float64, in this order.  That equals the
reference on every depth with three equal channels; on a few hundred of the 2^24 colours the reference's BLAS product differs
from it, and from itself between array shapes.

Out of scope: loading the diffusion models -- generate_stereo_fast calls the `inpaint` it is given (inpaint_runner.make_inpaint
builds it around the caller's inpainting UNet, VAE, text encoder and tokenizer, where the reference runs ComfyUIInpaintRunner),
generate_stereo_standard the `invert` it is given (inversion.make_invert builds it, where the reference runs NullInversion.invert)
and the UNet, VAE, text encoder and scheduler of the `model` it is given.  StereoDiffusionNode, the ComfyUI node (:64-206), builds
all of these from MODEL, CLIP and VAE through model_wrappers.py; with its DDIMScheduler (schedulers.py) a step of the Standard loop
is one UNet call on one persistent input and one engine.standard_step launch.  The model loaders and the diffusers
StableDiffusionInpaintPipeline branch are not here: there is no download path.
"""
import torch
import torch.nn.functional as F

from . import engine, stereo_utils
from .diffusion_utils import diffusion_step, init_latent
from .schedulers import DDIMScheduler, check_work_size, prediction_of


def prepare_inpaint(image, depth, scale_factor, threshold=0.05):
    """image [B,3,H,W] or [3,H,W] float (values k / 255), depth [B,H,W] or [H,W]; every frame on its own (the reference's
    per-frame decisions) -> (warped, filled, mask): float32 like image, bool like depth.  Host tensors go to the device and the
    results come back to the host; device tensors stay where they are."""
    if not (isinstance(image, torch.Tensor) and isinstance(depth, torch.Tensor)):
        raise ValueError("image and depth must be torch tensors")
    single = image.dim() == 3
    if single != (depth.dim() == 2):
        raise ValueError(f"image {tuple(image.shape)} and depth {tuple(depth.shape)} do not match ([B,3,H,W] / [B,H,W] or "
                         "[3,H,W] / [H,W])")
    if single:
        image, depth = image[None], depth[None]
    host = not image.is_cuda
    if host or not depth.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
        dev = image.device if image.is_cuda else (depth.device if depth.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        image, depth = image.to(dev), depth.to(dev)
    out = engine.inpaint_prepare(image, depth, scale_factor, threshold)
    if host:
        out = tuple(t.cpu() for t in out)
    return tuple(t[0] for t in out) if single else out


def compose_stereo(left_u8, warped_u8, inpainted_u8, mask):
    """The pixel-space blend and the pair: right = where(mask, inpainted, warped) -> (stereo [..,H,2W,3], left, right), uint8.
    left_u8, warped_u8 (the codes of `warped`), inpainted_u8 (the model's image): uint8 [..,H,W,3]; mask: bool [..,H,W]."""
    for name, t in (("left_u8", left_u8), ("warped_u8", warped_u8), ("inpainted_u8", inpainted_u8)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() < 3 or t.shape[-1] != 3:
            raise ValueError(f"{name} must be a uint8 tensor [..,H,W,3]")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError("mask must be a bool tensor")
    if not (left_u8.shape == warped_u8.shape == inpainted_u8.shape) or tuple(mask.shape) != tuple(warped_u8.shape[:-1]):
        raise ValueError("left_u8, warped_u8 and inpainted_u8 must have one shape [..,H,W,3], mask that shape without the 3")
    right = torch.where(mask.unsqueeze(-1), inpainted_u8, warped_u8)
    return torch.cat([left_u8, right], dim=-2), left_u8, right


def _device_for(*tensors):
    for t in tensors:
        if t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def pil_resize(image_u8, size):
    """PIL.Image.resize(size) of Pillow 12.2 with all defaults (bicubic), byte for byte: image_u8 uint8 [..,H,W,3] (mode RGB;
    a last axis of 3 is taken as channels) or [..,H,W] (mode L), size = (width, height) -> uint8 [..,oh,ow,3] or [..,oh,ow].
    Host tensors go to the device and the result comes back to the host; device tensors stay where they are."""
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
        raise ValueError("image_u8 must be a uint8 torch tensor")
    rgb = image_u8.dim() >= 3 and image_u8.shape[-1] == 3
    if image_u8.dim() < (3 if rgb else 2):
        raise ValueError(f"image_u8 must be [..,H,W,3] or [..,H,W], got shape {tuple(image_u8.shape)}")
    if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
        raise ValueError(f"size must be (width, height), both positive; got {size!r}")
    if image_u8.numel() == 0:
        raise ValueError(f"empty image {tuple(image_u8.shape)}")
    x = image_u8 if rgb else image_u8.unsqueeze(-1)
    lead = tuple(x.shape[:-3])
    host = not x.is_cuda
    x = x.to(_device_for(x)).reshape((-1,) + tuple(x.shape[-3:]))
    out = engine.pil_resize(x, size)
    out = out.reshape(lead + tuple(out.shape[1:]))
    if not rgb:
        out = out[..., 0]
    return out.cpu() if host else out


WORK_SIZE = 512   # the side of the square frame the reference's model works on (:422-423, :429)


def generate_stereo_fast(image, depth_map, scale_factor, inpaint, threshold=0.05):
    """Everything StereoDiffusionNode._generate_stereo_fast does per frame except loading and running its model.
    image [N,H,W,3] float; depth_map [N,H,W,3], [N,H,W,1] or [N,H,W] float (three channels are made gray, one is taken as it is);
    inpaint(filled_u8 [512,512,3] uint8, mask [512,512] bool, frame_index) -> uint8 [512,512,3], on device tensors: it stands
    where the reference calls its model, once per frame in frame order, and not for a frame whose mask is empty (the early return,
    :478).  -> (stereo [N,H,2W,3], left [N,H,W,3], right [N,H,W,3]) float32, left and right being the two halves of stereo.
    Host tensors go to the device and the results come back to the host; device tensors stay where they are."""
    if not (isinstance(image, torch.Tensor) and isinstance(depth_map, torch.Tensor)):
        raise ValueError("image and depth_map must be torch tensors")
    if not callable(inpaint):
        raise ValueError("inpaint must be callable: inpaint(filled_u8, mask, frame_index) -> uint8 [512,512,3]")
    if image.dim() != 4 or image.shape[-1] != 3 or not image.is_floating_point():
        raise ValueError(f"image must be a float tensor [N,H,W,3], got {image.dtype} {tuple(image.shape)}")
    if depth_map.dim() == 3:
        depth_map = depth_map.unsqueeze(-1)
    if (depth_map.dim() != 4 or depth_map.shape[-1] not in (1, 3) or not depth_map.is_floating_point()
            or tuple(depth_map.shape[:3]) != tuple(image.shape[:3])):
        raise ValueError(f"depth_map must be a float tensor [N,H,W,3], [N,H,W,1] or [N,H,W] matching image {tuple(image.shape)}, "
                         f"got {depth_map.dtype} {tuple(depth_map.shape)}")
    if image.numel() == 0:
        raise ValueError(f"empty image {tuple(image.shape)}")
    host = not image.is_cuda
    dev = _device_for(image, depth_map)
    image, depth_map = image.to(dev, torch.float32), depth_map.to(dev, torch.float32)
    n, h, w, _ = image.shape
    s = (WORK_SIZE, WORK_SIZE)
    # the front, all frames at once: codes, gray, the two resizes, the warp / mask / pre-fill
    left_u8, img = engine.pil_resize(image, s, f32="planar")
    depth_u8 = engine.pil_resize(depth_map, s, gray=depth_map.shape[-1] == 3)
    _, _, mask, warped_u8, filled_u8 = engine.inpaint_prepare(img, depth_u8[..., 0].float(), scale_factor, threshold, codes=True)
    # the model, frame by frame
    called = mask.flatten(1).any(1).tolist()
    inpainted = warped_u8.clone()
    for k in range(n):
        if not called[k]:
            continue
        r = inpaint(filled_u8[k], mask[k], k)
        if not isinstance(r, torch.Tensor) or r.dtype != torch.uint8 or tuple(r.shape) != (WORK_SIZE, WORK_SIZE, 3):
            raise ValueError(f"inpaint must return a uint8 tensor [{WORK_SIZE},{WORK_SIZE},3] (frame {k})")
        inpainted[k] = r.to(dev)
    # the back, all frames at once: the blend, the two resizes, the float outputs
    _, _, right_u8 = compose_stereo(left_u8, warped_u8, inpainted, mask)
    stereo = torch.empty((n, h, 2 * w, 3), dtype=torch.float32, device=dev)
    engine.pil_resize(left_u8, (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
    engine.pil_resize(right_u8, (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])
    if host:
        stereo = stereo.cpu()
    return stereo, stereo[:, :, :w], stereo[:, :, w:]


# ---- Standard mode (reference :208-307, :576-682) ------------------------------------------------------------------------------
class _EmptyControl:
    """The controller the reference's loop passes to diffusion_step (inversion.py EmptyControl): it changes nothing."""

    def step_callback(self, x_t):
        return x_t


def _shift_steps(num_inference_steps):
    """(shift_step, reshift_interval): both 20 % of the steps, at least 1 (:626-628)."""
    k = max(1, int(num_inference_steps * 0.2))
    return k, k


def _disparity_to_latent(disparity, size):
    """The disparity [B,H,W] at the latents' size (:617-622)."""
    return F.interpolate(disparity.unsqueeze(1), size=list(size), mode="bicubic", align_corners=False).squeeze(1).contiguous()


class _StandardLoop:
    """What the loop of _text2stereoimage carries from step to step (:624-667): the shift table, made once; the mask the
    first shift stores; the noise of `deblur`.  step() is one iteration; it launches kernels and nothing else."""

    def __init__(self, model, disp_latent, scale_factor, deblur, num_inference_steps, guidance_scale, noise, per_frame=False):
        self.model, self.guidance_scale, self.controller = model, guidance_scale, _EmptyControl()
        self.shift_step, self.reshift_interval = _shift_steps(num_inference_steps)
        # the plan normalises with the range of the tensor it is given, as the reference's stereo_shift_torch does: frames that
        # are to come out as they would alone (per_frame) get a plan each
        self.src_col = (torch.cat([engine.latent_shift_plan(d[None], scale_factor) for d in disp_latent]) if per_frame
                        else engine.latent_shift_plan(disp_latent, scale_factor))
        self.mask = torch.zeros(tuple(disp_latent.shape), dtype=torch.uint8, device=disp_latent.device)
        self.noise = noise if deblur else None   # [1,C,h,w]: the right view's
        self.shifted = False
        # the fused path: our own DDIM scheduler, whose step the kernel restates; any other scheduler keeps diffusion_step
        self.fused = isinstance(model.scheduler, DDIMScheduler)
        self.prediction = prediction_of(model.scheduler) if self.fused else "epsilon"   # what the fused step is told
        self.x = None

    def _op(self, i):
        """The shift of iteration i (:650-667): "first" at the shift step, "reshift" every interval after it, else "none"."""
        if i == self.shift_step:
            return "first"
        if self.shifted and i > self.shift_step and i % self.reshift_interval == 0:
            return "reshift"
        return "none"

    def begin(self, latents, timesteps):
        """The fused path's state: x [4,C,h,w], the UNet's one persistent input -- the latents twice --, every step's coefficients,
        evaluated on the host, and the timesteps on the device, moved once: a step then copies nothing from the host.
        -> the view of x that holds the latents"""
        latents = latents.detach()
        self.x = torch.cat([latents, latents]).contiguous()
        self.coeffs = [self.model.scheduler.coeffs(t, latents.dtype) for t in timesteps]
        self.timesteps = torch.as_tensor(timesteps).to(latents.device)
        return self.x[:latents.shape[0]]

    def fused_step(self, i, context):
        """One UNet call on x and one launch: guidance, the DDIM step and the shift, written into both halves of x.  No cat, no
        allocation of ours and no wait for the device."""
        noise_pred = self.model.unet(self.x, self.timesteps[i], encoder_hidden_states=context)["sample"].detach()
        if noise_pred.dtype != self.x.dtype:
            raise ValueError(f"the UNet answers in {noise_pred.dtype}, the latents are {self.x.dtype}: the Standard loop needs a "
                             "model whose dtype is the latents' (hand it latents in the model's dtype)")
        if not noise_pred.is_contiguous():
            noise_pred = noise_pred.contiguous()
        op = self._op(i)
        engine.standard_step(noise_pred, self.x, self.guidance_scale, self.coeffs[i], op, self.src_col, self.mask,
                             self.noise if op == "first" else None, prediction=self.prediction)
        self.shifted = self.shifted or op == "first"

    def step(self, i, t, latents, context):
        latents = diffusion_step(self.model, self.controller, latents, context, t, self.guidance_scale, low_resource=False)
        op = self._op(i)
        if op != "none":
            latents = latents.contiguous()
            engine.latent_shift_apply(latents[:1], latents[1:], self.src_col, self.mask, op, noise=self.noise if op == "first" else None)
            self.shifted = self.shifted or op == "first"
        return latents


@torch.no_grad()
def _stereo_latents(model, prompt, uncond_embeddings, latent, disparity, scale_factor, direction, deblur, num_inference_steps,
                    guidance_scale, noise=None, generator=None, on_step=None):
    """The loop of text2stereoimage without the decode -> (latents [2,C,h,w], mask uint8 [1,h,w] or None when the loop never
    reached the shift step).  on_step(i, latents) sees the latents after every iteration."""
    if not (isinstance(prompt, (list, tuple)) and len(prompt) == 2 and all(isinstance(p, str) for p in prompt)):
        raise ValueError("prompt must be a list of two strings (the left and the right view)")
    work_size = check_work_size(STANDARD_WORK_SIZE)
    if direction not in ("uni", "bi"):
        raise ValueError(f"direction must be 'uni' or 'bi', got {direction!r}")
    if not isinstance(num_inference_steps, int) or isinstance(num_inference_steps, bool) or num_inference_steps < 1:
        raise ValueError(f"num_inference_steps must be a positive int, got {num_inference_steps!r}")
    if latent is not None and not (isinstance(latent, torch.Tensor) and latent.dim() == 4 and latent.is_floating_point()):
        raise ValueError("latent must be None or a float tensor [1 or 2,C,h,w]")
    if not (isinstance(disparity, torch.Tensor) and disparity.dim() == 3 and disparity.shape[0] == 1 and disparity.dtype == torch.float32):
        raise ValueError("disparity must be a float32 tensor [1,H,W]")
    if noise is not None and not (isinstance(noise, torch.Tensor) and noise.dim() == 4 and noise.shape[0] == 2):
        raise ValueError("noise must be None or a tensor [2,C,h,w] like the latents (the right view's half is used)")
    stereo_utils._need_gpu()
    steps = num_inference_steps
    editor = stereo_utils.BNAttention(start_step=max(1, int(steps * 0.2)), total_steps=steps, direction=direction)
    stereo_utils.register_attention_editor_diffusers(model, editor)
    try:
        batch_size = len(prompt)
        height = width = work_size
        tok = model.tokenizer
        text_input = tok(list(prompt), padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        text_embeddings = model.text_encoder(text_input.input_ids.to(model.device))[0]
        uncond_emb = None
        if uncond_embeddings is None:
            uncond_input = tok([""] * batch_size, padding="max_length", max_length=tok.model_max_length, return_tensors="pt")
            uncond_emb = model.text_encoder(uncond_input.input_ids.to(model.device))[0]
        _, latents = init_latent(latent, model, height, width, generator, batch_size)
        if not latents.is_cuda:
            raise ValueError(f"the model's device must be the GPU, got latents on {latents.device}")
        if latents.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"latents must be float32, float16 or bfloat16, got {latents.dtype}")
        model.scheduler.set_timesteps(steps)
        disp_latent = _disparity_to_latent(disparity.to(latents.device), latents.shape[-2:])
        if deblur:
            if noise is None:
                # a generator draws on its own device (the reference's is a CPU one); the result goes to the latents'
                where = generator.device if generator is not None else latents.device
                noise = torch.randn(tuple(latents.shape), generator=generator, device=where, dtype=latents.dtype)
            elif tuple(noise.shape) != tuple(latents.shape):
                raise ValueError(f"noise {tuple(noise.shape)} must have the latents' shape {tuple(latents.shape)}")
            noise = noise.to(latents.device, latents.dtype)[1:].contiguous()
        loop = _StandardLoop(model, disp_latent, scale_factor, deblur, steps, guidance_scale, noise)
        timesteps = model.scheduler.timesteps[-steps:]

        def context(i):
            uncond = uncond_emb if uncond_embeddings is None else uncond_embeddings[i].expand(*text_embeddings.shape)
            return torch.cat([uncond, text_embeddings])

        if loop.fused:
            # every step's context before the loop (one for all without null-text embeddings): a fused step allocates nothing
            contexts = [context(0)] * len(timesteps) if uncond_embeddings is None else [context(i) for i in range(len(timesteps))]
            latents = loop.begin(latents, timesteps)
        for i in range(len(timesteps)):
            if loop.fused:
                loop.fused_step(i, contexts[i])
            else:
                latents = loop.step(i, timesteps[i], latents, context(i))
            if on_step is not None:
                on_step(i, latents)
        return latents, (loop.mask if loop.shifted else None)
    finally:
        stereo_utils.restore_attention(model)   # (the reference leaves its hooks in place when the loop raises)


@torch.no_grad()
def text2stereoimage(model, prompt, uncond_embeddings, latent, disparity, scale_factor, direction, deblur, num_inference_steps,
                     guidance_scale, noise=None, generator=None):
    """StereoDiffusionNode._text2stereoimage (:576-682) on the device -> uint8 [2,512,512,3], the left and the right view.
    model: the reference's `ldm_stable`, duck-typed: tokenizer, text_encoder, unet, vae, scheduler, device.  prompt: two strings;
    uncond_embeddings: one embedding per step (null-text inversion's) or None (the empty prompt's); latent [2,C,64,64] (the
    inverted x_t twice) or None; disparity float32 [1,512,512].  BNAttention is installed from step max(1, int(steps * 0.2)) on
    and removed again whatever happens; at that step the right view becomes the shifted left view (deblur: with noise in the
    holes), and every so many steps again under the mask of the first shift.  noise: the tensor [2,C,64,64] the deblur fill
    draws from (its right-view half); None: torch.randn in the latents' dtype, from `generator` when given -- on the generator's
    device (a CPU generator, the reference's kind, also serves init_latent when latent is None; a device generator needs a
    latent), moved to the latents' --, on the latents' device otherwise.
    Runs under torch.no_grad() like the reference (:575), the VAE decode included: a caller that has gradients enabled for the
    inversion need not switch them off.  The loop does not wait for the device.
    The side of the square work frame is the module switch STANDARD_WORK_SIZE, a positive multiple of 8 (768 for the SD 2.x 768-v
    checkpoints), read when the function runs; every 512 above is then that size and every 64 an eighth of it.  A scheduler whose
    config.prediction_type is "v_prediction" makes every step the
    v-prediction step, still one launch."""
    latents, _ = _stereo_latents(model, prompt, uncond_embeddings, latent, disparity, scale_factor, direction, deblur,
                                 num_inference_steps, guidance_scale, noise, generator)
    image = model.vae.decode(1 / 0.18215 * latents)["sample"]
    return engine.decode_to_codes(image.contiguous())


def _norm_depth(depth):
    """The reference's _norm_depth (:39-47) without reading the range back: (depth - min) / (max - min), zeros when the range is
    within float32's eps."""
    mn, mx = depth.min(), depth.max()
    rng = mx - mn
    return torch.where(rng > torch.finfo(torch.float32).eps, 1 * (depth - mn) / rng, torch.zeros_like(depth))


def generate_stereo_standard(image, depth_map, scale_factor, direction, deblur, num_inference_steps, guidance_scale, model, invert,
                             noise=None, generator=None):
    """The tensor work of StereoDiffusionNode._generate_stereo_impl (:249-307) around its models.
    image [N,H,W,3] float; depth_map [N,H,W,3], [N,H,W,1] or [N,H,W] float (three channels are made gray): only the first frame
    is processed, as in the reference.  invert(image_u8 [512,512,3] uint8, on the device) -> (x_t [1,C,64,64], uncond_embeddings
    or None): it stands where the reference calls NullInversion.invert.  model, direction, deblur, noise, generator: as for
    text2stereoimage.  -> (stereo [1,H,2W,3], left [1,H,W,3], right [1,H,W,3]) float32, left and right being the two halves of
    stereo.  Host tensors go to the device and the results come back to the host; device tensors stay where they are.
    STANDARD_WORK_SIZE, read when the function runs, is the side of the work frame where the text above says 512 (64: an eighth)."""
    work_size = check_work_size(STANDARD_WORK_SIZE)
    if not (isinstance(image, torch.Tensor) and isinstance(depth_map, torch.Tensor)):
        raise ValueError("image and depth_map must be torch tensors")
    if not callable(invert):
        raise ValueError(f"invert must be callable: invert(image_u8 [{work_size},{work_size},3]) -> (x_t, uncond_embeddings)")
    if image.dim() != 4 or image.shape[-1] != 3 or not image.is_floating_point():
        raise ValueError(f"image must be a float tensor [N,H,W,3], got {image.dtype} {tuple(image.shape)}")
    if depth_map.dim() == 3:
        depth_map = depth_map.unsqueeze(-1)
    if (depth_map.dim() != 4 or depth_map.shape[-1] not in (1, 3) or not depth_map.is_floating_point()
            or tuple(depth_map.shape[:3]) != tuple(image.shape[:3])):
        raise ValueError(f"depth_map must be a float tensor [N,H,W,3], [N,H,W,1] or [N,H,W] matching image {tuple(image.shape)}, "
                         f"got {depth_map.dtype} {tuple(depth_map.shape)}")
    if image.numel() == 0:
        raise ValueError(f"empty image {tuple(image.shape)}")
    if direction not in ("uni", "bi"):
        raise ValueError(f"direction must be 'uni' or 'bi', got {direction!r}")
    if image.shape[0] > 1:
        print("Warning: Standard (DDIM) mode processes only the first frame. "
              "Use Fast (Warp + Inpaint) mode for batch/video processing.")
    host = not image.is_cuda
    dev = _device_for(image, depth_map)
    image, depth_map = image[:1].to(dev, torch.float32), depth_map[:1].to(dev, torch.float32)
    _, h, w, _ = image.shape
    s = (work_size, work_size)
    img_u8 = engine.pil_resize(image, s)
    depth_u8 = engine.pil_resize(depth_map, s, gray=depth_map.shape[-1] == 3)
    disp = _norm_depth(depth_u8[..., 0].float() / 255.0)
    x_t, uncond_embeddings = invert(img_u8[0])
    if not isinstance(x_t, torch.Tensor) or x_t.dim() != 4 or x_t.shape[0] != 1:
        raise ValueError("invert must return (x_t [1,C,h,w], uncond_embeddings)")
    codes = text2stereoimage(model, [""] * 2, uncond_embeddings, torch.cat([x_t, x_t], 0), disp, scale_factor, direction, deblur,
                             num_inference_steps, guidance_scale, noise, generator)
    stereo = torch.empty((1, h, 2 * w, 3), dtype=torch.float32, device=dev)
    engine.pil_resize(codes[:1], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
    engine.pil_resize(codes[1:], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])
    if host:
        stereo = stereo.cpu()
    return stereo, stereo[:, :, :w], stereo[:, :, w:]


# Standard mode on every frame of a batch (not in the reference, which processes the first frame only: on its hardware one
# null-text inversion takes minutes).  False: StereoDiffusionNode behaves as the reference's; True: Standard mode with more than one
# frame goes through generate_stereo_standard_frames.  A module switch, like stereo_utils.HALF_ATTENTION.
STANDARD_ALL_FRAMES = False

# The side of the square frame Standard mode works on.  512 is the reference's constant; the SD 2.x 768-v checkpoints are trained
# at 768.  A positive multiple of 8, checked and read whenever generate_stereo_standard, generate_stereo_standard_frames,
# text2stereoimage or the callables of inversion.make_invert / make_invert_frames run: their signatures, and the node's INPUT_TYPES,
# stay what they were.  Fast mode keeps WORK_SIZE.  A module switch like the one above.
STANDARD_WORK_SIZE = 512

# Fast mode's sampler: "plms", the reference's loop, or for the few-step models its tooltips name (SD-Turbo, the LCM checkpoints)
# "euler" / "lcm" (inpaint_runner.SAMPLERS), which also take a 4-channel model and drop the unconditional batch when guidance_scale
# <= 1.  Read when generate_stereo runs and passed to make_inpaint_runner and make_inpaint, which refuse an unknown value by name;
# the node's INPUT_TYPES and signature stay the reference's.  A module switch like the two above.
FAST_SAMPLER = "plms"


def _norm_depth_frames(depth):
    """_norm_depth on [F,H,W] with every frame's own range."""
    flat = depth.flatten(1)
    mn, mx = flat.min(1).values[:, None, None], flat.max(1).values[:, None, None]
    rng = mx - mn
    return torch.where(rng > torch.finfo(torch.float32).eps, 1 * (depth - mn) / rng, torch.zeros_like(depth))


@torch.no_grad()
def _stereo_latents_frames(model, uncond_embeddings, x_t, disparity, scale_factor, direction, deblur, num_inference_steps,
                           guidance_scale, noise):
    """_stereo_latents on F frames down the fused path (the model's scheduler is our DDIMScheduler): x_t [F,C,h,w], disparity
    float32 [F,512,512], uncond_embeddings a list of [F,77,D] or None, noise [F,C,h,w] (the right views') or None ->
    latents [2F,C,h,w], the left views, then the right views.  The UNet's persistent input is [4F,C,h,w] as standard_step lays it
    out; BNAttention sees chunks = 2 and samples = F."""
    frames, steps = x_t.shape[0], num_inference_steps
    stereo_utils._need_gpu()
    editor = stereo_utils.BNAttention(start_step=max(1, int(steps * 0.2)), total_steps=steps, direction=direction)
    stereo_utils.register_attention_editor_diffusers(model, editor)
    try:
        tok = model.tokenizer
        text_input = tok([""] * (2 * frames), padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        text_embeddings = model.text_encoder(text_input.input_ids.to(model.device))[0]
        if tuple(text_embeddings.shape[:1]) != (2 * frames,):
            raise ValueError(f"the text encoder answered {tuple(text_embeddings.shape)} to {2 * frames} prompts")
        latents = torch.cat([x_t, x_t]).to(model.device)
        if not latents.is_cuda:
            raise ValueError(f"the model's device must be the GPU, got latents on {latents.device}")
        if latents.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"latents must be float32, float16 or bfloat16, got {latents.dtype}")
        model.scheduler.set_timesteps(steps)
        disp_latent = _disparity_to_latent(disparity.to(latents.device), latents.shape[-2:])
        if deblur:
            noise = noise.to(latents.device, latents.dtype).contiguous()
        loop = _StandardLoop(model, disp_latent, scale_factor, deblur, steps, guidance_scale, noise, per_frame=True)
        timesteps = model.scheduler.timesteps[-steps:]
        if uncond_embeddings is None:
            uncond_input = tok([""] * (2 * frames), padding="max_length", max_length=tok.model_max_length, return_tensors="pt")
            uncond_emb = model.text_encoder(uncond_input.input_ids.to(model.device))[0]
            contexts = [torch.cat([uncond_emb, text_embeddings])] * len(timesteps)
        else:
            # frame f's own null-text embedding for both of its views: rows f and F + f of either half
            contexts = [torch.cat([uncond_embeddings[i], uncond_embeddings[i], text_embeddings]) for i in range(len(timesteps))]
        latents = loop.begin(latents, timesteps)
        for i in range(len(timesteps)):
            loop.fused_step(i, contexts[i])
        return latents
    finally:
        stereo_utils.restore_attention(model)


def generate_stereo_standard_frames(image, depth_map, scale_factor, direction, deblur, num_inference_steps, guidance_scale, model,
                                    invert_frames, frames_per_batch=4, noise=None, generator=None):
    """generate_stereo_standard on every frame: groups of up to `frames_per_batch` frames go through the inversion, the loop and
    the VAE as one batch.  invert_frames(images_u8 [F,512,512,3] uint8, on the device) -> (x_t [F,C,64,64], uncond_embeddings:
    a list of [F,77,D] per step, or None): inversion.make_invert_frames builds it.  noise: the deblur fill of the right views,
    [N,C,64,64]; None: drawn per frame as text2stereoimage draws it ([2,C,64,64] from `generator`, the right view's half), in frame
    order, so that a batch equals N successive single-frame calls on that generator.  Every frame has its own depth range.
    A model whose scheduler is not our DDIMScheduler runs frame by frame through generate_stereo_standard.
    STANDARD_WORK_SIZE, read when the function runs, is the side of the work frame where the text above says 512 (64: an eighth).
    -> (stereo [N,H,2W,3], left [N,H,W,3], right [N,H,W,3]) float32, left and right being the two halves of stereo."""
    work_size = check_work_size(STANDARD_WORK_SIZE)
    if not (isinstance(image, torch.Tensor) and isinstance(depth_map, torch.Tensor)):
        raise ValueError("image and depth_map must be torch tensors")
    if not callable(invert_frames):
        raise ValueError(f"invert_frames must be callable: invert_frames(images_u8 [F,{work_size},{work_size},3]) -> (x_t, uncond_embeddings)")
    if image.dim() != 4 or image.shape[-1] != 3 or not image.is_floating_point():
        raise ValueError(f"image must be a float tensor [N,H,W,3], got {image.dtype} {tuple(image.shape)}")
    if depth_map.dim() == 3:
        depth_map = depth_map.unsqueeze(-1)
    if (depth_map.dim() != 4 or depth_map.shape[-1] not in (1, 3) or not depth_map.is_floating_point()
            or tuple(depth_map.shape[:3]) != tuple(image.shape[:3])):
        raise ValueError(f"depth_map must be a float tensor [N,H,W,3], [N,H,W,1] or [N,H,W] matching image {tuple(image.shape)}, "
                         f"got {depth_map.dtype} {tuple(depth_map.shape)}")
    if image.numel() == 0:
        raise ValueError(f"empty image {tuple(image.shape)}")
    if direction not in ("uni", "bi"):
        raise ValueError(f"direction must be 'uni' or 'bi', got {direction!r}")
    if not isinstance(num_inference_steps, int) or isinstance(num_inference_steps, bool) or num_inference_steps < 1:
        raise ValueError(f"num_inference_steps must be a positive int, got {num_inference_steps!r}")
    if isinstance(frames_per_batch, bool) or not isinstance(frames_per_batch, int) or frames_per_batch < 1:
        raise ValueError(f"frames_per_batch must be a positive int, got {frames_per_batch!r}")
    n, h, w, _ = image.shape
    if noise is not None and not (isinstance(noise, torch.Tensor) and noise.dim() == 4 and noise.shape[0] == n):
        raise ValueError(f"noise must be None or a tensor [N,C,h,w] like the inverted latents, one right view per frame (N = {n})")
    host = not image.is_cuda
    dev = _device_for(image, depth_map)
    stereo = torch.empty((n, h, 2 * w, 3), dtype=torch.float32, device=dev)
    if not isinstance(model.scheduler, DDIMScheduler):
        for k in range(n):
            one = generate_stereo_standard(image[k:k + 1], depth_map[k:k + 1], scale_factor, direction, deblur, num_inference_steps,
                                           guidance_scale, model, lambda image_u8: invert_frames(image_u8[None]),
                                           None if noise is None else torch.cat([noise[k:k + 1]] * 2), generator)
            stereo[k:k + 1] = one[0].to(dev)
    else:
        image, depth_map = image.to(dev, torch.float32), depth_map.to(dev, torch.float32)
        s = (work_size, work_size)
        for k in range(0, n, frames_per_batch):
            group = slice(k, min(k + frames_per_batch, n))
            frames = group.stop - group.start
            img_u8 = engine.pil_resize(image[group], s)
            depth_u8 = engine.pil_resize(depth_map[group], s, gray=depth_map.shape[-1] == 3)
            disp = _norm_depth_frames(depth_u8[..., 0].float() / 255.0)
            x_t, uncond_embeddings = invert_frames(img_u8)
            if not isinstance(x_t, torch.Tensor) or x_t.dim() != 4 or x_t.shape[0] != frames:
                raise ValueError(f"invert_frames must return (x_t [F,C,h,w], uncond_embeddings) for its F = {frames} frames")
            fill = None
            if deblur and noise is not None:
                if tuple(noise.shape[1:]) != tuple(x_t.shape[1:]):
                    raise ValueError(f"noise {tuple(noise.shape)} must be [N,C,h,w] with the latents' {tuple(x_t.shape[1:])}")
                fill = noise[group]
            elif deblur:
                # a generator draws on its own device (the reference's is a CPU one); the result goes to the latents'
                where = generator.device if generator is not None else x_t.device
                fill = torch.cat([torch.randn((2,) + tuple(x_t.shape[1:]), generator=generator, device=where, dtype=x_t.dtype)[1:]
                                  for _ in range(frames)])
            latents = _stereo_latents_frames(model, uncond_embeddings, x_t, disp, scale_factor, direction, deblur, num_inference_steps,
                                             guidance_scale, fill)
            with torch.no_grad():
                codes = engine.decode_to_codes(model.vae.decode(1 / 0.18215 * latents)["sample"].contiguous())
            engine.pil_resize(codes[:frames], (w, h), f32="nhwc", codes=False, f32_out=stereo[group, :, :w])
            engine.pil_resize(codes[frames:], (w, h), f32="nhwc", codes=False, f32_out=stereo[group, :, w:])
    if host:
        stereo = stereo.cpu()
    return stereo, stereo[:, :, :w], stereo[:, :, w:]


# ---- the ComfyUI node (reference :64-206, :685-692) -------------------------------------------------------------------------------
FAST_MODE, STANDARD_MODE = "Fast (Warp + Inpaint)", "Standard (DDIM)"


class StereoDiffusionNode:
    """StereoDiffusion as a ComfyUI node: an image and its depth map -> the side-by-side pair, the left and the right image.
    Connect MODEL, CLIP and VAE: an inpainting checkpoint (9-channel UNet) for Fast mode, any SD1 / SD2 checkpoint for Standard
    mode.  There is no download path: without the three inputs the node raises."""

    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "image": ("IMAGE",),
                "depth_map": ("IMAGE",),
                "scale_factor": ("FLOAT", {"default": 5.0, "min": 1.0, "max": 20.0, "step": 0.5,
                                           "tooltip": "Controls the strength of the stereo effect (disparity)"}),
                "direction": (["uni", "bi"], {"default": "uni",
                                              "tooltip": "uni: unidirectional attention, bi: bidirectional attention"}),
                "deblur": ("BOOLEAN", {"default": False, "tooltip": "Add noise to unfilled regions to avoid blurring"}),
                "pipeline_mode": ([STANDARD_MODE, FAST_MODE], {
                    "default": FAST_MODE,
                    "tooltip": "Standard: DDIM inversion (high quality, slow). Fast: Warp image with depth, then AI-inpaint only the "
                               "gap regions (fast, works with turbo/LCM models)"}),
                "guidance_scale": ("FLOAT", {"default": 3.0, "min": 0.0, "max": 20.0, "step": 0.5,
                                             "tooltip": "CFG scale. Standard mode: 3-10. Turbo models: 0.0. LCM: 1.0-2.0"}),
                "num_inference_steps": ("INT", {
                    "default": 20, "min": 1, "max": 100, "step": 1,
                    "tooltip": "Number of inference steps. Standard DDIM: 30-100 (default 50). Fast inpainting: 20-30. Turbo/LCM: 1-8"}),
                "seed": ("INT", {"default": 1337, "min": 0, "max": 0xffffffffffffffff, "control_after_generate": True,
                                 "tooltip": "Random seed for reproducible results"}),
            },
            "optional": {
                "null_text_optimization": ("BOOLEAN", {
                    "default": True, "tooltip": "Enable null-text optimization for better reconstruction (Standard mode only)"}),
                "denoise_strength": ("FLOAT", {
                    "default": 0.6, "min": 0.1, "max": 1.0, "step": 0.05,
                    "tooltip": "How much noise to add before denoising (Fast mode). Lower = preserve original more, Higher = more "
                               "model creativity for filling gaps"}),
                "model": ("MODEL", {"tooltip": "ComfyUI MODEL input. Fast mode: use inpainting model (9ch UNet). Standard mode: use "
                                               "any SD1/SD2 model."}),
                "clip": ("CLIP", {"tooltip": "CLIP from Load Checkpoint"}),
                "vae": ("VAE", {"tooltip": "VAE from Load Checkpoint"}),
                "model_id": ("STRING", {"default": "runwayml/stable-diffusion-v1-5",
                                        "tooltip": "Fallback HuggingFace model ID (Standard mode, when no ComfyUI model connected)"}),
                "inpaint_model_id": ("STRING", {"default": "runwayml/stable-diffusion-inpainting",
                                                "tooltip": "Fallback inpainting model ID (Fast mode, when no ComfyUI model connected)"}),
                "prompt": ("STRING", {"default": "", "multiline": True,
                                      "tooltip": "Optional text prompt to guide inpainting (Fast mode). Describe the image content for "
                                                 "better gap filling."}),
            },
        }

    RETURN_TYPES = ("IMAGE", "IMAGE", "IMAGE")
    RETURN_NAMES = ("stereo_pair", "left_image", "right_image")
    FUNCTION = "generate_stereo"
    CATEGORY = "image/stereo"

    def generate_stereo(self, image, depth_map, scale_factor, direction, deblur, pipeline_mode=STANDARD_MODE, guidance_scale=7.5,
                        num_inference_steps=50, seed=0, null_text_optimization=True, denoise_strength=0.5, model=None, clip=None,
                        vae=None, model_id="", inpaint_model_id="runwayml/stable-diffusion-inpainting", prompt=""):
        from . import inpaint_runner, inversion, model_wrappers
        generator = torch.Generator(device="cpu")
        generator.manual_seed(seed)
        if model is None or clip is None or vae is None:
            # (the reference downloads model_id / inpaint_model_id with diffusers here; this package has no network path)
            raise ValueError("StereoDiffusion: connect MODEL, CLIP and VAE (Load Checkpoint); this node does not download "
                             f"'{inpaint_model_id if pipeline_mode == FAST_MODE else model_id}'")
        # outside inference mode for the whole call: null-text optimisation differentiates through the UNet (:193-194)
        with torch.inference_mode(False):
            if pipeline_mode == FAST_MODE:
                # a model that is no inpainting model raises the 9-channel message (the reference falls back to a download)
                runner = model_wrappers.make_inpaint_runner(model, clip, vae, sampler=FAST_SAMPLER)
                inpaint = inpaint_runner.make_inpaint(runner, prompt, int(num_inference_steps), guidance_scale, denoise_strength, seed,
                                                      sampler=FAST_SAMPLER)
                return generate_stereo_fast(image, depth_map, scale_factor, inpaint)
            ldm_stable = model_wrappers.ComfyUIModelWrapper(model, clip, vae)
            if not ldm_stable.is_supported():
                raise ValueError(ldm_stable.get_unsupported_message())
            if STANDARD_ALL_FRAMES and image.shape[0] > 1:
                invert_frames = inversion.make_invert_frames(ldm_stable, int(num_inference_steps), guidance_scale, null_text_optimization)
                return generate_stereo_standard_frames(image, depth_map, scale_factor, direction, deblur, int(num_inference_steps),
                                                       guidance_scale, ldm_stable, invert_frames, generator=generator)
            invert = inversion.make_invert(ldm_stable, int(num_inference_steps), guidance_scale, null_text_optimization)
            return generate_stereo_standard(image, depth_map, scale_factor, direction, deblur, int(num_inference_steps), guidance_scale,
                                            ldm_stable, invert, generator=generator)


NODE_CLASS_MAPPINGS = {
    "StereoDiffusion": StereoDiffusionNode,
}

NODE_DISPLAY_NAME_MAPPINGS = {
    "StereoDiffusion": "StereoDiffusion",
}
