"""Drop-in for the reference's inversion.py: DDIM inversion with null-text optimisation.

`NullInversion` and `EmptyControl` with the reference's names, argument order, defaults and return values (reference
inversion.py:29-255).  The UNet, VAE, text encoder and scheduler are the caller's (`model`, the reference's `ldm_stable`,
duck-typed); everything between two UNet calls runs in one HIP launch each:

  ddim_loop           next_step (:67-75)                                        engine.ddim_step
  null_optimization   guidance + prev_step + mse_loss + its gradient (:198-201)  engine.NullTextLoss (cs_null_loss_grad)
                      Adam (:192, :202-204)                                      engine.adam_step
                      the guided step to the next latent (:209-211)              engine.ddim_step
  latent2image        (image / 2 + 0.5).clamp(0, 1) * 255 -> uint8 (:100-102)    engine.decode_to_codes
  invert              register_attention_control(model, None) (:216)             diffusion_utils' fused attention hook

`NullInversion.invert_frames` is not in the reference: F frames in one UNet batch (video in Standard mode), every frame with its
own loss, early stop and Adam state (engine.null_loss_grad_frames, engine.adam_step_frames), bit for bit what invert gives it alone.

The step's coefficients sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_other), sqrt(a_other) are the reference's own expressions on
scheduler.alphas_cumprod, evaluated once per timestep on the host and cached.  The inner loop reads the loss once per inner step,
for the early stop; nothing else waits for the device.

float16 / bfloat16: CPU torch -- the run the fixtures record -- converts a 0-dim float32 tensor that is the FIRST operand of a
product with a half tensor to the half dtype before it multiplies, and keeps the divisor's float32: c1, c3 and c4 are rounded to
the tensors' dtype when the scheduler's alphas are tensors, c2 is not (`_operand`).  float32 needs none of this.

A v-prediction model (scheduler.config.prediction_type == "v_prediction", the SD 2.x 768-v checkpoints): the same launches with
prediction="v_prediction" -- x0 = c2 * x - c1 * v; e = c2 * v + c1 * x; out = c4 * x0 + c3 * e --, c2 then rounded like the other
three (schedulers.step_coeffs).  A scheduler that does not say predicts epsilon.  NullInversion.work_size: the side of the square
work frame, 512 unless the caller sets it (768 for those checkpoints); the methods keep the reference's signatures.

No CPU fallback: without a GPU the first kernel raises RuntimeError, as the attention hook does.
"""
import math

import numpy as np
import torch

from . import diffusion_utils, engine
from .schedulers import _operand, _sqrt, check_work_size, prediction_of, step_coeffs   # noqa: F401  (inpaint_runner imports the first two from here)

try:
    from torch.func import functional_call
except ImportError:   # the reference's condition for its ComfyUI gradient mode (:20-26)
    functional_call = None


class EmptyControl:
    """Placeholder controller that passes attention through unchanged (reference :29-39)."""

    def step_callback(self, x_t):
        return x_t

    def between_steps(self):
        return

    def __call__(self, attn, is_cross: bool, place_in_unet: str):
        return attn


class NullInversion:
    """DDIM inversion with null-text optimisation for image-to-latent conversion (reference :42-255)."""

    # The side of the square frame invert and invert_frames work on: the reference's 512; 768 for the SD 2.x 768-v checkpoints.  An
    # attribute, not an argument: the methods keep the reference's signatures.  A positive multiple of 8, checked where it is used;
    # make_invert and make_invert_frames set it from stereodiffusion_nodes.STANDARD_WORK_SIZE.
    work_size = 512

    def __init__(self, model, num_ddim_steps: int = 50, guidance_scale: float = 7.5):
        self.model = model
        self.num_ddim_steps = num_ddim_steps
        self.guidance_scale = guidance_scale
        self.model.scheduler.set_timesteps(num_ddim_steps)
        self.prompt = None
        self.context = None
        self._is_comfyui = hasattr(model, 'comfy_model')
        self._coeffs = {}
        self.inner_steps_taken = []   # per outer step of the last null_optimization
        self.losses = []              # per outer step, the loss of every inner step taken

    # ---- the two steps: one formula, two choices of alphas ----
    def _step_coeffs(self, kind, timestep, dtype):
        sch = self.scheduler
        # the scheduler is the model's and shared: another set_timesteps, or another schedule, must not meet this one's values
        prediction = prediction_of(sch)
        key = (kind, int(timestep), dtype, sch.num_inference_steps, id(sch.alphas_cumprod), prediction)
        if key not in self._coeffs:
            ratio = sch.config.num_train_timesteps // sch.num_inference_steps
            if kind == "prev":   # (:58-63)
                prev_timestep = timestep - ratio
                alpha_prod_t = sch.alphas_cumprod[timestep]
                alpha_other = sch.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else sch.final_alpha_cumprod
            else:                # (:68-73)
                timestep, next_timestep = min(timestep - ratio, 999), timestep
                alpha_prod_t = sch.alphas_cumprod[timestep] if timestep >= 0 else sch.final_alpha_cumprod
                alpha_other = sch.alphas_cumprod[next_timestep]
            self._coeffs[key] = step_coeffs(alpha_prod_t, alpha_other, dtype, prediction)
        return self._coeffs[key]

    def _step(self, kind, eps_a, eps_b, guidance, timestep, sample):
        sample = sample.detach().contiguous()
        eps_a = eps_a.detach().contiguous()
        eps_b = None if eps_b is None else eps_b.detach().contiguous()
        return engine.ddim_step_pred(sample, eps_a, eps_b, guidance, self._step_coeffs(kind, timestep, sample.dtype),
                                     prediction=prediction_of(self.scheduler))

    # prev_step / next_step: the values of the reference's; not differentiable (the inputs are detached): inside the optimisation
    # the gradient goes through engine.NullTextLoss instead
    def prev_step(self, model_output, timestep: int, sample):
        return self._step("prev", model_output, None, 1.0, timestep, sample)

    def next_step(self, model_output, timestep: int, sample):
        return self._step("next", model_output, None, 1.0, timestep, sample)

    def get_noise_pred_single(self, latents, t, context):
        noise_pred = self.model.unet(latents, t, encoder_hidden_states=context)["sample"]
        return noise_pred

    def get_noise_pred(self, latents, t, is_forward=True, context=None):
        latents_input = torch.cat([latents] * 2)
        if context is None:
            context = self.context
        guidance_scale = 1 if is_forward else self.guidance_scale
        noise_pred = self.model.unet(latents_input, t, encoder_hidden_states=context)["sample"]
        noise_pred_uncond, noise_prediction_text = noise_pred.chunk(2)
        # guidance (:88) and the step (:89-92) in one launch
        return self._step("next" if is_forward else "prev", noise_pred_uncond, noise_prediction_text, guidance_scale, t, latents)

    @torch.no_grad()
    def latent2image(self, latents, return_type='np'):
        latents = 1 / 0.18215 * latents.detach()
        image = self.model.vae.decode(latents)['sample']
        if return_type == 'np':
            image = engine.decode_to_codes(image.contiguous())[0].cpu().numpy()
        return image

    def _get_device(self):
        device = self.model.device
        if isinstance(device, str):
            device = torch.device(device)
        return device

    @torch.no_grad()
    def image2latent(self, image):
        device = self._get_device()
        model_dtype = next(self.model.vae.parameters()).dtype
        if hasattr(image, "convert") and hasattr(image, "size") and not isinstance(image, (np.ndarray, torch.Tensor)):
            image = np.array(image)   # a PIL image
        if isinstance(image, torch.Tensor) and image.dim() == 4:
            latents = image.to(device=device, dtype=model_dtype)
        else:
            if isinstance(image, np.ndarray):
                image = torch.from_numpy(image)
            # on the host, as the reference: a device divides by a Python scalar through the reciprocal, which is not `/ 127.5`
            image = image.cpu().float() / 127.5 - 1
            image = image.permute(2, 0, 1).unsqueeze(0).to(device)
            image = image.to(dtype=model_dtype)
            latents = self.model.vae.encode(image)['latent_dist'].mean
            latents = latents * 0.18215
            latents = latents.to(device)
        return latents

    @torch.no_grad()
    def init_prompt(self, prompt: str):
        device = self._get_device()
        tok = self.model.tokenizer
        uncond_input = tok([""], padding="max_length", max_length=tok.model_max_length, return_tensors="pt")
        uncond_embeddings = self.model.text_encoder(uncond_input.input_ids.to(device))[0].to(device)
        text_input = tok([prompt], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt")
        text_embeddings = self.model.text_encoder(text_input.input_ids.to(device))[0].to(device)
        self.context = torch.cat([uncond_embeddings, text_embeddings])
        self.prompt = prompt

    @torch.no_grad()
    def ddim_loop(self, latent):
        uncond_embeddings, cond_embeddings = self.context.chunk(2)
        all_latent = [latent]
        latent = latent.clone().detach()
        for i in range(self.num_ddim_steps):
            t = self.model.scheduler.timesteps[len(self.model.scheduler.timesteps) - i - 1]
            noise_pred = self.get_noise_pred_single(latent, t, cond_embeddings)
            latent = self.next_step(noise_pred, t, latent)
            all_latent.append(latent)
        return all_latent

    @property
    def scheduler(self):
        return self.model.scheduler

    @torch.no_grad()
    def ddim_inversion(self, image):
        latent = self.image2latent(image)
        image_rec = self.latent2image(latent)
        ddim_latents = self.ddim_loop(latent)
        return image_rec, ddim_latents

    def null_optimization(self, latents, num_inner_steps, epsilon):
        uncond_embeddings, cond_embeddings = self.context.chunk(2)
        uncond_embeddings_list = []
        latent_cur = latents[-1]
        self.inner_steps_taken, self.losses = [], []
        for i in range(self.num_ddim_steps):
            uncond_embeddings = uncond_embeddings.clone().detach().contiguous()
            uncond_embeddings.requires_grad = True
            # a fresh Adam per outer step (:192): zero moments, step numbers from 1
            lr = 1e-2 * (1. - i / 100.)
            exp_avg, exp_avg_sq = torch.zeros_like(uncond_embeddings), torch.zeros_like(uncond_embeddings)
            latent_prev = latents[len(latents) - i - 2].detach().contiguous()
            latent_cur = latent_cur.detach().contiguous()
            t = self.model.scheduler.timesteps[i]
            coeffs = self._step_coeffs("prev", t, latent_cur.dtype)
            prediction = prediction_of(self.scheduler)
            with torch.no_grad():
                noise_pred_cond = self.get_noise_pred_single(latent_cur, t, cond_embeddings).contiguous()
            losses = []
            for j in range(num_inner_steps):
                noise_pred_uncond = self.get_noise_pred_single(latent_cur, t, uncond_embeddings).contiguous()
                loss = engine.NullTextLoss.apply(noise_pred_uncond, noise_pred_cond, latent_cur, latent_prev, self.guidance_scale, coeffs,
                                                 prediction)
                (grad,) = torch.autograd.grad(loss, [uncond_embeddings])
                engine.adam_step(uncond_embeddings, grad.contiguous(), exp_avg, exp_avg_sq, lr, j + 1)
                loss_item = loss.item()   # the one wait per inner step: the early stop needs it
                losses.append(loss_item)
                if loss_item < epsilon + i * 2e-5:
                    break
            self.inner_steps_taken.append(len(losses))
            self.losses.append(losses)
            uncond_embeddings_list.append(uncond_embeddings[:1].detach())
            with torch.no_grad():
                context = torch.cat([uncond_embeddings, cond_embeddings])
                latent_cur = self.get_noise_pred(latent_cur, t, False, context)
        return uncond_embeddings_list

    def invert(self, image, prompt: str, num_inner_steps=10, early_stop_epsilon=1e-5, null_text_optimization=True):
        work_size = check_work_size(self.work_size)
        self.init_prompt(prompt)
        diffusion_utils.register_attention_control(self.model, None)

        # an array comes back as an array (the reference's return tuple); the work on it is the device's
        as_array = isinstance(image, np.ndarray)
        if as_array:
            given = image
            image = torch.from_numpy(image)
        if isinstance(image, torch.Tensor) and image.dim() == 3:
            if image.shape[0] != work_size or image.shape[1] != work_size:
                image = engine.pil_resize(image.to(self._get_device())[None], (work_size, work_size))[0]
            if image.max() <= 1:
                image = (image * 255).to(torch.uint8)
        if as_array:
            given = given if image.data_ptr() == torch.from_numpy(given).data_ptr() else image.cpu().numpy()

        image_rec, ddim_latents = self.ddim_inversion(image)

        if null_text_optimization:
            if self._is_comfyui:
                if functional_call is not None:
                    self.model.unet.enable_gradient_mode()
                    try:
                        uncond_embeddings = self.null_optimization(ddim_latents, num_inner_steps, early_stop_epsilon)
                    finally:
                        self.model.unet.disable_gradient_mode()
                else:
                    uncond_embeddings, _ = self.context.chunk(2)
                    uncond_embeddings = [uncond_embeddings.clone().detach() for _ in range(self.num_ddim_steps)]
            else:
                uncond_embeddings = self.null_optimization(ddim_latents, num_inner_steps, early_stop_epsilon)
        else:
            uncond_embeddings, _ = self.context.chunk(2)
            uncond_embeddings = [uncond_embeddings.clone().detach() for _ in range(self.num_ddim_steps)]

        return (given if as_array else image, image_rec), ddim_latents[-1], uncond_embeddings

    # ---- F frames in one UNet batch: every frame its own loss, its own early stop and its own Adam state ----
    @torch.no_grad()
    def _images2latent(self, images):
        """image2latent on uint8 [F,512,512,3]: the same host arithmetic, one VAE call."""
        device = self._get_device()
        model_dtype = next(self.model.vae.parameters()).dtype
        images = images.cpu().float() / 127.5 - 1
        images = images.permute(0, 3, 1, 2).to(device).to(dtype=model_dtype)
        latents = self.model.vae.encode(images)['latent_dist'].mean
        return (latents * 0.18215).to(device)

    def _frame_contexts(self, frames):
        """(uncond [F,77,D], cond [F,77,D]): the prompt's two embeddings, one row per frame."""
        uncond_embeddings, cond_embeddings = self.context.chunk(2)
        return tuple(e.expand(frames, *e.shape[1:]).contiguous() for e in (uncond_embeddings, cond_embeddings))

    @torch.no_grad()
    def ddim_loop_frames(self, latent):
        """ddim_loop on [F,C,h,w]: engine.ddim_step is elementwise, the UNet runs at batch F."""
        _, cond_embeddings = self._frame_contexts(latent.shape[0])
        all_latent = [latent]
        latent = latent.clone().detach()
        for i in range(self.num_ddim_steps):
            t = self.model.scheduler.timesteps[len(self.model.scheduler.timesteps) - i - 1]
            noise_pred = self.get_noise_pred_single(latent, t, cond_embeddings)
            latent = self.next_step(noise_pred, t, latent)
            all_latent.append(latent)
        return all_latent

    def null_optimization_frames(self, latents, num_inner_steps, epsilon):
        """null_optimization on latents [F,C,h,w]: per outer step one conditional UNet call at batch F; per inner step one
        unconditional UNet call at batch F, one cs_null_loss_grad_frames launch, the UNet's backward from its gradient, one
        cs_adam_step_frames launch and one read of the flags and losses -- the inner step's single wait.  A frame whose loss
        falls below the threshold stops there, as it would alone: its flag is cleared on the device, its later gradients are
        zeros and Adam no longer writes it.  -> [F,77,D] per outer step; inner_steps_taken[i][f], losses[i][f][j]."""
        frames = latents[-1].shape[0]
        uncond_embeddings, cond_embeddings = self._frame_contexts(frames)
        uncond_embeddings_list = []
        latent_cur = latents[-1]
        self.inner_steps_taken, self.losses = [], []
        device = latent_cur.device
        # everything the inner loop writes, allocated once.  state: F float32 losses, then the two flag buffers, which swap roles
        # every inner step -- one tensor, so that one copy brings the losses and the flags to the host
        state = torch.zeros((6 * frames,), dtype=torch.uint8, device=device)
        loss = state[:4 * frames].view(torch.float32)
        flags = [state[4 * frames:5 * frames], state[5 * frames:]]
        rec, grad = torch.empty_like(latent_cur.contiguous()), torch.empty_like(latent_cur.contiguous())
        per = latent_cur[0].numel()
        workspace = torch.empty((max(engine.null_loss_frames_workspace_bytes(frames, per), 256),), dtype=torch.uint8, device=device)
        exp_avg, exp_avg_sq = torch.empty_like(uncond_embeddings), torch.empty_like(uncond_embeddings)
        for i in range(self.num_ddim_steps):
            uncond_embeddings = uncond_embeddings.clone().detach().contiguous()
            uncond_embeddings.requires_grad = True
            # a fresh Adam per outer step (:192): zero moments, step numbers from 1; every frame starts active
            lr = 1e-2 * (1. - i / 100.)
            exp_avg.zero_()
            exp_avg_sq.zero_()
            latent_prev = latents[len(latents) - i - 2].detach().contiguous()
            latent_cur = latent_cur.detach().contiguous()
            t = self.model.scheduler.timesteps[i]
            coeffs = self._step_coeffs("prev", t, latent_cur.dtype)
            prediction = prediction_of(self.scheduler)
            threshold = epsilon + i * 2e-5
            with torch.no_grad():
                noise_pred_cond = self.get_noise_pred_single(latent_cur, t, cond_embeddings).contiguous()
            cur = 0
            flags[cur].fill_(1)
            active = [True] * frames
            losses = [[] for _ in range(frames)]
            for j in range(num_inner_steps):
                noise_pred_uncond = self.get_noise_pred_single(latent_cur, t, uncond_embeddings).contiguous()
                engine.null_loss_grad_frames(noise_pred_uncond.detach(), noise_pred_cond, latent_cur, latent_prev, self.guidance_scale,
                                             coeffs, flags[cur], threshold, active_out=flags[1 - cur], loss=loss, rec=rec, grad=grad,
                                             workspace=workspace, prediction=prediction)
                (emb_grad,) = torch.autograd.grad(noise_pred_uncond, [uncond_embeddings], grad_outputs=grad)
                engine.adam_step_frames(uncond_embeddings, emb_grad.contiguous(), exp_avg, exp_avg_sq, flags[cur], lr, j + 1)
                host = state.cpu()   # the one wait per inner step: the early stops need it
                loss_host = host[:4 * frames].view(torch.float32).tolist()
                for f in range(frames):
                    if active[f]:
                        losses[f].append(loss_host[f])
                cur = 1 - cur
                active = [bool(a) for a in host[(4 + cur) * frames:(5 + cur) * frames].tolist()]
                if not any(active):
                    break
            self.inner_steps_taken.append([len(row) for row in losses])
            self.losses.append(losses)
            uncond_embeddings_list.append(uncond_embeddings.detach())
            with torch.no_grad():
                context = torch.cat([uncond_embeddings, cond_embeddings])
                latent_cur = self.get_noise_pred(latent_cur, t, False, context)
        return uncond_embeddings_list

    def invert_frames(self, images, prompt: str, num_inner_steps=10, early_stop_epsilon=1e-5, null_text_optimization=True):
        """invert on F frames at once: images uint8 [F,512,512,3] on the device (512: self.work_size) -> (x_t [F,C,h,w],
        uncond_embeddings): one
        [F,77,D] tensor per outer step, or None where invert returns plain copies of the empty prompt's embedding (no
        optimisation asked for, or a ComfyUI model without torch.func).  Every frame's x_t, embeddings, losses and inner-step
        counts are what invert gives on that frame alone wherever the model's own arithmetic does not depend on the batch."""
        work_size = check_work_size(self.work_size)
        if not (isinstance(images, torch.Tensor) and images.dtype == torch.uint8 and images.dim() == 4
                and tuple(images.shape[1:]) == (work_size, work_size, 3) and images.shape[0] > 0):
            raise ValueError(f"images must be a uint8 tensor [F,{work_size},{work_size},3]")
        self.init_prompt(prompt)
        diffusion_utils.register_attention_control(self.model, None)
        ddim_latents = self.ddim_loop_frames(self._images2latent(images))
        uncond_embeddings = None
        if null_text_optimization:
            if not self._is_comfyui:
                uncond_embeddings = self.null_optimization_frames(ddim_latents, num_inner_steps, early_stop_epsilon)
            elif functional_call is not None:
                self.model.unet.enable_gradient_mode()
                try:
                    uncond_embeddings = self.null_optimization_frames(ddim_latents, num_inner_steps, early_stop_epsilon)
                finally:
                    self.model.unet.disable_gradient_mode()
        return ddim_latents[-1], uncond_embeddings


def _standard_work_size():
    """stereodiffusion_nodes.STANDARD_WORK_SIZE as it stands now, checked: the one switch of Standard mode's work frame."""
    from . import stereodiffusion_nodes
    return check_work_size(stereodiffusion_nodes.STANDARD_WORK_SIZE)


def make_invert(model, num_ddim_steps, guidance_scale, null_text_optimization=True, num_inner_steps=10, early_stop_epsilon=1e-5):
    """-> invert(image_u8 [512,512,3]) -> (x_t, uncond_embeddings), 512 being stereodiffusion_nodes.STANDARD_WORK_SIZE when the
    callable runs: the callable stereodiffusion_nodes.generate_stereo_standard
    takes where the reference runs NullInversion(ldm_stable, steps, guidance_scale).invert(image, "", ...)
    (stereodiffusion_nodes.py:267-273).  The attention hook invert installs is removed again before it returns: the Standard
    loop installs its own."""
    from . import stereo_utils

    def invert(image_u8):
        work_size = _standard_work_size()   # (refused before the model is touched)
        inversion = NullInversion(model, num_ddim_steps, guidance_scale)
        inversion.work_size = work_size
        try:
            _, x_t, uncond_embeddings = inversion.invert(image_u8, "", num_inner_steps=num_inner_steps,
                                                         early_stop_epsilon=early_stop_epsilon,
                                                         null_text_optimization=null_text_optimization)
        finally:
            stereo_utils.restore_attention(model)
        return x_t, uncond_embeddings

    return invert


def make_invert_frames(model, num_ddim_steps, guidance_scale, null_text_optimization=True, num_inner_steps=10, early_stop_epsilon=1e-5):
    """-> invert_frames(images_u8 [F,512,512,3]) -> (x_t [F,C,h,w], uncond_embeddings), 512 being
    stereodiffusion_nodes.STANDARD_WORK_SIZE when the callable runs: make_invert for
    stereodiffusion_nodes.generate_stereo_standard_frames, F frames in one UNet batch."""
    from . import stereo_utils

    def invert_frames(images_u8):
        work_size = _standard_work_size()   # (refused before the model is touched)
        inversion = NullInversion(model, num_ddim_steps, guidance_scale)
        inversion.work_size = work_size
        try:
            return inversion.invert_frames(images_u8, "", num_inner_steps=num_inner_steps, early_stop_epsilon=early_stop_epsilon,
                                           null_text_optimization=null_text_optimization)
        finally:
            stereo_utils.restore_attention(model)

    return invert_frames
