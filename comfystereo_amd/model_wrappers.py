"""ComfyUI's MODEL / CLIP / VAE as the `ldm_stable` surface the StereoDiffusion code reads (reference model_wrappers.py:34-486):
tokenizer, text_encoder, unet, vae, scheduler, device.

  VAEWrapper            encode(x)['latent_dist'].mean, decode(z)['sample']: [-1,1] NCHW here, [0,1] NHWC at ComfyUI's VAE
  TextEncoderWrapper    encode_text(text) -> (cond, pooled), cached per text; __call__(input_ids) encodes "" and repeats it
  TokenizerWrapper      77 tokens, padded with 49407; the `l` tokens before the `g` ones before whatever comes first
  UNetWrapper           unet(latents, t, encoder_hidden_states=...)['sample']; enable_gradient_mode() runs the model through
                        torch.func.functional_call on cloned parameters and buffers, so that gradients reach an embedding although
                        ComfyUI created the weights under inference mode (null-text optimisation needs this)
  ComfyUIModelWrapper   the five above plus our DDIMScheduler, the model type by the reference's class-name rules
  make_inpaint_runner   inpaint_runner.InpaintRunner around a 9-channel MODEL (a 4-channel one with the few-step samplers), for
                        Fast mode

comfy.model_management.load_models_gpu is called where the reference calls it, inside the constructors, and skipped when `comfy`
cannot be imported: every class works on duck-typed stand-ins.  Importing this module needs neither comfy nor diffusers.

Not here: the reference's set_scheduler_for_mode, which nothing in the reference calls.  Its Euler scheduler with trailing spacing
(:419-459), which no model type the reference detects selects, lives as the sampler "euler" of inpaint_runner.InpaintRunner
(fewstep_timesteps, fewstep_coeffs, FewStepLoop; the step is cs_inpaint_fewstep_step), next to the "lcm" sampler.
"""
import types

import torch

from . import inpaint_runner
from .schedulers import DDIMScheduler

try:
    from torch.func import functional_call
except ImportError:
    functional_call = None

SUPPORTED_MODEL_TYPES = ["SD1", "SD2"]
FAST_PIPELINE_MODEL_TYPES = ["SD1", "SD2", "SD_TURBO"]
PAD_TOKEN = 49407   # CLIP's end-of-text id, which pads


def _load_to_gpu(model):
    """comfy.model_management.load_models_gpu([model]), where there is a ComfyUI."""
    try:
        import comfy.model_management as mm
    except ImportError:
        return
    mm.load_models_gpu([model])


def _in_channels(unet):
    return unet.in_channels if hasattr(unet, 'in_channels') else 4


class VAEWrapper:
    def __init__(self, comfy_vae, device="cuda"):
        self.comfy_vae = comfy_vae
        self.first_stage_model = comfy_vae.first_stage_model
        self._device = torch.device(device)

    def parameters(self):
        return self.first_stage_model.parameters()

    def _get_device(self):
        for p in self.first_stage_model.parameters():
            return p.device
        return self._device

    def encode(self, x):
        """x [B,C,H,W] in [-1, 1] -> {'latent_dist': an object whose .mean is ComfyUI's latents}.  ComfyUI's encode takes
        [B,H,W,C] in [0, 1] on the host and moves it itself."""
        pixels = ((x + 1.0) / 2.0).permute(0, 2, 3, 1).contiguous().cpu()
        return {'latent_dist': types.SimpleNamespace(mean=self.comfy_vae.encode(pixels))}

    def decode(self, z):
        """z [B,C,h,w] -> {'sample': [B,C,H,W] in [-1, 1]} from ComfyUI's [B,H,W,C] in [0, 1]."""
        return {'sample': self.comfy_vae.decode(z).permute(0, 3, 1, 2) * 2.0 - 1.0}


class TextEncoderWrapper:
    def __init__(self, comfy_clip, device="cuda"):
        self.comfy_clip = comfy_clip
        self.cond_stage_model = getattr(comfy_clip, "cond_stage_model", None)
        self._device = torch.device(device)
        self._embedding_cache = {}

    def encode_text(self, text, target_device=None):
        """-> (cond, pooled) of ComfyUI's own tokenize and encode_from_tokens, encoded once per text."""
        if text not in self._embedding_cache:
            tokens = self.comfy_clip.tokenize(text)
            self._embedding_cache[text] = tuple(self.comfy_clip.encode_from_tokens(tokens, return_pooled=True))
        cond, pooled = self._embedding_cache[text]
        if target_device is not None:
            cond = cond.to(target_device)
            pooled = None if pooled is None else pooled.to(target_device)
        return cond, pooled

    def __call__(self, input_ids):
        """The diffusers call.  StereoDiffusion encodes the empty prompt only: whatever the ids, the answer is the embedding of ""
        once per row of input_ids, on their device."""
        cond, pooled = self.encode_text("", target_device=input_ids.device)
        return (cond.repeat(input_ids.shape[0], 1, 1), pooled)


class TokenizerWrapper:
    def __init__(self, comfy_clip):
        self.comfy_clip = comfy_clip
        self.model_max_length = 77

    def __call__(self, text, padding="max_length", max_length=None, truncation=True, return_tensors="pt"):
        max_length = self.model_max_length if max_length is None else max_length
        rows = []
        for t in ([text] if isinstance(text, str) else text):
            tokens = self.comfy_clip.tokenize(t)
            # {'l': ..., 'g': ...}: lists, per chunk, of (token id, weight) pairs; the first chunk is the prompt's
            data = tokens['l'] if 'l' in tokens else tokens['g'] if 'g' in tokens else list(tokens.values())[0]
            ids = [pair[0] for pair in (data[0] if data else [])]
            if len(ids) < max_length:
                ids = ids + [PAD_TOKEN] * (max_length - len(ids))
            elif truncation:
                ids = ids[:max_length]
            rows.append(ids)
        return types.SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.long))


class UNetWrapper:
    def __init__(self, comfy_model, device="cuda"):
        self.comfy_model = comfy_model
        self.diffusion_model = comfy_model.model.diffusion_model
        self._device = torch.device(device)
        self.in_channels = _in_channels(self.diffusion_model)
        self._gradient_mode = False
        self._cloned_params = None
        self._cloned_buffers = None

    def _get_model_device(self):
        for p in self.diffusion_model.parameters():
            return p.device
        return self._device

    def enable_gradient_mode(self):
        """Clone every parameter and buffer: the clones are ordinary tensors, made outside inference mode, and the forward goes
        through them."""
        if not self._gradient_mode:
            self._cloned_params = {name: p.clone().detach() for name, p in self.diffusion_model.named_parameters()}
            self._cloned_buffers = {name: b.clone().detach() for name, b in self.diffusion_model.named_buffers()}
            self._gradient_mode = True

    def disable_gradient_mode(self):
        self._gradient_mode = False
        self._cloned_params = None
        self._cloned_buffers = None

    def __call__(self, latents, timestep, encoder_hidden_states=None):
        device = self._get_model_device()
        dtype = next(self.diffusion_model.parameters()).dtype

        def own(t):   # on the model's device and in its dtype; in gradient mode a copy that is no inference tensor
            return (t.clone() if self._gradient_mode else t).to(device=device, dtype=dtype)

        latents = own(latents)
        if encoder_hidden_states is not None:
            encoder_hidden_states = own(encoder_hidden_states)
        timestep = own(timestep) if isinstance(timestep, torch.Tensor) else torch.tensor([timestep], device=device, dtype=dtype)
        if timestep.dim() == 0 or (timestep.dim() == 1 and timestep.shape[0] == 1):
            timestep = timestep.expand(latents.shape[0])
        if self._gradient_mode and self._cloned_params is not None and functional_call is not None:
            noise_pred = functional_call(self.diffusion_model, (self._cloned_params, self._cloned_buffers), args=(latents, timestep),
                                         kwargs={'context': encoder_hidden_states})
        else:
            noise_pred = self.diffusion_model(latents, timestep, context=encoder_hidden_states)
        return {'sample': noise_pred}


class ComfyUIModelWrapper:
    def __init__(self, model, clip, vae, device="cuda"):
        self.comfy_model, self.comfy_clip, self.comfy_vae = model, clip, vae
        self._device = torch.device(device)
        _load_to_gpu(model)
        self.unet = UNetWrapper(model, device)
        self.vae = VAEWrapper(vae, device)
        self.text_encoder = TextEncoderWrapper(clip, device)
        self.tokenizer = TokenizerWrapper(clip)
        self._model_type = self._detect_model_type()
        self._prediction_kind = detect_prediction_kind(model)
        # the steps between two UNet calls restate epsilon and v-prediction; any other kind is refused by is_supported, and its
        # scheduler is never stepped
        self.scheduler = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                                       set_alpha_to_one=False, prediction_type=self.prediction_type or "epsilon")

    def _detect_model_type(self):
        """By the name of the model configuration's class; an unknown name with a 4-channel UNet counts as SD1."""
        try:
            name = self.comfy_model.model.model_config.__class__.__name__
            for needles, kind in ((("SD1", "SD10"), "SD1"), (("SD2", "SD20"), "SD2"), (("SDXL",), "SDXL"), (("Flux",), "FLUX")):
                if any(n in name for n in needles):
                    return kind
            return "SD1" if _in_channels(self.comfy_model.model.diffusion_model) == 4 else "UNKNOWN"
        except Exception:
            return "UNKNOWN"

    @property
    def device(self):
        for p in self.comfy_model.model.diffusion_model.parameters():
            return p.device
        return self._device

    @property
    def model_type(self):
        return self._model_type

    @property
    def prediction_type(self):
        """"epsilon" or "v_prediction" (the scheduler's prediction_type); None for a kind of model the steps do not restate."""
        return _PREDICTION_OF_KIND.get(self._prediction_kind)

    def is_supported(self, pipeline_mode="standard"):
        if self.prediction_type is None:
            return False
        return self._model_type in (FAST_PIPELINE_MODEL_TYPES if pipeline_mode == "fast" else SUPPORTED_MODEL_TYPES)

    def get_unsupported_message(self):
        if self.prediction_type is None:
            return (f"Model sampling type '{self._prediction_kind}' is not supported for stereo generation: the DDIM steps are "
                    "stated for epsilon (EPS) and v-prediction (V_PREDICTION) models only.")
        return (f"Model type '{self._model_type}' is not yet supported for stereo generation. "
                f"Currently supported: {', '.join(SUPPORTED_MODEL_TYPES)}. "
                f"SDXL and FLUX support may be added in future updates.")


_PREDICTION_OF_KIND = {"EPS": "epsilon", "V_PREDICTION": "v_prediction"}


def detect_prediction_kind(model):
    """ComfyUI's model.model.model_type, duck-typed -> its name, upper case: an enum member (comfy.model_base.ModelType: EPS,
    V_PREDICTION, EDM, FLOW, ...) gives its .name, a string itself.  A model that does not say is an epsilon model: "EPS"."""
    kind = getattr(getattr(model, "model", None), "model_type", None)
    if kind is None:
        return "EPS"
    name = kind if isinstance(kind, str) else getattr(kind, "name", None)
    if not isinstance(name, str):
        return str(kind).upper()
    name = name.upper()
    return {"EPSILON": "EPS", "V_PRED": "V_PREDICTION"}.get(name, name)


def make_inpaint_runner(model, clip, vae, device="cuda", sampler="plms"):
    """-> inpaint_runner.InpaintRunner around the MODEL's diffusion model and the wrapped VAE and CLIP (the reference's
    ComfyUIInpaintRunner.__init__, :496-520).  ValueError with the reference's message unless the UNet takes 9 channels; the
    few-step samplers ("euler", "lcm") take a 4-channel UNet too.  An unknown sampler is refused by name."""
    if sampler not in inpaint_runner.SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r} ({', '.join(inpaint_runner.SAMPLERS)})")
    unet = model.model.diffusion_model
    in_ch = _in_channels(unet)
    if in_ch != 9 and not (in_ch == 4 and sampler != "plms"):   # before anything is loaded
        raise ValueError(f"Connected model has {in_ch} UNet input channels, but inpainting requires 9 channels. "
                         f"Please use an inpainting checkpoint (e.g., sd-v1-5-inpainting).")
    kind = detect_prediction_kind(model)
    if kind != "EPS":   # the PLMS step restates epsilon prediction only (the published SD2 inpainting checkpoint is an epsilon model)
        raise ValueError(f"Connected inpainting model declares {'v-prediction' if kind == 'V_PREDICTION' else kind} "
                         f"(model_type {kind}); Fast mode's inpainting loop supports epsilon-prediction models only.")
    _load_to_gpu(model)
    return inpaint_runner.InpaintRunner(unet, VAEWrapper(vae, device), TextEncoderWrapper(clip, device), TokenizerWrapper(clip),
                                        sampler=sampler)
