"""The StereoDiffusion node's ComfyUI protocol and the MODEL / CLIP / VAE wrappers on duck-typed stand-ins: no comfy, no gpu."""
import inspect
import subprocess
import sys
import os
import types

import pytest
import torch
import torch.nn as nn

import comfystereo_amd
from comfystereo_amd import model_wrappers as mw
from comfystereo_amd import schedulers
from comfystereo_amd import stereodiffusion_nodes as sdn

# the reference node's INPUT_TYPES(), as data
REFERENCE_INPUT_TYPES = {
    "required": {
        "image": ("IMAGE",),
        "depth_map": ("IMAGE",),
        "scale_factor": ("FLOAT", {"default": 5.0, "min": 1.0, "max": 20.0, "step": 0.5,
                                   "tooltip": "Controls the strength of the stereo effect (disparity)"}),
        "direction": (["uni", "bi"], {"default": "uni", "tooltip": "uni: unidirectional attention, bi: bidirectional attention"}),
        "deblur": ("BOOLEAN", {"default": False, "tooltip": "Add noise to unfilled regions to avoid blurring"}),
        "pipeline_mode": (["Standard (DDIM)", "Fast (Warp + Inpaint)"], {
            "default": "Fast (Warp + Inpaint)",
            "tooltip": "Standard: DDIM inversion (high quality, slow). Fast: Warp image with depth, then AI-inpaint only the gap regions (fast, works with turbo/LCM models)"}),
        "guidance_scale": ("FLOAT", {"default": 3.0, "min": 0.0, "max": 20.0, "step": 0.5,
                                     "tooltip": "CFG scale. Standard mode: 3-10. Turbo models: 0.0. LCM: 1.0-2.0"}),
        "num_inference_steps": ("INT", {
            "default": 20, "min": 1, "max": 100, "step": 1,
            "tooltip": "Number of inference steps. Standard DDIM: 30-100 (default 50). Fast inpainting: 20-30. Turbo/LCM: 1-8"}),
        "seed": ("INT", {"default": 1337, "min": 0, "max": 18446744073709551615, "control_after_generate": True,
                         "tooltip": "Random seed for reproducible results"}),
    },
    "optional": {
        "null_text_optimization": ("BOOLEAN", {
            "default": True, "tooltip": "Enable null-text optimization for better reconstruction (Standard mode only)"}),
        "denoise_strength": ("FLOAT", {
            "default": 0.6, "min": 0.1, "max": 1.0, "step": 0.05,
            "tooltip": "How much noise to add before denoising (Fast mode). Lower = preserve original more, Higher = more model creativity for filling gaps"}),
        "model": ("MODEL", {"tooltip": "ComfyUI MODEL input. Fast mode: use inpainting model (9ch UNet). Standard mode: use any SD1/SD2 model."}),
        "clip": ("CLIP", {"tooltip": "CLIP from Load Checkpoint"}),
        "vae": ("VAE", {"tooltip": "VAE from Load Checkpoint"}),
        "model_id": ("STRING", {"default": "runwayml/stable-diffusion-v1-5",
                                "tooltip": "Fallback HuggingFace model ID (Standard mode, when no ComfyUI model connected)"}),
        "inpaint_model_id": ("STRING", {"default": "runwayml/stable-diffusion-inpainting",
                                        "tooltip": "Fallback inpainting model ID (Fast mode, when no ComfyUI model connected)"}),
        "prompt": ("STRING", {"default": "", "multiline": True,
                              "tooltip": "Optional text prompt to guide inpainting (Fast mode). Describe the image content for better gap filling."}),
    },
}


def test_node_protocol():
    node = sdn.StereoDiffusionNode
    got = node.INPUT_TYPES()
    assert got == REFERENCE_INPUT_TYPES
    assert list(got["required"]) == list(REFERENCE_INPUT_TYPES["required"]) and list(got["optional"]) == list(REFERENCE_INPUT_TYPES["optional"])
    assert node.RETURN_TYPES == ("IMAGE", "IMAGE", "IMAGE") and node.RETURN_NAMES == ("stereo_pair", "left_image", "right_image")
    assert node.FUNCTION == "generate_stereo" and node.CATEGORY == "image/stereo"
    sig = inspect.signature(node.generate_stereo)
    assert list(sig.parameters) == ["self", "image", "depth_map", "scale_factor", "direction", "deblur", "pipeline_mode", "guidance_scale",
                                    "num_inference_steps", "seed", "null_text_optimization", "denoise_strength", "model", "clip", "vae",
                                    "model_id", "inpaint_model_id", "prompt"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(pipeline_mode="Standard (DDIM)", guidance_scale=7.5, num_inference_steps=50, seed=0, null_text_optimization=True,
                            denoise_strength=0.5, model=None, clip=None, vae=None, model_id="",
                            inpaint_model_id="runwayml/stable-diffusion-inpainting", prompt="")


def test_registration_holds_both_nodes():
    from comfystereo_amd import GenerateStereo
    assert sdn.NODE_CLASS_MAPPINGS == {"StereoDiffusion": sdn.StereoDiffusionNode}
    assert sdn.NODE_DISPLAY_NAME_MAPPINGS == {"StereoDiffusion": "StereoDiffusion"}
    assert comfystereo_amd.NODE_CLASS_MAPPINGS == {"StereoImageNode": GenerateStereo.StereoImageNode, "StereoDiffusion": sdn.StereoDiffusionNode}
    assert comfystereo_amd.NODE_DISPLAY_NAME_MAPPINGS == {"StereoImageNode": "Stereo Image Node", "StereoDiffusion": "StereoDiffusion"}
    with pytest.raises(AttributeError):
        comfystereo_amd.NO_SUCH_NAME


def test_package_import_loads_no_node_module_and_wrappers_need_no_comfy():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\nimport comfystereo_amd\n"
            "assert 'torch' not in sys.modules and 'comfystereo_amd.stereodiffusion_nodes' not in sys.modules\n"
            "import comfystereo_amd.model_wrappers, comfystereo_amd.schedulers\n"
            "assert 'comfy' not in sys.modules and 'diffusers' not in sys.modules\n"
            "assert len(comfystereo_amd.NODE_CLASS_MAPPINGS) == 2\nprint('lazy')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "lazy" in out.stdout, out.stderr[-2000:]


def test_node_without_models_says_to_connect_them():
    node = sdn.StereoDiffusionNode()
    image = torch.zeros((1, 8, 8, 3))
    for mode in (sdn.FAST_MODE, sdn.STANDARD_MODE):
        for given in ({}, dict(model=object()), dict(model=object(), clip=object())):
            with pytest.raises(ValueError, match="connect MODEL, CLIP and VAE"):
                node.generate_stereo(image, image, 5.0, "uni", False, mode, **given)


# ---- stand-ins ------------------------------------------------------------------------------------------------------------------------
class Clip:
    def __init__(self, keys=("l",), length=3):
        self.keys, self.length, self.encoded = keys, length, 0
        self.cond_stage_model = object()

    def tokenize(self, text):
        return {k: [[(100 * (i + 1) + j, 1.0) for j in range(self.length)]] for i, k in enumerate(self.keys)}

    def encode_from_tokens(self, tokens, return_pooled=False):
        self.encoded += 1
        return torch.full((1, 77, 4), float(self.encoded)), torch.full((1, 4), -1.0)


def test_tokenizer_pads_truncates_and_prefers_l_then_g():
    tok = mw.TokenizerWrapper(Clip(("x", "g", "l")))
    assert tok.model_max_length == 77
    ids = tok(["a", "b"], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert ids.dtype == torch.long and tuple(ids.shape) == (2, 77)
    assert ids[0].tolist() == [300, 301, 302] + [49407] * 74
    assert mw.TokenizerWrapper(Clip(("x", "g")))("a").input_ids[0, :3].tolist() == [200, 201, 202]
    assert mw.TokenizerWrapper(Clip(("x", "y")))("a").input_ids[0, :3].tolist() == [100, 101, 102]
    long = mw.TokenizerWrapper(Clip(("l",), 90))
    assert tuple(long("a").input_ids.shape) == (1, 77) and long("a").input_ids[0, -1] == 176
    assert tuple(long("a", truncation=False).input_ids.shape) == (1, 90)
    assert tuple(long("a", max_length=5).input_ids.shape) == (1, 5)


def test_text_encoder_caches_and_repeats_the_empty_prompt():
    clip = Clip()
    enc = mw.TextEncoderWrapper(clip, "cpu")
    cond, pooled = enc.encode_text("a")
    again, _ = enc.encode_text("a", target_device="cpu")
    assert clip.encoded == 1 and torch.equal(cond, again) and pooled is not None
    emb, pooled = enc(torch.zeros((3, 77), dtype=torch.long))
    assert clip.encoded == 2 and tuple(emb.shape) == (3, 77, 4) and bool((emb == 2.0).all())
    enc(torch.zeros((1, 77), dtype=torch.long))
    assert clip.encoded == 2


class Vae:
    def __init__(self):
        self.first_stage_model = nn.Linear(2, 2)
        self.seen = None

    def encode(self, pixels):
        self.seen = pixels
        return pixels.permute(0, 3, 1, 2)[:, :, ::2, ::2] * 3.0

    def decode(self, z):
        return z.permute(0, 2, 3, 1) * 0.5


def test_vae_wrapper_converts_values_and_layout():
    vae = Vae()
    w = mw.VAEWrapper(vae, "cpu")
    assert list(w.parameters())[0] is vae.first_stage_model.weight and w.first_stage_model is vae.first_stage_model
    x = torch.randn((2, 3, 4, 6), generator=torch.Generator().manual_seed(1))
    mean = w.encode(x)["latent_dist"].mean
    want_pixels = ((x + 1.0) / 2.0).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(vae.seen, want_pixels) and vae.seen.is_contiguous() and vae.seen.device.type == "cpu"
    assert torch.equal(mean, want_pixels.permute(0, 3, 1, 2)[:, :, ::2, ::2] * 3.0)
    z = torch.randn((2, 4, 3, 5), generator=torch.Generator().manual_seed(2))
    sample = w.decode(z)["sample"]
    assert tuple(sample.shape) == (2, 4, 3, 5) and torch.equal(sample, (z.permute(0, 2, 3, 1) * 0.5).permute(0, 3, 1, 2) * 2.0 - 1.0)


class Diffusion(nn.Module):
    def __init__(self, in_channels=4):
        super().__init__()
        if in_channels is not None:
            self.in_channels = in_channels
        self.weight = nn.Parameter(torch.full((), 2.0))
        self.register_buffer("shift", torch.full((), 0.5))
        self.timesteps = None

    def forward(self, x, timesteps, context=None):
        self.timesteps = timesteps
        return x * self.weight + self.shift + context[:, 0, 0].reshape(-1, 1, 1, 1)


def comfy_model(config_name="SD15", in_channels=4, inference=False):
    if inference:
        with torch.inference_mode():
            unet = Diffusion(in_channels)
    else:
        unet = Diffusion(in_channels)
    config = type(config_name, (), {})()
    return types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet, model_config=config))


@pytest.mark.parametrize("name,channels,want,standard,fast", [
    ("SD15", 4, "SD1", True, True), ("SD20", 4, "SD2", True, True), ("SDXL", 4, "SDXL", False, False), ("Flux", 16, "FLUX", False, False),
    ("Other", 4, "SD1", True, True), ("Other", 9, "UNKNOWN", False, False), ("Other", None, "SD1", True, True)])
def test_model_type_detection_and_support(name, channels, want, standard, fast):
    m = mw.ComfyUIModelWrapper(comfy_model(name, channels), Clip(), Vae(), device="cpu")
    assert m.model_type == m._detect_model_type() == want
    assert m.is_supported() is standard and m.is_supported("standard") is standard and m.is_supported("fast") is fast
    assert m.get_unsupported_message() == (f"Model type '{want}' is not yet supported for stereo generation. "
                                           "Currently supported: SD1, SD2. SDXL and FLUX support may be added in future updates.")
    assert isinstance(m.scheduler, schedulers.DDIMScheduler) and m.device == torch.device("cpu")
    assert m.comfy_model.model.diffusion_model is m.unet.diffusion_model and m.unet.in_channels == (4 if channels is None else channels)
    assert isinstance(m.vae, mw.VAEWrapper) and isinstance(m.text_encoder, mw.TextEncoderWrapper) and isinstance(m.tokenizer, mw.TokenizerWrapper)
    broken = mw.ComfyUIModelWrapper.__new__(mw.ComfyUIModelWrapper)
    broken.comfy_model = object()
    assert broken._detect_model_type() == "UNKNOWN"


def test_inpaint_runner_needs_nine_channels():
    with pytest.raises(ValueError) as e:
        mw.make_inpaint_runner(comfy_model("SD15", 4), Clip(), Vae(), device="cpu")
    assert str(e.value) == ("Connected model has 4 UNet input channels, but inpainting requires 9 channels. "
                            "Please use an inpainting checkpoint (e.g., sd-v1-5-inpainting).")
    runner = mw.make_inpaint_runner(comfy_model("SD15", 9), Clip(), Vae(), device="cpu")
    assert runner.unet.in_channels == 9 and isinstance(runner.vae, mw.VAEWrapper) and isinstance(runner.tokenizer, mw.TokenizerWrapper)
    node = sdn.StereoDiffusionNode()
    image = torch.zeros((1, 8, 8, 3))
    with pytest.raises(ValueError, match="requires 9 channels"):
        node.generate_stereo(image, image, 5.0, "uni", False, sdn.FAST_MODE, model=comfy_model("SD15", 4), clip=Clip(), vae=Vae())
    with pytest.raises(ValueError, match="Model type 'SDXL' is not yet supported"):
        node.generate_stereo(image, image, 5.0, "uni", False, sdn.STANDARD_MODE, model=comfy_model("SDXL", 4), clip=Clip(), vae=Vae())


def test_unet_wrapper_expands_the_timestep_and_gradient_mode_reaches_an_embedding():
    model = comfy_model(inference=True)
    unet = mw.UNetWrapper(model, "cpu")
    assert unet.in_channels == 4 and model.model.diffusion_model.weight.is_inference()
    x = torch.ones((2, 4, 3, 3))
    ctx = torch.zeros((2, 77, 4))
    out = unet(x, 7, encoder_hidden_states=ctx)["sample"]
    assert bool((out == 2.5).all()) and model.model.diffusion_model.timesteps.tolist() == [7.0, 7.0]
    unet(x, torch.tensor(3), encoder_hidden_states=ctx)
    assert model.model.diffusion_model.timesteps.tolist() == [3.0, 3.0]
    emb = torch.zeros((2, 77, 4), requires_grad=True)
    unet.enable_gradient_mode()
    assert unet._gradient_mode and set(unet._cloned_params) == {"weight"} and set(unet._cloned_buffers) == {"shift"}
    assert not unet._cloned_params["weight"].is_inference()
    loss = unet(x, torch.tensor(3), encoder_hidden_states=emb)["sample"].sum()
    loss.backward()
    assert emb.grad is not None and float(emb.grad[0, 0, 0]) == 36.0 and float(emb.grad.sum()) == 72.0
    unet.disable_gradient_mode()
    assert not unet._gradient_mode and unet._cloned_params is None and unet._cloned_buffers is None
