"""The tensor work of StereoDiffusion's Fast mode around its inpainting model (reference stereodiffusion_nodes.py,
StereoDiffusionNode._generate_stereo_fast_single):

    prepare_inpaint  the backward warp, the inpaint mask and the gap pre-fill handed to the model (:425-542)
    compose_stereo   the model's pixels pasted back under the mask and the side-by-side pair (:563-571)

The arithmetic of prepare_inpaint runs in the HIP kernels behind cs_inpaint_prepare (there is no CPU fallback: without a GPU it
raises); compose_stereo is a `where` and a concatenation, plain torch plumbing on whatever device its tensors are on.

Out of scope: the PIL resizes to and from 512 x 512 around this work (:421-423, :569-570; the reference's default bicubic filter
is not restated here -- callers resize with the tool of their choice), and the diffusion model itself.
"""
import torch

from . import engine


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
