"""StereoDiffusion's Fast mode around its inpainting model (reference stereodiffusion_nodes.py,
StereoDiffusionNode._generate_stereo_fast and _generate_stereo_fast_single):

    generate_stereo_fast  the whole per-frame work of the mode at any frame size, batched, with the model as a callback (:378-573)
    pil_resize            PIL.Image.resize(size) with Pillow's defaults (8-bit bicubic), byte for byte (:422-423, :481-482, :569-570)
    prepare_inpaint       the backward warp, the inpaint mask and the gap pre-fill handed to the model (:425-542)
    compose_stereo        the model's pixels pasted back under the mask and the side-by-side pair (:563-571)

The arithmetic of pil_resize and prepare_inpaint runs in the HIP kernels behind cs_pil_resize and cs_inpaint_prepare (there is no
CPU fallback: without a GPU they raise); compose_stereo is a `where` and a concatenation, plain torch plumbing on whatever device
its tensors are on.

A coloured depth is made gray as trunc((r * 0.2989 + g * 0.5870) + b * 0.1140) in float64, in this order.  That equals the
reference on every depth with three equal channels; on a few hundred of the 2^24 colours the reference's BLAS product differs
from it, and from itself between array shapes.

Out of scope: loading and running the diffusion model itself -- generate_stereo_fast calls the `inpaint` it is given.
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
