"""Drop-in for the two module functions GenerateStereo.py calls in the reference
(`from . import stereoimage_generation as sig`, reference GenerateStereo.py:25,151,222):

    create_stereoimages      reference stereoimage_generation.py:1422-1574
    create_stereoimages_gpu  reference stereoimage_generation.py:1005-1128

Same names, argument order, defaults, return types and error behaviour; the arithmetic runs in the
HIP kernels behind the C ABI (there is no CPU fallback: without a GPU these functions raise).
Extras kept for callers of the reference's building blocks: apply_stereo_divergence (:1576-1620),
directional_motion_blur_gpu (:1171-1251), forward_warp_gpu (:277-450), forward_warp_mesh (:453-689), and the grid-sample
warps apply_stereo_divergence_gpu (:52-119), warp_and_fill_gpu (:122-274), compute_forward_mask_gpu (:692-757),
detect_disocclusions_gpu (:807-857), interpolate_fill_gpu (:860-920), apply_stereo_divergence_gpu_with_fill (:923-1002),
and the Gaussian depth blurs blur_depth_map (:1253-1281), edge_selective_blur_depth_map (:1283-1309),
left_direction_aware_blur_depth_map (:1311-1327), right_direction_aware_blur_depth_map (:1329-1344).
"""
import numpy as np
import torch
from PIL import Image

from . import engine

_CPU_FILLS = ('none', 'naive', 'naive_interpolating', 'polylines_soft', 'polylines_sharp', 'inverse', 'hybrid_edge',
              'none_post', 'inverse_post', 'hybrid_edge_plus')  # the last three: no UI string reaches them (:1605-1610)
_MODES = ('left-right', 'right-left', 'top-bottom', 'bottom-top', 'red-cyan-anaglyph', 'left-only', 'only-right',
          'cyan-red-reverseanaglyph')


# The reference's import-time switch (:18-24): True makes create_stereoimages_gpu warp through forward_warp_mesh, the
# mesh-quality rasteriser, instead of forward_warp_gpu (:1068-1071).  Both are HIP kernels here; False (the default) is the
# parity-pinned path.  engine.MESH_WARP is the same switch for the node.
MODERNGL_AVAILABLE = False


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _device_for(t):
    """Where a pass over the tensor `t` runs: t's device, else the current GPU (without one, _device's RuntimeError)."""
    return t.device if t.is_cuda else _device()


def _to_u8(x):
    """float32 outputs of the CPU-technique path are k/255 exactly -> recover k."""
    return torch.round(x * 255.0).to(torch.uint8)


def create_stereoimages(original_image, depthmap, divergence, separation=0.0, modes=None,
                        stereo_balance=0.0, stereo_offset_exponent=1.0, fill_technique='polylines_sharp',
                        depth_blur_strength=0.0, depth_blur_edge_threshold=6.0,
                        direction_aware_depth_blur=False, return_modified_depth=True, convergence_point=0.5,
                        depth_blur_falloff=1.0, depth_blur_vert_smooth=0):
    """One frame, CPU-technique semantics: returns PIL images like the reference.

    original_image: torch [3,H,W] (or [H,W,3]) float 0..1;  depthmap: torch [H,W] (or [1,H,W]).
    -> (list[PIL RGB], PIL L left, PIL L right) | (list, PIL L) | list       (reference :1564-1574)
    """
    if modes is None:
        modes = ['left-right']
    if not isinstance(modes, list):
        modes = [modes]
    if len(modes) == 0:
        return []
    if not (isinstance(depthmap, torch.Tensor) and isinstance(original_image, torch.Tensor)):
        return _create_stereoimages_numpy(original_image, depthmap, divergence, separation, modes, stereo_balance,
                                          stereo_offset_exponent, fill_technique, depth_blur_strength,
                                          direction_aware_depth_blur, return_modified_depth, convergence_point,
                                          depth_blur_edge_threshold, depth_blur_falloff, depth_blur_vert_smooth)
    for m in modes:
        if m not in _MODES:
            raise Exception('Unknown mode')
    dev = _device()
    depth = depthmap.to(dev, torch.float32)
    if depth.dim() == 3:
        depth = depth.squeeze()
    img = original_image.to(dev, torch.float32)
    if img.dim() == 3 and img.shape[0] == 3:
        img = img.permute(1, 2, 0)
    h, w = depth.shape
    assert tuple(img.shape[:2]) == (h, w), 'Depthmap and the image must have the same size'
    img = img.contiguous()[None]
    dep = depth.contiguous()[None, :, :, None]
    # an unknown technique falls through the reference's dispatch and returns the source image for both eyes (:1620)
    fill = fill_technique if fill_technique in _CPU_FILLS else 'none'
    div = divergence if fill_technique in _CPU_FILLS else 0.0
    results, left8, right8 = [], None, None
    for m in modes:
        stereo, dl, dr, _ = engine.generate(img, dep, div, separation, m, stereo_balance, convergence_point,
                                            stereo_offset_exponent, fill, depth_blur_edge_threshold, depth_blur_strength,
                                            direction_aware_depth_blur, depth_blur_falloff, depth_blur_vert_smooth, 1)
        results.append(_to_u8(stereo[0]).cpu().numpy())
        left8, right8 = _to_u8(dl[0, :, :, 0]).cpu().numpy(), _to_u8(dr[0, :, :, 0]).cpu().numpy()
    stereo_images = [Image.fromarray(r) for r in results]
    if return_modified_depth:
        if direction_aware_depth_blur:
            return stereo_images, Image.fromarray(left8), Image.fromarray(right8)
        return stereo_images, Image.fromarray(left8)
    return stereo_images


def _create_stereoimages_numpy(original_image, depthmap, divergence, separation, modes, stereo_balance,
                               stereo_offset_exponent, fill_technique, depth_blur_strength, direction_aware_depth_blur,
                               return_modified_depth, convergence_point, depth_blur_edge_threshold=6.0, depth_blur_falloff=1.0,
                               depth_blur_vert_smooth=0):
    """numpy / PIL inputs (reference :1486-1499, 1519-1574): the uint8 image is used as it is, the depth map as float32 without
    the x255 step of the tensor path, each eye is apply_stereo_divergence (HIP, cs_apply_stereo_divergence), the modified
    depth is clip(depth, 0, 255).astype(uint8).  With the depth blur ON the reference takes its scipy blur
    (`directional_motion_blur`: scipy.ndimage sobel + convolve1d in float64, :1346-1419, called with blur_mask_width =
    blur_strength, :1490-1493): cs_directional_blur_scipy (round 4), each eye warped with its own blurred map."""
    for m in modes:
        if m not in _MODES:
            raise Exception('Unknown mode')
    image = np.asarray(original_image)
    depth = np.asarray(depthmap).astype(np.float32)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("numpy / PIL images must be uint8 [H, W, 3] (the reference indexes them as such)")
    assert depth.shape == image.shape[:2], 'Depthmap and the image must have the same size'   # (reference :1586)
    dev = _device()
    img_t = torch.from_numpy(np.array(image, dtype=np.uint8, order='C', copy=True)).to(dev)   # (PIL arrays are read-only)
    dep_t = torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
    dep_l = dep_r = dep_t
    if direction_aware_depth_blur:   # (strength <= 0: the depth map itself for both eyes, :1374)
        # a strength that rounds to a box of 0 taps: scipy's convolve1d raises in the reference as well (:1402-1405).  Tested here,
        # not by re-labelling whatever the native call raises (a HIP failure or an out-of-memory error must stay what it is)
        if depth_blur_strength > 0 and int(round(depth_blur_strength)) < 1:
            raise RuntimeError("no filter weights given")
        dep_l, dep_r = engine.directional_blur_scipy(dep_t, depth_blur_strength, depth_blur_edge_threshold, depth_blur_strength,
                                                     depth_blur_falloff, depth_blur_vert_smooth)
    left_div, right_div = divergence * (1 + stereo_balance), divergence * (1 - stereo_balance)

    def eye(dep, div_signed, sep_signed, enabled):
        if not enabled or fill_technique not in _CPU_FILLS:   # (< 0.001: the source image, :1536; unknown technique: :1620)
            return img_t
        return engine.apply_stereo_divergence(img_t, dep, div_signed, sep_signed, stereo_offset_exponent, fill_technique,
                                              convergence_point)

    left = eye(dep_l, +1 * left_div, -1 * separation, not (left_div < 0.001))
    right = eye(dep_r, -1 * right_div, separation, not (right_div < 0.001))

    def anaglyph(a, b):   # overlap_red_cyan (:1996-2010): R from a, G and B from b
        return torch.cat([a[..., :1], b[..., 1:]], dim=-1)

    results = []
    for m in modes:
        r = {'left-right': lambda: torch.cat([left, right], 1), 'right-left': lambda: torch.cat([right, left], 1),
             'top-bottom': lambda: torch.cat([left, right], 0), 'bottom-top': lambda: torch.cat([right, left], 0),
             'red-cyan-anaglyph': lambda: anaglyph(left, right), 'left-only': lambda: left, 'only-right': lambda: right,
             'cyan-red-reverseanaglyph': lambda: anaglyph(right, left)}[m]()
        results.append(Image.fromarray(r.contiguous().cpu().numpy()))
    if not return_modified_depth:
        return results
    # np.clip(depth, 0, 255).astype(np.uint8) (:1567-1572): truncation of the clamped float
    if direction_aware_depth_blur:
        return (results, Image.fromarray(torch.clamp(dep_l, 0, 255).to(torch.uint8).cpu().numpy()),
                Image.fromarray(torch.clamp(dep_r, 0, 255).to(torch.uint8).cpu().numpy()))
    return results, Image.fromarray(torch.clamp(dep_t, 0, 255).to(torch.uint8).cpu().numpy())


def create_stereoimages_gpu(image_tensor, depth_tensor, divergence, separation=0.0, modes=None,
                            stereo_balance=0.0, stereo_offset_exponent=1.0, convergence_point=0.5,
                            depth_blur_strength=0.0, depth_blur_edge_threshold=6.0,
                            direction_aware_depth_blur=False, depth_blur_falloff=1.0,
                            depth_blur_vert_smooth=0):
    """Batched 'gpu_warp' driver: image [B,C,H,W] 0..1, depth [B,H,W] ->
    (list[Tensor[B,C,H',W']], left_depth [B,H,W], right_depth [B,H,W], BoolTensor[B,H,W]) on the device."""
    if modes is None:
        modes = ['left-right']
    if not isinstance(modes, list):
        modes = [modes]
    if len(modes) == 0:
        return [], None, None, None
    for m in modes:
        if m not in _MODES:
            raise ValueError(f'Unknown mode: {m}')
    dev = _device()
    img = image_tensor.to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()
    dep = depth_tensor.to(dev, torch.float32).contiguous()[..., None]
    b, h, w, _ = img.shape
    results, lo, ro, mask = [], None, None, None
    for m in modes:
        p = engine.make_params(b, h, w, h, w, 1, 'gpu_warp', m, divergence, separation, stereo_balance, convergence_point,
                               stereo_offset_exponent, direction_aware_depth_blur, depth_blur_strength,
                               depth_blur_edge_threshold, depth_blur_falloff, depth_blur_vert_smooth, b)
        p.flags |= 1  # module-level depth outputs are not clamped (the node clamps them afterwards)
        if MODERNGL_AVAILABLE:
            p.flags |= 4
        stereo, dl, dr, mk = engine.Plan(p, dev).run(img, dep)
        results.append(stereo.permute(0, 3, 1, 2))
        lo, ro, mask = dl[..., 0], dr[..., 0], mk > 0.5
    return results, lo, ro, mask


def apply_stereo_divergence(original_image, depth, divergence, separation, stereo_offset_exponent, fill_technique,
                            convergence_point=0.5):
    """uint8 [H,W,3] image + float32 [H,W] depth (numpy or torch) -> uint8 [H,W,3] numpy (reference :1576-1620)."""
    dev = _device()
    img = torch.as_tensor(np.asarray(original_image) if not isinstance(original_image, torch.Tensor) else original_image)
    dep = torch.as_tensor(np.asarray(depth) if not isinstance(depth, torch.Tensor) else depth)
    assert tuple(img.shape[:2]) == tuple(dep.shape), 'Depthmap and the image must have the same size'
    if fill_technique not in _CPU_FILLS:
        return img.cpu().numpy()  # reference fallback (:1620)
    out = engine.apply_stereo_divergence(img.to(dev, torch.uint8), dep.to(dev, torch.float32), divergence, separation,
                                         stereo_offset_exponent, fill_technique, convergence_point)
    return out.cpu().numpy()


def directional_motion_blur_gpu(depth_tensor, blur_strength, edge_threshold, blur_mask_width=5,
                                falloff_exponent=1.0, vert_smooth_px=0):
    """[H,W] or [B,H,W] depth on the 0..255 scale -> (left, right) device tensors (reference :1171-1251)."""
    if blur_strength <= 0:
        return depth_tensor, depth_tensor
    return engine.directional_blur(depth_tensor.to(_device(), torch.float32), blur_strength, edge_threshold,
                                   falloff_exponent, vert_smooth_px, blur_mask_width=blur_mask_width)


def forward_warp_gpu(image_tensor, depth_tensor, divergence_px, separation_px, stereo_offset_exponent,
                     convergence_point=0.5, gradient_threshold=1.5, max_stretch=8):
    """reference :277-450 -> (warped [B,C,H,W], gap_mask bool [B,H,W]).  gradient_threshold (connectivity, :339-340) and
    max_stretch (scatter rounds, :365) are kernel parameters; the reference's own call sites use the defaults."""
    dev = _device()
    return engine.forward_warp(image_tensor.to(dev, torch.float32), depth_tensor.to(dev, torch.float32), divergence_px,
                               separation_px, stereo_offset_exponent, convergence_point, gradient_threshold, max_stretch)


def forward_warp_mesh(image_tensor, depth_tensor, divergence_px, separation_px, stereo_offset_exponent,
                      convergence_point=0.5, gradient_threshold=1.5, max_stretch=8):
    """reference :453-689 -> (warped [B,C,H,W], gap_mask bool [B,H,W]); `max_stretch` is unused there as well."""
    dev = _device()
    return engine.forward_warp_mesh(image_tensor.to(dev, torch.float32), depth_tensor.to(dev, torch.float32), divergence_px,
                                    separation_px, stereo_offset_exponent, convergence_point, gradient_threshold)


# ---- the grid-sample warps (cs_grid_warp, cs_interpolate_fill, cs_detect_disocclusions) ---------
# Inputs are taken as float32 and moved to the device; results are float32 / bool device tensors.  `device` is accepted and ignored.
def apply_stereo_divergence_gpu(image_tensor, depth_tensor, divergence_px, separation_px,
                                stereo_offset_exponent, convergence_point=0.5):
    """reference :52-119: image [B,C,H,W], depth [B,H,W] -> warped [B,C,H,W] (bilinear grid_sample, border padding)."""
    dev = _device()
    warped, _ = engine.grid_warp(image_tensor.to(dev), depth_tensor.to(dev), divergence_px, separation_px,
                                 stereo_offset_exponent, convergence_point, "warp")
    return warped


def warp_and_fill_gpu(image_tensor, depth_tensor, divergence_px, separation_px,
                      stereo_offset_exponent, convergence_point=0.5):
    """reference :122-274: the warp with edge-stretch fill -> (warped [B,C,H,W], gap_mask bool [B,H,W])."""
    dev = _device()
    return engine.grid_warp(image_tensor.to(dev), depth_tensor.to(dev), divergence_px, separation_px, stereo_offset_exponent,
                            convergence_point, "stretch")


def compute_forward_mask_gpu(depth_tensor, divergence_px, separation_px,
                             stereo_offset_exponent, convergence_point, device):
    """reference :692-757: depth [B,H,W] -> forward gap mask bool [B,H,W] (dilated by one column at offset steps above 1.5)."""
    dev = _device()
    return engine.grid_warp(None, depth_tensor.to(dev), divergence_px, separation_px, stereo_offset_exponent,
                            convergence_point, "mask")[1]


def detect_disocclusions_gpu(depth_tensor, grid, grid_x_warped, device, threshold=0.02):
    """reference :807-857: depth [H,W], grid [1,H,W,2], grid_x_warped [H,W] -> bool [H,W].  W == 1 raises IndexError, as the
    reference's `warp_grad[:, -2]` does."""
    dev = _device()
    if isinstance(depth_tensor, torch.Tensor) and depth_tensor.dim() == 2 and depth_tensor.shape[1] == 1:
        raise IndexError("index -2 is out of bounds for dimension 1 with size 1")
    return engine.detect_disocclusions(depth_tensor.to(dev), grid.to(dev), grid_x_warped.to(dev), threshold)


def interpolate_fill_gpu(image_tensor, mask, device):
    """reference :860-920: image [B,C,H,W], mask bool [B,H,W] (True = fill) -> filled [B,C,H,W]."""
    dev = _device()
    return engine.interpolate_fill(image_tensor.to(dev), mask.to(dev))


def apply_stereo_divergence_gpu_with_fill(image_tensor, depth_tensor, divergence_px, separation_px,
                                          stereo_offset_exponent, convergence_point=0.5, fill_mode='border'):
    """reference :923-1002: one frame -> (warped [C,H,W], valid_mask bool [H,W]).  A 3-D image whose last dimension is 1, 3 or 4
    is read as HWC (so a CHW image with W in {1, 3, 4} is misread, as in the reference); depth is squeezed; fill_mode 'border',
    'zeros' or 'reflection' is the padding, anything else means 'border'."""
    dev = _device()
    img = image_tensor.to(dev)
    if img.dim() == 3 and img.shape[2] in [1, 3, 4]:
        img = img.permute(2, 0, 1)
    if img.dim() != 3:
        raise ValueError(f"image must be [C,H,W] or [H,W,C], got shape {tuple(img.shape)}")
    c, h, w = img.shape
    depth = depth_tensor.to(dev)
    if depth.dim() == 3:
        depth = depth.squeeze()
    if depth.shape not in (torch.Size([h, w]), torch.empty((h, w), device="meta").squeeze().shape):   # (H or W of 1: squeezed)
        raise ValueError(f"depth {tuple(depth_tensor.shape)} does not match the image's {h} x {w}")
    padding = fill_mode if fill_mode in ('border', 'zeros', 'reflection') else 'border'
    warped, valid = engine.grid_warp(img[None], depth.reshape(1, h, w), divergence_px, separation_px, stereo_offset_exponent,
                                     convergence_point, "fill", padding)
    return warped[0], valid[0]


# ---- the Gaussian depth blurs (cs_gaussian_blur) --------------------------------------------------
# numpy (or anything np.asarray takes) [H,W] in, float32 numpy [H,W] out, bit for bit the reference on float32 input.  The one
# deviation: input of another dtype is converted to float32 first (the reference would convolve float64 samples as they are).
def _gaussian(depth, sigma, op, edge_threshold=None):
    dev = _device()
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError(f"depth must be a 2-D map [H,W], got shape {d.shape}")
    d = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(dev)
    return engine.gaussian_blur(d, sigma, op, edge_threshold).cpu().numpy()


def blur_depth_map(depth, sigma):
    """reference :1253-1281: separable Gaussian, radius int(3 * sigma), replicate borders, rows then columns -> float32 [H,W].
    sigma <= 0 returns `depth` itself.  Input that is not float32 is converted to float32 first."""
    if sigma <= 0:
        return depth
    return _gaussian(depth, sigma, "plain")


def edge_selective_blur_depth_map(depth, sigma, edge_threshold):
    """reference :1283-1309: (1 - w) * depth + w * blur with w = min(|3x3 Sobel gradient| / edge_threshold, 1) -> float32 [H,W].
    sigma <= 0 blends the depth with itself.  Input that is not float32 is converted to float32 first."""
    return _gaussian(depth, sigma, "edge_selective", edge_threshold)


def left_direction_aware_blur_depth_map(depth, sigma, edge_threshold):
    """reference :1311-1327: the blend with w = min(g / edge_threshold, 1) where the central horizontal difference g is
    positive, else 0 -> float32 [H,W].  Input that is not float32 is converted to float32 first."""
    return _gaussian(depth, sigma, "left", edge_threshold)


def right_direction_aware_blur_depth_map(depth, sigma, edge_threshold):
    """reference :1329-1344: the blend with w = min(|g| / edge_threshold, 1) where g is negative, else 0 -> float32 [H,W].
    Input that is not float32 is converted to float32 first."""
    return _gaussian(depth, sigma, "right", edge_threshold)


# ---- the depth pre-passes of a clip: one driver of their sub-batches ------------------------------------------
class _DepthFrames:
    """The depth argument of a pre-pass, a host or device tensor (or anything numpy takes) [N,H,W] or [N,H,W,C], and the loop that
    feeds it to the device.  The steps run in the order the caller writes them, its own checks in between; none before run()
    asks for a device."""

    def __init__(self, depth, layout="[N,H,W]"):
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(depth))
        if depth.dim() not in (3, 4) or depth.numel() == 0:
            raise ValueError(f"depth must be a non-empty {layout} or {layout[:-1]},C], got shape {tuple(depth.shape)}")
        self.depth = depth
        self.d4 = depth if depth.dim() == 4 else depth.unsqueeze(-1)
        self.n = depth.shape[0]

    def in_batches_of(self, batch_size):
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size must be at least 1, got {self.batch_size}")
        return self

    def run(self, per_chunk, beside=()):
        """per_chunk(b0, b1, frames b0..b1 of the depth as float32 [k,H,W,C] on the device, the same frames of every tensor of
        `beside`) -> a tuple of device tensors, the first of them y [k,H',W'].  Device input goes in one call, host input in
        sub-batches of batch_size whose results come back to the host.  -> (y of all frames in the caller's layout -- [N,H,W]
        stays, C == 1 stays, any other C gets y in every channel --, the list of every call's other tensors)."""
        where, on_device = _device_for(self.depth), self.depth.is_cuda
        step = self.n if on_device else self.batch_size
        parts, others = [], []
        for b0 in range(0, self.n, step):
            chunks = [t[b0:b0 + step].to(where, torch.float32).contiguous() for t in (self.d4,) + tuple(beside)]
            y, *rest = (t if on_device else t.cpu() for t in per_chunk(b0, b0 + step, *chunks))
            parts.append(y)
            others.append(tuple(rest))
        y = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        if self.depth.dim() == 4:
            y = y.unsqueeze(-1).expand(-1, -1, -1, self.d4.shape[3]).contiguous()
        return y, others


# ---- temporal depth stabilisation of a video batch (cs_temporal_depth) -------------------------------------
def stabilize_depth(depth, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, batch_size=16, cuts=None):
    """The causal, motion-adaptive, scene-cut-aware temporal filter over the depth maps of a clip, run in front of the stereo
    step.  depth: a host or device tensor [N,H,W] or [N,H,W,C] (other dtypes are converted to float32) -> (the filtered depth in
    the input's layout, on the input's device, float32; state).  [N,H,W] and one channel keep their shape, any other C gets y in
    all of its channels.  state: what an earlier call returned for the clip's earlier frames (engine.TemporalState, kept on
    the device), or None.  Host input is uploaded in sub-batches of at most batch_size frames with the state carried on the
    device; the result is bit for bit the one of a single call.  cuts: a list that receives every sub-batch's cut flags (int32 [k]
    on the input's device), for callers that want them -- the node's scene-cut mask."""
    frames = _DepthFrames(depth).in_batches_of(batch_size)

    def filtered(b0, b1, chunk):
        nonlocal state
        y, _, cut, state = engine.temporal_depth(chunk, state, alpha, motion_threshold, cut_threshold)
        return y, cut

    y, flags = frames.run(filtered)
    if cuts is not None:
        cuts.extend(cut for cut, in flags)
    return y, state


# ---- motion-compensated temporal depth stabilisation of a video batch (cs_motion_depth) ----------------------
def stabilize_depth_motion(depth, image, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32,
                           match_threshold=12, batch_size=16, cuts=None, unmatched=None):
    """stabilize_depth with the filter's state read where each 16 x 16 block came from, so that moving content is filtered too; the
    motion is found on the clip's colour frames.  depth: as for stabilize_depth; image: a host or device tensor [N,H',W',3], the
    frames the depth maps belong to, where depth is -> (the filtered depth in the input's layout, on the input's device, float32;
    state: engine.MotionState).  An image at another size than the depth is brought there with engine.pil_resize (Pillow's 8-bit
    bicubic); its codes go on as codes / 255, which the luma conversion maps back to the codes exactly (code(k / 255) = k).
    search_range 0..32 pixels at the depth's resolution, smoothness 0..4096, match_threshold 0..255: engine.motion_depth; their
    defaults are starting values that nobody has tuned on footage.  Host input is uploaded in sub-batches of at most batch_size
    frames with the state carried on the device; the result is bit for bit the one of a single call.  cuts: a list that receives
    every sub-batch's cut flags (int32 [k]); unmatched: one that receives every sub-batch's unmatched-block flags (uint8
    [k,Hb,Wb], 1 where a block found no match and passed unfiltered), both on the input's device."""
    return _stabilize_with_motion(engine.motion_depth, engine._motion_args, depth, image, state, alpha, motion_threshold, cut_threshold,
                                  search_range, smoothness, match_threshold, batch_size, cuts, unmatched)


def stabilize_depth_motion_pyramid(depth, image, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=64,
                                   smoothness=32, match_threshold=12, batch_size=16, cuts=None, unmatched=None):
    """stabilize_depth_motion with the motion found coarse to fine on a three-level luma pyramid (engine.motion_depth_pyramid,
    cs_motion_depth_pyramid), for motion beyond the full search's 32 pixels: search_range is a multiple of 4 in 4..120 and the
    vectors reach search_range + 3 pixels at the depth's resolution.  Every other argument, the resize of an image at another size,
    the sub-batches, the state (an engine.MotionState), cuts, unmatched and the returns are stabilize_depth_motion's.  The
    defaults are starting values that nobody has tuned on footage."""
    return _stabilize_with_motion(engine.motion_depth_pyramid, engine._pyramid_args, depth, image, state, alpha, motion_threshold,
                                  cut_threshold, search_range, smoothness, match_threshold, batch_size, cuts, unmatched)


def _stabilize_with_motion(motion_depth, check_args, depth, image, state, alpha, motion_threshold, cut_threshold, search_range, smoothness,
                           match_threshold, batch_size, cuts, unmatched):
    """stabilize_depth_motion and stabilize_depth_motion_pyramid: the engine function and the refusals of its three integer
    parameters are what differs."""
    frames = _DepthFrames(depth).in_batches_of(batch_size)
    if not isinstance(image, torch.Tensor):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dim() != 4 or image.shape[3] != 3 or image.numel() == 0:
        raise ValueError(f"image must be a non-empty [N,H,W,3], got shape {tuple(image.shape)}")
    if frames.n != image.shape[0]:
        raise ValueError(f"image has {image.shape[0]} frames, depth has {frames.n}")
    if frames.depth.device != image.device:
        raise ValueError("image and depth must be on the same device")
    check_args(search_range, smoothness, match_threshold)   # (the refusals, before anything is uploaded)
    h, w = frames.d4.shape[1:3]

    def filtered(b0, b1, chunk, img):
        nonlocal state
        if tuple(img.shape[1:3]) != (h, w):
            img = engine.pil_resize(img, (w, h), f32="nhwc", codes=True)[1]
        y, _, cut, state, _, matched = motion_depth(chunk, img, state, alpha, motion_threshold, cut_threshold, search_range, smoothness,
                                                    match_threshold)
        return y, cut, 1 - matched

    y, flags = frames.run(filtered, beside=(image,))
    if cuts is not None:
        cuts.extend(cut for cut, _ in flags)
    if unmatched is not None:
        unmatched.extend(un for _, un in flags)
    return y, state


# ---- depth range clipping of a video batch (cs_depth_range) ------------------------------------------------
def clip_depth_range(depth, state=None, clip_low=0.005, clip_high=0.005, beta=1.0, normalize=False, batch_size=16, cuts=None,
                     bounds=None):
    """Percentile clipping of the near and far end of the depth maps of a clip, with the two bounds smoothed over time, run in
    front of the stereo step (behind stabilize_depth, if that runs).  depth: a host or device tensor [N,H,W] or [N,H,W,C] (other
    dtypes are converted to float32) -> (the clamped depth in the input's layout, on the input's device, float32; state).
    [N,H,W] and one channel keep their shape, any other C gets y in all of its channels.  clip_low / clip_high: the fractions of
    the pixels below / above the bounds, 0 <= clip < 0.5; beta: the weight of a frame's own bounds against the preceding
    frame's, 1 = no smoothing; normalize: map [lo, hi] to 0..1.  state: what an earlier call returned for the clip's earlier
    frames (engine.RangeState, kept on the device), or None.  Host input is uploaded in sub-batches of at most batch_size frames
    with the state carried on the device; the result is bit for bit the one of a single call.  cuts: the list stabilize_depth
    filled for the same frames (int32 flags, in any split): the bounds restart at every flagged frame.  bounds: a list that
    receives every sub-batch's (lo, hi, raw_lo, raw_hi), float32 [k] on the input's device."""
    frames = _DepthFrames(depth).in_batches_of(batch_size)
    engine.clip_ranks(clip_low, clip_high, 1)   # (the fractions' refusal, before anything is uploaded)
    cut = None
    if cuts is not None:
        cut = torch.cat([torch.as_tensor(k).reshape(-1) for k in cuts]) if len(cuts) else torch.zeros((0,), dtype=torch.int32)
        if cut.numel() != frames.n:
            raise ValueError(f"cuts hold {cut.numel()} flags, depth has {frames.n} frames")
        cut = cut.to(_device_for(frames.depth), torch.int32)

    def clipped(b0, b1, chunk):
        nonlocal state
        *y_and_four, state = engine.depth_range(chunk, state, clip_low, clip_high, beta, None if cut is None else cut[b0:b1].contiguous(),
                                                normalize)
        return y_and_four

    y, fours = frames.run(clipped)
    if bounds is not None:
        bounds.extend(fours)
    return y, state


# ---- image-guided depth upsampling (cs_guided_depth_plan / cs_guided_depth_apply) --------------------------
def upsample_depth_guided(image, depth, radius=2, sigma_s=1.0, sigma_r=0.1, batch_size=16):
    """Joint bilateral upsampling of depth maps to their frames' size, guided by the frames, run in front of the stereo step
    (behind stabilize_depth and clip_depth_range, which are cheaper at the estimator's resolution).  image: a host or device
    tensor [N,H,W,3], the frames; depth: [N,dh,dw] or [N,dh,dw,C] with dh <= H and dw <= W, where image is (other dtypes are
    converted to float32) -> the depth at H x W, float32, on the input's device: [N,dh,dw] gives [N,H,W], [N,dh,dw,C] gives
    [N,H,W,C] with the result in every channel.  radius: 1, 2 or 3 (K = 2 radius + 1 taps per axis); sigma_s: the spatial
    Gaussian's width in low-resolution pixels; sigma_r: the range Gaussian's width in units of the summed 8-bit colour difference
    over 255 (inf: no range term).  Host input is uploaded in sub-batches of at most batch_size frames; the plan is made once."""
    if not isinstance(image, torch.Tensor):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dim() != 4 or image.shape[3] != 3 or image.numel() == 0:
        raise ValueError(f"image must be a non-empty [N,H,W,3], got shape {tuple(image.shape)}")
    frames = _DepthFrames(depth, "[N,dh,dw]")
    if frames.n != image.shape[0]:
        raise ValueError(f"image has {image.shape[0]} frames, depth has {frames.n}")
    if frames.depth.device != image.device:
        raise ValueError("image and depth must be on the same device")
    frames.in_batches_of(batch_size)
    h, w = image.shape[1:3]
    dh, dw = frames.d4.shape[1:3]
    engine._guided_geometry(h, w, dh, dw, radius)   # (the refusals, before anything is uploaded)
    engine._guided_sigmas(sigma_s, sigma_r)
    plan = engine.guided_depth_plan(h, w, dh, dw, radius, sigma_s, sigma_r, device=_device_for(frames.depth))
    return frames.run(lambda b0, b1, d, img: (engine.guided_depth(img, d, plan),), beside=(image,))[0]


# ---- foreground depth edge dilation (cs_depth_dilate) -------------------------------------------------------
def dilate_depth_edges(depth, radius=2, shape="disc", near="bright", threshold=0.04, batch_size=16):
    """Grows the near surface of the depth maps outward by `radius` pixels at depth discontinuities, so the anti-aliased rim of an
    object travels with the object in the warp and not with the background.  The last pre-pass in front of the stereo step, at
    the frame's resolution (behind upsample_depth_guided, if that runs).  depth: a host or device tensor [N,H,W] or [N,H,W,C]
    (other dtypes are converted to float32) -> the dilated depth in the input's layout, on the input's device, float32: [N,H,W]
    and one channel keep their shape, any other C gets y in all of its channels.  radius: 1..8; shape: 'disc' or 'square'; near:
    'bright' where larger values are nearer (ComfyUI's depth maps), 'dark' otherwise; threshold >= 0: a pixel takes its window's
    nearest value only where that lies at least this far in front of it (0: plain dilation; +inf: nothing moves).  Every frame on
    its own; host input is uploaded in sub-batches of at most batch_size frames."""
    frames = _DepthFrames(depth).in_batches_of(batch_size)
    engine._dilate_args(radius, shape, near, threshold)   # (the refusals, before anything is uploaded)
    return frames.run(lambda b0, b1, d: (engine.depth_dilate(d, radius, shape, near, threshold),))[0]
