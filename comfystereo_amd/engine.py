"""Device-side engine: thin torch-tensor wrappers over the C ABI (libcomfystereo_hip.so).

Everything here takes and returns tensors that live on the MI355X (`cuda` device in PyTorch-ROCm);
PyTorch only provides the memory and the stream -- the arithmetic is in the HIP kernels.
"""
import copy
import ctypes
import math

import numpy as np
import torch

from . import _native
from ._native import FILL, MODE, Params


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _opt_ptr(t):
    return None if t is None else _ptr(t)


# ---- the wrappers' vocabulary: one refusal of a tensor, one device check, one workspace, one guarded launch ------------------------
_DTYPE_NAMES = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}   # keys of _native's dtype enums
_FLOATS = tuple(_DTYPE_NAMES)
_FLOATS_TEXT = "float32, float16 or bfloat16"


def _tensor(name, t, **checks):
    """The one refusal of a tensor argument: ValueError unless `t` is a torch.Tensor that passes `checks`.  They run in the order
    their keywords are written, which decides the fault reported for an argument that is bad in several ways:
      dims=(counts, what), shape=(shape, what)   "<name> must <what> <t's shape>"
      dtypes=(dtypes, what)                      "<name> must be <what>, got <t's dtype>"
      like=(dtype, message)                      message, its {got} filled with t's dtype
      not_empty=label                            "empty <label> <t's shape>"
      contiguous=True                            "<name> must be contiguous"
      no_grad=why                                "<name> requires grad: <why>" (why may be empty)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor")
    for check, want in checks.items():
        if check == "dims" and t.dim() not in want[0] or check == "shape" and tuple(t.shape) != tuple(want[0]):
            raise ValueError(f"{name} must {want[1]} {tuple(t.shape)}")
        if check == "dtypes" and t.dtype not in want[0]:
            raise ValueError(f"{name} must be {want[1]}, got {t.dtype}")
        if check == "like" and t.dtype != want[0]:
            raise ValueError(want[1].format(got=t.dtype))
        if check == "not_empty" and t.numel() == 0:
            raise ValueError(f"empty {want} {tuple(t.shape)}")
        if check == "contiguous" and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if check == "no_grad" and t.requires_grad:
            raise ValueError(f"{name} requires grad" + (f": {want}" if want else ""))
    return t


def _on_gpu(t, no_gpu_error=False):
    """`t` lives on the GPU, or ValueError.  no_gpu_error: where there is no GPU at all, the package's RuntimeError instead (the
    wrappers that run this after their argument checks).  -> t"""
    if not t.is_cuda:
        if no_gpu_error and not torch.cuda.is_available():
            raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
        raise ValueError("comfystereo_amd engine calls need device-resident tensors (there is no CPU path)")
    return t


def _same_device(first, *named, msg=None):
    """Every (name, tensor) of `named` lives where the tensor of `first` does, or ValueError."""
    for name, t in named:
        if t.device != first[1].device:
            raise ValueError(msg or f"{first[0]} and {name} must be on the same device")


def _workspace(nbytes, device, pass_floor=False):
    """The scratch of one call: at least 256 bytes -> (uint8 tensor, the byte count the native call is given: what the library
    asked for, or with pass_floor what was allocated)."""
    size = max(nbytes, 256)
    return torch.empty((size,), dtype=torch.uint8, device=device), size if pass_floor else nbytes


def _launch(device, fn, *args):
    """fn(*args, stream) on `device` -- the device of the call's tensors, whichever device is current -- and on that device's
    current stream; NativeError unless it returns CS_OK."""
    with torch.cuda.device(device):
        _native.check(fn(*args, _stream()))


def _like_x(name, t, x, shape, what, no_grad=""):
    """A tensor that goes with `x` in an in-place step: x's dtype, this shape ("<name> must <what> <t's shape>"), contiguous, no
    grad."""
    _tensor(name, t, like=(x.dtype, f"x and {name} must share one dtype, got {x.dtype} and {{got}}"), shape=(shape, what), contiguous=True,
            no_grad=no_grad)


def _numbers(lead, coeffs, names, counted=False):
    """`lead` (guidance, or nothing) and `coeffs`, as many as `names`, as finite floats, or ValueError.  counted: the wording of
    the DDIM wrappers, which name the count they got, show the values as a list and let float()'s own ValueError through."""
    def wanted(got=""):
        return f"coeffs must be {('two', 'three', 'four')[len(names) - 2]} numbers ({', '.join(names)}){got}"
    try:
        vals = [float(v) for v in lead] + [float(c) for c in coeffs]
    except (TypeError,) if counted else (TypeError, ValueError):
        raise ValueError(wanted()) from None
    if len(vals) != len(lead) + len(names):
        raise ValueError(wanted(f", got {len(vals) - len(lead)}" if counted else ""))
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{'guidance and ' if lead else ''}coeffs must be finite, got {vals if counted else tuple(vals)}")
    return vals


def _dtype_code(t, table):
    """t's dtype in one of the library's dtype enums (_native.ATTN_DTYPE, _native.LATENT_DTYPE)."""
    return table[_DTYPE_NAMES[t.dtype]]


# The reference picks its gpu_warp implementation at import time: forward_warp_mesh when `moderngl` is importable,
# forward_warp_gpu otherwise (stereoimage_generation.py:18-24, :1068-1071).  Here both are HIP kernels and the choice is
# this switch (cs_params.flags bit 2): False = forward_warp_gpu semantics (the parity-pinned default), True = mesh quality.
MESH_WARP = False
# Arithmetic dialect of the CPU techniques (cs_params.flags bits 3 / 4): "D32" = the reference as it runs WITHOUT numba
# (float32 disparities, wrapping uint8 pixel sums) -- what the goldens pin; "D64" = the typing numba gives the same
# source lines (float64 disparities, int64 sums), available for none / naive /
# naive_interpolating / inverse.
DIALECT = "D32"
DIALECTS = {"D32": 0, "D64": 3, "f64-disparity": 1, "int64-sum": 2}


def make_params(n, h, w, depth_h, depth_w, depth_c, fill, mode, divergence, separation, stereo_balance,
                convergence_point, stereo_offset_exponent, depth_map_blur, depth_blur_strength,
                depth_blur_edge_threshold, depth_blur_falloff, depth_blur_vert_smooth, batch_size):
    if mode not in MODE:
        raise ValueError(f"Unknown mode: {mode}")
    p = Params()
    p.n, p.h, p.w, p.depth_h, p.depth_w, p.depth_c = n, h, w, depth_h, depth_w, depth_c
    p.fill, p.mode, p.batch_size = FILL[fill], MODE[mode], int(batch_size)
    p.depth_map_blur, p.depth_blur_vert_smooth = int(bool(depth_map_blur)), int(depth_blur_vert_smooth)
    p.divergence, p.separation, p.stereo_balance = float(divergence), float(separation), float(stereo_balance)
    p.convergence_point, p.stereo_offset_exponent = float(convergence_point), float(stereo_offset_exponent)
    p.depth_blur_strength, p.depth_blur_edge_threshold = float(depth_blur_strength), float(depth_blur_edge_threshold)
    p.depth_blur_falloff = float(depth_blur_falloff)
    if MESH_WARP and fill == 'gpu_warp':
        p.flags |= 4
    if DIALECT != "D32":
        p.flags |= DIALECTS[DIALECT] << 3   # (cs_generate refuses techniques without a D64 instantiation)
    return p


def output_shape(p):
    L = _native.lib()
    oh, ow, mh, mw = (ctypes.c_int() for _ in range(4))
    _native.check(L.cs_output_shape(ctypes.byref(p), ctypes.byref(oh), ctypes.byref(ow), ctypes.byref(mh), ctypes.byref(mw)))
    return oh.value, ow.value, mh.value, mw.value


class Plan:
    """Pre-allocated outputs + workspace for repeated calls of one configuration (what bench.py times)."""

    def __init__(self, p, device, stereo_u8=False, tie_pool_bytes=0):
        """stereo_u8: the stereoscope is produced as its uint8 codes k (value k/255, CPU techniques only) --
        the compact form frame shards are all-gathered in; expand with `expand_u8`.
        tie_pool_bytes: workspace beyond cs_workspace_bytes; the polylines techniques add it to the pool their order-dependent
        rows export their stretches through (4 KB per image row by default: enough for saturated depth maps; a batch whose
        every row is ONE stretch -- depth noise, blur off -- needs 6 B per pixel and eye to keep all rows off the in-row replay)."""
        L = _native.lib()
        self.p = p
        if stereo_u8:
            p.flags |= 2
        oh, ow, mh, mw = output_shape(p)
        f32 = dict(dtype=torch.float32, device=device)
        self.stereo = torch.empty((p.n, oh, ow, 3), dtype=torch.uint8 if stereo_u8 else torch.float32, device=device)
        self.depth_l = torch.empty((p.n, p.h, p.w, 3), **f32)
        self.depth_r = torch.empty((p.n, p.h, p.w, 3), **f32)
        self.mask = torch.empty((p.n, mh, mw), **f32)
        self.ws_bytes = L.cs_workspace_bytes(ctypes.byref(p)) + int(tie_pool_bytes)
        self.ws, _ = _workspace(self.ws_bytes, device)

    def run(self, image, depth):
        _launch(self.ws.device, _native.lib().cs_generate, ctypes.byref(self.p), _ptr(image), _ptr(depth), _ptr(self.stereo),
                _ptr(self.depth_l), _ptr(self.depth_r), _ptr(self.mask), _ptr(self.ws), self.ws_bytes)
        return self.stereo, self.depth_l, self.depth_r, self.mask

    def stats(self):
        """Per-frame diagnostics words (see cs_common.h ST_*), e.g. polylines rows replayed sequentially, or the gpu_warp kernel
        instantiation that ran (column _native.ST_WARP_PATH, codes _native.WARP_PATH)."""
        return self.ws[: self.p.n * 64].view(torch.int32).view(self.p.n, 16).cpu()


def expand_u8(codes, out=None):
    """uint8 codes -> float32 k/255 on the device (true division, like the reference's np2tensor)."""
    L = _native.lib()
    codes = _on_gpu(codes).contiguous()
    if codes.dtype != torch.uint8:
        raise ValueError("codes must be uint8")
    if out is None:
        out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    _launch(codes.device, L.cs_expand_u8, _ptr(codes), _ptr(out), codes.numel())
    return out


def generate(image, depth_map, divergence, separation, modes, stereo_balance, convergence_point,
             stereo_offset_exponent, fill, depth_blur_edge_threshold, depth_blur_strength, depth_map_blur,
             depth_blur_falloff=1.0, depth_blur_vert_smooth=0, batch_size=4):
    """Fused batch path on device tensors: image [N,H,W,3], depth_map [N,H',W',C] float32 -> 4 device tensors."""
    image = _on_gpu(image).contiguous().float()
    depth_map = _on_gpu(depth_map).contiguous().float()
    n, h, w, c = image.shape
    if c != 3:
        raise ValueError("image must be [N,H,W,3]")
    p = make_params(n, h, w, depth_map.shape[1], depth_map.shape[2], depth_map.shape[3], fill, modes, divergence,
                    separation, stereo_balance, convergence_point, stereo_offset_exponent, depth_map_blur,
                    depth_blur_strength, depth_blur_edge_threshold, depth_blur_falloff, depth_blur_vert_smooth, batch_size)
    return Plan(p, image.device).run(image, depth_map)


def apply_stereo_divergence(image_u8, depth, divergence, separation, stereo_offset_exponent, fill, convergence_point=0.5,
                            dialect="D32"):
    """reference stereoimage_generation.py:1576-1620 for [N,H,W,3] uint8 + [N,H,W] float32 device tensors.
    dialect: "D32" = the reference without numba (the pinned contract); "D64" = numba's typing (float64 disparities,
    int64 pixel sums; for polylines_soft / polylines_sharp float64 point coordinates and the float64 sweep -- a literal
    one-lane replay per row, ~100x slower than D32); none / naive / naive_interpolating / inverse / polylines_* / hybrid_edge only."""
    L = _native.lib()
    image_u8 = _on_gpu(image_u8).contiguous()
    depth = _on_gpu(depth).contiguous().float()
    if image_u8.dtype != torch.uint8:
        raise ValueError("image_u8 must be uint8")
    squeeze = image_u8.dim() == 3
    if squeeze:
        image_u8, depth = image_u8[None], depth[None]
    n, h, w, _ = image_u8.shape
    out = torch.empty_like(image_u8)
    ws, nb = _workspace(L.cs_asd_workspace_bytes_for(n, h, w, FILL[fill]), image_u8.device)
    _launch(image_u8.device, L.cs_apply_stereo_divergence2, _ptr(image_u8), _ptr(depth), n, h, w, float(divergence), float(separation),
            float(stereo_offset_exponent), FILL[fill], float(convergence_point), DIALECTS[dialect], _ptr(out), _ptr(ws), nb)
    return out[0] if squeeze else out


def _directional_blur(entry, workspace_bytes, depth, scalars):
    """The two directional blurs on a device tensor [N,H,W] (or [H,W]).  scalars(): the call's five numbers, converted at the
    point and in the order the wrapper always converted them (which of two bad numbers is reported).  -> (left, right)"""
    L = _native.lib()
    shp = depth.shape
    d3 = depth.reshape((-1,) + tuple(shp[-2:]))
    n, h, w = d3.shape
    out_l, out_r = torch.empty_like(d3), torch.empty_like(d3)
    ws, nb = _workspace(getattr(L, workspace_bytes)(n, h, w), depth.device)
    _launch(depth.device, getattr(L, entry), _ptr(d3), n, h, w, *scalars(), _ptr(out_l), _ptr(out_r), _ptr(ws), nb)
    return out_l.reshape(shp), out_r.reshape(shp)


def directional_blur(depth, blur_strength, edge_threshold, falloff_exponent=1.0, vert_smooth_px=0, blur_mask_width=None):
    """reference stereoimage_generation.py:1171-1251 for a [N,H,W] (or [H,W]) float32 device tensor, 0..255 scale.
    blur_mask_width: reach of the blur weights from an edge (default: the blur strength, like the reference's callers)."""
    _native.lib()

    def scalars():
        mw = float(blur_strength if blur_mask_width is None else blur_mask_width)
        return float(blur_strength), float(edge_threshold), mw, float(falloff_exponent), int(vert_smooth_px)
    return _directional_blur("cs_directional_blur", "cs_blur_workspace_bytes", _on_gpu(depth).contiguous().float(), scalars)


def directional_blur_scipy(depth, blur_strength, edge_threshold, blur_mask_width=5, falloff_exponent=1.0, vert_smooth_px=0):
    """reference stereoimage_generation.py:1346-1419 (`directional_motion_blur`, the scipy blur of the numpy / PIL input path)
    for a [N,H,W] (or [H,W]) float32 device tensor, used as given (no 0..255 rescaling) -> (left, right)."""
    _native.lib()
    depth = _on_gpu(depth).contiguous().float()
    if blur_strength <= 0:   # (:1374)
        return depth, depth
    return _directional_blur("cs_directional_blur_scipy", "cs_blur_scipy_workspace_bytes", depth, lambda: (
        float(blur_strength), float(edge_threshold), float(blur_mask_width), float(falloff_exponent), int(vert_smooth_px)))


def _forward_warp(entry, workspace_bytes, image, depth, floats, ints=()):
    """The two forward warps: image [B,3,H,W], depth [B,H,W] on the device -> (warped, gap mask bool)."""
    L = _native.lib()
    image = _on_gpu(image).contiguous().float()
    depth = _on_gpu(depth).contiguous().float()
    b, c, h, w = image.shape
    if c != 3:
        raise ValueError("image must have 3 channels ([B,3,H,W])")
    warped = torch.empty_like(image)
    mask = torch.empty((b, h, w), dtype=torch.uint8, device=image.device)
    ws, nb = _workspace(getattr(L, workspace_bytes)(b, h, w), image.device)
    _launch(image.device, getattr(L, entry), _ptr(image), _ptr(depth), b, h, w, *[float(v) for v in floats], *[int(v) for v in ints],
            _ptr(warped), _ptr(mask), _ptr(ws), nb)
    return warped, mask.bool()


def forward_warp(image, depth, divergence_px, separation_px, stereo_offset_exponent, convergence_point=0.5,
                 gradient_threshold=1.5, max_stretch=8):
    """reference stereoimage_generation.py:277-450: image [B,3,H,W], depth [B,H,W] -> (warped, gap mask bool)."""
    return _forward_warp("cs_forward_warp2", "cs_warp_workspace_bytes", image, depth, (divergence_px, separation_px,
                         stereo_offset_exponent, convergence_point, gradient_threshold), (max_stretch,))


def forward_warp_mesh(image, depth, divergence_px, separation_px, stereo_offset_exponent, convergence_point=0.5,
                      gradient_threshold=1.5):
    """reference stereoimage_generation.py:453-689 (the mesh-quality warp): image [B,3,H,W], depth [B,H,W] ->
    (warped, gap mask bool)."""
    return _forward_warp("cs_forward_warp_mesh", "cs_warp_mesh_workspace_bytes", image, depth, (divergence_px, separation_px,
                         stereo_offset_exponent, convergence_point, gradient_threshold))


def stereo_shift(input_images, depthmaps, scale_factor=8.0, shift_both=False, stereo_offset_exponent=1.0):
    """reference stereo_utils.py:15-88 for device tensors: input [B,C,H,W], depth [B,H,W] float32 -> [2B,C,H,W]."""
    L = _native.lib()
    x = _on_gpu(input_images).contiguous().float()
    d = _on_gpu(depthmaps).contiguous().float()
    b, c, h, w = x.shape
    if tuple(d.shape) != (b, h, w):
        raise ValueError("depthmaps must be [B,H,W] like input_images [B,C,H,W]")
    out = torch.empty((2 * b, c, h, w), dtype=torch.float32, device=x.device)
    ws, nb = _workspace(L.cs_stereo_shift_workspace_bytes(), x.device)
    _launch(x.device, L.cs_stereo_shift, _ptr(x), _ptr(d), b, c, h, w, float(scale_factor), int(bool(shift_both)),
            float(stereo_offset_exponent), _ptr(out), _ptr(ws), nb)
    return out


def test_powf(x, y):
    L = _native.lib()
    x = _on_gpu(x).contiguous().float()
    out = torch.empty_like(x)
    _launch(x.device, L.cs_test_powf, _ptr(x), float(y), _ptr(out), x.numel())
    return out


def test_exp(x):
    L = _native.lib()
    x = _on_gpu(x).contiguous().double()
    out = torch.empty_like(x)
    _launch(x.device, L.cs_test_exp, _ptr(x), _ptr(out), x.numel())
    return out


# ---- the reference's grid-sample warps (cs_grid_warp, cs_interpolate_fill, cs_detect_disocclusions) -------------------------
def _grid_input(t, name, dims):
    """A float32, contiguous, device-resident tensor of `dims` dimensions, or ValueError."""
    _tensor(name, t, dims=((dims,), f"have {dims} dimensions, got shape"))
    if not (t.is_floating_point() or t.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)):
        raise ValueError(f"{name}: unsupported dtype {t.dtype}")
    return _on_gpu(t).to(torch.float32).contiguous()


def grid_warp(image, depth, divergence_px, separation_px, stereo_offset_exponent, convergence_point, op, padding="border"):
    """cs_grid_warp on device tensors: image [B,C,H,W] (ignored for op "mask"), depth [B,H,W] ->
    (warped float32 [B,C,H,W] or None, mask bool [B,H,W] or None).  op: "warp" (apply_stereo_divergence_gpu), "fill"
    (apply_stereo_divergence_gpu_with_fill: mask = valid), "mask" (compute_forward_mask_gpu), "stretch" (warp_and_fill_gpu)."""
    L = _native.lib()
    if op not in _native.GRID_OP or padding not in _native.GRID_PADDING:
        raise ValueError(f"unknown grid operation {op!r} / padding {padding!r}")
    depth = _grid_input(depth, "depth", 3)
    b, h, w = depth.shape
    c = 0
    if op != "mask":
        image = _grid_input(image, "image", 4)
        _same_device(("image", image), ("depth", depth))
        if image.shape[0] != b or tuple(image.shape[2:]) != (h, w):
            raise ValueError(f"image {tuple(image.shape)} and depth {tuple(depth.shape)} do not match ([B,C,H,W] / [B,H,W])")
        c = image.shape[1]
        if c < 1:
            raise ValueError("image has no channels")
    if b == 0 or h == 0 or w == 0:
        raise ValueError(f"empty depth {tuple(depth.shape)}")
    # (a frame wider than cs_grid_warp_max_width: the native call refuses it, NativeError CS_ELIMIT)
    warped = torch.empty((b, c, h, w), dtype=torch.float32, device=depth.device) if op != "mask" else None
    mask = torch.empty((b, h, w), dtype=torch.uint8, device=depth.device) if op != "warp" else None
    ws, nb = _workspace(L.cs_grid_warp_workspace_bytes(b, h, w), depth.device)
    _launch(depth.device, L.cs_grid_warp, _ptr(image) if warped is not None else None, _ptr(depth), b, c, h, w, float(divergence_px),
            float(separation_px), float(stereo_offset_exponent), float(convergence_point), _native.GRID_OP[op],
            _native.GRID_PADDING[padding], _opt_ptr(warped), _opt_ptr(mask), _ptr(ws), nb)
    return warped, (mask.bool() if mask is not None else None)


def interpolate_fill(image, mask):
    """cs_interpolate_fill: image [B,C,H,W], mask bool [B,H,W] (True = fill) -> filled float32 [B,C,H,W]."""
    L = _native.lib()
    image = _grid_input(image, "image", 4)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError("mask must be a bool tensor")
    if mask.dim() != 3 or mask.shape[0] != image.shape[0] or tuple(mask.shape[1:]) != tuple(image.shape[2:]):
        raise ValueError(f"mask {tuple(mask.shape)} does not match image {tuple(image.shape)} ([B,H,W] / [B,C,H,W])")
    mask = _on_gpu(mask).to(image.device).contiguous().view(torch.uint8)
    b, c, h, w = image.shape
    if image.numel() == 0:
        raise ValueError(f"empty image {tuple(image.shape)}")
    out = torch.empty_like(image)
    _launch(image.device, L.cs_interpolate_fill, _ptr(image), _ptr(mask), b, c, h, w, _ptr(out))
    return out


def detect_disocclusions(depth, grid, grid_x_warped, threshold=0.02):
    """cs_detect_disocclusions: depth [H,W], grid [1,H,W,2], grid_x_warped [H,W] -> bool [H,W]."""
    L = _native.lib()
    depth = _grid_input(depth, "depth", 2)
    grid = _grid_input(grid, "grid", 4)
    gxw = _grid_input(grid_x_warped, "grid_x_warped", 2)
    h, w = depth.shape
    if tuple(grid.shape) != (1, h, w, 2) or tuple(gxw.shape) != (h, w):
        raise ValueError(f"grid {tuple(grid.shape)} / grid_x_warped {tuple(gxw.shape)} do not match depth {(h, w)}")
    _same_device(("depth", depth), ("grid", grid), ("grid_x_warped", gxw), msg="depth, grid and grid_x_warped must be on the same device")
    if h == 0 or w < 2:
        raise ValueError(f"detect_disocclusions needs H >= 1 and W >= 2, got {(h, w)}")
    out = torch.empty((h, w), dtype=torch.uint8, device=depth.device)
    _launch(depth.device, L.cs_detect_disocclusions, _ptr(depth), _ptr(grid), _ptr(gxw), h, w, float(threshold), _ptr(out))
    return out.bool()


# ---- the reference's Gaussian depth blurs (cs_gaussian_blur) ------------------------------------------
def gaussian_taps(sigma):
    """The reference's tap array (stereoimage_generation.py:1261-1264) for sigma > 0: 2 * int(3 * sigma) + 1 float64 values.
    Evaluated by numpy on the host, as the reference does: numpy's float64 exp is a SIMD routine that need not equal libm's or
    the device's, so the library takes the taps as data and never recomputes them."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError(f"gaussian_taps needs sigma > 0, got {sigma}")
    radius = int(3 * sigma)
    x = np.arange(-radius, radius + 1)
    k = np.exp(-(x ** 2) / (2 * sigma * sigma))
    k /= k.sum()
    return k


def gaussian_blur(depth, sigma, op="plain", edge_threshold=None):
    """cs_gaussian_blur on a float32 device tensor [H,W] or [B,H,W] (every frame on its own) -> float32 tensor of that shape.
    op: "plain" (blur_depth_map), "edge_selective", "left", "right" (the three blends of depth and blur, which need
    edge_threshold).  sigma <= 0 blurs nothing: "plain" returns a copy, the blends blend the depth with itself, as the
    reference does.  More taps than cs_gaussian_blur_max_taps(): NativeError CS_ELIMIT."""
    L = _native.lib()
    if op not in _native.GAUSS_OP:
        raise ValueError(f"unknown Gaussian blur operation {op!r}")
    # (_tensor checks in the order written: the ladder this wrapper always had)
    _tensor("depth", depth, dims=((2, 3), "be [H,W] or [B,H,W], got shape"), dtypes=((torch.float32,), "float32"), not_empty="depth")
    if op != "plain" and edge_threshold is None:
        raise ValueError(f"operation {op!r} needs an edge_threshold")
    depth = _on_gpu(depth).contiguous()
    taps = gaussian_taps(sigma) if sigma > 0 else np.ones(1)
    d3 = depth.reshape((-1,) + tuple(depth.shape[-2:]))
    n, h, w = d3.shape
    taps_dev = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).to(depth.device)
    out = torch.empty_like(d3)
    ws, nb = _workspace(L.cs_gaussian_blur_workspace_bytes(n, h, w, taps.shape[0]), depth.device)
    _launch(depth.device, L.cs_gaussian_blur, _native.GAUSS_OP[op], _ptr(d3), _ptr(taps_dev), taps.shape[0],
            float(edge_threshold) if edge_threshold is not None else 0.0, n, h, w, _ptr(out), _ptr(ws), nb)
    return out.reshape(depth.shape)


# ---- what the depth pre-passes share: the refusal of a frames argument, the state of a clip and its check -------------------------
def _frames(name, t, layout="[N,H,W,C]"):
    """The refusal of a pre-pass's frames argument (depth, or the guide image): float32 `layout`, not empty, contiguous, no grad.  -> t"""
    return _tensor(name, t, dims=((4,), f"be {layout}, got shape"), dtypes=((torch.float32,), "float32"), not_empty=name,
                   contiguous=True, no_grad="")


class _ClipState:
    """What a depth pre-pass carries from one call of a clip to the next: `shape`, the clip's frame size (h, w), and the device
    tensors a subclass makes in its constructor, `valid` (one int32, 0: no frame seen yet) among them.  The pass updates them in
    place."""

    def __init__(self, h, w):
        self.shape = (int(h), int(w))

    @property
    def tensors(self):
        return [t for t in vars(self).values() if isinstance(t, torch.Tensor)]

    @property
    def device(self):
        return self.valid.device

    def clone(self):
        return copy.deepcopy(self)   # (every tensor cloned, `shape` kept)


def _clip_state(kind, state, depth):
    """The state a call on `depth` [N,H,W,C] works with: a new one of `kind` for None (a clip's first frames), else `state`, or
    ValueError unless it is one of `kind`, for frames of depth's size and on depth's device."""
    h, w = depth.shape[1:3]
    if state is None:
        return kind(h, w, depth.device)
    if not isinstance(state, kind):
        raise ValueError(f"state must be a {kind.__name__} or None")
    if state.shape != (h, w):
        raise ValueError(f"state is for frames of {state.shape}, depth has {(h, w)}")
    _same_device(("depth", depth), *(("state", t) for t in state.tensors))
    return state


# ---- temporal depth stabilisation of a video batch (cs_temporal_depth) ----------------------------------
class TemporalState(_ClipState):
    """What cs_temporal_depth carries from one call to the next: prev_raw and prev, float32 [H,W] (the last frame's gray value
    and its filtered value), and `valid`, one int32 on the device (0: no frame seen yet).  temporal_depth updates it in place."""

    def __init__(self, h, w, device):
        super().__init__(h, w)
        self.prev_raw = torch.empty((h, w), dtype=torch.float32, device=device)
        self.prev = torch.empty((h, w), dtype=torch.float32, device=device)
        self.valid = torch.zeros((1,), dtype=torch.int32, device=device)


def temporal_depth(depth, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08):
    """cs_temporal_depth on a float32 device tensor [N,H,W,C] (C == 3: gray value, C == 1: the value, else channel 0) ->
    (y float32 [N,H,W], m float32 [N], cut int32 [N] of 0 / 1, state).  state: the TemporalState of the clip's earlier frames,
    updated in place and returned, or None for a clip's first frames (a new one is returned).  A clip fed in sub-batches gives
    bit for bit what one call gives.  Nothing waits for the device; a call with a given state can be captured into a graph."""
    L = _native.lib()
    _on_gpu(_frames("depth", depth), no_gpu_error=True)
    n, h, w, c = depth.shape
    state = _clip_state(TemporalState, state, depth)
    y = torch.empty((n, h, w), dtype=torch.float32, device=depth.device)
    m = torch.empty((n,), dtype=torch.float32, device=depth.device)
    cut = torch.empty((n,), dtype=torch.int32, device=depth.device)
    ws, nb = _workspace(L.cs_temporal_depth_workspace_bytes(n, h, w, c), depth.device)
    _launch(depth.device, L.cs_temporal_depth, _ptr(depth), n, h, w, c, float(alpha), float(motion_threshold), float(cut_threshold),
            _ptr(state.prev_raw), _ptr(state.prev), _ptr(state.valid), _ptr(y), _ptr(m), _ptr(cut), _ptr(ws), nb)
    return y, m, cut, state


# ---- motion-compensated temporal depth stabilisation of a video batch (cs_motion_depth) ----------------------
MOTION_BLOCK = 16
MOTION_RANGES = {"search_range": 32, "smoothness": 4096, "match_threshold": 255}   # each an integer from 0 to this


class MotionState(_ClipState):
    """What cs_motion_depth carries from one call to the next: prev_raw and prev, float32 [H,W] (the last frame's gray value and
    its filtered value), prev_luma, uint8 [H,W] (the luma of its colour frame), and `valid`, one int32 on the device (0: no frame
    seen yet).  motion_depth updates it in place."""

    def __init__(self, h, w, device):
        super().__init__(h, w)
        self.prev_raw = torch.empty((h, w), dtype=torch.float32, device=device)
        self.prev = torch.empty((h, w), dtype=torch.float32, device=device)
        self.prev_luma = torch.empty((h, w), dtype=torch.uint8, device=device)
        self.valid = torch.zeros((1,), dtype=torch.int32, device=device)


def _motion_args(search_range, smoothness, match_threshold):
    """The refusals of motion_depth's three integer parameters -> them as ints."""
    given = dict(search_range=search_range, smoothness=smoothness, match_threshold=match_threshold)
    for name, v in given.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not 0 <= int(v) <= MOTION_RANGES[name]:
            raise ValueError(f"{name} must be an integer in 0..{MOTION_RANGES[name]}, got {v}")
    return tuple(int(v) for v in given.values())


def _motion_guide(guide, depth):
    """The refusal of motion_depth's guide: float32 [N,H,W,3] with depth's N, H and W."""
    _frames("guide", guide, "[N,H,W,3]")
    if guide.shape[3] != 3 or tuple(guide.shape[:3]) != tuple(depth.shape[:3]):
        raise ValueError(f"guide must be [N,H,W,3] at the depth's size {tuple(depth.shape[:3])}, got shape {tuple(guide.shape)}")


def motion_depth(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32,
                 match_threshold=12):
    """motion_depth_detail without the SADs: -> (y, m, cut, state, vec, matched)."""
    return motion_depth_detail(depth, guide, state, alpha, motion_threshold, cut_threshold, search_range, smoothness, match_threshold)[:6]


def motion_depth_detail(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32,
                        match_threshold=12):
    """cs_motion_depth on float32 device tensors: depth [N,H,W,C] (C == 3: gray value, C == 1: the value, else channel 0) and
    guide [N,H,W,3], the clip's colour frames at the depth's size -> (y float32 [N,H,W], m float32 [N], cut int32 [N] of 0 / 1,
    state, vec int8 [N,Hb,Wb,2] of (dx, dy), matched uint8 [N,Hb,Wb] of 0 / 1, sad int32 [N,Hb,Wb]: the vectors' SADs),
    Hb = ceil(H / 16), Wb = ceil(W / 16).
    temporal_depth's filter with y_{t-1} read where the pixel's 16 x 16 block came from: a full-search block matcher on the guide's
    8-bit luma over |dx|, |dy| <= search_range (0..32), cost SAD + smoothness (|dx| + |dy|) (0..4096); a block whose SAD exceeds
    match_threshold (0..255) per pixel passes unfiltered.  The three defaults are starting values that nobody has tuned on
    footage.  state: the MotionState of the clip's earlier frames, updated in place and returned, or None for a clip's first
    frames (a new one is returned).  A clip fed in sub-batches gives bit for bit what one call gives; search_range 0 with
    match_threshold 255 gives temporal_depth's y, m, cut and float state.  Nothing waits for the device; a call with a given state
    can be captured into a graph."""
    _frames("depth", depth)
    _motion_guide(guide, depth)
    search_range, smoothness, match_threshold = _motion_args(search_range, smoothness, match_threshold)
    return _motion_launch("cs_motion_depth", depth, guide, state, alpha, motion_threshold, cut_threshold, search_range, smoothness,
                          match_threshold)


def _motion_launch(entry, depth, guide, state, alpha, motion_threshold, cut_threshold, search_range, smoothness, match_threshold):
    """What motion_depth_detail and motion_depth_pyramid_detail share behind their refusals: the device checks, the state, the
    outputs, the workspace of `entry` and its launch."""
    L = _native.lib()
    _on_gpu(depth, no_gpu_error=True)
    _same_device(("depth", depth), ("guide", guide))
    n, h, w, c = depth.shape
    state = _clip_state(MotionState, state, depth)
    dev = depth.device
    hb, wb = -(-h // MOTION_BLOCK), -(-w // MOTION_BLOCK)
    y = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    m = torch.empty((n,), dtype=torch.float32, device=dev)
    cut = torch.empty((n,), dtype=torch.int32, device=dev)
    vec = torch.empty((n, hb, wb, 2), dtype=torch.int8, device=dev)
    sad = torch.empty((n, hb, wb), dtype=torch.int32, device=dev)
    matched = torch.empty((n, hb, wb), dtype=torch.uint8, device=dev)
    ws, nb = _workspace(getattr(L, entry + "_workspace_bytes")(n, h, w, c, search_range), dev)
    _launch(dev, getattr(L, entry), _ptr(depth), _ptr(guide), n, h, w, c, float(alpha), float(motion_threshold), float(cut_threshold),
            search_range, smoothness, match_threshold, _ptr(state.prev_raw), _ptr(state.prev), _ptr(state.prev_luma), _ptr(state.valid),
            _ptr(y), _ptr(m), _ptr(cut), _ptr(vec), _ptr(sad), _ptr(matched), _ptr(ws), nb)
    return y, m, cut, state, vec, matched, sad


# ---- the same filter with a coarse-to-fine motion search (cs_motion_depth_pyramid) ---------------------------
PYRAMID_SEARCH = (4, 120, 4)   # search_range: from, to, step


def _pyramid_args(search_range, smoothness, match_threshold):
    """The refusals of motion_depth_pyramid's three integer parameters -> them as ints."""
    lo, hi, step = PYRAMID_SEARCH
    v = search_range
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not lo <= int(v) <= hi or int(v) % step:
        raise ValueError(f"search_range must be a multiple of {step} in {lo}..{hi}, got {v}")
    return (int(v),) + _motion_args(0, smoothness, match_threshold)[1:]


def motion_depth_pyramid(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=64, smoothness=32,
                         match_threshold=12):
    """motion_depth_pyramid_detail without the SADs: -> (y, m, cut, state, vec, matched)."""
    return motion_depth_pyramid_detail(depth, guide, state, alpha, motion_threshold, cut_threshold, search_range, smoothness,
                                       match_threshold)[:6]


def motion_depth_pyramid_detail(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=64,
                                smoothness=32, match_threshold=12):
    """cs_motion_depth_pyramid: motion_depth_detail's arguments, returns, filter and state (a MotionState: the two may continue
    each other's clip), with the vectors found coarse to fine on a three-level luma pyramid, so that they reach |dx|, |dy| <=
    search_range + 3, search_range a multiple of 4 in 4..120: a full search over search_range / 4 on the quarter-size luma, then at
    most 46 candidates per block on the half- and the full-size luma (twice the vectors of the block's parent and of the parent's
    four neighbours, +-1, and (0, 0)).  tools/motion_pyramid_oracle.py states it.  Unlike the full search it can miss the best
    vector: it follows what the coarse levels found.  The defaults are starting values that nobody has tuned on footage.  A clip
    fed in sub-batches gives bit for bit what one call gives; nothing waits for the device; a call with a given state can be
    captured into a graph."""
    _frames("depth", depth)
    _motion_guide(guide, depth)
    search_range, smoothness, match_threshold = _pyramid_args(search_range, smoothness, match_threshold)
    return _motion_launch("cs_motion_depth_pyramid", depth, guide, state, alpha, motion_threshold, cut_threshold, search_range, smoothness,
                          match_threshold)


# ---- depth range clipping of a video batch (cs_depth_range) ------------------------------------------------
class RangeState(_ClipState):
    """What cs_depth_range carries from one call to the next: lo and hi, one float32 each (the last frame's bounds), and `valid`,
    one int32 (0: no frame seen yet), all on the device.  `shape` is the frame size the clip has.  depth_range updates it in place."""

    def __init__(self, h, w, device):
        super().__init__(h, w)
        self.lo = torch.zeros((1,), dtype=torch.float32, device=device)
        self.hi = torch.zeros((1,), dtype=torch.float32, device=device)
        self.valid = torch.zeros((1,), dtype=torch.int32, device=device)


def clip_ranks(clip_low, clip_high, count):
    """The two 0-based ranks among `count` keys that the clip fractions stand for (float64, as tools/range_oracle.py states it):
    floor(clip_low * (count - 1)) and (count - 1) - floor(clip_high * (count - 1)); ValueError outside 0 <= clip < 0.5."""
    clip_low, clip_high = float(clip_low), float(clip_high)
    if not (0.0 <= clip_low < 0.5 and 0.0 <= clip_high < 0.5):
        raise ValueError(f"clip_low and clip_high must lie in [0, 0.5), got {clip_low} and {clip_high}")
    last = int(count) - 1
    return int(math.floor(clip_low * last)), last - int(math.floor(clip_high * last))


def depth_range(depth, state=None, clip_low=0.005, clip_high=0.005, beta=1.0, cut=None, normalize=False):
    """cs_depth_range on a float32 device tensor [N,H,W,C] (C == 3: gray value, C == 1: the value, else channel 0) ->
    (y float32 [N,H,W], lo, hi, raw_lo, raw_hi float32 [N], state).  raw_lo / raw_hi: per frame the values at the clip fractions'
    ranks (exact order statistics); lo / hi: those smoothed along t with weight beta, restarted where cut [N] (int32, device;
    what temporal_depth returns) is non-zero; y: the gray depth clamped to [lo, hi], and with normalize mapped to 0..1.  state:
    the RangeState of the clip's earlier frames, updated in place and returned, or None for a clip's first frames (a new one is
    returned).  A clip fed in sub-batches gives bit for bit what one call gives.  Nothing waits for the device; a call with a given
    state can be captured into a graph."""
    L = _native.lib()
    n, h, w, c = _frames("depth", depth).shape
    rank_lo, rank_hi = clip_ranks(clip_low, clip_high, h * w)
    beta = float(beta)
    if not 0.0 <= beta <= 1.0:
        raise ValueError(f"beta must lie in [0, 1], got {beta}")
    if cut is not None:
        _tensor("cut", cut, shape=((n,), f"be [{n}], one flag per frame, got shape"), dtypes=((torch.int32,), "int32"), contiguous=True)
    _on_gpu(depth, no_gpu_error=True)
    state = _clip_state(RangeState, state, depth)
    if cut is not None:
        _same_device(("depth", depth), ("cut", cut))
    y = torch.empty((n, h, w), dtype=torch.float32, device=depth.device)
    lo, hi, raw_lo, raw_hi = (torch.empty((n,), dtype=torch.float32, device=depth.device) for _ in range(4))
    ws, nb = _workspace(L.cs_depth_range_workspace_bytes(n, h, w, c), depth.device)
    _launch(depth.device, L.cs_depth_range, _ptr(depth), n, h, w, c, rank_lo, rank_hi, beta, int(bool(normalize)), _opt_ptr(cut),
            _ptr(state.lo), _ptr(state.hi), _ptr(state.valid), _ptr(y), _ptr(lo), _ptr(hi), _ptr(raw_lo), _ptr(raw_hi), _ptr(ws), nb)
    return y, lo, hi, raw_lo, raw_hi, state


# ---- image-guided depth upsampling (cs_guided_depth_plan / cs_guided_depth_apply) --------------------------
GUIDED_RADII = (1, 2, 3)
_GUIDED_WR_WORDS = 768   # the range table's block in the plan: 766 weights and two words of padding (cs_guideddepth.hip)


class GuidedPlan:
    """What cs_guided_depth_plan writes for one geometry (h, w, dh, dw, radius) and two sigmas: the taps' centres and spatial
    weights per column and row, the range table and the guide positions of the low-resolution samples, in one device buffer.
    Made once (guided_depth_plan) and read by every guided_depth call of that geometry.  The accessors return the blocks by
    value, whatever the buffer's byte layout: cx, cy int32 [w], [h]; wx, wy float32 [w,K], [h,K]; wr float32 [766]; gx, gy
    int32 [dw], [dh]."""

    def __init__(self, h, w, dh, dw, radius, sigma_s, sigma_r, buffer, nbytes):
        self.h, self.w, self.dh, self.dw, self.radius = h, w, dh, dw, radius
        self.sigma_s, self.sigma_r = sigma_s, sigma_r
        self.buffer, self.nbytes = buffer, nbytes

    @property
    def device(self):
        return self.buffer.device

    @property
    def taps(self):
        return 2 * self.radius + 1

    def _block(self, name):
        k = self.taps
        sizes = (("wr", _GUIDED_WR_WORDS), ("cx", self.w), ("cy", self.h), ("gx", self.dw), ("gy", self.dh), ("wx", self.w * k),
                 ("wy", self.h * k))
        at = 0
        for block, words in sizes:
            if block == name:
                return self.buffer[4 * at:4 * (at + words)]
            at += words
        raise KeyError(name)

    def _ints(self, name):
        return self._block(name).view(torch.int32).clone()

    def _floats(self, name):
        return self._block(name).view(torch.float32).clone()

    cx = property(lambda self: self._ints("cx"))
    cy = property(lambda self: self._ints("cy"))
    gx = property(lambda self: self._ints("gx"))
    gy = property(lambda self: self._ints("gy"))
    wx = property(lambda self: self._floats("wx").view(self.w, self.taps))
    wy = property(lambda self: self._floats("wy").view(self.h, self.taps))
    wr = property(lambda self: self._floats("wr")[:766])


def _guided_geometry(h, w, dh, dw, radius):
    h, w, dh, dw, radius = int(h), int(w), int(dh), int(dw), int(radius)
    if min(h, w, dh, dw) < 1:
        raise ValueError(f"the sizes must be positive, got an image of {(h, w)} and a depth map of {(dh, dw)}")
    if dh > h or dw > w:
        raise ValueError(f"the depth map {(dh, dw)} is larger than the image {(h, w)}: guided upsampling only enlarges")
    if radius not in GUIDED_RADII:
        raise ValueError(f"radius must be 1, 2 or 3, got {radius}")
    return h, w, dh, dw, radius


def _guided_sigmas(sigma_s, sigma_r):
    sigma_s, sigma_r = float(sigma_s), float(sigma_r)
    if not (sigma_s > 0.0 and sigma_r > 0.0):
        raise ValueError(f"sigma_s and sigma_r must be positive, got {sigma_s} and {sigma_r}")
    return sigma_s, sigma_r


def guided_depth_plan(h, w, dh, dw, radius=2, sigma_s=1.0, sigma_r=0.1, device=None):
    """cs_guided_depth_plan: the plan of the guided upsampling of depth maps of dh x dw to frames of h x w (dh <= h, dw <= w) ->
    GuidedPlan on `device` (None: the current GPU).  radius: 1, 2 or 3, K = 2 radius + 1 taps per axis; sigma_s > 0: the spatial
    Gaussian's width in low-resolution pixels; sigma_r > 0: the range Gaussian's width in units of the summed colour difference
    (inf: no range term, a pure spatial filter).  One small launch; nothing waits for the device."""
    L = _native.lib()
    h, w, dh, dw, radius = _guided_geometry(h, w, dh, dw, radius)
    sigma_s, sigma_r = _guided_sigmas(sigma_s, sigma_r)
    if not torch.cuda.is_available():
        raise RuntimeError("comfystereo_amd needs an MI355X (PyTorch-ROCm `cuda` device); there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError("comfystereo_amd engine calls need device-resident tensors (there is no CPU path)")
    buffer, nbytes = _workspace(L.cs_guided_depth_plan_bytes(h, w, dh, dw, radius), device)
    _launch(device, L.cs_guided_depth_plan, h, w, dh, dw, radius, sigma_s, sigma_r, _ptr(buffer), nbytes)
    return GuidedPlan(h, w, dh, dw, radius, sigma_s, sigma_r, buffer, nbytes)


def guided_depth(image, depth, plan):
    """cs_guided_depth_apply on float32 device tensors: image [N,H,W,3], the guide, and depth [N,dh,dw,C] (C == 3: gray value,
    C == 1: the value, else channel 0) -> float32 [N,H,W], the depth at the image's size with its edges on the image's edges.
    plan: the GuidedPlan of this geometry (guided_depth_plan), reused for every batch.  One launch; nothing waits for the device;
    a call can be captured into a graph."""
    L = _native.lib()
    _frames("image", image, "[N,H,W,3]")
    _frames("depth", depth, "[N,dh,dw,C]")
    n, h, w, ic = image.shape
    if ic != 3:
        raise ValueError(f"image must be [N,H,W,3], got shape {tuple(image.shape)}")
    if depth.shape[0] != n:
        raise ValueError(f"image has {n} frames, depth has {depth.shape[0]}")
    _, dh, dw, c = depth.shape
    if not isinstance(plan, GuidedPlan):
        raise ValueError("plan must be a GuidedPlan (guided_depth_plan)")
    if (plan.h, plan.w, plan.dh, plan.dw) != (h, w, dh, dw):
        raise ValueError(f"plan is for depth maps of {(plan.dh, plan.dw)} and frames of {(plan.h, plan.w)}, got {(dh, dw)} and {(h, w)}")
    _on_gpu(image, no_gpu_error=True)
    _same_device(("image", image), ("depth", depth), ("plan", plan.buffer))
    out = torch.empty((n, h, w), dtype=torch.float32, device=image.device)
    _launch(image.device, L.cs_guided_depth_apply, _ptr(image), _ptr(depth), n, h, w, dh, dw, c, plan.radius, _ptr(plan.buffer),
            plan.nbytes, _ptr(out))
    return out


# ---- foreground depth edge dilation (cs_depth_dilate) -------------------------------------------------------
DILATE_RADII = tuple(range(1, 9))


def _dilate_args(radius, shape, near, threshold):
    """The refusals of depth_dilate's parameters -> (radius, shape code, near code, threshold)."""
    if isinstance(radius, bool) or int(radius) != radius or int(radius) not in DILATE_RADII:
        raise ValueError(f"radius must be an integer in 1..8, got {radius}")
    if shape not in _native.DILATE_SHAPE:
        raise ValueError(f"shape must be 'square' or 'disc', got {shape!r}")
    if near not in _native.DILATE_NEAR:
        raise ValueError(f"near must be 'bright' or 'dark', got {near!r}")
    threshold = float(threshold)
    if not threshold >= 0.0:
        raise ValueError(f"threshold must be >= 0 (+inf allowed), got {threshold}")
    return int(radius), _native.DILATE_SHAPE[shape], _native.DILATE_NEAR[near], threshold


def depth_dilate(depth, radius=2, shape="disc", near="bright", threshold=0.04):
    """cs_depth_dilate on a float32 device tensor [N,H,W,C] (C == 3: gray value, C == 1: the value, else channel 0) -> y float32
    [N,H,W]: the near surface (near: 'bright' or 'dark' values) grown outward by `radius` pixels (1..8) over a 'square' or 'disc'
    window, where the window's nearest value is at least `threshold` in front of the pixel; every other pixel keeps its gray value
    bit for bit.  threshold 0 is plain grayscale dilation (dark: erosion).  One launch, no workspace; nothing waits for the device;
    a call can be captured into a graph."""
    L = _native.lib()
    n, h, w, c = _frames("depth", depth).shape
    radius, shape, near, threshold = _dilate_args(radius, shape, near, threshold)
    _on_gpu(depth, no_gpu_error=True)
    y = torch.empty((n, h, w), dtype=torch.float32, device=depth.device)
    _launch(depth.device, L.cs_depth_dilate, _ptr(depth), n, h, w, c, radius, shape, near, threshold, _ptr(y))
    return y


# ---- StereoDiffusion Fast mode's warp, inpaint mask and gap pre-fill (cs_inpaint_prepare) ---------------
def inpaint_prepare(image, depth, scale_factor, threshold=0.05, codes=False):
    """cs_inpaint_prepare on device tensors: image [B,3,H,W] (values k / 255), depth [B,H,W], every frame on its own ->
    (warped float32 [B,3,H,W], filled float32 [B,3,H,W], mask bool [B,H,W]), with codes=True followed by
    (warped_u8, filled_u8), uint8 [B,H,W,3]: trunc(value * 255), the images the reference hands to its inpainting model and
    blends the model's answer into.  scale_factor is the reference's (divergence_px = scale_factor / 100 * W).
    A frame wider than cs_inpaint_prepare_max_width(): NativeError CS_ELIMIT."""
    L = _native.lib()
    image = _grid_input(image, "image", 4)
    depth = _grid_input(depth, "depth", 3)
    _same_device(("image", image), ("depth", depth))
    b, h, w = depth.shape
    if image.shape[1] != 3 or image.shape[0] != b or tuple(image.shape[2:]) != (h, w):
        raise ValueError(f"image {tuple(image.shape)} and depth {tuple(depth.shape)} do not match ([B,3,H,W] / [B,H,W])")
    if b == 0 or h == 0 or w == 0:
        raise ValueError(f"empty depth {tuple(depth.shape)}")
    dev = depth.device
    warped = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    filled = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    mask = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    wu8 = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev) if codes else None
    fu8 = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev) if codes else None
    ws, nb = _workspace(L.cs_inpaint_prepare_workspace_bytes(b, h, w), dev)
    divergence_px = (float(scale_factor) / 100.0) * w
    _launch(dev, L.cs_inpaint_prepare, _ptr(image), _ptr(depth), b, h, w, divergence_px, float(threshold), _ptr(warped), _ptr(filled),
            _ptr(mask), _opt_ptr(wu8), _opt_ptr(fu8), _ptr(ws), nb)
    out = (warped, filled, mask.bool())
    return out + (wu8, fu8) if codes else out


# ---- Pillow's 8-bit bicubic resize with the Fast mode's code conversions (cs_pil_resize) ----------------
def pil_resize(x, size, gray=False, f32=None, codes=True, f32_out=None):
    """cs_pil_resize on a device tensor: x [N,H,W,C] (C 1 or 3) or [N,H,W], uint8 codes or float32 (codes
    trunc(clip(255 * x, 0, 255))); size = (width, height), PIL's order -> the uint8 codes [N,oh,ow,C] of
    PIL.Image.resize(size) (Pillow 12.2, all defaults), byte for byte.  gray=True: x has 3 channels, the result one, the
    Fast mode's gray of a coloured depth taken before the resize.
    f32: None, "nhwc" ([N,oh,ow,C]) or "planar" ([N,C,oh,ow]): also return code / 255 as float32 -> (codes, floats).
    codes=False: no uint8 result (None in its place).  f32_out: a float32 [N,oh,ow,C] destination for "nhwc" whose rows may be
    a slice of wider rows (one eye of a side-by-side frame).
    A reduction by more than a factor of 64, or a side above 65 535: NativeError CS_ELIMIT."""
    L = _native.lib()
    _tensor("x", x, dtypes=((torch.uint8, torch.float32), "uint8 or float32"))
    if x.dim() == 3:
        x = x.unsqueeze(-1)
    if x.dim() != 4 or x.shape[-1] not in (1, 3):
        raise ValueError(f"x must be [N,H,W,C] with C 1 or 3, or [N,H,W]; got shape {tuple(x.shape)}")
    if gray and x.shape[-1] != 3:
        raise ValueError("gray=True takes 3 channels")
    if f32 not in (None, "nhwc", "planar"):
        raise ValueError(f"f32 must be None, 'nhwc' or 'planar', got {f32!r}")
    if f32_out is not None and f32 != "nhwc":
        raise ValueError("f32_out needs f32='nhwc'")
    if not codes and f32 is None:
        raise ValueError("nothing asked for: codes=False without f32")
    ow, oh = (int(v) for v in size)
    if ow <= 0 or oh <= 0 or x.numel() == 0:
        raise ValueError(f"empty image: {tuple(x.shape)} -> {(oh, ow)}")
    x = _on_gpu(x).contiguous()
    n, h, w, c = x.shape
    co = 1 if gray else c
    dev = x.device
    out = torch.empty((n, oh, ow, co), dtype=torch.uint8, device=dev) if codes else None
    flt, pitch = None, 0
    if f32 == "planar":
        flt = torch.empty((n, co, oh, ow), dtype=torch.float32, device=dev)
    elif f32_out is not None:
        flt = f32_out
        if (not isinstance(flt, torch.Tensor) or flt.dtype != torch.float32 or flt.device != dev
                or tuple(flt.shape) != (n, oh, ow, co)):
            raise ValueError(f"f32_out must be a float32 tensor {(n, oh, ow, co)} on {dev}")
        st = flt.stride()
        pitch = st[1] if oh > 1 else (st[0] if n > 1 else ow * co)
        dense_pixels = (co == 1 or st[3] == 1) and (ow == 1 or st[2] == co)
        if not dense_pixels or pitch < ow * co or (n > 1 and oh > 1 and st[0] != oh * pitch):
            raise ValueError("f32_out must have dense pixels, and rows and frames one row pitch apart")
    elif f32 == "nhwc":
        flt = torch.empty((n, oh, ow, co), dtype=torch.float32, device=dev)
    flags = (_native.PIL_FLAG["in_f32"] if x.dtype == torch.float32 else 0) | (_native.PIL_FLAG["gray"] if gray else 0) | \
        (_native.PIL_FLAG["out_planar"] if f32 == "planar" else 0)
    ws, nb = _workspace(L.cs_pil_resize_workspace_bytes(n, h, w, c, oh, ow), dev, pass_floor=True)
    _launch(dev, L.cs_pil_resize, _ptr(x), n, h, w, c, oh, ow, flags, _opt_ptr(out), _opt_ptr(flt), pitch, _ptr(ws), nb)
    return out if f32 is None else (out, flt)


# ---- the reference's stereo attention (cs_stereo_attention) ---------------------------------------------
def _qkv_shapes(q, k, v):
    """q [B, n, d], k and v [B, n_k, d], none of them empty, or ValueError -> (B, n, n_k, d)"""
    bh, n, d = q.shape
    if k.shape != v.shape or k.shape[0] != bh or k.shape[2] != d:
        raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} do not match")
    n_k = k.shape[1]
    if bh == 0 or n == 0 or n_k == 0 or d == 0:
        raise ValueError(f"empty attention: q {tuple(q.shape)}, k {tuple(k.shape)}")
    return bh, n, n_k, d


def _head_dim_and_scale(d, half, scale, kernel):
    """The head dimension the attention kernels take and a finite scale, or ValueError."""
    d_max = _native.lib().cs_stereo_attention_max_head_dim()   # (host only: no device work)
    if d % (8 if half else 4) or d > d_max:
        raise ValueError(f"head dimension {d}: {kernel} takes multiples of 4 (float16 / bfloat16: of 8) up to {d_max}")
    if not math.isfinite(float(scale)):
        raise ValueError(f"scale must be finite, got {scale}")


def stereo_attention(q, k, v, heads, scale, mode, chunks=1, out=None):
    """cs_stereo_attention on float32 device tensors: q [(c s b h), n, d], k and v [(c s b h), n_k, d] -> [(c s b), n, h * d],
    softmax(scale * q k^T) v over the keys `mode` selects, in one fused kernel (no score matrix is ever written).
    mode: "self" (every batch entry sees its own keys; n_k may differ from n), "uni" (both views see the left view's keys) or
    "bi" (both views see both views' keys); "uni" / "bi" take two views (s = 2) and `chunks` = c CFG chunks, "self" takes
    the batch as it is.  heads = h.  out: an optional destination of the result's shape and the inputs' dtype.
    d must be a multiple of 4 up to cs_stereo_attention_max_head_dim(): ValueError before anything is launched.
    q, k, v all float16 or all bfloat16 go to cs_stereo_attention_half (half matrix operands, float32 scores, softmax and
    accumulators; the result has the inputs' dtype); there d must be a multiple of 8.  Mixed dtypes are a ValueError."""
    if mode not in _native.ATTN_MODE:
        raise ValueError(f"unknown attention mode {mode!r} (self, uni, bi)")
    # (_tensor checks in the order written: the ladder this wrapper always had)
    _tensor("q", q)
    for name, t in (("q", q), ("k", k), ("v", v)):
        _tensor(name, t, dims=((3,), "be [(c s b h), tokens, d], got shape"), dtypes=(_FLOATS, _FLOATS_TEXT),
                like=(q.dtype, f"q, k and v must share one dtype, got {q.dtype} and {{got}} ({name})"), contiguous=True,
                no_grad="cs_stereo_attention is forward only")
    half = q.dtype != torch.float32
    heads, chunks = int(heads), int(chunks)
    bh, n, n_k, d = _qkv_shapes(q, k, v)
    views = 1 if mode == "self" else 2
    if mode == "self":
        chunks = 1
    if heads <= 0 or chunks <= 0 or bh % (heads * views * chunks):
        raise ValueError(f"batch {bh} is not chunks * views * samples * heads = {chunks} * {views} * b * {heads}")
    if mode != "self" and n_k != n:
        raise ValueError(f"mode {mode!r} needs as many keys as queries per view, got {n_k} and {n}")
    _head_dim_and_scale(d, half, scale, "cs_stereo_attention")
    samples = bh // (heads * views * chunks)
    shape = (bh // heads, n, heads * d)
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != q.dtype or tuple(out.shape) != shape or not out.is_contiguous()
                or out.device != q.device):
            raise ValueError(f"out must be a contiguous {q.dtype} tensor {shape} on {q.device}")
    _on_gpu(q)
    _same_device(("q", q), ("k", k), ("v", v), msg="q, k and v must be on the same device")
    L = _native.lib()
    if out is None:
        out = torch.empty(shape, dtype=q.dtype, device=q.device)
    _launch(q.device, L.cs_stereo_attention_half if half else L.cs_stereo_attention, _ptr(q), _ptr(k), _ptr(v), _ptr(out),
            *([_dtype_code(q, _native.ATTN_DTYPE)] if half else []), chunks, views, samples, heads, n, n_k, d, float(scale),
            _native.ATTN_MODE[mode])
    return out


# ---- the differentiable fused attention (cs_attention_fwd_lse / cs_attention_bwd and their _half forms) -------------------
def _attention_grad_args(heads, scale, **tensors):
    """The checks of stereo_attention for the 'self' form: q [(b h), n, d], k and v [(b h), n_k, d] and, where given,
    out / d_out [(b), n, h * d] and lse [(b h), n].  q, k, v, out and d_out are all float32, all float16 or all bfloat16; lse is
    float32 whatever they are.  ValueError before anything is launched.  -> (b, h, n, n_k, d)"""
    # (_tensor checks in the order written: the ladder this wrapper always had)
    for name, t in tensors.items():
        _tensor(name, t)
    q, k, v = tensors["q"], tensors["k"], tensors["v"]
    _tensor("q", q, dtypes=(_FLOATS, _FLOATS_TEXT))
    for name, t in tensors.items():
        want = torch.float32 if name == "lse" else q.dtype
        _tensor(name, t, like=(want, f"{name} must be {want}" + ("" if name == "lse" else " like q (one dtype for q, k, v, out and d_out)")
                               + ", got {got}"), contiguous=True)
    half = q.dtype != torch.float32
    for name in ("q", "k", "v"):
        _tensor(name, tensors[name], dims=((3,), "be [(b h), tokens, d], got shape"))
    heads = int(heads)
    bh, n, n_k, d = _qkv_shapes(q, k, v)
    if heads <= 0 or bh % heads:
        raise ValueError(f"batch {bh} is not samples * heads = b * {heads}")
    _head_dim_and_scale(d, half, scale, "the fused attention")
    for name, shape in (("out", (bh // heads, n, heads * d)), ("d_out", (bh // heads, n, heads * d)), ("lse", (bh, n))):
        if name in tensors:
            _tensor(name, tensors[name], shape=(shape, f"have shape {shape}, got"))
    _on_gpu(q)
    _same_device(("q", q), *tensors.items(), msg="all tensors must be on the same device")
    return bh // heads, heads, n, n_k, d


def attention_lse(q, k, v, heads, scale):
    """cs_attention_fwd_lse: stereo_attention(q, k, v, heads, scale, "self") -- the same kernel, `out` bit for bit the same -- that
    also returns lse [(b h), n], the log-sum-exp of every query's scaled scores in log2 units: what attention_backward needs
    instead of the [(b h), n, n_k] probabilities.  q, k, v all float16 or all bfloat16 go to cs_attention_half_fwd_lse (d a multiple
    of 8): `out` has their dtype, lse stays float32.  Argument checks as in stereo_attention.  -> (out, lse)"""
    b, h, n, n_k, d = _attention_grad_args(heads, scale, q=q, k=k, v=v)
    out = torch.empty((b, n, h * d), dtype=q.dtype, device=q.device)
    lse = torch.empty((b * h, n), dtype=torch.float32, device=q.device)
    L = _native.lib()
    half = q.dtype != torch.float32
    _launch(q.device, L.cs_attention_half_fwd_lse if half else L.cs_attention_fwd_lse, _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse),
            *([_dtype_code(q, _native.ATTN_DTYPE)] if half else []), b, h, n, n_k, d, float(scale))
    return out, lse


def attention_backward(q, k, v, out, lse, d_out, heads, scale):
    """cs_attention_bwd: the gradients of sum(out * d_out) with respect to q, k and v, from attention_lse's out and lse.  The
    probabilities are recomputed tile by tile; the only scratch is one float per query.  No atomics: two calls on the same inputs
    return bit-identical tensors.  float16 / bfloat16 q, k, v, out, d_out (one dtype, lse float32) go to cs_attention_half_bwd and
    the gradients have that dtype.  -> (dq, dk, dv), shaped like q, k, v"""
    b, h, n, n_k, d = _attention_grad_args(heads, scale, q=q, k=k, v=v, out=out, lse=lse, d_out=d_out)
    L = _native.lib()
    half = q.dtype != torch.float32
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws, nb = _workspace((L.cs_attention_half_bwd_workspace_bytes if half else L.cs_attention_bwd_workspace_bytes)(b, h, n, n_k, d), q.device)
    _launch(q.device, L.cs_attention_half_bwd if half else L.cs_attention_bwd, _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse),
            _ptr(d_out), _ptr(dq), _ptr(dk), _ptr(dv), *([_dtype_code(q, _native.ATTN_DTYPE)] if half else []), b, h, n, n_k, d,
            float(scale), _ptr(ws), nb)
    return dq, dk, dv


class _DifferentiableAttention(torch.autograd.Function):
    """Saves q, k, v, out and lse -- O(n d), never the O(n n_k) probabilities autograd keeps for einsum / softmax / einsum.  The
    tensors keep the dtype they come in (float32, or one half dtype: attention_lse / attention_backward dispatch on it)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        out, lse = attention_lse(q, k, v, heads, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = attention_backward(q, k, v, out, lse, d_out.contiguous(), ctx.heads, ctx.scale)
        return dq, dk, dv, None, None


def differentiable_attention(q, k, v, heads, scale, native_half=False):
    """stereo_attention(q, k, v, heads, scale, "self") that autograd can differentiate: q [(b h), n, d], k and v [(b h), n_k, d] ->
    [(b), n, h * d].  float16 / bfloat16 q, k, v are upcast to float32 before the fused kernels and the result is cast back to q's
    dtype, as BNAttention's default path does (autograd differentiates the casts).  native_half=True: q, k, v of ONE half dtype with
    d a multiple of 8 run the half kernels instead (cs_attention_half_fwd_lse / cs_attention_half_bwd): no conversion pass, and what
    is saved for the backward is the half q, k, v, out plus the float32 lse; any other input keeps the upcast.  Gradients of
    gradients are not supported."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        _tensor(name, t, dtypes=(_FLOATS, _FLOATS_TEXT))
    if (native_half and q.dtype != torch.float32 and k.dtype == q.dtype and v.dtype == q.dtype and q.dim() == 3
            and q.shape[-1] % 8 == 0):
        return _DifferentiableAttention.apply(q.contiguous(), k.contiguous(), v.contiguous(), int(heads), float(scale))
    out = _DifferentiableAttention.apply(q.float().contiguous(), k.float().contiguous(), v.float().contiguous(), int(heads), float(scale))
    return out.to(q.dtype)


# ---- StereoDiffusion Standard mode's latent shift, mask and merge (cs_latent_shift_*, cs_decode_to_codes) ----
LATENT_MAX_WIDTH = 8192   # the columns cs_latent_shift_plan takes, and cs_standard_step with its tables (cs_latent.h LATENT_MAX_WIDTH)


def latent_shift_plan(disp, scale_factor, stereo_offset_exponent=1.0):
    """cs_latent_shift_plan on a device tensor: disp [B,H,W] float32, the disparity at the latents' size -> src_col int32
    [B,H,W]: for every destination column of the right view of stereo_shift_torch(latents, disp, scale_factor) the source
    column that ends up there, -1 in a hole.  Made once per image: the table does not depend on the latents."""
    # (_tensor checks in the order written: the ladder this wrapper always had)
    _tensor("disp", disp, dtypes=((torch.float32,), "float32 (the reference's disparity dtype)"), dims=((3,), "be [B,H,W], got shape"),
            not_empty="disp", contiguous=True)
    if not (math.isfinite(float(scale_factor)) and math.isfinite(float(stereo_offset_exponent))):
        raise ValueError(f"scale_factor and stereo_offset_exponent must be finite, got {scale_factor} and {stereo_offset_exponent}")
    b, h, w = disp.shape
    if w > LATENT_MAX_WIDTH:
        raise ValueError(f"rows of {w} columns: cs_latent_shift_plan takes up to {LATENT_MAX_WIDTH} (it is made for latents)")
    _on_gpu(disp, no_gpu_error=True)
    L = _native.lib()
    src_col = torch.empty((b, h, w), dtype=torch.int32, device=disp.device)
    ws, nb = _workspace(L.cs_latent_shift_plan_workspace_bytes(), disp.device, pass_floor=True)
    _launch(disp.device, L.cs_latent_shift_plan, _ptr(disp), b, h, w, float(scale_factor), float(stereo_offset_exponent), _ptr(src_col),
            _ptr(ws), nb)
    return src_col


def latent_shift_apply(left, right, src_col, mask, op, noise=None):
    """cs_latent_shift_apply on device tensors, in place on `right` and `mask`: left, right (and noise) [B,C,H,W] of one dtype
    (float32, float16, bfloat16), contiguous -- they may be the two halves of one [2B,C,H,W] tensor; src_col int32 [B,H,W] from
    latent_shift_plan; mask uint8 [B,H,W].
    op "first": right = left gathered through src_col (0 in a hole), mask = (channel 0 of that != 0), and with `noise` right =
    noise wherever the mask is 0.  op "reshift": right = left gathered wherever the mask "first" stored is 1; the rest of right
    stays.  Values are moved, never computed.  Returns right."""
    if op not in _native.LATENT_OP:
        raise ValueError(f"unknown op {op!r} (first, reshift)")
    if noise is not None and op != "first":
        raise ValueError("noise goes with op 'first' only")
    tensors = [("left", left), ("right", right)] + ([("noise", noise)] if noise is not None else [])
    # (_tensor checks in the order written: the ladder this wrapper always had)
    like_left = f"be [B,C,H,W] like left {tuple(_tensor('left', left).shape)}, got shape"
    for name, t in tensors:
        _tensor(name, t, dtypes=(_FLOATS, _FLOATS_TEXT),
                like=(left.dtype, f"left, right and noise must share one dtype, got {left.dtype} and {{got}} ({name})"),
                dims=((4,), like_left), shape=(left.shape, like_left), contiguous=True, no_grad="cs_latent_shift_apply works in place")
    b, c, h, w = left.shape
    if left.numel() == 0:
        raise ValueError(f"empty latents {tuple(left.shape)}")
    if not isinstance(src_col, torch.Tensor) or src_col.dtype != torch.int32 or tuple(src_col.shape) != (b, h, w) or not src_col.is_contiguous():
        raise ValueError(f"src_col must be a contiguous int32 tensor {(b, h, w)} (latent_shift_plan's)")
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != (b, h, w) or not mask.is_contiguous():
        raise ValueError(f"mask must be a contiguous uint8 tensor {(b, h, w)}")
    _same_device(("left", left), *tensors[1:], ("src_col", src_col), ("mask", mask))
    _on_gpu(left, no_gpu_error=True)
    _launch(left.device, _native.lib().cs_latent_shift_apply, _ptr(left), _ptr(right), _ptr(src_col), _ptr(mask), _opt_ptr(noise),
            _dtype_code(left, _native.LATENT_DTYPE), b, c, h, w, _native.LATENT_OP[op])
    return right


def decode_to_codes(image):
    """cs_decode_to_codes on a device tensor: image [N,C,H,W] float32, float16 or bfloat16, the VAE's output -> uint8 [N,H,W,C]:
    trunc(nan_to_num((image / 2 + 0.5).clamp(0, 1)).float() * 255), the quotient and the sum rounded to the tensor's dtype as
    torch rounds them (reference stereodiffusion_nodes.py:673-677)."""
    # (_tensor checks in the order written: the ladder this wrapper always had)
    _tensor("image", image, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [N,C,H,W], got shape"), not_empty="image", contiguous=True)
    _on_gpu(image, no_gpu_error=True)
    n, c, h, w = image.shape
    codes = torch.empty((n, h, w, c), dtype=torch.uint8, device=image.device)
    _launch(image.device, _native.lib().cs_decode_to_codes, _ptr(image), _dtype_code(image, _native.LATENT_DTYPE), n, c, h, w, _ptr(codes))
    return codes


# ---- null-text inversion outside the UNet (cs_ddim_step, cs_null_loss_grad, cs_adam_step) ----
def _flat_like(first, tensors, what):
    """The shared checks of the three wrappers: tensors of first's shape, dtype and device, contiguous, not empty."""
    name0, t0 = first
    # (_tensor checks in the order written: the ladder this wrapper always had)
    _tensor(name0, t0, dtypes=(_FLOATS, _FLOATS_TEXT), not_empty=name0)
    for name, t in [first] + list(tensors):
        _tensor(name, t, like=(t0.dtype, f"{what} must share one dtype, got {t0.dtype} ({name0}) and {{got}} ({name})"),
                shape=(t0.shape, f"have {name0}'s shape {tuple(t0.shape)}, got"), contiguous=True)
        _same_device(first, (name, t))
    return _dtype_code(t0, _native.LATENT_DTYPE), t0.numel()


def _prediction(prediction):
    """`prediction` in enum cs_prediction, or ValueError: the first check of every wrapper that takes it, before any tensor is
    looked at."""
    if not isinstance(prediction, str) or prediction not in _native.PREDICTION:
        raise ValueError(f"unknown prediction {prediction!r} ({', '.join(_native.PREDICTION)})")
    return _native.PREDICTION[prediction]


def _step_scalars(guidance, coeffs, prediction=0):
    vals = _numbers((guidance,), coeffs, ("c1", "c2", "c3", "c4"), counted=True)
    if vals[2] == 0.0 and prediction == _native.PREDICTION["epsilon"]:   # (under v-prediction c2 multiplies and divides nothing)
        raise ValueError("coeffs[1] (the square root of alpha_t) must not be 0")
    return vals


def ddim_step(sample, eps_a, eps_b, guidance, coeffs, out=None):
    """ddim_step_pred for an epsilon model (the signature this function always had; a v-prediction model takes ddim_step_pred)."""
    return ddim_step_pred(sample, eps_a, eps_b, guidance, coeffs, out)


def ddim_step_pred(sample, eps_a, eps_b, guidance, coeffs, out=None, prediction="epsilon"):
    """cs_ddim_step_pred: guidance and one DDIM step in one launch.  e = eps_a + guidance * (eps_b - eps_a), or eps_a when eps_b is
    None; out = c4 * ((sample - c1 * e) / c2) + c3 * e with coeffs = (c1, c2, c3, c4) = (sqrt(1 - a_t), sqrt(a_t),
    sqrt(1 - a_other), sqrt(a_other)) as float32 values: NullInversion.prev_step and next_step (reference inversion.py:57-75) are
    this formula with their two alphas.  Tensors of one shape and dtype (float32, float16, bfloat16), contiguous; every operation is
    rounded to the dtype as torch rounds the reference's expression.  out: None (a new tensor) or a tensor to write, which may be
    `sample` itself.  prediction "v_prediction": eps_a and eps_b are the answers of a v-prediction model (Salimans & Ho 2022), and
    with v the guided one, x0 = c2 * sample - c1 * v; e = c2 * v + c1 * sample; out = c4 * x0 + c3 * e (c2 a first operand: rounded
    to a half dtype like c1, c3 and c4, and free to be 0).  -> out"""
    pred = _prediction(prediction)
    ins = [("eps_a", eps_a)] + ([("eps_b", eps_b)] if eps_b is not None else []) + ([("out", out)] if out is not None else [])
    dtype, n = _flat_like(("sample", sample), ins, "sample, eps_a, eps_b and out")
    g, c1, c2, c3, c4 = _step_scalars(guidance, coeffs, pred)
    for name, t in [("sample", sample)] + ins:
        _tensor(name, t, no_grad="cs_ddim_step is not differentiable (detach it, or run under no_grad on detached tensors)")
    _on_gpu(sample, no_gpu_error=True)
    if out is None:
        out = torch.empty_like(sample)
    _launch(sample.device, _native.lib().cs_ddim_step_pred, _ptr(sample), _ptr(eps_a), _opt_ptr(eps_b), _ptr(out), dtype, n, g, c1, c2, c3,
            c4, pred)
    return out


def null_loss_grad(eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs, prediction="epsilon"):
    """cs_null_loss_grad: the inner step of null-text optimisation outside the UNet (reference inversion.py:198-201) in one
    launch -> (rec, loss, grad): rec = prev_step(eps_uncond + guidance * (eps_cond - eps_uncond), t, latent_cur) bit for bit,
    loss = mean((rec - latent_prev)^2) as a float32 tensor [] (a fixed summation order: the same bits on every run), grad =
    d loss / d eps_uncond in the tensors' dtype.  prediction: as for ddim_step (the gradient is then with respect to the
    unconditional v).  Nothing here waits for the device."""
    pred = _prediction(prediction)
    dtype, n = _flat_like(("eps_uncond", eps_uncond), [("eps_cond", eps_cond), ("latent_cur", latent_cur), ("latent_prev", latent_prev)],
                          "eps_uncond, eps_cond, latent_cur and latent_prev")
    g, c1, c2, c3, c4 = _step_scalars(guidance, coeffs, pred)
    _on_gpu(eps_uncond, no_gpu_error=True)
    L = _native.lib()
    rec, grad = torch.empty_like(eps_uncond), torch.empty_like(eps_uncond)
    loss = torch.empty((), dtype=torch.float32, device=eps_uncond.device)
    ws, nb = _workspace(L.cs_null_loss_workspace_bytes(n), eps_uncond.device)
    _launch(eps_uncond.device, L.cs_null_loss_grad_pred, _ptr(eps_uncond), _ptr(eps_cond), _ptr(latent_cur), _ptr(latent_prev), _ptr(rec),
            _ptr(loss), _ptr(grad), dtype, n, g, c1, c2, c3, c4, pred, _ptr(ws) if nb else None, nb)
    return rec, loss, grad


class NullTextLoss(torch.autograd.Function):
    """loss = NullTextLoss.apply(eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs): mse_loss(prev_step(guided
    prediction), latent_prev) of null-text optimisation (reference inversion.py:199-201) as one node of the graph.  The forward is
    one cs_null_loss_grad launch and keeps the gradient with respect to eps_uncond; the backward scales it by grad_output.  Only
    eps_uncond gets a gradient -- the reference computes eps_cond under no_grad and the latents are constants.  The loss is float32
    whatever the dtype.  ctx.rec: the reconstructed latent, for callers that want it."""

    @staticmethod
    def forward(ctx, eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs, prediction="epsilon"):
        rec, loss, grad = null_loss_grad(eps_uncond.detach(), eps_cond, latent_cur, latent_prev, guidance, coeffs, prediction)
        ctx.save_for_backward(grad)
        ctx.rec = rec
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output.to(grad.dtype)), None, None, None, None, None, None


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """cs_adam_step: one torch.optim.Adam step (no weight decay, no amsgrad) in place on param, exp_avg and exp_avg_sq, one launch.
    Four tensors of one shape and dtype (float32, float16, bfloat16), contiguous; step: the 1-based number of this step (the bias
    corrections are computed from it in double on the host).  A param that requires grad is updated through its data, as an
    optimizer does.  -> param"""
    dtype, n = _flat_like(("param", param), [("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)],
                          "param, grad, exp_avg and exp_avg_sq")
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"step must be an int counting from 1, got {step!r}")
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    if not (math.isfinite(lr) and math.isfinite(eps) and eps >= 0 and 0 <= beta1 < 1 and 0 <= beta2 < 1):
        raise ValueError(f"lr and eps must be finite, eps >= 0 and the betas in [0, 1), got {lr}, {eps}, {beta1}, {beta2}")
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _tensor(name, t, no_grad="")
    _on_gpu(param, no_gpu_error=True)
    _launch(param.device, _native.lib().cs_adam_step, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), dtype, n, lr, beta1, beta2,
            eps, step)
    return param


# ---- null-text optimisation on F frames at once (cs_null_loss_grad_frames, cs_adam_step_frames) ----
MAX_FRAMES = 65535                         # the grid's second dimension
NULL_LOSS_MAX_COUNT = 32768 * 0x7fffffff   # null_loss_max_count(): a 32-bit grid of 32768-element workgroups
_NULL_LOSS_BLOCK = 32768                   # elements per workgroup of the loss: above it a frame needs the second stage


def null_loss_frames_workspace_bytes(frames, per):
    """cs_null_loss_frames_workspace_bytes, restated: two floats per block of 32 768 elements and frame when per > 32 768."""
    blocks = (per + _NULL_LOSS_BLOCK - 1) // _NULL_LOSS_BLOCK
    return frames * blocks * 8 if blocks > 1 else 0


def _frames_like(first, tensors, what):
    """_flat_like on tensors [F, ...]: -> (dtype code, F, elements per frame), within the kernels' limits."""
    dtype, n = _flat_like(first, tensors, what)
    name0, t0 = first
    _tensor(name0, t0, dims=(range(2, 9), "be [F, ...] (frames first), got shape"))
    frames, per = t0.shape[0], n // t0.shape[0]
    if frames > MAX_FRAMES:
        raise ValueError(f"{name0} has {frames} frames, more than the {MAX_FRAMES} of one launch")
    if per > NULL_LOSS_MAX_COUNT:
        raise ValueError(f"{name0} has {per} elements per frame, more than the {NULL_LOSS_MAX_COUNT} of a 32-bit grid")
    return dtype, frames, per


def _frame_flags(name, t, frames, first):
    _tensor(name, t, dtypes=((torch.uint8,), "uint8"), shape=((frames,), f"be [F] = {(frames,)}, got shape"), contiguous=True)
    _same_device(first, (name, t))
    return t


def null_loss_grad_frames(eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs, active_in, threshold, active_out=None,
                          loss=None, rec=None, grad=None, workspace=None, prediction="epsilon"):
    """cs_null_loss_grad_frames: null_loss_grad on F frames in one launch -> (rec, loss [F] float32, grad, active_out).  Tensors
    [F, ...]; a frame's rec, grad and loss are bit for bit null_loss_grad's on that frame alone.  active_in uint8 [F]: a frame whose
    flag is 0 gets a zero grad, its rec and loss are not touched.  active_out uint8 [F], another buffer than active_in:
    active_in[f] and not float64(loss[f]) < threshold -- the reference's early stop, left on the device.  active_out, loss, rec,
    grad, workspace (uint8, null_loss_frames_workspace_bytes(F, per) bytes): buffers to write, or None for new ones (a new loss
    is NaNs, a new rec zeros: what an inactive frame then shows).  prediction: as for ddim_step.  Nothing here waits for the
    device."""
    pred = _prediction(prediction)
    first = ("eps_uncond", eps_uncond)
    dtype, frames, per = _frames_like(first, [("eps_cond", eps_cond), ("latent_cur", latent_cur), ("latent_prev", latent_prev)]
                                      + [(n, t) for n, t in (("rec", rec), ("grad", grad)) if t is not None],
                                      "eps_uncond, eps_cond, latent_cur, latent_prev, rec and grad")
    g, c1, c2, c3, c4 = _step_scalars(guidance, coeffs, pred)
    threshold = float(threshold)
    if math.isnan(threshold):
        raise ValueError("threshold must not be a NaN")
    _frame_flags("active_in", active_in, frames, first)
    if active_out is not None:
        _frame_flags("active_out", active_out, frames, first)
        if active_out is active_in or active_out.data_ptr() == active_in.data_ptr():
            raise ValueError("active_out must be another buffer than active_in (swap two buffers between inner steps)")
    if loss is not None:
        _tensor("loss", loss, dtypes=((torch.float32,), "float32"), shape=((frames,), f"be [F] = {(frames,)}, got shape"), contiguous=True)
        _same_device(first, ("loss", loss))
    need = null_loss_frames_workspace_bytes(frames, per)
    if workspace is not None:
        _tensor("workspace", workspace, dtypes=((torch.uint8,), "uint8"), contiguous=True)
        _same_device(first, ("workspace", workspace))
        if workspace.numel() < need:
            raise ValueError(f"workspace has {workspace.numel()} bytes, {need} are needed")
    _on_gpu(eps_uncond, no_gpu_error=True)
    L = _native.lib()
    dev = eps_uncond.device
    rec = torch.zeros_like(eps_uncond) if rec is None else rec
    grad = torch.empty_like(eps_uncond) if grad is None else grad
    loss = torch.full((frames,), math.nan, dtype=torch.float32, device=dev) if loss is None else loss
    active_out = torch.empty((frames,), dtype=torch.uint8, device=dev) if active_out is None else active_out
    if workspace is None:
        workspace, _ = _workspace(need, dev)
    _launch(dev, L.cs_null_loss_grad_frames_pred, _ptr(eps_uncond), _ptr(eps_cond), _ptr(latent_cur), _ptr(latent_prev), _ptr(rec),
            _ptr(loss), _ptr(grad), _ptr(active_in), _ptr(active_out), dtype, frames, per, g, c1, c2, c3, c4, pred, threshold,
            _ptr(workspace) if need else None, need)
    return rec, loss, grad, active_out


class NullTextLossFrames(torch.autograd.Function):
    """loss [F] = NullTextLossFrames.apply(eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs, active_in, threshold,
    active_out): NullTextLoss per frame, one cs_null_loss_grad_frames launch.  The backward hands the kept gradient to eps_uncond;
    the incoming gradient of the loss is taken as ones (loss.sum().backward(), or grad_outputs of ones) and any other value is
    refused -- a per-frame scale would be one more pass over the tensor, and null-text optimisation has none.  ctx.rec, ctx.active_out:
    the reconstructed latents and the flags of the next inner step."""

    @staticmethod
    def forward(ctx, eps_uncond, eps_cond, latent_cur, latent_prev, guidance, coeffs, active_in, threshold, active_out=None,
                prediction="epsilon"):
        rec, loss, grad, active_out = null_loss_grad_frames(eps_uncond.detach(), eps_cond, latent_cur, latent_prev, guidance, coeffs,
                                                            active_in, threshold, active_out, prediction=prediction)
        ctx.save_for_backward(grad)
        ctx.rec, ctx.active_out = rec, active_out
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        if not bool((grad_output == 1).all()):
            raise ValueError("NullTextLossFrames takes the gradient of its loss as ones (loss.sum().backward()); got another value")
        return (grad,) + (None,) * 9


def adam_step_frames(param, grad, exp_avg, exp_avg_sq, active, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """cs_adam_step_frames: adam_step, with one lr and one step number, on the rows [f] of four tensors [F, ...] whose active[f]
    (uint8 [F]) is set; the rows of every other frame are not written at all.  One launch.  -> param"""
    first = ("param", param)
    dtype, frames, per = _frames_like(first, [("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)],
                                      "param, grad, exp_avg and exp_avg_sq")
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"step must be an int counting from 1, got {step!r}")
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    if not (math.isfinite(lr) and math.isfinite(eps) and eps >= 0 and 0 <= beta1 < 1 and 0 <= beta2 < 1):
        raise ValueError(f"lr and eps must be finite, eps >= 0 and the betas in [0, 1), got {lr}, {eps}, {beta1}, {beta2}")
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _tensor(name, t, no_grad="")
    _frame_flags("active", active, frames, first)
    _on_gpu(param, no_gpu_error=True)
    _launch(param.device, _native.lib().cs_adam_step_frames, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(active), dtype,
            frames, per, lr, beta1, beta2, eps, step)
    return param


# ---- StereoDiffusion Fast mode's inpainting loop outside its models (cs_inpaint_*) ----
def _unet_input(x, n, hl, wl, like=None):
    """x: the persistent UNet input [2n, 9, hl, wl], contiguous, of a latent dtype (of `like`'s, when given)."""
    _tensor("x", x, dtypes=(_FLOATS, _FLOATS_TEXT), shape=((2 * n, 9, hl, wl), f"be [2n,9,hl,wl] = {(2 * n, 9, hl, wl)}, got shape"),
            contiguous=True, no_grad="the inpainting loop works in place")
    if like is not None:
        _tensor("x", x, like=(like[1].dtype, f"x and {like[0]} must share one dtype, got {{got}} and {like[1].dtype}"))


def inpaint_image_prep(filled_u8, mask, x, latent_size):
    """cs_inpaint_image_prep: what ComfyUIInpaintRunner.__call__ does to its image and mask before the VAE (reference
    model_wrappers.py:562-572, :580).  filled_u8 uint8 [N,H,W,3]; mask uint8 or bool [N,H,W] (non-zero: inpaint); x [2N,9,hl,wl] of
    the model's dtype, latent_size = (hl, wl).  -> (img, masked) [N,3,H,W] of x's dtype: codes / 255 * 2 - 1, and that times
    (1 - mask); channel 4 of both halves of x receives F.interpolate(mask, (hl, wl), mode="nearest")."""
    _tensor("filled_u8", filled_u8, dtypes=((torch.uint8,), "uint8"), dims=((4,), "be [N,H,W,3], got shape"), not_empty="filled_u8",
            contiguous=True)
    n, h, w, c = filled_u8.shape
    if c != 3:
        raise ValueError(f"filled_u8 must be [N,H,W,3], got shape {tuple(filled_u8.shape)}")
    _tensor("mask", mask, dtypes=((torch.uint8, torch.bool), "uint8 or bool"), shape=((n, h, w), f"be [N,H,W] = {(n, h, w)}, got shape"),
            contiguous=True)
    hl, wl = (int(v) for v in latent_size)
    if hl <= 0 or wl <= 0:
        raise ValueError(f"latent_size must be positive, got {(hl, wl)}")
    _unet_input(x, n, hl, wl)
    _same_device(("filled_u8", filled_u8), ("mask", mask), ("x", x))
    _on_gpu(filled_u8, no_gpu_error=True)
    img = torch.empty((n, 3, h, w), dtype=x.dtype, device=x.device)
    masked = torch.empty_like(img)
    _launch(x.device, _native.lib().cs_inpaint_image_prep, _ptr(filled_u8), _ptr(mask), n, h, w, hl, wl, _dtype_code(x, _native.LATENT_DTYPE),
            _ptr(img), _ptr(masked), _ptr(x))
    return img, masked


def inpaint_latent_init(mean_img, mean_masked, noise, coeffs, x, img_latent=None, decode_in=None):
    """cs_inpaint_latent_init (reference model_wrappers.py:575-602): the VAE's two means [N,4,hl,wl] (one dtype, any of the three)
    -> img_latent = (mean_img * 0.18215).to(x.dtype), returned; channels 0..3 of both halves of x = sa * img_latent + sb * noise
    (scheduler.add_noise; coeffs = (sa, sb), noise [N,4,hl,wl] of x's dtype), or img_latent when noise is None (no timestep left);
    channels 5..8 = (mean_masked * 0.18215).to(x.dtype); decode_in, when given, receives latents / 0.18215 (:628: a loop of no step)."""
    _tensor("mean_img", mean_img, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [N,4,hl,wl], got shape"), not_empty="mean_img", contiguous=True)
    n, c, hl, wl = mean_img.shape
    if c != 4:
        raise ValueError(f"mean_img must be [N,4,hl,wl], got shape {tuple(mean_img.shape)}")
    what = f"have mean_img's shape {tuple(mean_img.shape)}, got"
    _tensor("mean_masked", mean_masked, like=(mean_img.dtype, f"mean_img and mean_masked must share one dtype, got {mean_img.dtype} and {{got}}"),
            shape=(mean_img.shape, what), contiguous=True)
    _unet_input(x, n, hl, wl)
    named = [("mean_masked", mean_masked), ("x", x)]
    for name, t in (("noise", noise), ("img_latent", img_latent), ("decode_in", decode_in)):
        if t is not None:
            _like_x(name, t, x, mean_img.shape, what)
            named.append((name, t))
    sa, sb = (1.0, 0.0) if noise is None else _numbers((), coeffs, ("sa", "sb"))
    _same_device(("mean_img", mean_img), *named)
    _on_gpu(mean_img, no_gpu_error=True)
    if img_latent is None:
        img_latent = torch.empty(mean_img.shape, dtype=x.dtype, device=x.device)
    _launch(x.device, _native.lib().cs_inpaint_latent_init, _ptr(mean_img), _ptr(mean_masked), _dtype_code(mean_img, _native.LATENT_DTYPE),
            _opt_ptr(noise), _dtype_code(x, _native.LATENT_DTYPE), n, hl, wl, sa, sb, _ptr(x), _ptr(img_latent), _opt_ptr(decode_in))
    return img_latent


def plms_step(noise_pred, x, kind, guidance, coeffs, e_out=None, history=(), cur_sample=None, decode_in=None):
    """cs_inpaint_plms_step: classifier-free guidance and one PLMS step in one launch, in place on the UNet's input (reference
    model_wrappers.py:621-625).  noise_pred [2N,4,hl,wl] (uncond, cond) and x [2N,9,hl,wl] of one dtype; kind: a key of
    _native.PLMS_KIND; coeffs = (sc, da, denom): prev = sc * sample - da * m / denom with m the kind's combination of
    e = u + guidance * (t - u) and `history` (the earlier predictions, the latest first; 0 to 3 of them as the kind asks).
    prev goes into channels 0..3 of both halves of x, e into e_out (every kind but "second"), the sample into cur_sample ("first";
    "second" reads it), prev / 0.18215 into decode_in when given.  All of these [N,4,hl,wl] of x's dtype.  -> x"""
    if kind not in _native.PLMS_KIND:
        raise ValueError(f"unknown kind {kind!r} ({', '.join(_native.PLMS_KIND)})")
    k = _native.PLMS_KIND[kind]
    _tensor("noise_pred", noise_pred, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [2N,4,hl,wl], got shape"), not_empty="noise_pred",
            contiguous=True, no_grad="cs_inpaint_plms_step is not differentiable")
    n2, c, hl, wl = noise_pred.shape
    if c != 4 or n2 % 2:
        raise ValueError(f"noise_pred must be [2N,4,hl,wl], got shape {tuple(noise_pred.shape)}")
    n = n2 // 2
    _unet_input(x, n, hl, wl, like=("noise_pred", noise_pred))
    history = tuple(history)
    need = (0, 1, 1, 2, 3)[k]
    if len(history) != need:
        raise ValueError(f"kind {kind!r} takes {need} earlier prediction(s), got {len(history)}")
    if (e_out is None) != (kind == "second"):
        raise ValueError("e_out goes with every kind but 'second', whose prediction is not kept")
    if (cur_sample is None) != (k > 1):
        raise ValueError("cur_sample goes with the kinds 'first' (which writes it) and 'second' (which reads it) only")
    named = [(f"history[{i}]", t) for i, t in enumerate(history)]
    named += [(name, t) for name, t in (("e_out", e_out), ("cur_sample", cur_sample), ("decode_in", decode_in)) if t is not None]
    shape = (n, 4, hl, wl)
    what = f"be [N,4,hl,wl] = {shape}, got shape"
    for name, t in named:
        _like_x(name, t, x, shape, what)
    g, sc, da, denom = _numbers((guidance,), coeffs, ("sc", "da", "denom"))
    if denom == 0.0:
        raise ValueError("coeffs[2] (denom) must not be 0")
    _same_device(("noise_pred", noise_pred), ("x", x), *named)
    _on_gpu(noise_pred, no_gpu_error=True)
    h = [_ptr(t) for t in history] + [None] * (3 - len(history))
    _launch(x.device, _native.lib().cs_inpaint_plms_step, _ptr(noise_pred), _ptr(x), _dtype_code(x, _native.LATENT_DTYPE), n, hl, wl, k, g, sc,
            da, denom, _opt_ptr(e_out), h[0], h[1], h[2], _opt_ptr(cur_sample), _opt_ptr(decode_in))
    return x


# ---- Fast mode's loop for few-step models (cs_inpaint_fewstep_*) ----
FEWSTEP_COEFFS = {"euler": ("sigma_next - sigma_t", "sqrt(sigma_next^2 + 1)", "sigma_next"),
                  "lcm": ("sqrt(1 - a_t)", "sqrt(a_t)", "c_out", "c_skip", "sqrt(a_next)", "sqrt(1 - a_next)")}


def _fewstep_sampler(sampler):
    if sampler not in _native.FEWSTEP_SAMPLER:
        raise ValueError(f"unknown sampler {sampler!r} ({', '.join(_native.FEWSTEP_SAMPLER)})")
    return _native.FEWSTEP_SAMPLER[sampler]


def _fewstep_numbers(lead, coeffs, names):
    """_numbers for any count of coefficients."""
    try:
        vals = [float(v) for v in lead] + [float(c) for c in coeffs]
    except (TypeError, ValueError):
        vals = None
    if vals is None or len(vals) != len(lead) + len(names):
        raise ValueError(f"coeffs must be {len(names)} numbers ({', '.join(names)})")
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{'guidance and ' if lead else ''}coeffs must be finite, got {tuple(vals)}")
    return vals


def _fewstep_input(x, n, hl, wl, cfg):
    """x: the persistent UNet input [2n or n, 9 or 4, hl, wl] of a latent dtype, contiguous -> its channel count."""
    _tensor("x", x, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [2N or N,C,hl,wl], got shape"), contiguous=True,
            no_grad="the inpainting loop works in place")
    channels = x.shape[1]
    if channels not in (4, 9):
        raise ValueError(f"x must have 9 channels (an inpainting UNet) or 4, got shape {tuple(x.shape)}")
    shape = ((2 if cfg else 1) * n, channels, hl, wl)
    _tensor("x", x, shape=(shape, f"be [{'2N' if cfg else 'N'},{channels},hl,wl] = {shape} {'under' if cfg else 'without'} guidance, got shape"))
    return channels


def fewstep_latent_init(img_latent, noise, coeffs, x, sampler, cfg, state=None, prep=None, mask_l=None):
    """cs_inpaint_fewstep_init: the first latents of a few-step loop.  img_latent [N,4,hl,wl] (inpaint_latent_init's), noise
    the same or None (no timestep left: x = img_latent); x [2N,C,hl,wl] with cfg, [N,C,hl,wl] without, C = 9 or 4; sampler
    "euler": coeffs = (sigma_0, sqrt(sigma_0^2 + 1)), state [N,4,hl,wl] receives img_latent + sigma_0 * noise and channels 0..3
    of x that divided by the second coefficient; "lcm": coeffs = add_noise's (sa, sb), x = sa * img_latent + sb * noise as
    inpaint_latent_init forms it.  C = 4: mask_l [N,1,hl,wl] receives channel 4 of prep [2N,9,hl,wl], the mask
    inpaint_image_prep put there.  -> x"""
    code = _fewstep_sampler(sampler)
    _tensor("img_latent", img_latent, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [N,4,hl,wl], got shape"), not_empty="img_latent",
            contiguous=True, no_grad="")
    n, c, hl, wl = img_latent.shape
    if c != 4:
        raise ValueError(f"img_latent must be [N,4,hl,wl], got shape {tuple(img_latent.shape)}")
    channels = _fewstep_input(x, n, hl, wl, cfg)
    _tensor("x", x, like=(img_latent.dtype, f"x and img_latent must share one dtype, got {{got}} and {img_latent.dtype}"))
    what = f"have img_latent's shape {tuple(img_latent.shape)}, got"
    named = [("x", x)]
    for name, t in (("noise", noise), ("state", state)):
        if t is not None:
            _like_x(name, t, x, img_latent.shape, what)
            named.append((name, t))
    if sampler == "euler" and state is None:
        raise ValueError("sampler 'euler' takes state, the un-scaled sample")
    if channels == 4:
        if prep is None or mask_l is None:
            raise ValueError("a 4-channel x takes prep (inpaint_image_prep's x) and mask_l")
        _unet_input(prep, n, hl, wl, like=("img_latent", img_latent))
        _like_x("mask_l", mask_l, x, (n, 1, hl, wl), f"be [N,1,hl,wl] = {(n, 1, hl, wl)}, got shape")
        named += [("prep", prep), ("mask_l", mask_l)]
    else:
        prep = mask_l = None
    k0, k1 = (1.0, 1.0) if noise is None else _fewstep_numbers((), coeffs, ("sigma_0", "sqrt(sigma_0^2 + 1)") if sampler == "euler" else ("sa", "sb"))
    if noise is not None and sampler == "euler" and k1 == 0.0:
        raise ValueError("coeffs[1] (the input scale) must not be 0")
    _same_device(("img_latent", img_latent), *named)
    _on_gpu(img_latent, no_gpu_error=True)
    _launch(x.device, _native.lib().cs_inpaint_fewstep_init, _ptr(img_latent), _opt_ptr(noise), _opt_ptr(prep),
            _dtype_code(x, _native.LATENT_DTYPE), n, hl, wl, channels, int(bool(cfg)), code, k0, k1, _ptr(x), _opt_ptr(state), _opt_ptr(mask_l))
    return x


def fewstep_step(noise_pred, x, sampler, guidance, coeffs, cfg, last=False, state=None, step_noise=None, img_latent=None, noise0=None,
                 mask_l=None, decode_in=None):
    """cs_inpaint_fewstep_step: guidance and one Euler or LCM step in one launch, in place on the UNet's input.  With cfg
    noise_pred [2N,4,hl,wl] (uncond, cond), x [2N,C,hl,wl] and e = u + guidance * (t - u) in the dtype; without, noise_pred
    [N,4,hl,wl] is e and x [N,C,hl,wl].  After e everything is float32 with one rounding per stored tensor (tools/fewstep_oracle.py
    is the specification).  coeffs: FEWSTEP_COEFFS[sampler].
      "euler"  prev = state + e * (sigma_next - sigma_t); state (the un-scaled sample, [N,4,hl,wl]) = lat; channels 0..3 of x =
               lat / sqrt(sigma_next^2 + 1), the next step's scaled input
      "lcm"    s = channels 0..3 of x; x0 = (s - sqrt(1 - a_t) e) / sqrt(a_t); den = c_out x0 + c_skip s; prev = sqrt(a_next) den +
               sqrt(1 - a_next) step_noise, den on the last step; channels 0..3 of x = lat
    C = 9: lat = prev.  C = 4: lat = mask_l != 0 ? prev : keep -- a select: values are moved, not multiplied -- with keep the
    image's latents at the next noise level from img_latent and noise0 (the initial noise), img_latent itself on the last step;
    mask_l [N,1,hl,wl].  decode_in, when given, receives lat / 0.18215.  -> x"""
    code = _fewstep_sampler(sampler)
    _tensor("noise_pred", noise_pred, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [2N or N,4,hl,wl], got shape"), not_empty="noise_pred",
            contiguous=True, no_grad="cs_inpaint_fewstep_step is not differentiable")
    rows, c, hl, wl = noise_pred.shape
    if c != 4 or (cfg and rows % 2):
        raise ValueError(f"noise_pred must be [{'2N' if cfg else 'N'},4,hl,wl], got shape {tuple(noise_pred.shape)}")
    n = rows // 2 if cfg else rows
    channels = _fewstep_input(x, n, hl, wl, cfg)
    _tensor("x", x, like=(noise_pred.dtype, f"x and noise_pred must share one dtype, got {{got}} and {noise_pred.dtype}"))
    last = bool(last)
    if (state is None) != (sampler != "euler"):
        raise ValueError("state goes with sampler 'euler' only, which keeps the un-scaled sample there")
    if (step_noise is None) != (sampler != "lcm" or last):
        raise ValueError("step_noise goes with every step of sampler 'lcm' but the last, and with no other")
    if channels == 4 and (img_latent is None or mask_l is None or (noise0 is None and not last)):
        raise ValueError("a 4-channel x takes img_latent, mask_l and, before the last step, noise0 (the blend)")
    if channels == 9:
        img_latent = noise0 = mask_l = None
    if last:
        noise0 = None
    shape = (n, 4, hl, wl)
    what = f"be [N,4,hl,wl] = {shape}, got shape"
    named = [(name, t) for name, t in (("state", state), ("step_noise", step_noise), ("img_latent", img_latent), ("noise0", noise0),
                                       ("decode_in", decode_in)) if t is not None]
    for name, t in named:
        _like_x(name, t, x, shape, what)
    if mask_l is not None:
        _like_x("mask_l", mask_l, x, (n, 1, hl, wl), f"be [N,1,hl,wl] = {(n, 1, hl, wl)}, got shape")
        named.append(("mask_l", mask_l))
    names = FEWSTEP_COEFFS[sampler]
    vals = _fewstep_numbers((guidance,), coeffs, names)
    g, k = vals[0], vals[1:] + [0.0] * (6 - len(names))
    if k[1] == 0.0:
        raise ValueError(f"coeffs[1] ({names[1]}) must not be 0")
    _same_device(("noise_pred", noise_pred), ("x", x), *named)
    _on_gpu(noise_pred, no_gpu_error=True)
    _launch(x.device, _native.lib().cs_inpaint_fewstep_step, _ptr(noise_pred), _ptr(x), _dtype_code(x, _native.LATENT_DTYPE), n, hl, wl,
            channels, code, int(bool(cfg)), int(last), g, *k, _opt_ptr(state), _opt_ptr(step_noise), _opt_ptr(img_latent), _opt_ptr(noise0),
            _opt_ptr(mask_l), _opt_ptr(decode_in))
    return x


# ---- StereoDiffusion Standard mode between two UNet calls (cs_standard_step) ----
def standard_step(noise_pred, x, guidance, coeffs, op="none", src_col=None, mask=None, noise=None, prediction="epsilon"):
    """cs_standard_step: classifier-free guidance, one DDIM step and the latent shift in one launch, in place on the UNet's
    persistent input.  x [4B,C,h,w]: rows 0..B-1 the left views, B..2B-1 the right views, 2B..4B-1 their copy for the conditional
    half; noise_pred [4B,C,h,w], the unconditional half first; both of one dtype (float32, float16, bfloat16), contiguous.
    e = u + guidance * (c - u); new = c4 * ((x - c1 * e) / c2) + c3 * e with coeffs = (c1, c2, c3, c4) as for ddim_step; then by
    `op` ("none", "first", "reshift") what latent_shift_apply does to (new left, new right) with src_col int32 [B,h,w], mask uint8
    [B,h,w] and, for "first", an optional noise [B,C,h,w].  The result goes into both halves of x: bit for bit ddim_step on the
    two halves, then latent_shift_apply, then the copy.  prediction: as for ddim_step, whose v-prediction step this then is.  -> x"""
    pred = _prediction(prediction)
    if op not in _native.STANDARD_OP:
        raise ValueError(f"unknown op {op!r} (none, first, reshift)")
    if noise is not None and op != "first":
        raise ValueError("noise goes with op 'first' only")
    if op != "none" and (src_col is None or mask is None):
        raise ValueError(f"op {op!r} takes src_col and mask")
    _tensor("x", x, dtypes=(_FLOATS, _FLOATS_TEXT), dims=((4,), "be [4B,C,h,w], got shape"), not_empty="x", contiguous=True,
            no_grad="cs_standard_step works in place")
    n4, c, h, w = x.shape
    if n4 % 4:
        raise ValueError(f"x must be [4B,C,h,w] (left views, right views, and their copy), got shape {tuple(x.shape)}")
    b = n4 // 4
    _like_x("noise_pred", noise_pred, x, x.shape, f"have x's shape {tuple(x.shape)}, got", no_grad="cs_standard_step is not differentiable")
    named = [("noise_pred", noise_pred)]
    if noise is not None:
        _like_x("noise", noise, x, (b, c, h, w), f"be [B,C,h,w] = {(b, c, h, w)}, got shape")
        named.append(("noise", noise))
    if op != "none":
        _tensor("src_col", src_col, dtypes=((torch.int32,), "int32 (latent_shift_plan's)"),
                shape=((b, h, w), f"be [B,h,w] = {(b, h, w)}, got shape"), contiguous=True)
        _tensor("mask", mask, dtypes=((torch.uint8,), "uint8"), shape=((b, h, w), f"be [B,h,w] = {(b, h, w)}, got shape"), contiguous=True)
        named += [("src_col", src_col), ("mask", mask)]
    else:
        src_col = mask = None
    if w > LATENT_MAX_WIDTH:
        raise ValueError(f"rows of {w} columns: cs_standard_step takes up to {LATENT_MAX_WIDTH} (latent_shift_plan's limit)")
    g, c1, c2, c3, c4 = _step_scalars(guidance, coeffs, pred)
    _same_device(("x", x), *named)
    _on_gpu(x, no_gpu_error=True)
    _launch(x.device, _native.lib().cs_standard_step_pred, _ptr(x), _ptr(noise_pred), _dtype_code(x, _native.LATENT_DTYPE), b, c, h, w, g, c1,
            c2, c3, c4, pred, _native.STANDARD_OP[op], _opt_ptr(src_col), _opt_ptr(mask), _opt_ptr(noise))
    return x
