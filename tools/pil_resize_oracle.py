"""numpy restatement of Pillow's 8-bit bicubic resize (PIL.Image.resize with all defaults on modes L and RGB, Pillow 12.2) and of
the gray rule StereoDiffusion's Fast mode applies to a coloured depth -- TEST INFRASTRUCTURE, the checker of the cs_pilresize
kernels.

Written from Pillow's observable behaviour and the rules in DESIGN.md section 2 (Pillow-exact resize): integer arithmetic on
fixed-point taps that are computed in float64.  Horizontal pass first, then vertical; a pass whose sizes agree is skipped; the
image between the passes is uint8.  tests/test_fastmode_surface.py holds it to PIL.Image.resize byte for byte where Pillow
imports.
"""
import math

import numpy as np

PRECISION_BITS = 22
A = -0.5


def bicubic(t):
    """The Keys kernel with a = -0.5 on a float64 array, every product in the order written."""
    t = np.abs(np.asarray(t, dtype=np.float64))
    near = ((A + 2.0) * t - (A + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * A
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def axis_taps(n_in, n_out):
    """-> (xmin int64 [n_out], count int64 [n_out], taps int32 [n_out, ksize]): the window of input samples of every output
    sample and its fixed-point taps (zero beyond count)."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin = np.zeros(n_out, dtype=np.int64)
    count = np.zeros(n_out, dtype=np.int64)
    taps = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        n = hi - lo
        k = bicubic((np.arange(n, dtype=np.float64) + lo - center + 0.5) * ss)
        ww = 0.0
        for v in k:          # left to right
            ww += float(v)
        if ww != 0.0:
            k = k / ww
        fixed = k * float(1 << PRECISION_BITS)
        taps[xx, :n] = np.where(k < 0, np.trunc(fixed - 0.5), np.trunc(fixed + 0.5)).astype(np.int32)
        xmin[xx], count[xx] = lo, n
    return xmin, count, taps


def resample_axis(a, axis, n_out):
    """One pass over `axis` of a uint8 array -> uint8."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a.copy()
    xmin, count, taps = axis_taps(n_in, n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int32)
    acc = np.full((n_out,) + src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
    idx = np.minimum(xmin[:, None] + np.arange(taps.shape[1])[None], n_in - 1)   # (taps beyond count are 0)
    for k in range(taps.shape[1]):
        acc += src[idx[:, k]] * taps[:, k].reshape((-1,) + (1,) * (src.ndim - 1))
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(a, size):
    """uint8 [..,H,W,C] -> [..,oh,ow,C]; size = (ow, oh), PIL's order."""
    return resize_hw(a, size[1], size[0])


def resize_hw(a, oh, ow):
    """uint8 [..,H,W,C] -> [..,oh,ow,C] (pass a trailing axis of 1 for gray images)."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim >= 3
    return resample_axis(resample_axis(a, -2, ow), -3, oh)


def gray_codes(rgb):
    """uint8 [..,3] -> uint8 [..]: trunc((r * 0.2989 + g * 0.5870) + b * 0.1140) in float64, in this order."""
    v = np.asarray(rgb).astype(np.float64)
    return ((v[..., 0] * 0.2989 + v[..., 1] * 0.5870) + v[..., 2] * 0.1140).astype(np.uint8)


def float_codes(x):
    """float32 -> uint8: trunc(clip(255 * x, 0, 255)), the product in float32."""
    return np.clip(np.float32(255.0) * np.asarray(x, dtype=np.float32), 0, 255).astype(np.uint8)


def code_floats(u8):
    """uint8 -> float32 code / 255 (a true division)."""
    return np.asarray(u8).astype(np.float32) / np.float32(255.0)


# ---- the whole of the Fast mode around its model ---------------------------------------------------------------------------
WORK = 512


def fast_mode_frame(image, depth, scale_factor, inpaint, threshold=0.05):
    """One frame as the node is handed it: image float32 [H,W,3], depth float32 [H,W,3], [H,W,1] or [H,W];
    inpaint(filled_u8 [512,512,3], mask bool [512,512]) -> uint8 [512,512,3], not called when the mask is empty.
    -> dict(left, right: uint8 [H,W,3] codes (the float outputs are code / 255), depth512, mask, filled_u8, warped_u8, called)."""
    import inpaint_oracle as io
    h, w = image.shape[:2]
    img_u8 = float_codes(image)
    dep = float_codes(depth)
    if dep.ndim == 3 and dep.shape[2] == 3:
        dep = gray_codes(dep)
    dep = dep.reshape(h, w, 1)
    img512 = resize_hw(img_u8, WORK, WORK)
    dep512 = resize_hw(dep, WORK, WORK)[..., 0]
    img_t = np.ascontiguousarray(code_floats(img512).transpose(2, 0, 1))
    warped, filled, mask = (a[0] for a in io.prepare(img_t[None], dep512.astype(np.float32)[None], scale_factor, threshold))
    warped_u8, filled_u8 = io.codes(warped), io.codes(filled)
    called = bool(mask.any())
    right512 = io.blend(mask, inpaint(filled_u8, mask), warped_u8) if called else warped_u8
    return dict(left=resize_hw(img512, h, w), right=resize_hw(right512, h, w), depth512=dep512, mask=mask, filled_u8=filled_u8,
                warped_u8=warped_u8, called=called)
