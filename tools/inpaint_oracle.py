"""numpy float32 restatement of the front half of StereoDiffusion's Fast mode (reference stereodiffusion_nodes.py:425-571,
StereoDiffusionNode._generate_stereo_fast_single): the backward warp, the inpaint mask and the per-row gap pre-fill the
reference hands to its inpainting model -- TEST INFRASTRUCTURE, the checker of the cs_inpaintprep kernels.

Written from the rules in DESIGN.md section 2 (inpaint preparation), not from the reference's lines; built on the linspace and
grid_sample pieces of tools/grid_oracle.py.  Every step is one float32 operation in the order CPU torch evaluates it.
Canonical shapes: image [B,3,H,W] (values k / 255), depth [B,H,W]; every frame is on its own (the reference runs one frame at a
time), so a batch is its frames one by one by construction.
"""
import hashlib

import numpy as np

import grid_oracle as go

F32 = np.float32


def depth_chain(depth):
    """depth [H,W] -> d - 0.5: divided by 255 when the frame's maximum is above 1, normalised by the frame's own min / max when
    max - min is above 1e-6 (zeros otherwise)."""
    d = np.asarray(depth, dtype=F32)
    if go.above(d.max(), F32(1.0)):
        d = d / F32(255.0)
    mn, mx = d.min(), d.max()
    rng = mx - mn
    if go.above(rng, F32(1e-6)):
        d = (d - mn) / rng
    else:
        d = np.zeros_like(d)
    return (d - F32(0.5)).astype(F32)


def dilate3(m):
    """3 x 3 dilation of a bool [H,W] (nothing beyond the frame)."""
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), dtype=bool)
    p[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def nearest_borders(valid):
    """valid [H,W] -> (left, right): the nearest valid column at or before / at or after each column; -1 / W where none."""
    w = valid.shape[-1]
    cols = np.arange(w, dtype=np.int64)
    left = np.maximum.accumulate(np.where(valid, cols, -1), axis=-1)
    right = np.minimum.accumulate(np.where(valid, cols, w)[..., ::-1], axis=-1)[..., ::-1]
    return left, right


def frame(img, depth, divergence_px, threshold=0.05):
    """One frame: img [3,H,W], depth [H,W] -> dict(warped [3,H,W], filled [3,H,W], mask bool [H,W], mask0 bool [H,W])."""
    img = np.asarray(img, dtype=F32)
    c, h, w = img.shape
    d = depth_chain(depth)
    offset = d * F32(-divergence_px)
    gxw = (go.linspace(w) - offset / F32(w / 2)).astype(F32)[None]
    gy = np.broadcast_to(go.linspace(h)[None, :, None], (1, h, w))
    warped = go.sample_bilinear(img[None], gxw, gy, "border")[0]
    valid = (gxw[0] >= F32(-1.0)) & (gxw[0] <= F32(1.0))
    d2 = d + F32(0.5)
    wd = go.sample_nearest(d2[None, None], gxw, gy, "border")[0, 0]
    dis = dilate3(go.above(wd - d2, F32(threshold)))
    mask0 = ~valid | dis
    mask = dilate3(mask0)   # (an empty mask0 stays empty: the reference's early return)
    left, right = nearest_borders(~mask)
    cols = np.arange(w, dtype=np.int64)
    ld = (cols - left).astype(F32)      # the frame edge counts as the column before 0 / after W - 1
    rd = (right - cols).astype(F32)
    t = ld / np.maximum(ld + rd, F32(1.0))
    none = mask.all(-1, keepdims=True)  # no unmasked pixel in the row: has_left and has_right both false
    t = np.where(none, F32(1.0), t)
    t = np.where(none, F32(0.0), t).astype(F32)
    lc = np.where((left >= 0)[None], np.take_along_axis(warped, np.clip(left, 0, w - 1)[None].repeat(c, 0), axis=-1), F32(0.0))
    rc = np.where((right < w)[None], np.take_along_axis(warped, np.clip(right, 0, w - 1)[None].repeat(c, 0), axis=-1), F32(0.0))
    interp = lc * (F32(1.0) - t)[None] + rc * t[None]
    filled = np.where(mask[None], interp, warped).astype(F32)
    return dict(warped=warped, filled=filled, mask=mask, mask0=mask0)


def prepare(image, depth, scale_factor, threshold=0.05):
    """image [B,3,H,W], depth [B,H,W] -> (warped, filled, mask) stacked over the frames."""
    w = image.shape[-1]
    dpx = (scale_factor / 100.0) * w
    fr = [frame(image[k], depth[k], dpx, threshold) for k in range(image.shape[0])]
    return tuple(np.stack([f[k] for f in fr]) for k in ("warped", "filled", "mask"))


def codes(x):
    """[..,3,H,W] float32 -> uint8 [..,H,W,3]: trunc(x * 255) (float32 product), the image the reference hands on."""
    v = np.asarray(x, dtype=F32) * F32(255.0)
    return np.moveaxis(v, -3, -1).astype(np.uint8)


def blend(mask, inpainted_u8, warped_u8):
    """where(mask, inpainted, warped codes): [H,W] bool, [H,W,3] uint8 twice."""
    return np.where(mask[..., None], inpainted_u8, warped_u8)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- seeded integer-only inputs (bit-identical on every machine) -------------------------------------------------------------
def image_u8(h, w, seed):
    """uint8 [h, w, 3]: seeded random colours."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def depth_u8(kind, h, w, seed=0):
    """uint8 depth [h, w] by kind:
    disc   -- a stepped gradient plus a near disc (disocclusions on both sides of the disc)
    flat   -- one value (no range: no offsets, empty mask)
    edges  -- near plateaus on both frame edges over a far middle (disocclusions that touch both frame edges)
    band   -- like disc, with a band of rows that alternates near / far every two columns (fully masked rows)
    """
    y, x = np.mgrid[0:h, 0:w]
    if kind == "flat":
        return np.full((h, w), 128, dtype=np.uint8)
    if kind == "edges":
        d = np.full((h, w), 20, dtype=np.int64)
        d[:, :max(w // 10, 1)] = 240
        d[:, w - max(w // 12, 1):] = 250
        d[h // 3:h // 2, :] = 20 + (x[h // 3:h // 2] * 60) // max(w, 1)
        d[0, 0] = 0
        d[h - 1, w - 1] = 255
        return d.astype(np.uint8)
    d = ((x * 8) // max(w, 1)) * 12 + (y * 40) // max(h, 1)
    cy, cx, r = h // 2, w // 2, max(min(h, w) // 5, 1)
    d = np.where((y - cy) ** 2 + (x - cx) ** 2 <= r * r, 250, d)
    if kind == "band":
        lo, hi = h // 8, h // 8 + max(h // 16, 3)
        d[lo:hi] = np.where((x[lo:hi] // 2) % 2 == 0, 255, 0)
    elif kind != "disc":
        raise ValueError(kind)
    if seed:
        d = d + np.random.default_rng(seed).integers(0, 3, (h, w))
    return np.clip(d, 0, 255).astype(np.uint8)
