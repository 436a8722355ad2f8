"""numpy restatement of the reference's Gaussian depth blurs (stereoimage_generation.py :1253-1344): blur_depth_map,
edge_selective_blur_depth_map, left_direction_aware_blur_depth_map, right_direction_aware_blur_depth_map.

The specification of cs_gaussblur.hip.  Vectorised: whole maps per numpy operation, one
operation per arithmetic step of the reference, in its order and precision:
  taps     float64, the reference's own numpy expression (numpy's SIMD exp is not libm's: never recomputed elsewhere)
  one pass replicate borders; float32 samples times float64 taps; the products added one tap at a time in the order of the
           FLIPPED tap array (np.convolve), unfused, from +0.0; the sum rounded to float32
  weights  float32 steps (the 3x3 Sobel sums in float64, in np.sum's pairwise order, rounded to float32)
  blend    (1 - w) * depth + w * blurred: two float32 products and one float32 add
Depth maps are float32 [H, W] (or [B, H, W]: every frame on its own).
"""
import numpy as np

F32 = np.float32
OPS = ("plain", "edge_selective", "left", "right")


def gaussian_taps(sigma):
    """The reference's tap array for a sigma > 0 (float64, 2 * int(3 * sigma) + 1 values)."""
    radius = int(3 * sigma)
    x = np.arange(-radius, radius + 1)
    k = np.exp(-(x ** 2) / (2 * sigma * sigma))
    k /= k.sum()
    return k


def convolve_axis(x, taps, axis):
    """np.convolve(np.pad(line, radius, 'edge'), taps, 'valid') along `axis` of float32 x, for an odd number of float64
    taps (symmetric or not) -> float32."""
    taps = np.asarray(taps, dtype=np.float64)
    n = taps.shape[0]
    assert n % 2 == 1 and x.dtype == F32
    r, length = n // 2, x.shape[axis]
    pad = [(0, 0)] * x.ndim
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode="edge").astype(np.float64)
    flipped = taps[::-1]
    acc = np.zeros(x.shape, dtype=np.float64)
    idx = [slice(None)] * x.ndim
    for j in range(n):
        idx[axis] = slice(j, j + length)
        acc = acc + xp[tuple(idx)] * flipped[j]
    return acc.astype(F32)


def blur_taps(depth, taps):
    """Rows, then columns (the column pass reads the float32 intermediate)."""
    depth = np.asarray(depth)
    assert depth.dtype == F32 and depth.ndim >= 2
    return convolve_axis(convolve_axis(depth, taps, depth.ndim - 1), taps, depth.ndim - 2)


def _shift(p, dy, dx, h, w):
    return p[..., 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def sobel_f32(depth):
    """(grad_x, grad_y): the 3x3 Sobel responses on the edge-padded map; nine float64 products (the zero weights included)
    added in np.sum's order for nine values -- ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), then + p8 -- and
    rounded to float32."""
    h, w = depth.shape[-2:]
    pad = [(0, 0)] * (depth.ndim - 2) + [(1, 1), (1, 1)]
    p = np.pad(depth, pad, mode="edge").astype(np.float64)
    out = []
    for kern in (((-1, 0, 1), (-2, 0, 2), (-1, 0, 1)), ((-1, -2, -1), (0, 0, 0), (1, 2, 1))):
        q = [_shift(p, dy, dx, h, w) * np.float64(kern[dy + 1][dx + 1]) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        s = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) + q[8]
        out.append(s.astype(F32))
    return out[0], out[1]


def weight(depth, op, edge_threshold):
    """The blend weight of a blending operation (float32)."""
    thr = F32(edge_threshold)
    with np.errstate(all="ignore"):
        if op == "edge_selective":
            gx, gy = sobel_f32(depth)
            mag = np.sqrt(gx * gx + gy * gy)
            return np.minimum(mag / thr, F32(1.0))
        pad = [(0, 0)] * (depth.ndim - 1) + [(1, 1)]
        p = np.pad(depth, pad, mode="edge")
        grad = (p[..., 2:] - p[..., :-2]) / F32(2.0)
        if op == "left":
            return np.where(grad > 0, np.minimum(grad / thr, F32(1.0)), F32(0.0))
        if op == "right":
            return np.where(grad < 0, np.minimum(np.abs(grad) / thr, F32(1.0)), F32(0.0))
    raise ValueError(f"unknown operation {op!r}")


def blend(depth, blurred, w):
    return (F32(1.0) - w) * depth + w * blurred


def gaussian_blur_taps(depth, taps, op="plain", edge_threshold=None):
    """cs_gaussian_blur: any odd tap array."""
    depth = np.asarray(depth)
    blurred = blur_taps(depth, taps)
    if op == "plain":
        return blurred
    return blend(depth, blurred, weight(depth, op, edge_threshold)).astype(F32)


def gaussian_blur(depth, sigma, op="plain", edge_threshold=None):
    """engine.gaussian_blur: sigma <= 0 blurs nothing (the blending operations then blend the depth with itself)."""
    taps = gaussian_taps(sigma) if sigma > 0 else np.ones(1)
    return gaussian_blur_taps(depth, taps, op, edge_threshold)


def blur_depth_map(depth, sigma):
    if sigma <= 0:
        return depth
    return gaussian_blur(depth, sigma)


def edge_selective_blur_depth_map(depth, sigma, edge_threshold):
    return gaussian_blur(depth, sigma, "edge_selective", edge_threshold)


def left_direction_aware_blur_depth_map(depth, sigma, edge_threshold):
    return gaussian_blur(depth, sigma, "left", edge_threshold)


def right_direction_aware_blur_depth_map(depth, sigma, edge_threshold):
    return gaussian_blur(depth, sigma, "right", edge_threshold)


# ---- seeded depth maps of the fixtures and the GPU tests (integer / float32 steps only: the same on every machine) -------------
def depth_map(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "codes":        # 8-bit codes in blocks with noise on top
        b = max(2, min(h, w) // 4)
        base = rng.integers(0, 256, (h // b + 1, w // b + 1))
        d = np.repeat(np.repeat(base, b, 0), b, 1)[:h, :w] + rng.integers(-3, 4, (h, w))
        return np.clip(d, 0, 255).astype(F32)
    if kind == "unit":         # k / 255
        return (rng.integers(0, 256, (h, w)).astype(F32) / F32(255.0)).astype(F32)
    if kind == "noise":        # float noise on the 0..255 scale
        return (rng.random((h, w), dtype=F32) * F32(255.0)).astype(F32)
    if kind == "ellipse":      # a gradient with two ellipses on it (integer arithmetic)
        d = (xx * 200) // max(w - 1, 1)
        e1 = (xx - w // 3) ** 2 * max(h, 1) ** 2 + (yy - h // 2) ** 2 * max(w, 1) ** 2 * 4 < (max(w, 1) * max(h, 1)) ** 2 // 9
        e2 = (xx - 3 * w // 4) ** 2 * 9 + (yy - h // 3) ** 2 * 4 < (min(h, w) ** 2)
        d = np.where(e1, 240, d)
        d = np.where(e2, 15, d)
        return d.astype(F32)
    if kind == "flat":
        return np.full((h, w), 77, dtype=F32)
    raise ValueError(kind)
