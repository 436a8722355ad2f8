"""numpy float32 restatement of the reference's grid-sample warps (stereoimage_generation.py: apply_stereo_divergence_gpu,
warp_and_fill_gpu, compute_forward_mask_gpu, detect_disocclusions_gpu, interpolate_fill_gpu,
apply_stereo_divergence_gpu_with_fill) -- TEST INFRASTRUCTURE, the checker of the cs_gridwarp kernels.

Written from the rules in DESIGN.md section 2 (grid-sample warps), not from the reference's lines.  Every step is one float32
operation in the order CPU torch evaluates it (numpy float32 arithmetic does not contract).  The only torch primitive it calls
is `torch.pow` (CPU, scalar exponent) for the exponents torch does not special-case; `grid_sample` is restated here as well (bilinear with the zeros /
border / reflection paddings and nearest, align_corners=True) and tests/test_grid_surface.py holds it against CPU torch.
Canonical shapes: image [B,C,H,W], depth [B,H,W]; the layout quirks of the module functions are the callers' business.
"""
import numpy as np
import torch

F32 = np.float32
PADDINGS = ("border", "zeros", "reflection")
STRETCH_PIXELS = 3
# the two operations whose edge cases the designed inputs of tools/grid_edge_inputs.py sit on, as names, so that
# tests/test_grid_edges_surface.py can put a wrong one in their place and see the designed cases notice
rint = np.rint            # nearest sampling rounds half to even
above = np.greater        # every threshold is a strict comparison


def linspace(n):
    """torch.linspace(-1, 1, n) (float32): step = 2 / (n - 1) in float32; the lower half start + step * i, the upper half
    end - step * (n - 1 - i), each a single rounding (a fused multiply-add)."""
    if n == 1:
        return np.array([-1.0], dtype=F32)
    step = np.float64(F32(2.0) / F32(n - 1))
    i = np.arange(n, dtype=np.float64)
    lo = (step * i - 1.0).astype(F32)            # exact in float64, then one rounding
    hi = (1.0 - step * (n - 1 - i)).astype(F32)
    return np.where(np.arange(n) < n // 2, lo, hi)


def fma32(a, b, c):
    """float32 fused multiply-add a * b + c (one rounding), exact: the product is exact in float64, the sum is an error-free
    TwoSum, and a float64 sum that sits exactly on a float32 midpoint is resolved by the sign of its error term.  An infinite or
    NaN sum (an infinite operand, inf * 0, inf - inf) is the float64 result as it stands: there is no midpoint to resolve."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bv = s - p
        err = (p - (s - bv)) + (c - bv)
        r = s.astype(F32)
        diff = s - r.astype(np.float64)
        nb = np.nextafter(r, np.where(diff > 0, F32(np.inf), F32(-np.inf))).astype(F32)
        mid = (r.astype(np.float64) + nb.astype(np.float64)) * 0.5
        past = np.isfinite(diff) & (s == mid) & (diff != 0) & (err != 0) & ((err > 0) == (diff > 0))
    return np.where(past, nb, r).astype(F32)


def _pow(ax, e):
    """torch.pow(ax, e) for a scalar exponent: torch's special cases (1, 0.5, 2, 3, 0) restated in numpy, so that the result does
    not depend on the CPU torch runs on; every other exponent through CPU torch itself."""
    ax = np.ascontiguousarray(ax, dtype=F32)
    if e == 1.0:
        return ax.copy()
    if e == 0.5:
        return np.sqrt(ax)
    if e == 2.0:
        return ax * ax
    if e == 3.0:
        return ax * ax * ax
    if e == 0.0:
        return np.ones_like(ax)
    return torch.pow(torch.from_numpy(ax), float(e)).numpy()


def pixel_offset(depth, div, sep, e, conv):
    """depth [B,H,W] -> pixel offsets [B,H,W]: the batch is divided by 255 when any value is above 1, then each frame is
    normalised by its own min / max (zero when the range is not above 1e-6), shifted by the convergence point and curved."""
    d = np.asarray(depth, dtype=F32)
    b = d.shape[0]
    if above(d.reshape(b, -1).max(1), F32(1.0)).any():
        d = d / F32(255.0)
    mn = d.reshape(b, -1).min(1)[:, None, None]
    mx = d.reshape(b, -1).max(1)[:, None, None]
    rng = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        nd = np.where(above(rng, F32(1e-6)), (d - mn) / np.maximum(rng, F32(1e-6)), F32(0.0)).astype(F32)
    s = nd - F32(conv)
    od = np.sign(s) * _pow(np.abs(s), e)
    return od * F32(div) + F32(sep)


def grid_x(po):
    """linspace(-1, 1, W) - offset / (W / 2)"""
    w = po.shape[-1]
    return linspace(w) - po / F32(w / 2)


def forward_gap_mask(po):
    """Forward gap mask of offsets [B,H,W]: a column is a gap when no source column's trunc(col + offset) lands on it, then the
    gap spreads one column to a neighbour where the offset difference of adjacent SOURCE columns is above 1.5."""
    b, h, w = po.shape
    dest = np.arange(w, dtype=F32) + po
    ok = (dest > F32(-1.0)) & (dest < F32(w))
    hit = np.zeros((b, h, w), dtype=bool)
    bi, yi, _ = np.nonzero(ok)
    hit[bi, yi, np.trunc(dest[ok]).astype(np.int64)] = True
    gap = ~hit
    grad = above(np.abs(po[:, :, 1:] - po[:, :, :-1]), F32(1.5))
    edge = np.zeros((b, h, w), dtype=bool)
    edge[:, :, :-1] = grad
    edge[:, :, 1:] |= grad
    out = gap.copy()
    out[:, :, 1:] |= gap[:, :, :-1] & edge[:, :, 1:]
    out[:, :, :-1] |= gap[:, :, 1:] & edge[:, :, :-1]
    return out


def borders(valid):
    """valid [..., W] -> (left, right): left = nearest valid column at or before c, right = the row's LAST valid column when
    it is at or after c (not the nearest one); -1 where there is none."""
    w = valid.shape[-1]
    cols = np.arange(w, dtype=np.int64)
    left = np.maximum.accumulate(np.where(valid, cols, -1), axis=-1)
    last = np.where(valid, cols, -1).max(-1, keepdims=True)
    right = np.where(last >= cols, last, -1)
    return left, right


def stretch_grid(gx, gap):
    """warp_and_fill_gpu's edge stretch: the grid x of gap pixels from the border grid values 3 columns apart."""
    w = gx.shape[-1]
    left, right = borders(~gap)
    cols = np.arange(w, dtype=np.int64)
    ld = (cols - left).astype(F32)
    rd = (right - cols).astype(F32)
    total = np.maximum(ld + rd, F32(1.0))
    half = total * F32(0.5)
    take = lambda idx: np.take_along_axis(gx, np.clip(idx, 0, w - 1), axis=-1)   # noqa: E731
    lt = np.clip(ld / half, F32(0.0), F32(1.0))
    ls = take(left) * (F32(1.0) - lt) + take(left - STRETCH_PIXELS) * lt
    rt = np.clip(rd / half, F32(0.0), F32(1.0))
    rs = take(right) * (F32(1.0) - rt) + take(right + STRETCH_PIXELS) * rt
    t = ld / total
    t = np.where(left < 0, F32(1.0), t)
    t = np.where(right < 0, F32(0.0), t)
    bl = np.clip((t - F32(0.35)) / F32(0.3), F32(0.0), F32(1.0))
    bl = bl * bl * (F32(3.0) - F32(2.0) * bl)
    g = ls * (F32(1.0) - bl) + rs * bl
    return np.where(gap, g, gx).astype(F32)


def source_coord(g, size, padding):
    """grid_sample's unnormalisation (align_corners=True) and padding of one axis.  The clip of border and reflection padding
    takes a NaN coordinate to 0 (CPU torch orders its clamp so; an infinite grid value reflects to NaN: inf - inf * span)."""
    with np.errstate(invalid="ignore"):
        x = (np.asarray(g, dtype=F32) + F32(1.0)) * (F32(size - 1) / F32(2.0))
        if padding == "reflection":
            if size <= 1:
                x = np.zeros_like(x)
            else:
                span = F32(size - 1) * F32(2.0)
                a = np.abs(x)
                flips = np.trunc(a / span)
                extra = fma32(-flips, span, a)
                x = np.minimum(extra, span - extra)
        if padding in ("border", "reflection"):
            x = np.minimum(np.fmax(x, F32(0.0)), F32(size - 1))
    return x.astype(F32)


def sample_bilinear(img, gx, gy, padding="border"):
    """F.grid_sample(img, stack([gx, gy], -1), 'bilinear', padding, align_corners=True); img [B,C,H,W], gx / gy [B,Ho,Wo]."""
    b, c, h, w = img.shape
    x = source_coord(gx, w, padding)
    y = source_coord(gy, h, padding)
    with np.errstate(invalid="ignore"):
        xw, yn = np.floor(x), np.floor(y)
        wt = x - xw
        et = F32(1.0) - wt
        nt = y - yn
        st = F32(1.0) - nt
        weights = (st * et, st * wt, nt * et, nt * wt)
        out = None
        bi = np.arange(b)[:, None, None]
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            xi, yi = xw + F32(dx), yn + F32(dy)
            inb = (xi > F32(-1.0)) & (xi < F32(w)) & (yi > F32(-1.0)) & (yi < F32(h))
            xs = np.where(inb, xi, F32(0.0)).astype(np.int64)
            ys = np.where(inb, yi, F32(0.0)).astype(np.int64)
            v = np.where(inb[:, None], img[bi, :, ys, xs].transpose(0, 3, 1, 2), F32(0.0))
            out = v * weights[k][:, None] if out is None else fma32(v, weights[k][:, None], out)
    return out.astype(F32)


def sample_nearest(img, gx, gy, padding="border"):
    """F.grid_sample(..., mode='nearest', align_corners=True): coordinates rounded half to even."""
    b, c, h, w = img.shape
    x = rint(source_coord(gx, w, padding))
    y = rint(source_coord(gy, h, padding))
    inb = (x > F32(-1.0)) & (x < F32(w)) & (y > F32(-1.0)) & (y < F32(h))
    xs = np.where(inb, x, F32(0.0)).astype(np.int64)
    ys = np.where(inb, y, F32(0.0)).astype(np.int64)
    bi = np.arange(b)[:, None, None]
    return np.where(inb[:, None], img[bi, :, ys, xs].transpose(0, 3, 1, 2), F32(0.0)).astype(F32)


def _grid_y(b, h, w):
    return np.broadcast_to(linspace(h)[None, :, None], (b, h, w))


# ---- the six functions --------------------------------------------------------------------------------------------------
def apply_stereo_divergence_gpu(img, depth, div, sep, e, conv=0.5):
    b, _, h, w = img.shape
    gx = grid_x(pixel_offset(depth, div, sep, e, conv))
    return sample_bilinear(img, gx, _grid_y(b, h, w), "border")


def warp_and_fill_gpu(img, depth, div, sep, e, conv=0.5):
    b, _, h, w = img.shape
    po = pixel_offset(depth, div, sep, e, conv)
    gap = forward_gap_mask(po)
    gx = stretch_grid(grid_x(po), gap)
    return sample_bilinear(img, gx, _grid_y(b, h, w), "border"), gap


def compute_forward_mask_gpu(depth, div, sep, e, conv):
    return forward_gap_mask(pixel_offset(depth, div, sep, e, conv))


def detect_disocclusions_gpu(depth, grid, gxw, threshold=0.02):
    """depth [H,W], grid [1,H,W,2], gxw [H,W] -> bool [H,W]"""
    h, w = depth.shape
    if w < 2:
        raise IndexError("detect_disocclusions_gpu needs W >= 2 (the last column copies the one before it)")
    wd = sample_nearest(np.asarray(depth, F32)[None, None], grid[..., 0], grid[..., 1], "border")[0, 0]
    deep = above(wd - depth, F32(threshold))
    grad = np.empty((h, w), dtype=F32)
    grad[:, :-1] = np.abs(gxw[:, 1:] - gxw[:, :-1])
    grad[:, -1] = grad[:, -2]
    return deep | above(grad, F32(2.0 / w * 3.0))


def interpolate_fill_gpu(img, mask):
    """img [B,C,H,W], mask bool [B,H,W] (True = fill) -> filled"""
    w = img.shape[-1]
    left, right = borders(~mask)
    cols = np.arange(w, dtype=np.int64)
    ld = (cols - left).astype(F32)
    rd = (right - cols).astype(F32)
    t = ld / np.maximum(ld + rd, F32(1.0))
    t = np.where(left < 0, F32(1.0), t)
    t = np.where(right < 0, F32(0.0), t)
    lc = np.take_along_axis(img, np.clip(left, 0, w - 1)[:, None], axis=-1)
    rc = np.take_along_axis(img, np.clip(right, 0, w - 1)[:, None], axis=-1)
    t = t[:, None]
    return np.where(mask[:, None], lc * (F32(1.0) - t) + rc * t, img).astype(F32)


def apply_stereo_divergence_gpu_with_fill(img, depth, div, sep, e, conv=0.5, fill_mode="border"):
    """img [C,H,W], depth [H,W] (one frame: normalised over the whole tensor) -> (warped [C,H,W], valid [H,W])"""
    c, h, w = img.shape
    gx = grid_x(pixel_offset(np.asarray(depth, F32)[None], div, sep, e, conv))
    pad = fill_mode if fill_mode in PADDINGS else "border"
    out = sample_bilinear(np.asarray(img, F32)[None], gx, _grid_y(1, h, w), pad)[0]
    return out, ((gx >= F32(-1.0)) & (gx <= F32(1.0)))[0]


# ---- seeded integer-only inputs (bit-identical on every machine: no libm) --------------------------------------------------
def block_depth_u8(h, w, seed, block=40):
    """uint8 depth [h, w]: random plateaus of block x block pixels over an integer ramp (sharp steps -> disocclusions)."""
    rng = np.random.default_rng(seed)
    tiles = rng.integers(0, 160, (h // block + 1, w // block + 1))
    plateau = np.repeat(np.repeat(tiles, block, 0), block, 1)[:h, :w]
    ramp = (np.arange(w)[None, :] * 96) // max(w, 1)
    return (plateau + ramp).astype(np.uint8)


def block_image_u8(c, h, w, seed):
    """uint8 image [c, h, w]: integer gradients plus seeded noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (3 + k) + y * (5 + 2 * k)) % 256 for k in range(c)])
    return ((base + rng.integers(0, 32, (c, h, w))) % 256).astype(np.uint8)
