"""The specification of the foreground depth edge dilation (cs_depth_dilate) in numpy -- a CPU statement, the
yardstick of the kernel; not a capture of any reference: the reference has no such pass.

Input: depth [n,h,w,C] float32.  g is its gray map by the contract of comfystereo_amd/csrc/cs_gray4.h:
    (0.2989 R + 0.5870 G) + 0.1140 B for C == 3, the value for C == 1, channel 0 otherwise (float32, every operation rounded once)
Parameters: radius R, an integer in 1..8; shape "square" or "disc"; near "bright" or "dark"; threshold float32 >= 0 (+inf allowed).

WINDOW (offsets()), in integers, no square root:
    square  |dx| <= R and |dy| <= R
    disc    dx dx + dy dy <= R R          (R = 1: the 4-neighbour cross, 5 taps; R = 2: 13; R = 8: 197)
The window is clipped to the frame: pixels outside take no part -- not padded, not reflected, not zero.

ORDER (key()): the monotone key of the depth range clipping, a total order with -0 below +0:
    key(x) = bits(x) ^ 0x80000000 where the sign bit is clear, ~bits(x) otherwise                      (uint32)
NaN pixels are never candidates.
    near = bright   M(p) = the non-NaN g(q) of largest key over p's clipped window
    near = dark     M(p) = the non-NaN g(q) of smallest key

OUTPUT y [n,h,w] float32:
    y(p) = M(p)  if g(p) is not NaN, a candidate exists and M(p) - g(p) >= threshold (dark: g(p) - M(p) >= threshold) -- one
                 float32 subtraction and one comparison, which is false when the difference is NaN (inf - inf)
    y(p) = g(p)  otherwise, bit for bit (a NaN centre keeps its bits)

Consequences: threshold 0 is plain grayscale dilation (dark: erosion); a positive threshold moves only discontinuities and leaves
smooth slopes bit for bit; dark(g) == -bright(-g) bit for bit (negation is exact and key(-x) == ~key(x)).
"""
import numpy as np

F32 = np.float32
RADII = tuple(range(1, 9))
SHAPES = ("square", "disc")
NEARS = ("bright", "dark")


def _check(radius, shape, near, threshold):
    if radius not in RADII:
        raise ValueError("the radius must lie in 1..8")
    if shape not in SHAPES:
        raise ValueError("unknown shape")
    if near not in NEARS:
        raise ValueError("unknown near")
    if not F32(threshold) >= 0:
        raise ValueError("threshold must be >= 0 (+inf allowed)")


def offsets(radius, shape):
    """The window's (dy, dx) pairs, row by row."""
    r = int(radius)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if shape == "square" or dx * dx + dy * dy <= r * r]


def chords(radius):
    """The disc as rows: {dy: a}, a the largest integer with a a + dy dy <= R R; row dy holds |dx| <= a."""
    r = int(radius)
    return {dy: max(a for a in range(r + 1) if a * a + dy * dy <= r * r) for dy in range(-r, r + 1)}


def key(x):
    """float32 array -> uint32 keys."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def value(k):
    """The inverse of key()."""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F32)


def gray(depth):
    """[N,H,W,C] float32 -> [N,H,W] float32."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 4
    if d.shape[3] == 3:
        return (F32(0.2989) * d[..., 0] + F32(0.5870) * d[..., 1]) + F32(0.1140) * d[..., 2]
    return np.ascontiguousarray(d[..., 0])


def window_extreme(g, radius, shape, near):
    """g [n,h,w] float32 -> (M float32 [n,h,w], has bool [n,h,w]: a candidate exists; M is arbitrary where it does not)."""
    n, h, w = g.shape
    bright = near == "bright"
    k = key(g).astype(np.int64)
    nan = np.isnan(g)
    none = np.int64(-1) if bright else np.int64(1) << 32       # beyond every key: "no candidate"
    k[nan] = none
    best = np.full(g.shape, none, np.int64)
    for dy, dx in offsets(radius, shape):
        ys, ye = max(0, -dy), min(h, h - dy)                  # the pixels p whose neighbour p + (dy, dx) lies in the frame
        xs, xe = max(0, -dx), min(w, w - dx)
        if ys >= ye or xs >= xe:
            continue
        cand = k[:, ys + dy:ye + dy, xs + dx:xe + dx]
        into = best[:, ys:ye, xs:xe]
        into[...] = np.maximum(into, cand) if bright else np.minimum(into, cand)
    has = best != none
    return value(np.where(has, best, 0).astype(np.uint32)), has


def dilate_gray(g, radius=2, shape="disc", near="bright", threshold=0.04):
    """The pass on a gray map g [n,h,w] float32 -> y [n,h,w] float32."""
    _check(radius, shape, near, threshold)
    g = np.ascontiguousarray(g, dtype=F32)
    assert g.ndim == 3 and g.size > 0
    thr = F32(threshold)
    m, has = window_extreme(g, radius, shape, near)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (m - g) if near == "bright" else (g - m)       # float32, one subtraction
        take = has & ~np.isnan(g) & (diff >= thr)             # (a NaN difference compares false)
    return np.where(take, m, g).astype(F32)


def dilate(depth, radius=2, shape="disc", near="bright", threshold=0.04):
    """depth [n,h,w,C] float32 -> y [n,h,w] float32."""
    return dilate_gray(gray(depth), radius, shape, near, threshold)
