"""The specification of the image-guided depth upsampling (cs_guided_depth_plan / cs_guided_depth_apply) in
numpy -- a CPU statement of joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele, SIGGRAPH 2007), restated from the
paper; not a capture of any reference: the reference stretches a smaller depth map bilinearly.

Inputs: image [n,h,w,3] float32 (the guide), depth [n,dh,dw,C] float32 with dh <= h and dw <= w, a radius R in {1, 2, 3}
(K = 2R + 1 taps per axis), sigma_s > 0 in low-resolution pixels, sigma_r > 0 (+inf allowed).  Output [n,h,w] float32.

PLAN (plan()): depends on h, w, dh, dw, R, sigma_s, sigma_r only.  float64, every operation rounded once; integers in int64.
    u        = ((2x + 1) dw - w) / (2w)              one division of the two integers (each converted to float64)
    cx[x]    = floor(u + 0.5)
    wx[x][j] = float32(exp(-(t t) / (2 sigma_s sigma_s))),  t = (cx[x] + j - R) - u,  j = 0..K-1;   (2 sigma_s) sigma_s in that order
    cy, wy   likewise from h, dh
    wr[d]    = float32(exp(-(a a) / (2 sigma_r sigma_r))),  a = d / 255.0,  d = 0..765
    gx[qx]   = min(w - 1, ((2 qx + 1) w) // (2 dw)),  gy likewise: the guide pixel under the centre of a low-resolution sample
exp is the platform's double exp (math.exp here, csm::exp_exact on the device; tests/test_cs_math_host.py holds them together).

APPLY (apply()): float32, every operation rounded once, no product contracted with a sum.
    code(v)  = uint8(trunc(min(max(v, 0), 1) * 255 + 0.5)), NaN -> 0, per channel
    g        = the low-resolution gray: (0.2989 R + 0.5870 G) + 0.1140 B for C == 3, the value for C == 1, channel 0 otherwise
    for pixel (y, x) of frame f, p = code(image[f, y, x]); i = 0..K-1 outer, j = 0..K-1 inner:
        qy = clamp(cy[y] + i - R, 0, dh - 1);  qx = clamp(cx[x] + j - R, 0, dw - 1)
        ws = wy[y][i] * wx[x][j]
        d  = |p.r - q.r| + |p.g - q.g| + |p.b - q.b|,  q = code(image[f, gy[qy], gx[qx]])
        wg = ws * wr[d];  v = g[f, qy, qx]
        num += wg * v;  den += wg;  ns += ws * v;  ds += ws
    out = den > 0 ? num / den : ns / ds        (IEEE division)
The spatial weight uses the unclamped tap position and the index is clamped, so border samples are replicated.  The fallback is
reached when every range weight times its spatial weight has rounded to zero; it is the pure spatial mean.  Non-finite depth
follows the arithmetic (0 * NaN is NaN).
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
RADII = (1, 2, 3)
WR_COUNT = 766


class Plan:
    """cx, cy int32 [w], [h]; wx, wy float32 [w,K], [h,K]; wr float32 [766]; gx, gy int32 [dw], [dh]."""

    def __init__(self, h, w, dh, dw, radius, cx, wx, cy, wy, wr, gx, gy):
        self.h, self.w, self.dh, self.dw, self.radius = h, w, dh, dw, radius
        self.cx, self.wx, self.cy, self.wy, self.wr, self.gx, self.gy = cx, wx, cy, wy, wr, gx, gy


def _check(h, w, dh, dw, radius, sigma_s, sigma_r):
    if min(h, w, dh, dw) < 1:
        raise ValueError("non-positive size")
    if dh > h or dw > w:
        raise ValueError("the depth map is larger than the image")
    if radius not in RADII:
        raise ValueError("the radius must be 1, 2 or 3")
    if not (sigma_s > 0 and sigma_r > 0):
        raise ValueError("sigma_s and sigma_r must be positive")


def _exp32(e):
    """float64 array -> float32(math.exp(e)) element by element."""
    return np.array([math.exp(v) for v in e.ravel()], F64).reshape(e.shape).astype(F32)


def _axis(size, dsize, radius, sigma_s):
    x = np.arange(size, dtype=np.int64)
    with np.errstate(all="ignore"):
        u = ((2 * x + 1) * dsize - size).astype(F64) / F64(2 * size)
        c = np.floor(u + F64(0.5)).astype(np.int64)
        t = (c[:, None] + np.arange(2 * radius + 1, dtype=np.int64)[None, :] - radius).astype(F64) - u[:, None]
        e = -(t * t) / ((F64(2.0) * F64(sigma_s)) * F64(sigma_s))
    return c.astype(np.int32), _exp32(e)


def _guide_index(size, dsize):
    q = np.arange(dsize, dtype=np.int64)
    return np.minimum(size - 1, ((2 * q + 1) * size) // (2 * dsize)).astype(np.int32)


def plan(h, w, dh, dw, radius=2, sigma_s=1.0, sigma_r=0.1):
    h, w, dh, dw, radius, sigma_s, sigma_r = int(h), int(w), int(dh), int(dw), int(radius), float(sigma_s), float(sigma_r)
    _check(h, w, dh, dw, radius, sigma_s, sigma_r)
    cx, wx = _axis(w, dw, radius, sigma_s)
    cy, wy = _axis(h, dh, radius, sigma_s)
    with np.errstate(all="ignore"):
        a = np.arange(WR_COUNT, dtype=np.int64).astype(F64) / F64(255.0)
        e = -(a * a) / ((F64(2.0) * F64(sigma_r)) * F64(sigma_r))
    return Plan(h, w, dh, dw, radius, cx, wx, cy, wy, _exp32(e), _guide_index(w, dw), _guide_index(h, dh))


def code(v):
    """float32 [...] -> uint8 codes."""
    v = np.asarray(v, dtype=F32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(v), F32(0.0), np.minimum(np.maximum(v, F32(0.0)), F32(1.0)))
    return np.trunc(c * F32(255.0) + F32(0.5)).astype(np.uint8)


def gray(depth):
    """[N,dh,dw,C] float32 -> [N,dh,dw] float32."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 4
    if d.shape[3] == 3:
        return (F32(0.2989) * d[..., 0] + F32(0.5870) * d[..., 1]) + F32(0.1140) * d[..., 2]
    return np.ascontiguousarray(d[..., 0])


def apply(image, depth, p, parts=None):
    """image [n,h,w,3], depth [n,dh,dw,C], both float32, p a Plan -> out float32 [n,h,w].  parts: a dict that receives den and
    the smallest non-zero wg of every pixel (what the fixture generator asserts its conditions on)."""
    image, depth = np.asarray(image), np.asarray(depth)
    assert image.dtype == np.float32 and image.ndim == 4 and image.shape[3] == 3 and depth.dtype == np.float32 and depth.ndim == 4
    n, h, w, _ = image.shape
    assert (h, w) == (p.h, p.w) and depth.shape[:3] == (n, p.dh, p.dw)
    R, K = p.radius, 2 * p.radius + 1
    g = gray(depth)
    pc = code(image).astype(np.int32)                                  # [n,h,w,3]
    qc = pc[:, p.gy.astype(np.int64)][:, :, p.gx.astype(np.int64)]     # [n,dh,dw,3]: the guide at the samples' positions
    num, den, ns, ds = (np.zeros((n, h, w), F32) for _ in range(4))
    least = np.full((n, h, w), np.inf, F32)
    cy, cx = p.cy.astype(np.int64), p.cx.astype(np.int64)
    with np.errstate(all="ignore"):
        for i in range(K):
            qy = np.clip(cy + i - R, 0, p.dh - 1)
            for j in range(K):
                qx = np.clip(cx + j - R, 0, p.dw - 1)
                ws = (p.wy[:, i][:, None] * p.wx[:, j][None, :])[None]            # [1,h,w]
                q = qc[:, qy][:, :, qx]                                          # [n,h,w,3]
                d = np.abs(pc - q).sum(axis=3)
                wg = ws * p.wr[d]
                v = g[:, qy][:, :, qx]
                num = num + wg * v
                den = den + wg
                ns = ns + ws * v
                ds = ds + ws
                least = np.where(wg > 0, np.minimum(least, wg), least)
        out = np.where(den > 0, num / den, ns / ds).astype(F32)
    if parts is not None:
        parts["den"], parts["least_wg"] = den, least
    return out


def guided_depth(image, depth, radius=2, sigma_s=1.0, sigma_r=0.1):
    image, depth = np.asarray(image), np.asarray(depth)
    return apply(image, depth, plan(image.shape[1], image.shape[2], depth.shape[1], depth.shape[2], radius, sigma_s, sigma_r))


def bilinear(depth, h, w):
    """What the stereo step does with a smaller depth map today (half-pixel centres, edges clamped), float64 arithmetic rounded to
    float32 at the end: the thing the guided upsampling replaces; for the edge property's contrast only."""
    g = gray(depth).astype(F64)
    n, dh, dw = g.shape
    def taps(size, dsize):
        u = np.clip((np.arange(size) + 0.5) * dsize / size - 0.5, 0.0, dsize - 1.0)
        i0 = np.floor(u).astype(np.int64)
        return i0, np.minimum(i0 + 1, dsize - 1), u - i0
    y0, y1, fy = taps(h, dh)
    x0, x1, fx = taps(w, dw)
    top = g[:, y0][:, :, x0] * (1 - fx) + g[:, y0][:, :, x1] * fx
    bot = g[:, y1][:, :, x0] * (1 - fx) + g[:, y1][:, :, x1] * fx
    return (top * (1 - fy)[None, :, None] + bot * fy[None, :, None]).astype(F32)
