"""The specification of the depth range clipping (cs_depth_range) in numpy -- a CPU statement of it, not a
capture of any reference: the reference normalises every frame by its own extremes.

    g_t      = gray value of frame t: (0.2989 R + 0.5870 G) + 0.1140 B for C == 3, the value for C == 1, channel 0 otherwise
    key(x)   = bits(x) ^ 0x80000000 if the sign bit is clear, else ~bits(x): uint32, monotone in x; -0 sorts below +0, the
               infinities and NaNs where their bits put them
    raw_lo_t = the element of g_t whose key has rank rank_lo (0-based) among the frame's H * W keys: np.sort(keys)[rank_lo]
               mapped back, the element's own bits; raw_hi_t likewise for rank_hi
    lo_t     = raw_lo_t if frame t has no predecessor, if cut[t] != 0 or if s is not finite,
               else s = lo_{t-1} + beta * (raw_lo_t - lo_{t-1}): one difference, one product, one sum.  hi_t likewise.
    y        = g where g is NaN; else (g < lo_t ? lo_t : g), and then hi_t where that exceeds hi_t -- comparisons, so a NaN bound
               clamps nothing and lo_t > hi_t has a defined result (hi_t wherever g <= hi_t or g < lo_t)
    normalize: y = 0 where hi_t == lo_t, else (y - lo_t) / (hi_t - lo_t): one subtraction, one correctly rounded division

float32 with every operation rounded once, exactly as the kernels compute it.  beta is rounded to float32 first, as the library
does.  beta = 1 returns the raw bounds wherever raw - prev is exact (any raw within a factor 2 of prev); elsewhere the two
roundings of the stated formula leave the bound within 2^-22 max(|raw|, |prev|) of raw.

The Python layers derive the ranks from the clip fractions in float64 (ranks_of): rank_lo = floor(clip_low * (H * W - 1)),
rank_hi = (H * W - 1) - floor(clip_high * (H * W - 1)), 0 <= clip < 0.5, so rank_lo <= rank_hi; clip = 0 gives the minimum / maximum.
"""
import math

import numpy as np

F32 = np.float32


class State:
    """lo, hi: the last frame's bounds, float32 scalars."""

    def __init__(self, lo, hi):
        self.lo, self.hi = F32(lo), F32(hi)


def gray(depth):
    """[N,H,W,C] float32 -> [N,H,W] float32."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 4
    if d.shape[3] == 3:
        return (F32(0.2989) * d[..., 0] + F32(0.5870) * d[..., 1]) + F32(0.1140) * d[..., 2]
    return np.ascontiguousarray(d[..., 0])


def key(x):
    """float32 array -> uint32 keys."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 == 0, u ^ np.uint32(0x80000000), ~u)


def unkey(k):
    """uint32 keys -> the float32 values they came from, bit for bit."""
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 == 1, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def ranks_of(clip_low, clip_high, count):
    """The two 0-based ranks among `count` keys, from the clip fractions, in float64."""
    if not (0.0 <= clip_low < 0.5 and 0.0 <= clip_high < 0.5):
        raise ValueError("the clip fractions must lie in [0, 0.5)")
    last = count - 1
    return int(math.floor(clip_low * last)), last - int(math.floor(clip_high * last))


def select(g, rank):
    """[N,H,W] float32, one rank -> float32 [N]: per frame the element whose key has that rank."""
    k = np.sort(key(g).reshape(g.shape[0], -1), axis=1)
    return unkey(k[:, rank])


def smooth(raw, prev, beta, take_raw):
    """One step of one bound, float32 scalars."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = F32(prev + F32(beta * F32(raw - prev)))
    return raw if (take_raw or not np.isfinite(s)) else s


def depth_range(depth, state=None, rank_lo=0, rank_hi=0, beta=1.0, cut=None, normalize=False):
    """-> (y float32 [N,H,W], lo, hi, raw_lo, raw_hi float32 [N], the new State)."""
    g = gray(depth)
    n = g.shape[0]
    assert 0 <= rank_lo <= rank_hi < g[0].size
    b = F32(beta)
    raw_lo, raw_hi = select(g, rank_lo), select(g, rank_hi)
    lo, hi = np.empty(n, F32), np.empty(n, F32)
    plo, phi = (state.lo, state.hi) if state is not None else (None, None)
    for t in range(n):
        take_raw = plo is None or (cut is not None and cut[t] != 0)
        plo = smooth(raw_lo[t], F32(0) if plo is None else plo, b, take_raw)
        phi = smooth(raw_hi[t], F32(0) if phi is None else phi, b, take_raw)
        lo[t], hi[t] = plo, phi
    l, h = lo[:, None, None], hi[:, None, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        y = np.where(g < l, l, g)
        y = np.where(y > h, h, y).astype(F32)
        if normalize:
            y = np.where(h == l, F32(0), (y - l) / (h - l)).astype(F32)
    return y, lo, hi, raw_lo, raw_hi, State(lo[-1], hi[-1])
