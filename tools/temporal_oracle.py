"""The specification of the temporal depth filter (cs_temporal_depth) in numpy -- a CPU statement of it,
not a capture of any reference: the reference treats every frame alone.

    g_t   = gray value of frame t: (0.2989 R + 0.5870 G) + 0.1140 B for C == 3, the value for C == 1, channel 0 otherwise
    m_t   = mean over the pixels of |g_t - g_{t-1}|        (frame 0 of a call: g_{-1} = the state's prev_raw; none -> no m)
    cut_t = m_t > cut_threshold (a NaN mean is no cut); a frame without predecessor is a cut, its m is 0
    y_t   = g_t                                 if cut_t or not (|g_t - y_{t-1}| < motion_threshold)
          = y_{t-1} + alpha * (g_t - y_{t-1})   otherwise: one product, one sum

y is float32 with every operation rounded once, exactly as the kernels compute it; m is stated in float64 (the kernels add it up
in float32 in a fixed order: tests bound the difference, tests/test_gpu_temporal_depth.py).  alpha and the thresholds are
rounded to float32 first, as the library does.
"""
import numpy as np

F32 = np.float32


class State:
    """prev_raw, prev: the last frame's g and y, float32 [H,W]."""

    def __init__(self, prev_raw, prev):
        self.prev_raw, self.prev = prev_raw, prev


def gray(depth):
    """[N,H,W,C] float32 -> [N,H,W] float32."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 4
    if d.shape[3] == 3:
        return (F32(0.2989) * d[..., 0] + F32(0.5870) * d[..., 1]) + F32(0.1140) * d[..., 2]
    return np.ascontiguousarray(d[..., 0])


def temporal_depth(depth, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08):
    """-> (y float32 [N,H,W], m float64 [N], cut int32 [N], the new State, still bool [N,H,W]: the pixels that took the blend)."""
    g = gray(depth)
    n = g.shape[0]
    a, mt, ct = F32(alpha), F32(motion_threshold), float(F32(cut_threshold))
    y = np.empty_like(g)
    m = np.zeros(n, np.float64)
    cut = np.zeros(n, np.int32)
    still = np.zeros(g.shape, bool)
    prev_raw, prev = (state.prev_raw, state.prev) if state is not None else (None, None)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n):
            if prev_raw is None:
                is_cut = True
            else:
                m[t] = np.abs(g[t].astype(np.float64) - prev_raw.astype(np.float64)).mean()
                is_cut = bool(m[t] > ct)
            cut[t] = is_cut
            if is_cut:
                y[t] = g[t]
            else:
                delta = g[t] - prev
                blend = prev + a * delta
                still[t] = np.abs(delta) < mt
                y[t] = np.where(still[t], blend, g[t])
            prev_raw, prev = g[t], y[t]
    return y, m, cut, State(prev_raw.copy(), prev.copy()), still
