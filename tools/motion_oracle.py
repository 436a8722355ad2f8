"""The specification of the motion-compensated temporal depth filter (cs_motion_depth) in numpy -- a CPU
statement of it, not a capture of any reference: the reference treats every frame alone.

It is tools/temporal_oracle.py's filter with one change: y_{t-1} is read where the pixel's 16 x 16 block came from, found by a
full-search block matcher on the 8-bit luma of the clip's colour frames.

Inputs: depth [N,H,W,C] float32, guide [N,H,W,3] float32 (the colour frames at the depth's size).
    g_t, m_t, cut_t   tools/temporal_oracle.py's, on the unwarped g, unchanged
    code(v)           tools/guided_oracle.py's: uint8(trunc(min(max(v, 0), 1) * 255 + 0.5)), NaN -> 0
    L                 (77 R + 150 G + 29 B + 128) >> 8 on the three codes, in integers: uint8
    blocks            16 x 16 from the top-left corner, clipped at the right and bottom edge: Hb = ceil(H / 16), Wb = ceil(W / 16);
                      npix = a block's real pixel count
    candidates        the integer (dx, dy) with |dx|, |dy| <= S (search_range, 0..32) for which every pixel of the block, displaced,
                      lies inside the frame: (0, 0) is always one
    sad(dx, dy)       sum over the block's pixels p of |L_t(p) - L_{t-1}(p + (dx, dy))|
    cost              sad + smoothness * (|dx| + |dy|), smoothness an integer 0..4096
    v_t(block)        the candidate that minimises (cost, |dx| + |dy|, |dy|, dy, dx) lexicographically: a total order
    matched           sad(v) <= match_threshold * npix (an integer 0..255; the SAD without the penalty)
    q                 y_{t-1}(p + v_t(block(p)))
    y_t(p)            g_t(p)                       if cut_t, or the block is unmatched, or not (|g_t(p) - q| < motion_threshold)
                      q + alpha * (g_t(p) - q)     otherwise: one product, one sum, float32, rounded once
Frame 0 of a call takes L_{-1}, g_{-1} and y_{-1} from the state; without one it is a cut, its vectors are 0, its SADs 0 and its
blocks matched.  The vectors of a cut frame with a predecessor are computed and reported all the same.

With search_range 0 and match_threshold 255 every vector is (0, 0) and every block matched (a SAD is at most 255 npix): y, m, cut
and the float state are tools/temporal_oracle.py's bit for bit.

The order is stated twice: key() packs it into one integer, which is what motion_search minimises (and what the kernel does);
best_vector() is the literal statement on tuples, for one block, that tests hold key() against.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_oracle   # noqa: E402
import temporal_oracle   # noqa: E402

F32 = np.float32
BLOCK = 16
MAX_SEARCH = 32
MAX_SMOOTHNESS = 4096
# the packed key: cost << 27 | (|dx| + |dy|) << 20 | |dy| << 14 | (dy + 32) << 7 | (dx + 32); cost <= 255 * 256 + 4096 * 64 < 2^19
KEY_COST, KEY_MAG, KEY_ADY, KEY_DY = 27, 20, 14, 7


class State:
    """prev_raw, prev: the last frame's g and y, float32 [H,W]; prev_luma: its luma, uint8 [H,W]."""

    def __init__(self, prev_raw, prev, prev_luma):
        self.prev_raw, self.prev, self.prev_luma = prev_raw, prev, prev_luma


def luma(guide):
    """[N,H,W,3] float32 -> [N,H,W] uint8."""
    c = guided_oracle.code(np.asarray(guide)).astype(np.int64)
    assert c.ndim == 4 and c.shape[3] == 3
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def check_params(search_range, smoothness, match_threshold):
    for name, v, hi in (("search_range", search_range, MAX_SEARCH), ("smoothness", smoothness, MAX_SMOOTHNESS),
                        ("match_threshold", match_threshold, 255)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in 0..{hi}, got {v}")
    return int(search_range), int(smoothness), int(match_threshold)


def key(cost, dx, dy):
    """The order (cost, |dx| + |dy|, |dy|, dy, dx) as one int64 (arrays or numbers)."""
    cost, dx, dy = (np.asarray(v, np.int64) for v in (cost, dx, dy))
    return (cost << KEY_COST) | ((np.abs(dx) + np.abs(dy)) << KEY_MAG) | (np.abs(dy) << KEY_ADY) | ((dy + 32) << KEY_DY) | (dx + 32)


def block_grid(h, w):
    return -(-h // BLOCK), -(-w // BLOCK)


def npix(h, w):
    """[Hb,Wb] int64: every block's real pixel count."""
    hb, wb = block_grid(h, w)
    bh = np.minimum(BLOCK, h - BLOCK * np.arange(hb))
    bw = np.minimum(BLOCK, w - BLOCK * np.arange(wb))
    return (bh[:, None] * bw[None, :]).astype(np.int64)


def block_sads(cur, ref, dx, dy):
    """sad(dx, dy) of every block, int64 [Hb,Wb], and which blocks have (dx, dy) as a valid candidate, bool [Hb,Wb]."""
    h, w = cur.shape
    hb, wb = block_grid(h, w)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    diff = np.zeros((hb * BLOCK, wb * BLOCK), np.int64)
    if y1 > y0 and x1 > x0:
        diff[y0:y1, x0:x1] = np.abs(cur[y0:y1, x0:x1].astype(np.int64) - ref[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int64))
    sad = diff.reshape(hb, BLOCK, wb, BLOCK).sum(axis=(1, 3))
    by0 = BLOCK * np.arange(hb)
    bx0 = BLOCK * np.arange(wb)
    by1, bx1 = np.minimum(by0 + BLOCK, h), np.minimum(bx0 + BLOCK, w)
    ok_y = (by0 + dy >= 0) & (by1 + dy <= h)
    ok_x = (bx0 + dx >= 0) & (bx1 + dx <= w)
    return sad, ok_y[:, None] & ok_x[None, :]


def motion_search(cur, ref, search_range, smoothness, match_threshold):
    """One frame pair, uint8 [H,W] each -> (vec int8 [Hb,Wb,2] of (dx, dy), sad int32 [Hb,Wb], matched uint8 [Hb,Wb])."""
    S, lam, thr = check_params(search_range, smoothness, match_threshold)
    h, w = cur.shape
    hb, wb = block_grid(h, w)
    best = np.full((hb, wb), np.iinfo(np.int64).max, np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            sad, ok = block_sads(cur, ref, dx, dy)
            k = key(sad + lam * (abs(dx) + abs(dy)), dx, dy)
            best = np.where(ok & (k < best), k, best)
    dx = (best & 127) - 32
    dy = ((best >> KEY_DY) & 127) - 32
    sad = (best >> KEY_COST) - lam * (np.abs(dx) + np.abs(dy))
    vec = np.stack([dx, dy], axis=-1).astype(np.int8)
    return vec, sad.astype(np.int32), (sad <= thr * npix(h, w)).astype(np.uint8)


def best_vector(cur, ref, by, bx, search_range, smoothness):
    """The literal statement for block (by, bx): -> ((cost, |dx| + |dy|, |dy|, dy, dx) of the winner, the list of every valid
    candidate's tuple)."""
    h, w = cur.shape
    y0, x0 = BLOCK * by, BLOCK * bx
    y1, x1 = min(y0 + BLOCK, h), min(x0 + BLOCK, w)
    c = cur[y0:y1, x0:x1].astype(np.int64)
    tuples = []
    for dy in range(-search_range, search_range + 1):
        for dx in range(-search_range, search_range + 1):
            if y0 + dy < 0 or y1 + dy > h or x0 + dx < 0 or x1 + dx > w:
                continue
            sad = int(np.abs(c - ref[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int64)).sum())
            tuples.append((sad + smoothness * (abs(dx) + abs(dy)), abs(dx) + abs(dy), abs(dy), dy, dx))
    return min(tuples), tuples


def gather(prev, vec):
    """q [H,W]: prev at p + v(block(p))."""
    h, w = prev.shape
    ys, xs = np.mgrid[0:h, 0:w]
    v = vec.astype(np.int64)
    return prev[ys + v[ys // BLOCK, xs // BLOCK, 1], xs + v[ys // BLOCK, xs // BLOCK, 0]]


def motion_depth(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=16, smoothness=32,
                 match_threshold=12, search=None):
    """-> (y float32 [N,H,W], m float64 [N], cut int32 [N], the new State, vec int8 [N,Hb,Wb,2], sad int32 [N,Hb,Wb],
    matched uint8 [N,Hb,Wb], blended bool [N,H,W]: the pixels that took the blend).
    search: None for the full search above, or another one, search(cur, ref) -> (vec, sad, matched) on two uint8 [H,W] lumas with its
    own parameters bound and checked (tools/motion_pyramid_oracle.py): the filter around it is stated here alone."""
    if search is None:
        S, lam, thr = check_params(search_range, smoothness, match_threshold)

        def search(cur, ref):
            return motion_search(cur, ref, S, lam, thr)
    g = temporal_oracle.gray(depth)
    lum = luma(guide)
    n, h, w = g.shape
    assert lum.shape == g.shape
    hb, wb = block_grid(h, w)
    a, mt, ct = F32(alpha), F32(motion_threshold), float(F32(cut_threshold))
    y = np.empty_like(g)
    m = np.zeros(n, np.float64)
    cut = np.zeros(n, np.int32)
    vec = np.zeros((n, hb, wb, 2), np.int8)
    sad = np.zeros((n, hb, wb), np.int32)
    matched = np.ones((n, hb, wb), np.uint8)
    blended = np.zeros(g.shape, bool)
    prev_raw, prev, prev_luma = (state.prev_raw, state.prev, state.prev_luma) if state is not None else (None, None, None)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n):
            if prev_raw is None:
                is_cut = True
            else:
                m[t] = np.abs(g[t].astype(np.float64) - prev_raw.astype(np.float64)).mean()
                is_cut = bool(m[t] > ct)
                vec[t], sad[t], matched[t] = search(lum[t], prev_luma)
            cut[t] = is_cut
            if is_cut:
                y[t] = g[t]
            else:
                q = gather(prev, vec[t])
                delta = g[t] - q
                blend = q + a * delta
                ok = np.repeat(np.repeat(matched[t] != 0, BLOCK, axis=0), BLOCK, axis=1)[:h, :w]
                blended[t] = ok & (np.abs(delta) < mt)
                y[t] = np.where(blended[t], blend, g[t])
            prev_raw, prev, prev_luma = g[t], y[t], lum[t]
    return y, m, cut, State(prev_raw.copy(), prev.copy(), prev_luma.copy()), vec, sad, matched, blended
