"""The specification of the wide-range, coarse-to-fine motion search of the motion-compensated temporal depth filter
(cs_motion_depth_pyramid) in numpy -- a CPU statement of it, not a capture of any reference.

The filter is tools/motion_oracle.py's motion_depth, stated there alone; only the search differs:

    planes      L0 = motion_oracle.luma; L(k+1)(y, x) = (a + b + c + d + 2) >> 2 over the 2 x 2 cell of Lk, Lk edge-replicated to even
                sizes: ceil(h_k / 2) x ceil(w_k / 2), uint8.  Levels 0, 1, 2.
    blocks      16 x 16 from the top-left corner of every level's own plane, clipped at the right and bottom edge; the parent of
                level-k block (by, bx) is level-(k+1) block (by >> 1, bx >> 1), which always exists
    R           search_range, a multiple of 4 in 4..120; the final |dx|, |dy| <= R + 3 <= 123
    level 2     motion_oracle.motion_search(L2_t, L2_{t-1}, R / 4, smoothness, 255): the plain matcher, unchanged
    levels 1, 0 a block's candidates are (0, 0) and, for its parent and the parent's up, down, left and right neighbours that exist
                in the parent grid, 2 v + (ex, ey) with |ex|, |ey| <= 1, v that block's vector one level up: at most 46 distinct
                ones.  A candidate is admissible if every pixel of the block, displaced, lies inside the level's plane ((0, 0)
                always is).  The winner minimises (sad + smoothness (|dx| + |dy|), |dx| + |dy|, |dy|, dy, dx) over the distinct
                admissible candidates: the plain matcher's order on the level's own vector and the level's own SAD.
    outputs     vec, sad (without the penalty) and matched = sad <= match_threshold * npix are level 0's

The state is motion_oracle.State (g, y and L0 of the last frame): the pyramid of its luma is rebuilt per call, so a clip in
sub-batches gives bit for bit what one call gives.

The order is stated twice, as in motion_oracle: key() packs it into one integer (52 bits here: dx + 128 and dy + 128 need 8 bits
each), which refine() minimises and the kernel does; best_vector() is the literal statement on tuples for one block at one level.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_oracle   # noqa: E402,F401
import motion_oracle   # noqa: E402
import temporal_oracle   # noqa: E402,F401

BLOCK = motion_oracle.BLOCK
LEVELS = 3
MIN_SEARCH, MAX_SEARCH, SEARCH_STEP = 4, 120, 4
# the packed key: cost << 31 | (|dx| + |dy|) << 23 | |dy| << 16 | (dy + 128) << 8 | (dx + 128)
# cost <= 255 * 256 + 4096 * 246 < 2^21; |dx| + |dy| <= 246 < 2^8; |dy| <= 123 < 2^7: 52 bits
KEY_COST, KEY_MAG, KEY_ADY, KEY_DY = 31, 23, 16, 8
BIAS = 128
PARENTS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))   # (row, column) steps in the parent grid: the parent, up, down, left, right
OFFSETS = tuple((ex, ey) for ey in (-1, 0, 1) for ex in (-1, 0, 1))


def check_range(search_range):
    v = search_range
    if isinstance(v, bool) or int(v) != v or not MIN_SEARCH <= int(v) <= MAX_SEARCH or int(v) % SEARCH_STEP:
        raise ValueError(f"search_range must be a multiple of {SEARCH_STEP} in {MIN_SEARCH}..{MAX_SEARCH}, got {v}")
    return int(v)


def check_params(search_range, smoothness, match_threshold):
    R = check_range(search_range)
    _, lam, thr = motion_oracle.check_params(0, smoothness, match_threshold)
    return R, lam, thr


def down(plane):
    """uint8 [h,w] -> uint8 [ceil(h / 2), ceil(w / 2)]: the rounded mean of every 2 x 2 cell of the plane, edge-replicated to even sizes."""
    h, w = plane.shape
    p = np.pad(plane.astype(np.int64), ((0, h & 1), (0, w & 1)), mode="edge")
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(plane):
    """L0 -> [L0, L1, L2]."""
    out = [plane]
    for _ in range(LEVELS - 1):
        out.append(down(out[-1]))
    return out


def key(cost, dx, dy):
    """The order (cost, |dx| + |dy|, |dy|, dy, dx) as one int64 (arrays or numbers)."""
    cost, dx, dy = (np.asarray(v, np.int64) for v in (cost, dx, dy))
    return (cost << KEY_COST) | ((np.abs(dx) + np.abs(dy)) << KEY_MAG) | (np.abs(dy) << KEY_ADY) | ((dy + BIAS) << KEY_DY) | (dx + BIAS)


def unkey(k, smoothness):
    """-> (dx, dy, sad) of packed keys."""
    dx = (k & 255) - BIAS
    dy = ((k >> KEY_DY) & 255) - BIAS
    return dx, dy, (k >> KEY_COST) - smoothness * (np.abs(dx) + np.abs(dy))


def block_sads_each(cur, ref, dx, dy):
    """block_sads with a vector of its own per block: dx, dy int64 [Hb,Wb] -> (sad int64 [Hb,Wb], admissible bool [Hb,Wb])."""
    h, w = cur.shape
    hb, wb = motion_oracle.block_grid(h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    sy, sx = ys + dy[ys // BLOCK, xs // BLOCK], xs + dx[ys // BLOCK, xs // BLOCK]
    inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    there = ref[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64)
    diff = np.zeros((hb * BLOCK, wb * BLOCK), np.int64)
    out = np.zeros((hb * BLOCK, wb * BLOCK), np.int64)
    diff[:h, :w] = np.where(inside, np.abs(cur.astype(np.int64) - there), 0)
    out[:h, :w] = ~inside
    return diff.reshape(hb, BLOCK, wb, BLOCK).sum(axis=(1, 3)), out.reshape(hb, BLOCK, wb, BLOCK).sum(axis=(1, 3)) == 0


def refine(cur, ref, parent_vec, smoothness):
    """One frame pair at level 1 or 0, uint8 [h,w] each, and the vectors one level up, int8 [Hp,Wp,2] -> (vec int8 [Hb,Wb,2],
    sad int32 [Hb,Wb])."""
    h, w = cur.shape
    hb, wb = motion_oracle.block_grid(h, w)
    hp, wp = parent_vec.shape[:2]
    assert hp >= -(-hb // 2) and wp >= -(-wb // 2)
    by, bx = np.mgrid[0:hb, 0:wb]
    zero = np.zeros((hb, wb), np.int64)
    sad, ok = block_sads_each(cur, ref, zero, zero)
    assert ok.all()
    best = key(sad, zero, zero)
    for oy, ox in PARENTS:
        qy, qx = (by >> 1) + oy, (bx >> 1) + ox
        exists = (qy >= 0) & (qy < hp) & (qx >= 0) & (qx < wp)
        v = parent_vec[np.clip(qy, 0, hp - 1), np.clip(qx, 0, wp - 1)].astype(np.int64)
        for ex, ey in OFFSETS:
            dx, dy = 2 * v[..., 0] + ex, 2 * v[..., 1] + ey
            sad, ok = block_sads_each(cur, ref, dx, dy)
            k = key(sad + smoothness * (np.abs(dx) + np.abs(dy)), dx, dy)
            best = np.where(exists & ok & (k < best), k, best)
    dx, dy, sad = unkey(best, smoothness)
    return np.stack([dx, dy], axis=-1).astype(np.int8), sad.astype(np.int32)


def candidates(parent_vec, by, bx):
    """The distinct candidates (dx, dy) of block (by, bx), admissible or not: a sorted list."""
    hp, wp = parent_vec.shape[:2]
    out = {(0, 0)}
    for oy, ox in PARENTS:
        qy, qx = (by >> 1) + oy, (bx >> 1) + ox
        if 0 <= qy < hp and 0 <= qx < wp:
            vx, vy = (int(c) for c in parent_vec[qy, qx])
            out.update((2 * vx + ex, 2 * vy + ey) for ex, ey in OFFSETS)
    return sorted(out)


def best_vector(cur, ref, by, bx, parent_vec, smoothness):
    """The literal statement for block (by, bx) of one level: -> ((cost, |dx| + |dy|, |dy|, dy, dx) of the winner, the list of every
    distinct admissible candidate's tuple)."""
    h, w = cur.shape
    y0, x0 = BLOCK * by, BLOCK * bx
    y1, x1 = min(y0 + BLOCK, h), min(x0 + BLOCK, w)
    c = cur[y0:y1, x0:x1].astype(np.int64)
    tuples = []
    for dx, dy in candidates(parent_vec, by, bx):
        if y0 + dy < 0 or y1 + dy > h or x0 + dx < 0 or x1 + dx > w:
            continue
        sad = int(np.abs(c - ref[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int64)).sum())
        tuples.append((sad + smoothness * (abs(dx) + abs(dy)), abs(dx) + abs(dy), abs(dy), dy, dx))
    return min(tuples), tuples


def pyramid_search_levels(cur, ref, search_range, smoothness, match_threshold):
    """One frame pair, uint8 [H,W] each -> [(vec, sad) of level 0, of level 1, of level 2] and matched of level 0."""
    R, lam, thr = check_params(search_range, smoothness, match_threshold)
    pc, pr = pyramid(cur), pyramid(ref)
    vec, sad, _ = motion_oracle.motion_search(pc[2], pr[2], R // 4, lam, 255)
    levels = [(vec, sad)]
    for k in (1, 0):
        vec, sad = refine(pc[k], pr[k], vec, lam)
        levels.insert(0, (vec, sad))
    h, w = cur.shape
    return levels, (levels[0][1] <= thr * motion_oracle.npix(h, w)).astype(np.uint8)


def pyramid_search(cur, ref, search_range, smoothness, match_threshold):
    """motion_oracle.motion_search's counterpart: -> (vec int8 [Hb,Wb,2] of (dx, dy), sad int32 [Hb,Wb], matched uint8 [Hb,Wb])."""
    levels, matched = pyramid_search_levels(cur, ref, search_range, smoothness, match_threshold)
    return levels[0][0], levels[0][1], matched


def motion_depth(depth, guide, state=None, alpha=0.5, motion_threshold=0.1, cut_threshold=0.08, search_range=64, smoothness=32,
                 match_threshold=12):
    """motion_oracle.motion_depth with the search swapped: the same returns."""
    R, lam, thr = check_params(search_range, smoothness, match_threshold)
    return motion_oracle.motion_depth(depth, guide, state, alpha, motion_threshold, cut_threshold,
                                      search=lambda cur, ref: pyramid_search(cur, ref, R, lam, thr))
