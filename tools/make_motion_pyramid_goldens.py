"""Writes tests/golden/motion_pyramid.npz: the cases of the coarse-to-fine motion search's tests, evaluated by
tools/motion_pyramid_oracle.py.  A CPU evaluation of the specification, NOT a reference capture: the
reference has no temporal filter.

The clips are made here from a seed (make_input: tools/make_motion_goldens.py's moving windows into noise canvases, plus what the
cases below add), so the file stays small: per case it holds vec, sad, matched, m (float64) and cut; meta holds every case's
parameters and the SHA-256 of its y and of its final state, both with every NaN mapped to one pattern (digest_f32).  The
translation cases hold the level-0 vectors of the designed pairs of tests/test_motion_pyramid_surface.py.

Every case keeps each finite m_t at least 1 % away from its cut_threshold (asserted here), so that the cut flags do not hang on
the order in which the kernels add m_t up.

    python tools/make_motion_pyramid_goldens.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_motion_goldens as motion_goldens   # noqa: E402
import make_temporal_goldens as temporal_goldens   # noqa: E402
import motion_oracle   # noqa: E402
import motion_pyramid_oracle as oracle   # noqa: E402

NAN, INF = np.float32(np.nan), np.float32(np.inf)
# the shapes: a level-2 grid of one block / odd planes, clipped blocks and pitches off the 4-byte grid at every level / a parent
# with all four neighbours and grids whose halves are odd / planes smaller than a block at the coarse levels
SHAPES = [(64, 64), (65, 97), (70, 131), (144, 208), (16, 16), (17, 33)]
TRANSLATIONS = [(40, -24), (37, 13), (-52, 6)]
TRANSLATION_SHAPE, TRANSLATION_SEED, TRANSLATION_R, TRANSLATION_SMOOTHNESS = (256, 384), 5, 64, 32


def _case(h, w, tag, c=1, n=5, R=64, smooth=32, match=12, mv=(0, 0), cut=0.3, cut_at=None, change=False, special=False, constant=False,
          alpha=0.37, motion=0.1, amp=0.45):
    return dict(id=f"{h}x{w}_{tag}", h=h, w=w, c=c, n=n, search_range=R, smoothness=smooth, match_threshold=match, mv=list(mv), alpha=alpha,
                motion_threshold=motion, cut_threshold=cut, cut_at=cut_at, change=change, special=False, specials=special, constant=constant,
                ties=False, amp=amp, offset=0, seed=4000 + 7 * h + 13 * w + sum(map(ord, tag)))


def cases():
    out = []
    for h, w in SHAPES:
        out += [
            _case(h, w, "c1_r64", mv=(9, -6), change=True),
            _case(h, w, "c3_r4_l0_m0", c=3, R=4, smooth=0, match=0, mv=(2, -1)),
            _case(h, w, "c1_r120_l4096_m255", R=120, smooth=4096, match=255, mv=(21, 10), n=3),
            _case(h, w, "c1_r120_l0", R=120, smooth=0, mv=(-26, 17), n=3),
            _case(h, w, "c3_r64_cut", c=3, mv=(5, 3), cut_at=2),
            _case(h, w, "c1_r4_beyond", R=4, mv=(12, -9), n=3),              # a global shift beyond R + 3: nothing matches
            _case(h, w, "c1_r64_constant", constant=True, smooth=0, n=3),    # every candidate ties: the order alone decides
            _case(h, w, "c3_r64_special", c=3, mv=(3, 2), special=True, n=3),
        ]
    return out


def specials(h, w):
    """(frame, row, column, channel, value) written into the guide and into channel 0 of the depth of a `specials` case."""
    at = lambda y, x: (y % h, x % w)   # noqa: E731
    guide = [(1, *at(3, 5), 0, NAN), (1, *at(3, 6), 1, INF), (1, *at(3, 7), 2, -INF), (1, *at(4, 5), 0, np.float32(-0.5)),
             (1, *at(4, 6), 1, np.float32(1.5)), (1, *at(4, 7), 2, np.float32(-0.0)), (2, *at(20, 9), 0, NAN), (2, *at(20, 9), 1, NAN),
             (2, *at(20, 9), 2, NAN)]
    depth = [(1, *at(2, 2), NAN), (1, *at(2, 9), INF), (1, *at(6, 3), -INF), (1, *at(7, 7), np.float32(-0.0)), (2, *at(30, 40), NAN),
             (1, *at(9, 1), np.float32(1.75)), (2, *at(11, 4), np.float32(-0.25))]
    return guide, depth


def make_input(case):
    """-> (depth float32 [N,H,W,C], guide float32 [N,H,W,3]): motion_goldens.make_input's clip; constant: one gray guide for every
    frame; specials: NaN, infinities and values outside 0..1 in guide and depth."""
    depth, guide = motion_goldens.make_input(case)
    if case["constant"]:
        guide[:] = np.float32(90.0 / 255.0)
    if case["specials"]:
        g_sp, d_sp = specials(case["h"], case["w"])
        for t, y, x, ch, v in g_sp:
            guide[t, y, x, ch] = v
        for t, y, x, v in d_sp:
            depth[t, y, x, 0] = v
    return depth, guide


def params(case):
    return (case["alpha"], case["motion_threshold"], case["cut_threshold"], case["search_range"], case["smoothness"], case["match_threshold"])


def evaluate(case, depth=None, guide=None, state=None):
    if depth is None:
        depth, guide = make_input(case)
    return oracle.motion_depth(depth, guide, state, *params(case))


def digest_f32(*arrays):
    """SHA-256 of float32 / uint8 arrays with every NaN mapped to one pattern."""
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        if a.dtype == np.float32:
            v = a.view(np.int32).copy()
            v[np.isnan(a)] = 0x7fc00000
            a = v
        out.append(a)
    return temporal_goldens.digest(*out)


def translation_pair(mv):
    """(cur, ref) uint8 [256,384]: uniform noise, seed 5, box-filtered with 9 taps per axis and scaled to 0..255; the current frame
    is the reference displaced by mv = (dx, dy): cur(p) = ref(p + mv) wherever both lie inside the frame."""
    h, w = TRANSLATION_SHAPE
    rng = np.random.RandomState(TRANSLATION_SEED)
    M = 64
    c = rng.uniform(0.0, 1.0, (h + 2 * M + 8, w + 2 * M + 8))
    box = np.ones(9) / 9.0
    c = np.apply_along_axis(lambda r: np.convolve(r, box, "valid"), 1, c)
    c = np.apply_along_axis(lambda r: np.convolve(r, box, "valid"), 0, c)
    c = np.floor((c - c.min()) / (c.max() - c.min()) * 255.0 + 0.5).astype(np.uint8)
    dx, dy = mv
    return np.ascontiguousarray(c[M + dy:M + dy + h, M + dx:M + dx + w]), np.ascontiguousarray(c[M:M + h, M:M + w])


def translation_clip(mv):
    """The pair as a clip of two frames for the filter: (depth [2,H,W,1], guide [2,H,W,3]); equal channels, so L is the code itself."""
    cur, ref = translation_pair(mv)
    lum = np.stack([ref, cur]).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(lum[..., None] * np.float32(0.5)), np.ascontiguousarray(np.repeat(lum[..., None], 3, axis=-1))


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/motion_pyramid_oracle.py (written by tools/make_motion_pyramid_goldens.py); "
                    "not a reference capture", "tool": "tools/make_motion_pyramid_goldens.py", "cases": []}
    for case in cases():
        y, m, cut, state, vec, sad, matched, blended = evaluate(case)
        assert temporal_goldens.margin_ok(m, case["cut_threshold"]), (case["id"], m)
        cid = case["id"]
        for name, a in (("m", m), ("cut", cut), ("vec", vec), ("sad", sad), ("matched", matched)):
            arrays[f"{cid}/{name}"] = a
        meta["cases"].append(dict(case, y_sha256=digest_f32(y), state_sha256=digest_f32(state.prev_raw, state.prev, state.prev_luma),
                                  blended=int(blended.sum()), unmatched=int((matched == 0).sum()), moved=int(vec.any(axis=-1).sum())))
    for mv in TRANSLATIONS:
        cur, ref = translation_pair(mv)
        vec, sad, matched = oracle.pyramid_search(cur, ref, TRANSLATION_R, TRANSLATION_SMOOTHNESS, 12)
        tag = f"translation_{mv[0]}_{mv[1]}"
        arrays[f"{tag}/vec"], arrays[f"{tag}/sad"], arrays[f"{tag}/matched"] = vec, sad, matched
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "motion_pyramid.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
