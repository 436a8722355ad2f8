"""Writes tests/golden/motion_depth.npz: the cases of the motion-compensated temporal depth filter's tests, evaluated by
tools/motion_oracle.py.  A CPU evaluation of the specification, NOT a reference capture: the reference has
no temporal filter.

The clips are made here from a seed (make_input), so the file stays small: per case it holds vec, sad, matched, m (float64) and
cut; meta holds every case's parameters, the SHA-256 of its y and of its final state, and which branches of the specification it
takes, so the tests can tell a drifting oracle or generator from a drifting kernel and can check that every branch is met.

Every case keeps each finite m_t at least 1 % away from its cut_threshold (asserted here), so that the cut flags do not hang on
the order in which the kernels add m_t up.

    python tools/make_motion_goldens.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_temporal_goldens as temporal_goldens   # noqa: E402
import motion_oracle as oracle   # noqa: E402

digest = temporal_goldens.digest
NAN, INF = np.float32(np.nan), np.float32(np.inf)
# (frame, row, column, channel, value) written into the guide and (channel 0 of) the depth of a `special` case
GUIDE_SPECIALS = [(1, 3, 5, 0, NAN), (1, 3, 6, 1, INF), (1, 3, 7, 2, -INF), (1, 4, 5, 0, np.float32(-0.5)), (1, 4, 6, 1, np.float32(1.5)),
                  (1, 4, 7, 2, np.float32(-0.0)), (2, 20, 9, 0, NAN), (2, 20, 9, 1, NAN), (2, 20, 9, 2, NAN)]
DEPTH_SPECIALS = [(1, 2, 2, NAN), (1, 2, 9, INF), (1, 6, 3, -INF), (1, 7, 7, np.float32(-0.0)), (2, 30, 40, NAN)]
TIE_REGION = 48   # the tie clip: five regions of 48 x 48, the centre block of each decides its vector on another key component


def _case(h, w, c=1, n=3, S=16, smooth=32, match=12, mv=(0, 0), cut=0.3, cut_at=None, change=False, special=False, offset=0,
          alpha=0.37, motion=0.1, ties=False, amp=0.45, tag=""):
    cid = f"{h}x{w}_c{c}_s{S}" + (f"_{tag}" if tag else "")
    return dict(id=cid, h=h, w=w, c=c, n=n, search_range=S, smoothness=smooth, match_threshold=match, mv=list(mv), alpha=alpha,
                motion_threshold=motion, cut_threshold=cut, cut_at=cut_at, change=change, special=special, offset=offset, ties=ties, amp=amp,
                seed=2000 + 7 * h + 13 * w + 31 * S + c + sum(map(ord, tag)))


def cases():
    out = [
        _case(16, 16, S=0), _case(16, 16, S=32, mv=(1, 0)),                  # one block; a search range larger than the frame
        _case(17, 33, S=1, mv=(1, -1)), _case(17, 33, S=7, mv=(-2, 1)),      # clipped blocks both ways
        _case(48, 80, S=16, mv=(5, -3), change=True),
        _case(48, 80, S=16, smooth=0, match=0, mv=(5, -3), change=True, tag="l0_m0"),
        _case(48, 80, S=16, smooth=4096, match=255, mv=(5, -3), change=True, tag="l4096_m255"),
        _case(48, 80, S=32, mv=(-20, 11), tag="far"),
        _case(48, 80, S=7, mv=(3, 2), n=4, cut_at=2, tag="cut"),
        _case(48, 80, S=7, mv=(3, 2), special=True, tag="special"),
        _case(48, 80, S=7, mv=(3, 2), offset=1, tag="offgrid"),
        _case(48, 80, S=0, match=255, mv=(1, 1), tag="degenerate"),          # the plain filter: tools/temporal_oracle.py's results
        _case(50, 70, c=3, S=7, mv=(-4, 6), change=True),
        _case(50, 70, c=2, S=1, mv=(1, 0), tag="c2"),
        _case(130, 258, S=16, mv=(9, -7), change=True),                      # five workgroups per block row, shared halos
        # the clip of "moving content is filtered": a pan over depth of high contrast, so few pixels pass the plain filter's test by chance
        _case(96, 128, n=4, S=8, mv=(3, -2), cut=0.6, amp=0.9, tag="scene"),
        _case(TIE_REGION, 5 * TIE_REGION, n=2, S=2, smooth=0, ties=True, tag="ties"),
    ]
    return out


def _tie_luma(rng):
    """(L_0, L_1) uint8 [48, 240]: regions random / flat / f(x + y) / alternating rows / alternating columns."""
    R = TIE_REGION
    ys, xs = np.mgrid[0:R, 0:R]
    f = rng.randint(0, 256, 2 * R + 2)
    a = [rng.randint(0, 256, (R, R)), np.full((R, R), 90), f[xs + ys], np.where(ys % 2 == 0, 40, 200), np.where(xs % 2 == 0, 60, 180)]
    b = [a[0], a[1], f[xs + ys + 1], np.where(ys % 2 == 0, 200, 40), np.where(xs % 2 == 0, 180, 60)]
    return np.concatenate(a, axis=1).astype(np.uint8), np.concatenate(b, axis=1).astype(np.uint8)


def make_input(case):
    """-> (depth float32 [N,H,W,C], guide float32 [N,H,W,3]).  Frame t is a window into noise canvases that moves by `mv` per
    frame, so L_t(p) = L_{t-1}(p + mv) wherever both lie inside the frame; the depth (codes / 255 * amp) moves with it and gets
    +-0.01 of noise per frame.  change: the lower right quarter of the last frame's guide is new noise (blocks without a match).
    cut_at: new canvases from that frame on, the depth 0.5 higher.  special / ties: see above."""
    rng = np.random.RandomState(case["seed"])
    n, h, w, c = case["n"], case["h"], case["w"], case["c"]
    dx, dy = case["mv"]
    M = n * max(abs(dx), abs(dy)) + 1

    def canvases():
        return rng.randint(0, 256, (4, h + 2 * M, w + 2 * M)).astype(np.float32) / np.float32(255.0)

    cv = canvases()
    guide = np.empty((n, h, w, 3), np.float32)
    g = np.empty((n, h, w), np.float32)
    for t in range(n):
        lift = np.float32(0.0)
        if case["cut_at"] is not None and t >= case["cut_at"]:
            if t == case["cut_at"]:
                cv = canvases()
            lift = np.float32(0.5)
        oy, ox = M + t * dy, M + t * dx
        win = cv[:, oy:oy + h, ox:ox + w]
        guide[t] = np.moveaxis(win[:3], 0, -1)
        g[t] = (win[3] * np.float32(case["amp"]) + rng.uniform(-0.01, 0.01, (h, w)).astype(np.float32)) + lift
    if case["change"]:
        guide[n - 1, h // 2:, w // 2:] = rng.randint(0, 256, (h - h // 2, w - w // 2, 3)).astype(np.float32) / np.float32(255.0)
    if case["ties"]:
        for t, lum in enumerate(_tie_luma(rng)):
            guide[t] = (lum.astype(np.float32) / np.float32(255.0))[..., None]     # (equal channels: L is the code itself)
    if c == 1:
        d = g[..., None].copy()
    elif c == 3:
        d = np.stack([g, g * np.float32(0.97), g + np.float32(0.015625)], axis=-1)
    else:
        d = np.stack([g] + [rng.uniform(0, 1, g.shape).astype(np.float32) for _ in range(c - 1)], axis=-1)
    if case["special"]:
        for t, y, x, ch, v in GUIDE_SPECIALS:
            guide[t, y, x, ch] = v
        for t, y, x, v in DEPTH_SPECIALS:
            d[t, y, x, 0] = v
    return np.ascontiguousarray(d, dtype=np.float32), np.ascontiguousarray(guide, dtype=np.float32)


def params(case):
    return (case["alpha"], case["motion_threshold"], case["cut_threshold"], case["search_range"], case["smoothness"], case["match_threshold"])


def evaluate(case, depth=None, guide=None, state=None):
    if depth is None:
        depth, guide = make_input(case)
    return oracle.motion_depth(depth, guide, state, *params(case))


def branches(case, result):
    """Which branches of the specification the case takes (frames with a predecessor only)."""
    y, m, cut, state, vec, sad, matched, blended = result
    h, w = case["h"], case["w"]
    live = np.zeros(len(cut), bool)
    live[1:] = cut[1:] == 0
    ok = np.repeat(np.repeat(matched != 0, 16, axis=1), 16, axis=2)[:, :h, :w]
    return dict(cut=bool(cut[1:].any()), unmatched=bool((matched[live] == 0).any()), moved=bool((ok[live] & ~blended[live]).any()),
                blended=bool(blended.any()), clipped=bool(h % 16 or w % 16), vector=bool(vec[live].any()),
                edge_refused=bool((np.abs(vec[live].astype(int)).max(axis=-1, initial=0) < max(map(abs, case["mv"]))).any()))


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/motion_oracle.py (written by tools/make_motion_goldens.py); "
                    "not a reference capture", "tool": "tools/make_motion_goldens.py", "cases": []}
    for case in cases():
        result = evaluate(case)
        y, m, cut, state, vec, sad, matched, blended = result
        assert temporal_goldens.margin_ok(m, case["cut_threshold"]), (case["id"], m)
        cid = case["id"]
        for name, a in (("m", m), ("cut", cut), ("vec", vec), ("sad", sad), ("matched", matched)):
            arrays[f"{cid}/{name}"] = a
        meta["cases"].append(dict(case, y_sha256=digest(y), state_sha256=digest(state.prev_raw, state.prev, state.prev_luma),
                                  blended=int(blended.sum()), branches=branches(case, result)))
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "motion_depth.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
