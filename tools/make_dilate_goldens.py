"""Writes tests/golden/depth_dilate.npz: the cases of the depth edge dilation's tests, evaluated by tools/dilate_oracle.py.
A CPU evaluation of the specification, NOT a reference capture: the reference has no such pass.

The depth maps are made here from a seed (make_input), so the file stays small: for the small cases it holds the output, and
meta holds every case's parameters and the SHA-256 of its output, so the tests can tell a drifting oracle or generator from a
drifting kernel.

    python tools/make_dilate_goldens.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dilate_oracle as oracle   # noqa: E402

TILE_W, TILE_H = 64, 16          # the tile of a workgroup (cs_depthdilate.hip DD_TW, DD_TH)
INF = float("inf")
KINDS = ("levels", "silhouette", "negative", "tiny", "specials")
THRESHOLDS = (0.0, 0.04, INF)
# smaller than the window in one or both axes; exactly one tile; the guarded 4-byte path with partial tiles; the 16-byte path over
# several tiles with partial edges; five tiles across
SIZES = ((1, 1), (1, 9), (9, 1), (3, 5), (16, 64), (17, 67), (33, 132), (40, 260))
STORE_OUT_BELOW = 600            # pixels: the cases whose whole output the file holds


def _case(h, w, n=1, c=1, radius=2, shape="disc", near="bright", threshold=0.04, kind="levels", off=None):
    """off: the tensor ("depth" or "out") whose first element lies one float behind the 16-byte grid."""
    thr = "inf" if threshold == INF else f"{threshold:g}"
    cid = f"{h}x{w}_n{n}_c{c}_r{radius}_{shape}_{near}_t{thr}_{kind}" + (f"_off{off}" if off else "")
    return dict(id=cid, h=h, w=w, n=n, c=c, radius=radius, shape=shape, near=near, threshold=threshold, kind=kind, off=off,
                seed=5000 + 7 * h + 13 * w + 31 * n + c + 101 * radius + 211 * KINDS.index(kind))


def cases():
    out = []
    # every size with one frame and with three, both shapes; the other parameters take turns
    k = 0
    for h, w in SIZES:
        for n in (1, 3):
            for shape in oracle.SHAPES:
                out.append(_case(h, w, n=n, c=(1, 3, 4)[k % 3], radius=(1, 2, 3, 5, 8)[k % 5], shape=shape, near=oracle.NEARS[(k // 2) % 2],
                                 threshold=THRESHOLDS[k % 3], kind=KINDS[k % 5]))
                k += 1
    # every radius with both shapes and both directions on the two sizes that take the two access paths over several tiles
    for h, w in ((17, 67), (33, 132)):
        for radius in oracle.RADII:
            for shape in oracle.SHAPES:
                for near in oracle.NEARS:
                    out.append(_case(h, w, n=1 if k % 4 else 3, c=(1, 3, 4)[k % 3], radius=radius, shape=shape, near=near,
                                     threshold=THRESHOLDS[(k // 3) % 3], kind=("levels", "silhouette", "specials")[k % 3]))
                    k += 1
    # every kind of input with every threshold and both directions
    for kind in KINDS:
        for threshold in THRESHOLDS:
            for near in oracle.NEARS:
                out.append(_case(17, 67, c=1, radius=2 if k % 2 else 3, shape=oracle.SHAPES[k % 2], near=near, threshold=threshold, kind=kind))
                k += 1
    # each tensor one element off the 16-byte grid at a size that otherwise takes the 16-byte path: the guarded path, same results
    for c in (1, 3):
        out += [_case(16, 64, c=c, kind="specials", off=off) for off in (None, "depth", "out")]
    seen = set()
    return [c for c in out if not (c["id"] in seen or seen.add(c["id"]))]


def _levels(rng, n, h, w):
    """8-bit-like levels, few of them, in patches: many ties."""
    yy, xx = np.mgrid[0:h, 0:w]
    frames = np.stack([0.5 + 0.35 * np.sin(0.35 * xx + 0.9 * t) * np.cos(0.5 * yy - 0.4 * t) for t in range(n)])
    frames = frames + rng.uniform(-0.03, 0.03, frames.shape)
    return (np.round(frames * 32) * 8 / 255).astype(np.float32)


def _silhouette(rng, n, h, w):
    """A near disc with an anti-aliased rim of 1 to 3 pixels on a smooth gradient."""
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for t in range(n):
        background = 0.15 + 0.3 * xx / max(w - 1, 1) + 0.1 * yy / max(h - 1, 1)
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        rad, ramp = 2.0 + 0.3 * min(h, w) + t, 1 + (t + h) % 3
        alpha = np.clip((rad - np.hypot(yy - cy, (xx - cx) * 0.5)) / ramp + 0.5, 0.0, 1.0)
        frames.append(background * (1 - alpha) + 0.85 * alpha)
    return np.stack(frames).astype(np.float32)


def _tiny(rng, n, h, w):
    """+0 and -0 in every neighbouring arrangement, subnormals and the smallest normals of both signs."""
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38], np.float32)
    frames = pool[rng.randint(0, len(pool), (n, h, w))]
    zeros = pool[rng.randint(0, 2, (n, h, w))]
    half = w // 2
    frames[:, :, :half] = zeros[:, :, :half]                  # the left half holds nothing but the two zeros
    return frames


def _specials(rng, n, h, w):
    """Levels with isolated NaNs, both infinities and -0; a band of NaN wider than any window; with three frames an all-NaN one."""
    frames = _levels(rng, n, h, w)
    draw = rng.uniform(0, 1, frames.shape)
    frames[draw < 0.04] = np.nan
    frames[(draw >= 0.04) & (draw < 0.05)] = np.inf
    frames[(draw >= 0.05) & (draw < 0.06)] = -np.inf
    frames[(draw >= 0.06) & (draw < 0.08)] = -0.0
    if w >= 41:
        frames[:, :, 20:41] = np.nan
    if n >= 3:
        frames[1] = np.nan
    return frames


def make_gray(case):
    """The frames a case is about, float32 [n,h,w], before they are spread over the channels."""
    rng = np.random.RandomState(case["seed"])
    n, h, w = case["n"], case["h"], case["w"]
    kind = case["kind"]
    if kind == "levels":
        return _levels(rng, n, h, w)
    if kind == "silhouette":
        return _silhouette(rng, n, h, w)
    if kind == "negative":
        return ((_levels(rng, n, h, w) - np.float32(0.5)) * np.float32(4.0)).astype(np.float32)
    if kind == "tiny":
        return _tiny(rng, n, h, w)
    return _specials(rng, n, h, w)


def make_input(case):
    """depth float32 [n,h,w,c] of a case; every frame differs.  C == 3 scales the frames per channel (zeros keep their sign, NaN and
    the infinities stay), any other C > 1 has noise behind channel 0."""
    frames = make_gray(case)
    c = case["c"]
    rng = np.random.RandomState(case["seed"] + 1)
    if c == 1:
        depth = frames[..., None]
    elif c == 3:
        depth = np.stack([frames, frames * np.float32(0.97), frames * np.float32(1.05)], axis=-1)
    else:
        depth = np.stack([frames] + [rng.uniform(0, 1, frames.shape).astype(np.float32) for _ in range(c - 1)], axis=-1)
    return np.ascontiguousarray(depth, dtype=np.float32)


def evaluate(case, depth=None):
    """-> y float32 [n,h,w]."""
    depth = make_input(case) if depth is None else depth
    return oracle.dilate(depth, case["radius"], case["shape"], case["near"], case["threshold"])


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def canonical(a):
    """float32 -> uint32 bits with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    v = a.view(np.uint32).copy()
    v[np.isnan(a)] = 0x7fc00000
    return v


def check_conditions(case, depth, out):
    """What a case is there for must actually occur in its input."""
    g = oracle.gray(depth)
    if case["kind"] == "levels" and g.size > 512:
        assert len(np.unique(g)) < g.size // 2, "no ties"
    if case["kind"] == "negative" and g.size > 16:
        assert (g < 0).any() and (g > 0).any()
    if case["kind"] == "tiny" and g.size > 64:
        sub = (g != 0) & (np.abs(g) < np.float32(1.1754944e-38))
        assert sub.any() and (np.signbit(g) & (g == 0)).any() and (~np.signbit(g) & (g == 0)).any()
    if case["kind"] == "specials" and g.size > 512:
        assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any() and (np.signbit(g) & (g == 0)).any()
        _, has = oracle.window_extreme(g, case["radius"], case["shape"], case["near"])
        assert (~has).any() and (np.isnan(g) & has).any(), "no all-NaN window, or no NaN centre with candidates around it"
        assert (np.isnan(out) == np.isnan(g)).all()          # a NaN centre stays, nothing else becomes NaN


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/dilate_oracle.py (written by tools/make_dilate_goldens.py); "
                    "not a reference capture", "tool": "tools/make_dilate_goldens.py", "cases": []}
    for case in cases():
        depth = make_input(case)
        out = evaluate(case, depth)
        check_conditions(case, depth, out)
        if case["h"] * case["w"] * case["n"] < STORE_OUT_BELOW:
            arrays[case["id"] + "/out"] = canonical(out)
        meta["cases"].append(dict(case, out_sha256=digest(canonical(out))))
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "depth_dilate.npz")
    np.savez_compressed(path, **build())
    print(path, os.path.getsize(path), "bytes")
