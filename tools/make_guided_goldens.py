"""Writes tests/golden/guided_depth.npz: the cases of the guided depth upsampling's tests, evaluated by tools/guided_oracle.py.
A CPU evaluation of the specification, NOT a reference capture: the reference has no guided upsampling.

The frames and depth maps are made here from a seed (make_input), so the file stays small: per case it holds the plan's integer
blocks and, for the small cases, the output; meta holds every case's parameters and the SHA-256 of its output and of the plan's
weights, so the tests can tell a drifting oracle or generator from a drifting kernel.

    python tools/make_guided_goldens.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import guided_oracle as oracle   # noqa: E402

TILE_W, TILE_H = 64, 16          # the output tile of a workgroup (cs_guideddepth.hip GD_TW, GD_TH)
INF = float("inf")
GUIDES = ("blocks", "noise", "wild")
DEPTHS = ("smooth", "nonfinite")
SMALLEST_NORMAL = np.float32(1.1754944e-38)
STORE_OUT_BELOW = 600            # pixels: the cases whose whole output the file holds


def _case(h, w, dh, dw, n=1, c=1, radius=2, sigma_s=1.0, sigma_r=0.1, guide="blocks", depth="smooth", off=None, tag=""):
    """off: the tensor ("image", "depth" or "out") whose first element lies one float behind the 16-byte grid."""
    cid = f"{dh}x{dw}_to_{h}x{w}_n{n}_c{c}_r{radius}" + (f"_{guide}" if guide != "blocks" else "") + \
        (f"_{depth}" if depth != "smooth" else "") + (f"_off{off}" if off else "") + (f"_{tag}" if tag else "")
    return dict(id=cid, h=h, w=w, dh=dh, dw=dw, n=n, c=c, radius=radius, sigma_s=sigma_s, sigma_r=sigma_r, guide=guide, depth=depth,
                off=off, seed=3000 + 7 * h + 13 * w + 17 * dh + 19 * dw + 31 * n + c + 101 * radius + 211 * GUIDES.index(guide))


def cases():
    out = []
    # the tile's own edges: output sizes tw - 1, tw, tw + 1 by th - 1, th, th + 1 from about half the size; every radius with every C
    combos = [(r, c) for r in (1, 2, 3) for c in (1, 2, 3)]
    for k, (h, w) in enumerate((h, w) for h in (TILE_H - 1, TILE_H, TILE_H + 1) for w in (TILE_W - 1, TILE_W, TILE_W + 1)):
        r, c = combos[k]
        out.append(_case(h, w, (h + 1) // 2, (w + 1) // 2, n=3 if k % 3 == 0 else 1, c=c, radius=r))
    # scale ratios; 20 x 68 is more than one tile on either axis and a multiple of 4 wide (the 16-byte path)
    for r in (1, 2, 3):
        out.append(_case(20, 68, 20, 68, radius=r, tag="identity"))
        out.append(_case(20, 68, 10, 34, c=3, radius=r, tag="twice"))
        out.append(_case(17, 23, 5, 7, n=3, c=3, radius=r, tag="noninteger"))
    out += [_case(18, 70, 1, 9, tag="onerow"), _case(18, 70, 6, 1, tag="onecolumn"), _case(18, 70, 1, 1, radius=3, tag="onepixel"),
            _case(1, 1, 1, 1, tag="oneout"), _case(1, 1, 1, 1, radius=3, c=3, tag="oneout")]
    # a 4x enlargement, the ordinary use: 33 x 132 from 8 x 33 (three tiles by three)
    out += [_case(33, 132, 8, 33, n=3, c=3, tag="fourfold"), _case(33, 132, 8, 33, c=1, radius=3, tag="fourfold")]
    # each tensor one element off the 16-byte grid at a size that otherwise takes the 16-byte path: the guarded path, same results
    out += [_case(16, 64, 8, 32, c=3), _case(16, 64, 8, 32, c=3, off="image"), _case(16, 64, 8, 32, c=3, off="depth"),
            _case(16, 64, 8, 32, c=3, off="out")]
    # the range term's ends: den == 0 (the fallback), subnormal weights, no range term at all
    # (fourfold, so that whole blocks of pixels lie between the guide positions of the samples, where d == 0)
    out += [_case(17, 65, 5, 17, guide="noise", sigma_r=0.02, tag="fallback"), _case(17, 65, 5, 17, guide="noise", sigma_r=0.085, tag="subnormal"),
            _case(17, 65, 5, 17, guide="noise", sigma_r=INF, tag="norange"), _case(20, 68, 10, 34, c=3, sigma_r=INF, tag="norange"),
            _case(17, 65, 9, 33, sigma_s=0.4, tag="narrow"), _case(17, 65, 9, 33, radius=3, sigma_s=2.5, sigma_r=0.5, tag="wide")]
    # guide values below 0, above 1 and NaN; depth with NaN, the infinities and -0
    out += [_case(17, 65, 9, 33, c=3, guide="wild"), _case(20, 68, 10, 34, guide="wild", radius=1),
            _case(17, 65, 9, 33, depth="nonfinite"), _case(20, 68, 10, 34, depth="nonfinite", radius=3, sigma_r=INF, tag="norange")]
    return out


def make_input(case):
    """(image float32 [n,h,w,3], depth float32 [n,dh,dw,c]) of a case; every frame differs."""
    rng = np.random.RandomState(case["seed"])
    n, h, w, dh, dw, c = (case[k] for k in ("n", "h", "w", "dh", "dw", "c"))
    if case["guide"] == "blocks":        # flat patches of 5 x 9 pixels with a little noise: small and large colour differences side by side
        coarse = rng.uniform(0, 1, (n, -(-h // 5), -(-w // 9), 3))
        image = np.repeat(np.repeat(coarse, 5, axis=1), 9, axis=2)[:, :h, :w] + rng.uniform(-0.02, 0.02, (n, h, w, 3))
    elif case["guide"] == "noise":
        image = rng.uniform(0, 1, (n, h, w, 3))
    else:                                # wild: values on either side of 0..1, and NaNs
        image = rng.uniform(-0.5, 1.5, (n, h, w, 3))
        image[rng.uniform(0, 1, image.shape) < 0.03] = np.nan
    image = image.astype(np.float32)
    yy, xx = np.mgrid[0:dh, 0:dw]
    frames = np.stack([0.5 + 0.4 * np.sin(0.9 * xx + 0.3 * t) * np.cos(0.7 * yy - 0.2 * t) for t in range(n)]) + rng.uniform(-0.05, 0.05, (n, dh, dw))
    frames = frames.astype(np.float32)
    if case["depth"] == "nonfinite":
        flat = frames.reshape(n, -1)
        for t in range(n):
            where = rng.permutation(flat.shape[1])[:4]
            flat[t, where] = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)[:len(where)]
    if c == 1:
        depth = frames[..., None].copy()
    elif c == 3:
        depth = np.stack([frames, frames * np.float32(0.97), frames + np.float32(0.015625)], axis=-1)
    else:
        depth = np.stack([frames] + [rng.uniform(0, 1, frames.shape).astype(np.float32) for _ in range(c - 1)], axis=-1)
    return np.ascontiguousarray(image), np.ascontiguousarray(depth, dtype=np.float32)


def plan_of(case):
    return oracle.plan(case["h"], case["w"], case["dh"], case["dw"], case["radius"], case["sigma_s"], case["sigma_r"])


def evaluate(case, inputs=None, parts=None):
    """-> (plan, out)."""
    image, depth = make_input(case) if inputs is None else inputs
    p = plan_of(case)
    return p, oracle.apply(image, depth, p, parts)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def canonical(a):
    """float32 -> uint32 bits with every NaN mapped to one pattern (the payload an operation hands on is the implementation's)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    v = a.view(np.uint32).copy()
    v[np.isnan(a)] = 0x7fc00000
    return v


def check_conditions(case, inputs, out, parts):
    """What a case is there for must actually occur in its input."""
    image, depth = inputs
    if case["id"].endswith("fallback"):
        blocks = parts["den"][0] == 0
        assert blocks[:-1, :-1][blocks[1:, 1:] & blocks[:-1, 1:] & blocks[1:, :-1]].any(), "no 2 x 2 block of pixels takes the fallback"
        assert (parts["den"][0] > 0).any() and np.isfinite(out).all()
    if case["id"].endswith("subnormal"):
        assert ((parts["least_wg"] > 0) & (parts["least_wg"] < SMALLEST_NORMAL)).any(), "no subnormal weight"
    if case["guide"] == "wild":
        assert np.isnan(image).any() and (image < 0).any() and (image > 1).any()
    if case["depth"] == "nonfinite":
        assert np.isnan(depth).any() and np.isposinf(depth).any() and np.isneginf(depth).any() and (np.signbit(depth) & (depth == 0)).any()
        assert np.isnan(out).any() and np.isfinite(out).any()


# ---- the edge property's scene and check, shared by the CPU and the GPU test ------------------------------------------------------------
def edge_scene(radius):
    """A frame of 16 x 64, black left of column 32 and white from it on -- no low-resolution sample's centre (columns 4 q + 2) falls on
    32 -- and a 4x smaller depth map that steps from 0.2 to 0.8 between its columns 7 and 8, the corresponding place."""
    image = np.zeros((1, 16, 64, 3), np.float32)
    image[:, :, 32:] = 1.0
    depth = np.full((1, 4, 16, 1), 0.2, np.float32)
    depth[:, :, 8:] = 0.8
    assert 32 not in oracle.plan(16, 64, 4, 16, radius).gx.tolist()
    return image, depth


def check_edge_property(out, radius):
    """Every pixel on one of the two plateaus, to the rounding of a weighted mean of K * K equal values; the switch at column 32."""
    k2 = (2 * radius + 1) ** 2
    bound = (2 * k2 + 2) * 2.0 ** -24
    assert np.abs(out[:, :, :32] - np.float32(0.2)).max() <= bound * 0.2
    assert np.abs(out[:, :, 32:] - np.float32(0.8)).max() <= bound * 0.8
    return bound


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/guided_oracle.py (written by tools/make_guided_goldens.py); "
                    "not a reference capture", "tool": "tools/make_guided_goldens.py", "cases": []}
    for case in cases():
        inputs, parts = make_input(case), {}
        p, out = evaluate(case, inputs, parts)
        check_conditions(case, inputs, out, parts)
        cid = case["id"]
        for name in ("cx", "cy", "gx", "gy"):
            arrays[f"{cid}/{name}"] = getattr(p, name)
        if case["h"] * case["w"] * case["n"] < STORE_OUT_BELOW:
            arrays[f"{cid}/out"] = canonical(out)
        meta["cases"].append(dict(case, out_sha256=digest(canonical(out)), weights_sha256=digest(canonical(p.wx), canonical(p.wy), canonical(p.wr))))
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "guided_depth.npz")
    np.savez_compressed(path, **build())
    print(path, os.path.getsize(path), "bytes")
