"""Writes tests/golden/depth_range.npz: the cases of the depth range clipping's tests, evaluated by tools/range_oracle.py.
A CPU evaluation of the specification, NOT a reference capture: the reference has no range clipping.

The clips are made here from a seed (make_input), so the file stays small: per case it holds the four bound vectors; meta holds
every case's parameters and the SHA-256 of its y and of its final state, so the tests can tell a drifting oracle or generator
from a drifting kernel.

    python tools/make_range_goldens.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import range_oracle as oracle   # noqa: E402

CHUNK = 32768   # pixels per workgroup of the histogram kernel (cs_depthrange.hip RH_CHUNK)
# 1 x 1 (both ranks 0); 1 x 3 and 5 x 7 (h * w no multiple of 4: the guarded 4-byte path); 7 x 64 (whole 16-byte groups); 129 x 128
# (16 512 pixels: seventeen trips of a workgroup's loop); 129 x 256 (33 024 pixels: a second pixel range per frame)
SHAPES = [(1, 1), (1, 3), (5, 7), (7, 64), (129, 128), (129, 256)]
KINDS = ("noise", "const", "two", "low10", "mid11", "top11", "negzero", "inf", "nan", "8bit", "8bit_smooth", "huge", "outliers")


def _case(h, w, n, c, kind="noise", ranks=None, clip=None, beta=1.0, cut_at=(), normalize=False, offset=0, tag=""):
    """ranks: (rank_lo, rank_hi) given to the C entry point; clip: (clip_low, clip_high) given to the Python layer, which
    derives the ranks.  One of the two."""
    assert (ranks is None) != (clip is None)
    if clip is not None:
        ranks = oracle.ranks_of(clip[0], clip[1], h * w)
    cid = f"{h}x{w}_n{n}_c{c}_{kind}" + (f"_{tag}" if tag else "") + ("_norm" if normalize else "")
    return dict(id=cid, h=h, w=w, n=n, c=c, kind=kind, rank_lo=int(ranks[0]), rank_hi=int(ranks[1]),
                clip=None if clip is None else list(clip), beta=beta, cut_at=list(cut_at), normalize=bool(normalize), offset=offset,
                seed=2000 + 7 * h + 13 * w + 31 * n + c + 101 * KINDS.index(kind))


def cases():
    out = []
    for h, w in SHAPES:                                   # every shape, C of 1 and 3, a batch whose frames differ, default clip
        for c in (1, 3):
            out.append(_case(h, w, 3, c, clip=(0.005, 0.005)))
    out += [_case(5, 7, 3, 2, clip=(0.1, 0.1)), _case(7, 64, 3, 4, clip=(0.1, 0.2), normalize=True)]   # channel 0 of two and of four
    for norm in (False, True):
        out += [
            _case(7, 64, 2, 1, "const", clip=(0.005, 0.005), normalize=norm),                # lo == hi: normalised output zeros
            _case(5, 7, 2, 1, "two", ranks=(9, 10), normalize=norm, tag="straddle"),          # the ranks on either side of a tie's end
            _case(5, 7, 2, 1, "two", ranks=(3, 8), normalize=norm, tag="inlow"),              # both inside the lower value's ties
            _case(7, 64, 2, 1, "low10", clip=(0.1, 0.1), normalize=norm),                     # only the third digit pass decides
            _case(7, 64, 2, 1, "mid11", clip=(0.1, 0.1), normalize=norm),                     # only the second
            _case(7, 64, 2, 1, "top11", clip=(0.1, 0.1), normalize=norm),                     # only the first
            _case(5, 7, 2, 1, "negzero", ranks=(12, 17), normalize=norm),                     # lo = -0, hi = +0
            _case(7, 64, 2, 1, "inf", ranks=(0, 447), normalize=norm, tag="clip0"),           # bounds -inf, +inf
            _case(7, 64, 2, 1, "inf", clip=(0.05, 0.05), normalize=norm),                     # finite bounds, infinite pixels clamped
            _case(7, 64, 2, 1, "nan", ranks=(0, 447), normalize=norm, tag="clip0"),           # NaN bounds: they clamp nothing
            # finite bounds, NaN pixels pass (one channel: the sign of a NaN that went through gray_of is the implementation's)
            _case(7, 64, 2, 1, "nan", clip=(0.05, 0.05), normalize=norm),
            _case(33, 64, 2, 1, "outliers", clip=(0.005, 0.005), normalize=norm),             # the feature's purpose
        ]
    out += [_case(7, 64, 3, 1, ranks=(0, 447), tag="clip0"), _case(5, 7, 3, 3, ranks=(0, 34), tag="clip0"),
            _case(7, 64, 3, 1, ranks=(200, 200), tag="rankeq"), _case(5, 7, 3, 1, ranks=(34, 34), tag="rankeq")]
    out += [_case(64, 64, 2, 1, "8bit", clip=(0.005, 0.005)), _case(64, 64, 2, 3, "8bit", clip=(0.01, 0.02), normalize=True),
            _case(64, 64, 2, 1, "8bit_smooth", clip=(0.005, 0.005))]
    # the base pointer 4 bytes off the 16-byte grid at a size that otherwise takes the 16-byte path
    out += [_case(7, 64, 2, c, clip=(0.05, 0.05), offset=1, tag="offgrid") for c in (1, 3)]
    for c in (1, 3):                                                                         # smoothing over nine frames
        out += [_case(5, 67, 9, c, clip=(0.02, 0.02), beta=0.0, cut_at=(4,), tag="beta0"),
                _case(5, 67, 9, c, clip=(0.02, 0.02), beta=0.25, cut_at=(4,), tag="beta025"),
                _case(5, 67, 9, c, clip=(0.02, 0.02), beta=1.0, cut_at=(4,), tag="beta1"),
                _case(5, 67, 9, c, clip=(0.02, 0.02), beta=0.25, tag="nocut")]
    out += [_case(129, 256, 9, 1, clip=(0.005, 0.005), beta=0.25, cut_at=(4,), normalize=True, tag="beta025"),
            _case(5, 7, 9, 1, "huge", ranks=(0, 34), beta=0.5, tag="nonfinite")]             # raw - prev overflows: s is not finite
    return out


def make_input(case):
    """The clip of a case, float32 [N,H,W,C].  Frame t of every kind has its own distribution (an offset and a scale that
    depend on t), so a frame's bounds are its own."""
    rng = np.random.RandomState(case["seed"])
    n, h, w, c, kind = case["n"], case["h"], case["w"], case["c"], case["kind"]
    hw = h * w
    frames = np.empty((n, hw), np.float32)
    for t in range(n):
        if kind == "noise":
            g = rng.uniform(0, 1, hw).astype(np.float32) * np.float32(0.3 + 0.1 * (t % 5)) + np.float32(0.05 * (t % 3))
        elif kind == "const":
            g = np.full(hw, 0.625 + t, np.float32)
        elif kind == "two":                       # 10 x the lower value, the rest the higher one: ties on either side of rank 9 | 10
            g = np.where(rng.permutation(hw) < 10, np.float32(0.25 + t), np.float32(0.75 + t)).astype(np.float32)
        elif kind == "low10":                     # keys that differ in their low 10 bits only
            g = (np.uint32(0x3f000000 + (t << 10)) | rng.randint(0, 1 << 10, hw).astype(np.uint32)).view(np.float32)
        elif kind == "mid11":                     # ... in their middle 11 bits only
            g = (np.uint32(0x3f000155) | (rng.randint(0, 1 << 11, hw).astype(np.uint32) << np.uint32(10))).view(np.float32)
        elif kind == "top11":                     # ... in their top 11 bits only: sign, exponent 1..254, two mantissa bits
            top = (rng.randint(0, 2, hw) << 10) | (rng.randint(1, 255, hw) << 2) | rng.randint(0, 4, hw)
            g = ((top.astype(np.uint32) << np.uint32(21)) | np.uint32(0x000aaaaa)).view(np.float32)
        elif kind == "negzero":                   # 10 x -1, 5 x -0, 5 x +0, the rest 0.5
            g = np.select([np.arange(hw) < 10, np.arange(hw) < 15, np.arange(hw) < 20], [np.float32(-1.0 - t), np.float32(-0.0), np.float32(0.0)],
                          np.float32(0.5)).astype(np.float32)[rng.permutation(hw)]
        elif kind in ("inf", "nan"):
            g = rng.uniform(-1, 1, hw).astype(np.float32) * np.float32(1 + t)
            where = rng.permutation(hw)[:8]
            if kind == "inf":
                g[where] = np.array([np.inf, -np.inf] * 4, np.float32)
            else:                                 # NaNs of either sign: their keys lie above +inf and below -inf
                g[where] = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001] * 2, np.uint32).view(np.float32)
        elif kind == "8bit":
            g = rng.randint(0, 256, hw).astype(np.float32) / np.float32(255.0)
        elif kind == "8bit_smooth":               # a ramp in 8-bit steps: long runs of one value, every lane of a wave on few bins
            g = np.floor(np.linspace(0, 255.999, hw) * (0.5 + 0.5 * (t % 2))).astype(np.float32) / np.float32(255.0)
        elif kind == "huge":                      # bounds that jump between the ends of the range: raw - prev overflows
            g = rng.uniform(0.9, 1.0, hw).astype(np.float32) * np.float32(3.0e38 if t % 2 == 0 else -3.0e38)
            if t >= 6:
                g = rng.uniform(0.0, 1.0, hw).astype(np.float32)
        elif kind == "outliers":                  # a scene in 0.3 .. 0.6 with a speck at 0 and a specular hit at 1
            g = rng.uniform(0.3, 0.6, hw).astype(np.float32)
            g[rng.permutation(hw)[:4]] = np.array([0.0, 0.0, 1.0, 1.0], np.float32)
        frames[t] = g
    frames = frames.reshape(n, h, w)
    if c == 1:
        d = frames[..., None].copy()
    elif c == 3:
        d = np.stack([frames, frames * np.float32(0.97), frames + np.float32(0.015625)], axis=-1)
    else:
        d = np.stack([frames] + [rng.uniform(0, 1, frames.shape).astype(np.float32) for _ in range(c - 1)], axis=-1)
    return np.ascontiguousarray(d, dtype=np.float32)


def cut_of(case):
    """int32 [N], or None for a case without cuts (the call gets no cut array at all)."""
    if not case["cut_at"]:
        return None
    cut = np.zeros(case["n"], np.int32)
    cut[case["cut_at"]] = 1
    return cut


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


def evaluate(case, depth=None):
    depth = make_input(case) if depth is None else depth
    return oracle.depth_range(depth, None, case["rank_lo"], case["rank_hi"], case["beta"], cut_of(case), case["normalize"])


def digits_of(value):
    """The three digits (11, 11, 10 bits from the top) of a float32 value's key."""
    k = int(oracle.key(np.float32(value).reshape(1))[0])
    return k >> 21, (k >> 10) & 2047, k & 1023


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/range_oracle.py (written by tools/make_range_goldens.py); "
                    "not a reference capture", "tool": "tools/make_range_goldens.py", "cases": []}
    for case in cases():
        y, lo, hi, raw_lo, raw_hi, state = evaluate(case)
        cid = case["id"]
        for name, a in (("lo", lo), ("hi", hi), ("raw_lo", raw_lo), ("raw_hi", raw_hi)):
            arrays[f"{cid}/{name}"] = canonical(a)
        meta["cases"].append(dict(case, y_sha256=digest(canonical(y)), state_sha256=digest(canonical(state.lo), canonical(state.hi))))
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "depth_range.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
