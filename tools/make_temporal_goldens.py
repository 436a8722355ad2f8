"""Writes tests/golden/temporal_depth.npz: the cases of the temporal depth filter's tests, evaluated by tools/temporal_oracle.py.
A CPU evaluation of the specification, NOT a reference capture: the reference has no temporal filter.

The clips are made here from a seed (make_input), so the file stays small: per case it holds m (float64), cut, and for the small
cases the input and y themselves; meta holds every case's parameters and the SHA-256 of its y and of its final state, so the
tests can tell a drifting oracle or generator from a drifting kernel.

Every case keeps each finite m_t at least 1 % away from its cut_threshold (asserted here and in
tests/test_temporal_depth_surface.py), so that the cut flags do not hang on the order in which the kernels add m_t up.

    python tools/make_temporal_goldens.py
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import temporal_oracle as oracle   # noqa: E402

INF = float("inf")
SMALL = 1024  # cases of at most this many gray values keep their arrays in the file
# 1 x 1; 3 x 5; 7 x 64 (whole 16-byte groups); 5 x 67 (h * w no multiple of 4: the 4-byte path, a row tail in the last group);
# 33 x 131 (five trips of the statistic kernel's loop, h * w odd); 129 x 128 (16 512 pixels: a second partial sum per frame and
# a seventeenth trip's worth of pixels)
SHAPES = [(1, 1), (3, 5), (7, 64), (5, 67), (33, 131), (129, 128)]
LARGE = [(2049, 2048), (4097, 4096)]
CHUNK = 16384   # pixels per partial sum (cs_temporal.hip TS_CHUNK)
SPECIALS = {"nan": np.float32(np.nan), "pinf": np.float32(np.inf), "ninf": np.float32(-np.inf), "nzero": np.float32(-0.0)}


def _case(h, w, n, c, alpha=0.37, motion=0.1, cut=0.08, cut_at="mid", special=None, offset=0, tag=""):
    cut_at = (n // 2 if n > 2 else None) if cut_at == "mid" else cut_at
    cid = f"{h}x{w}_n{n}_c{c}" + (f"_{tag}" if tag else "")
    return dict(id=cid, h=h, w=w, n=n, c=c, alpha=alpha, motion_threshold=motion, cut_threshold=cut, cut_at=cut_at, special=special,
                offset=offset, seed=1000 + 7 * h + 13 * w + 31 * n + c)


def cases():
    out = []
    for h, w in SHAPES:
        for n in (1, 2, 9):
            for c in (1, 3):
                out.append(_case(h, w, n, c))
    out += [_case(7, 64, 9, 2), _case(5, 67, 2, 2)]                                   # channel 0 of two
    for c in (1, 3):
        out += [_case(33, 131, 9, c, alpha=0.0, tag="alpha0"), _case(33, 131, 9, c, alpha=1.0, tag="alpha1"),
                _case(33, 131, 9, c, motion=0.0, tag="motion0"), _case(33, 131, 9, c, motion=INF, tag="motioninf"),
                _case(33, 131, 9, c, cut=0.0, tag="cut0"), _case(33, 131, 9, c, cut=INF, tag="cutinf"),
                _case(33, 131, 9, c, alpha=1.0, motion=INF, cut=INF, tag="identity")]
        for name in SPECIALS:                                                        # one special value, in frame 3, pixel 70
            out.append(_case(7, 64, 9, c, special=name, cut_at=None, tag=name))
        # the base pointer 4 bytes off the 16-byte grid at a size that otherwise takes the 16-byte path
        out.append(_case(7, 64, 2, c, offset=1, tag="offgrid"))
    # the finalising kernel's two stride loops (cs_temporal.hip k_temporal_final; P partial sums of 16 384 pixels per frame):
    # 2049 x 2048 has P = 257, a second trip of the 256 threads that stage the partials; 4097 x 4096 has P = 1025, a second
    # stage of 1024 partials through the same LDS array.  4K frames have P = 507, 8K frames 2025.
    out += [_case(*LARGE[0], 2, 1, tag="p257"), _case(*LARGE[1], 2, 1, cut_at=1, tag="p1025")]
    return out


def make_input(case):
    """The clip of a case, float32 [N,H,W,C]: random codes / 255 (8-bit origin) plus +-0.01 of noise per frame; for w >= 32 a
    step of 0.5 whose edge moves one column per frame (the pixels it passes move, the others stand still); new codes from frame
    cut_at on (a hard cut); for C == 3 three channels that differ a little, for other C > 1 channel 0 and noise."""
    rng = np.random.RandomState(case["seed"])
    n, h, w, c = case["n"], case["h"], case["w"], case["c"]
    base = rng.randint(0, 256, (h, w)).astype(np.float32) / np.float32(255.0) * np.float32(0.45)
    frames = np.empty((n, h, w), np.float32)
    cols = np.arange(w)[None, :]
    for t in range(n):
        if case["cut_at"] is not None and t == case["cut_at"]:
            base = np.float32(0.5) + rng.randint(0, 256, (h, w)).astype(np.float32) / np.float32(255.0) * np.float32(0.45)
        noise = rng.uniform(-0.01, 0.01, (h, w)).astype(np.float32)
        step = np.where(cols < w // 4 + t, np.float32(0.5), np.float32(0.0)) if w >= 32 else np.float32(0.0)
        frames[t] = (base + noise) + step
    if c == 1:
        d = frames[..., None].copy()
    elif c == 3:
        d = np.stack([frames, frames * np.float32(0.97), frames + np.float32(0.015625)], axis=-1)
    else:
        d = np.stack([frames] + [rng.uniform(0, 1, frames.shape).astype(np.float32) for _ in range(c - 1)], axis=-1)
    if case["special"]:
        d[min(3, n - 1)].reshape(-1, c)[min(70, h * w - 1), 0] = SPECIALS[case["special"]]
    return np.ascontiguousarray(d, dtype=np.float32)


def margin_ok(m, cut_threshold):
    """Every finite m is at least 1 % of the threshold away from it; against a threshold of 0 it is 0 or a normal number."""
    thr = float(np.float32(cut_threshold))
    m = np.asarray(m, np.float64)
    fin = np.isfinite(m)
    if thr == 0.0:
        return bool(np.all((m[fin] == 0.0) | (m[fin] > 1e-30)))
    if not np.isfinite(thr):
        return True
    return bool(np.all(np.abs(m[fin] - thr) >= 0.01 * thr))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def evaluate(case, depth=None):
    depth = make_input(case) if depth is None else depth
    return oracle.temporal_depth(depth, None, case["alpha"], case["motion_threshold"], case["cut_threshold"])


def build():
    arrays = {}
    meta = {"note": "CPU evaluation of the specification by tools/temporal_oracle.py (written by tools/make_temporal_goldens.py); "
                    "not a reference capture", "tool": "tools/make_temporal_goldens.py", "cases": []}
    for case in cases():
        depth = make_input(case)
        y, m, cut, state, still = evaluate(case, depth)
        assert margin_ok(m, case["cut_threshold"]), (case["id"], m)
        cid = case["id"]
        arrays[cid + "/m"] = m
        arrays[cid + "/cut"] = cut
        if y.size <= SMALL:
            arrays[cid + "/depth"] = depth
            arrays[cid + "/y"] = y
        entry = dict(case, y_sha256=digest(y), state_sha256=digest(state.prev_raw, state.prev))
        for k in ("motion_threshold", "cut_threshold"):   # (json has no infinity)
            entry[k] = "inf" if entry[k] == INF else entry[k]
        meta["cases"].append(entry)
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "temporal_depth.npz")
    np.savez_compressed(out, **build())
    print(out, os.path.getsize(out), "bytes")
