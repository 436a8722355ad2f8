"""Times the motion-compensated temporal depth filter (engine.motion_depth: 3 + N HIP launches) on 64 x 1080p and 64 x 4K, C of 1
and 3, at search ranges 8, 16 and 32, against
  * engine.temporal_depth on the same depth: the plain filter, i.e. what the motion search costs on top of it, and
  * a stock-torch composition of the same arithmetic -- luma, then per frame pair `unfold` of the padded predecessor into the
    (2S + 1)^2 displaced frames (a band of dy at a time), SAD per block, `argmin` of the packed key, `gather` of y_{t-1}, blend --
    on `--stock-frames` frames of the same clip (it is slow), its results compared with the HIP pass's before anything is timed.
Best of `--reps` between HIP events.  Prints one line per configuration and one JSON line with all of it.

    python tools/motion_bench.py [--frames 64] [--reps 5] [--stock-frames 3] [--sizes 1080p,4K] [--ranges 8,16,32]

The filter's state is made once, outside the timed region: a timed call is a later sub-batch of a clip (frame 0 has a
predecessor), its kernels and its output allocations.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from comfystereo_amd import engine   # noqa: E402
from temporal_bench import timed   # noqa: E402

B = 16
BIG = 1 << 62


def stock_luma(guide):
    c = torch.where(torch.isnan(guide), torch.zeros_like(guide), guide.clamp(0.0, 1.0))
    c = torch.trunc(c * 255.0 + 0.5).to(torch.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def stock_search(cur, ref, S, smoothness):
    """One frame pair of int64 luma [H,W] -> the minimal packed key per block [Hb,Wb] (tools/motion_oracle.py key())."""
    h, w = cur.shape
    hb, wb = -(-h // B), -(-w // B)
    K = 2 * S + 1
    pad = F.pad(ref.float()[None, None], (S, S, S, S))[0, 0]
    curp = F.pad(cur.float(), (0, wb * B - w, 0, hb * B - h))
    inside = F.pad(torch.ones_like(cur, dtype=torch.float32), (0, wb * B - w, 0, hb * B - h))
    by0 = torch.arange(hb, device=cur.device) * B
    bx0 = torch.arange(wb, device=cur.device) * B
    by1, bx1 = (by0 + B).clamp(max=h), (bx0 + B).clamp(max=w)
    dxs = torch.arange(-S, S + 1, device=cur.device)
    ok_x = (bx0[None, :] + dxs[:, None] >= 0) & (bx1[None, :] + dxs[:, None] <= w)                   # [K,Wb]
    best = torch.full((hb, wb), BIG, dtype=torch.int64, device=cur.device)
    for dy in range(-S, S + 1):
        rows = F.pad(pad[S + dy:S + dy + h], (0, wb * B - w, 0, hb * B - h))                           # the predecessor, displaced by dy
        shifted = rows.unfold(1, wb * B, 1)[:, :K].permute(1, 0, 2)                                    # [K,H',W']: every dx of the band
        sad = ((curp[None] - shifted).abs() * inside[None]).reshape(K, hb, B, wb, B).sum(dim=(2, 4)).to(torch.int64)
        mag = dxs.abs() + abs(dy)
        key = ((sad + smoothness * mag[:, None, None]) << 27) | (mag[:, None, None] << 20) | (abs(dy) << 14) | ((dy + 32) << 7) | (dxs[:, None, None] + 32)
        ok = ok_x[:, None, :] & ((by0 + dy >= 0) & (by1 + dy <= h))[None, :, None]
        best = torch.minimum(best, torch.where(ok, key, torch.full_like(key, BIG)).min(dim=0).values)
    return best


def stock(depth, guide, state_like, alpha, motion_threshold, cut_threshold, S, smoothness, match_threshold):
    """The same arithmetic in stock torch ops on frames 1.. of the clip (frame 0 is the predecessor) -> (y, vec, matched)."""
    g = (0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2] if depth.shape[3] == 3 else depth[..., 0].contiguous()
    lum = stock_luma(guide)
    n, h, w = g.shape
    hb, wb = -(-h // B), -(-w // B)
    npix = ((torch.arange(hb, device=g.device) * B + B).clamp(max=h) - torch.arange(hb, device=g.device) * B)[:, None] * \
           ((torch.arange(wb, device=g.device) * B + B).clamp(max=w) - torch.arange(wb, device=g.device) * B)[None, :]
    ys, xs = torch.meshgrid(torch.arange(h, device=g.device), torch.arange(w, device=g.device), indexing="ij")
    y = torch.empty_like(g)
    y[0] = g[0]
    vecs, flags = [], []
    for t in range(1, n):
        key = stock_search(lum[t], lum[t - 1], S, smoothness)
        dx, dy = (key & 127) - 32, ((key >> 7) & 127) - 32
        sad = (key >> 27) - smoothness * (dx.abs() + dy.abs())
        matched = sad <= match_threshold * npix
        cut = (g[t] - g[t - 1]).abs().mean() > cut_threshold
        src = (ys + dy[ys // B, xs // B]) * w + xs + dx[ys // B, xs // B]
        q = y[t - 1].reshape(-1).gather(0, src.reshape(-1)).reshape(h, w)
        delta = g[t] - q
        keep = cut | ~matched[ys // B, xs // B] | ~(delta.abs() < motion_threshold)
        y[t] = torch.where(keep, g[t], q + alpha * delta)
        vecs.append(torch.stack([dx, dy], dim=-1).to(torch.int8))
        flags.append(matched.to(torch.uint8))
    return y, torch.stack(vecs), torch.stack(flags)


def clip(n, h, w, c):
    """A pan of (3, -2) pixels per frame over a noise canvas, 4 x 4 patches; the depth moves with it, +-0.01 of noise per frame."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    M = 3 * n + 4
    canvas = torch.rand((1, 4, (h + 2 * M) // 4 + 1, (w + 2 * M) // 4 + 1), device="cuda", generator=gen)
    canvas = F.interpolate(canvas, scale_factor=4, mode="nearest")[0]
    guide = torch.stack([canvas[:3, M - 2 * t:M - 2 * t + h, M + 3 * t:M + 3 * t + w].permute(1, 2, 0) for t in range(n)]).contiguous()
    depth = torch.stack([canvas[3, M - 2 * t:M - 2 * t + h, M + 3 * t:M + 3 * t + w] for t in range(n)])
    depth = (depth * 0.9 + (torch.rand(depth.shape, device="cuda", generator=gen) - 0.5) * 0.02)[..., None].expand(-1, -1, -1, c).contiguous()
    return depth, guide


def pyramid_leg(args, sizes):
    """--search pyramid: engine.motion_depth_pyramid at R = 32 / 64 / 120 next to engine.motion_depth at S = 16 / 32 on the same
    batch, C = 1; `moved` is the fraction of blocks of frames 1.. on the clip's true vector (3, -2)."""
    rows = []
    prm = (0.5, 0.1, 0.6)
    for name in args.sizes.split(","):
        h, w = sizes[name]
        depth, guide = clip(args.frames, h, w, 1)
        for search, fn, ranges in (("full", engine.motion_depth, (16, 32)), ("pyramid", engine.motion_depth_pyramid, (32, 64, 120))):
            for R in ranges:
                state = engine.MotionState(h, w, depth.device)
                vec = fn(depth, guide, state, *prm, R, 32, 12)[4]
                on_true = float(((vec[1:, ..., 0] == 3) & (vec[1:, ..., 1] == -2)).float().mean())
                ms = timed(lambda: fn(depth, guide, state, *prm, R, 32, 12), args.reps)
                rows.append(dict(size=name, frames=args.frames, c=1, search=search, search_range=R, hip_ms=round(ms, 3),
                                 blocks_on_true_vector=round(on_true, 4)))
                print(json.dumps(rows[-1]))
        del depth, guide
        torch.cuda.empty_cache()
    print(json.dumps({"motion_bench_pyramid": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stock-frames", type=int, default=3)
    ap.add_argument("--sizes", default="1080p,4K")
    ap.add_argument("--ranges", default="8,16,32")
    ap.add_argument("--search", default="full", choices=("full", "pyramid"),
                    help="pyramid: time the coarse-to-fine search at R = 32 / 64 / 120 next to the full search at S = 16 / 32 instead")
    args = ap.parse_args()
    sizes = {"1080p": (1080, 1920), "4K": (2160, 3840)}
    if args.search == "pyramid":
        return pyramid_leg(args, sizes)
    rows = []
    prm = (0.5, 0.1, 0.6)
    for name in args.sizes.split(","):
        h, w = sizes[name]
        for c in (1, 3):
            n = args.frames
            depth, guide = clip(n, h, w, c)
            plain_state = engine.TemporalState(h, w, depth.device)
            engine.temporal_depth(depth, plain_state, *prm)
            ms_plain = timed(lambda: engine.temporal_depth(depth, plain_state, *prm), args.reps)
            for S in (int(v) for v in args.ranges.split(",")):
                state = engine.MotionState(h, w, depth.device)
                y, _, cut, _, vec, matched = engine.motion_depth(depth, guide, state, *prm, S, 32, 12)
                blended = float((y[1:] != ((0.2989 * depth[1:, ..., 0] + 0.5870 * depth[1:, ..., 1]) + 0.1140 * depth[1:, ..., 2] if c == 3
                                           else depth[1:, ..., 0])).float().mean())
                ms_hip = timed(lambda: engine.motion_depth(depth, guide, state, *prm, S, 32, 12), args.reps)
                row = dict(size=name, frames=n, c=c, search_range=S, hip_ms=round(ms_hip, 3), plain_ms=round(ms_plain, 3),
                           over_plain=round(ms_hip / ms_plain, 2), changed_fraction=round(blended, 4), cuts=int(cut[1:].sum()))
                if c == 1 and args.stock_frames > 1:
                    k = args.stock_frames
                    y_s, vec_s, matched_s = stock(depth[:k], guide[:k], None, *prm, S, 32, 12)
                    same = bool(torch.equal(vec_s, vec[1:k]) and torch.equal(matched_s, matched[1:k]))
                    ms_stock = timed(lambda: stock(depth[:k], guide[:k], None, *prm, S, 32, 12), max(1, args.reps // 2))
                    row.update(stock_ms_per_pair=round(ms_stock / (k - 1), 3), stock_same_vectors=same,
                               stock_max_abs_diff=float((y_s[1:] - y[1:k]).abs().max()), hip_ms_per_frame=round(ms_hip / n, 3))
                rows.append(row)
                print(json.dumps(row))
            del depth, guide
            torch.cuda.empty_cache()
    print(json.dumps({"motion_bench": rows}))


if __name__ == "__main__":
    main()
