#!/usr/bin/env python3
"""Time cs_inpaint_prepare (engine.inpaint_prepare) against a stock-torch composition of the same arithmetic on the same GPU, in
the same process: device tensors in, HIP events around each call, the two alternated call by call.

  python tools/inpaint_bench.py [--iters 30] [--warmup 5]
Sizes: 64 frames of 512 x 512 (the reference's working size) and 16 frames of 1080 x 1920.  Per size it prints ms per batch for
both paths, their ratio, and the HIP path's GB/s over the algorithmic bytes (per pixel: image 12 + depth 2 x 4 in, warped 12 +
filled 12 + mask 1 out), and how far the two masks agree (the torch path's grid_sample is the GPU's, not the CPU's, so an ulp of
grid x can move a pixel).  The last line is the JSON of all of it.

The torch composition is the fastest honest stock form, not the reference's column loops: batched per-frame min / max,
F.grid_sample twice, max_pool2d twice, cummax / cummin for the nearest unmasked columns, gathers for their colours.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import inpaint_oracle as io  # noqa: E402
from comfystereo_amd import engine  # noqa: E402

BYTES_PER_PIXEL = 12 + 2 * 4 + 12 + 12 + 1


def torch_prepare(img, depth, scale_factor, threshold=0.05):
    b, _, h, w = img.shape
    dpx = (scale_factor / 100.0) * w
    d = torch.where(depth.amax((1, 2), keepdim=True) > 1.0, depth / 255.0, depth)
    mn, mx = d.amin((1, 2), keepdim=True), d.amax((1, 2), keepdim=True)
    rng = mx - mn
    d = torch.where(rng > 1e-6, (d - mn) / rng.clamp(min=1e-6), torch.zeros_like(d)) - 0.5
    gx = torch.linspace(-1, 1, w, device=img.device) - (d * (-dpx)) / (w / 2)
    gy = torch.linspace(-1, 1, h, device=img.device)[None, :, None].expand(b, h, w)
    grid = torch.stack([gx, gy], -1)
    warped = F.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)
    valid = (gx >= -1) & (gx <= 1)
    d2 = d + 0.5
    wd = F.grid_sample(d2[:, None], grid, mode="nearest", padding_mode="border", align_corners=True)[:, 0]
    dis = F.max_pool2d(((wd - d2) > threshold).float()[:, None], 3, 1, 1)[:, 0] > 0.5
    mask = F.max_pool2d((~valid | dis).float()[:, None], 3, 1, 1)[:, 0] > 0.5
    cols = torch.arange(w, device=img.device).expand(b, h, w)
    left = torch.cummax(torch.where(mask, -1, cols), -1).values
    right = torch.cummin(torch.where(mask, w, cols).flip(-1), -1).values.flip(-1)
    ld, rd = (cols - left).float(), (right - cols).float()
    t = (ld / (ld + rd).clamp(min=1.0))[:, None]
    lc = torch.gather(warped, -1, left.clamp(min=0)[:, None].expand(-1, 3, -1, -1)) * (left >= 0)[:, None]
    rc = torch.gather(warped, -1, right.clamp(max=w - 1)[:, None].expand(-1, 3, -1, -1)) * (right < w)[:, None]
    filled = torch.where(mask[:, None], lc * (1 - t) + rc * t, warped)
    return warped, filled, mask


def inputs(b, h, w):
    imgs = np.stack([io.image_u8(h, w, 40 + k) for k in range(min(b, 4))]).astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    deps = np.stack([io.depth_u8("disc" if k % 2 == 0 else "edges", h, w, 50 + k) for k in range(min(b, 4))]).astype(np.float32)
    reps = (b + 3) // 4
    return (torch.from_numpy(np.ascontiguousarray(np.tile(imgs, (reps, 1, 1, 1))[:b])).cuda(),
            torch.from_numpy(np.ascontiguousarray(np.tile(deps, (reps, 1, 1))[:b])).cuda())


def time_pair(fa, fb, iters, warmup):
    """Median ms of fa and of fb, alternated."""
    ta, tb = [], []
    for i in range(warmup + iters):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                acc.append(e0.elapsed_time(e1))
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale-factor", type=float, default=5.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_bench needs a GPU")
    results = []
    for name, (b, h, w) in (("512x512 x64", (64, 512, 512)), ("1080p x16", (16, 1080, 1920))):
        img, dep = inputs(b, h, w)
        hip = engine.inpaint_prepare(img, dep, a.scale_factor)
        ref = torch_prepare(img, dep, a.scale_factor)
        mask_diff = int((hip[2] != ref[2]).sum())
        same = hip[2] == ref[2]
        err = float(((hip[1] - ref[1]).abs() * same[:, None]).max())
        del hip, ref
        ms_hip, ms_torch = time_pair(lambda: engine.inpaint_prepare(img, dep, a.scale_factor),
                                     lambda: torch_prepare(img, dep, a.scale_factor), a.iters, a.warmup)
        r = dict(size=name, frames=b, h=h, w=w, hip_ms=round(ms_hip, 4), torch_ms=round(ms_torch, 4),
                 ratio=round(ms_torch / ms_hip, 2), hip_gbps=round(b * h * w * BYTES_PER_PIXEL / ms_hip / 1e6, 1),
                 mask_pixels_different=mask_diff, filled_max_abs_diff_where_masks_agree=err)
        print(f"{name}: HIP {ms_hip:.3f} ms/batch, torch {ms_torch:.3f} ms/batch, ratio {r['ratio']}x, "
              f"HIP {r['hip_gbps']} GB/s algorithmic; masks differ on {mask_diff} pixels, filled max |diff| {err:.3g}")
        results.append(r)
    print(json.dumps(dict(bench="inpaint_prepare", scale_factor=a.scale_factor, iters=a.iters, results=results)))


if __name__ == "__main__":
    main()
