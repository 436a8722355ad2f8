#!/usr/bin/env python3
"""Throughput of the grid-sample warps (cs_gridwarp.hip) on one MI355X: 16 frames of 3840 x 2160, C = 3.

For each of the six operations: ms per call from device events after warm-up, frames/s, the algorithmic bytes per pixel (what
the operation must read and write once) and the bandwidth that implies against the 8 TB/s HBM peak.  The baseline is the same
warp + stretch and plain warp as ATen passes on the same GPU (torch ops written from the rules in DESIGN.md section 2, the
way the reference runs them).  Kernel-only time: run under `rocprofv3 --kernel-trace --stats -- python tools/grid_bench.py`.

  python tools/grid_bench.py [--frames 16] [--iters 20] [--warmup 3] [--no-baseline]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import stereoimage_generation as sig  # noqa: E402

PEAK = 8.0e12
H, W, C = 2160, 3840, 3
# algorithmic bytes per pixel at C = 3 (float32 image and output, float32 depth, uint8 masks)
BYTES = {
    "apply_stereo_divergence_gpu": 4 + 12 + 12,
    "apply_stereo_divergence_gpu_with_fill": 4 + 12 + 12 + 1,
    "compute_forward_mask_gpu": 4 + 1,
    "warp_and_fill_gpu": 4 + 12 + 12 + 1,
    "interpolate_fill_gpu": 12 + 1 + 12,
    "detect_disocclusions_gpu": 4 + 8 + 4 + 4 + 1,   # depth, grid, grid_x_warped, the sampled depth, the mask
}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_offsets(depth, div, sep, e, conv):
    d = depth
    if (d.amax(dim=(1, 2)) > 1.0).any():
        d = d / 255.0
    mn, mx = d.amin(dim=(1, 2), keepdim=True), d.amax(dim=(1, 2), keepdim=True)
    rng = mx - mn
    nd = torch.where(rng > 1e-6, (d - mn) / rng.clamp(min=1e-6), torch.zeros_like(d))
    s = nd - conv
    return torch.sign(s) * torch.pow(torch.abs(s), e) * div + sep


def torch_warp(img, depth, div, sep, e, conv, stretch):
    """The ATen chain on the GPU: offsets, (forward gap mask and edge stretch), one grid_sample."""
    b, _, h, w = img.shape
    po = torch_offsets(depth, div, sep, e, conv)
    gx = torch.linspace(-1, 1, w, device=img.device) - po / (w / 2)
    gy = torch.linspace(-1, 1, h, device=img.device)[None, :, None].expand(b, h, w)
    gap = None
    if stretch:
        cols = torch.arange(w, device=img.device)
        dest = (cols.float() + po).long()
        ok = (dest >= 0) & (dest < w)
        hit = torch.zeros(b, h, w, device=img.device)
        hit.scatter_add_(2, dest.clamp(0, w - 1), ok.float())
        gap = hit < 0.5
        step = torch.abs(po[:, :, 1:] - po[:, :, :-1]) > 1.5
        edge = torch.zeros_like(gap)
        edge[:, :, :-1] = step
        edge[:, :, 1:] |= step
        dil = gap.clone()
        dil[:, :, 1:] |= gap[:, :, :-1] & edge[:, :, 1:]
        dil[:, :, :-1] |= gap[:, :, 1:] & edge[:, :, :-1]
        gap = dil
        valid = ~gap
        left = torch.cummax(torch.where(valid, cols, -1), dim=2)[0]
        right = torch.flip(torch.cummax(torch.where(torch.flip(valid, [2]), torch.flip(cols, [0]), -1), dim=2)[0], [2])
        ld, rd = (cols - left).float(), (right - cols).float()
        total = torch.clamp(ld + rd, min=1.0)
        half = total * 0.5
        lt, rt = torch.clamp(ld / half, 0.0, 1.0), torch.clamp(rd / half, 0.0, 1.0)
        ls = gx.gather(2, left.clamp(0, w - 1)) * (1.0 - lt) + gx.gather(2, (left - 3).clamp(0, w - 1)) * lt
        rs = gx.gather(2, right.clamp(0, w - 1)) * (1.0 - rt) + gx.gather(2, (right + 3).clamp(0, w - 1)) * rt
        t = torch.where(left < 0, torch.ones_like(ld), ld / total)
        t = torch.where(right < 0, torch.zeros_like(t), t)
        bl = torch.clamp((t - 0.35) / 0.3, 0.0, 1.0)
        bl = bl * bl * (3.0 - 2.0 * bl)
        gx = torch.where(gap, ls * (1.0 - bl) + rs * bl, gx)
    out = F.grid_sample(img, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)
    return out, gap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    n = a.frames
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.rand((n, C, H, W), device="cuda", generator=g)
    depth = (torch.rand((n, H // 60 + 1, W // 60 + 1), device="cuda", generator=g) * 255).round()
    depth = depth.repeat_interleave(60, 1).repeat_interleave(60, 2)[:, :H, :W].contiguous()
    args = (0.02 * W, 0.0, 2.0, 0.5)
    mask = torch.rand((n, H, W), device="cuda", generator=g) < 0.2
    d0 = depth[0] / 255.0
    _, gap0 = sig.warp_and_fill_gpu(img[:1], depth[:1], *args)
    po = torch_offsets(depth[:1], *args)
    gxw = (torch.linspace(-1, 1, W, device="cuda") - po / (W / 2))[0].contiguous()
    grid = torch.stack([gxw, torch.linspace(-1, 1, H, device="cuda")[:, None].expand(H, W)], -1)[None].contiguous()
    ops = {
        "apply_stereo_divergence_gpu": (lambda: sig.apply_stereo_divergence_gpu(img, depth, *args), n),
        "apply_stereo_divergence_gpu_with_fill": (lambda: sig.apply_stereo_divergence_gpu_with_fill(img[0], depth[0], *args,
                                                                                                   fill_mode="reflection"), 1),
        "compute_forward_mask_gpu": (lambda: sig.compute_forward_mask_gpu(depth, *args, "cuda"), n),
        "warp_and_fill_gpu": (lambda: sig.warp_and_fill_gpu(img, depth, *args), n),
        "interpolate_fill_gpu": (lambda: sig.interpolate_fill_gpu(img, mask, "cuda"), n),
        "detect_disocclusions_gpu": (lambda: sig.detect_disocclusions_gpu(d0, grid, gxw, "cuda"), 1),
    }
    res = {}
    for name, (fn, frames) in ops.items():
        ms = timed(fn, a.iters, a.warmup)
        bpx = BYTES[name]
        res[name] = dict(ms_per_call=round(ms, 4), frames_per_call=frames, frames_per_s=round(frames / ms * 1e3, 1),
                         bytes_per_px=bpx, tb_per_s=round(bpx * frames * H * W / (ms * 1e-3) / 1e12, 3),
                         fraction_of_peak=round(bpx * frames * H * W / (ms * 1e-3) / PEAK, 3))
        print(json.dumps(dict(op=name, **res[name])), flush=True)
    if not a.no_baseline:
        for name, stretch in (("warp_and_fill_gpu", True), ("apply_stereo_divergence_gpu", False)):
            ms = timed(lambda: torch_warp(img, depth, *args, stretch), max(2, a.iters // 4), 1)
            print(json.dumps(dict(op=name, baseline="ATen on the same GPU", ms_per_call=round(ms, 3),
                                  speedup=round(ms / res[name]["ms_per_call"], 1))), flush=True)


if __name__ == "__main__":
    main()
