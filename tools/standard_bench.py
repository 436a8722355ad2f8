#!/usr/bin/env python3
"""Times the per-step kernels of StereoDiffusion's Standard mode next to the stock-torch composition of the same arithmetic on
the same GPU, with HIP events:

  FIRST and RESHIFT (engine.latent_shift_apply on a plan made once) at [2, 4, 64, 64] and [2, 4, 128, 128] latents, against a
  gather through the same table followed by the reference's boolean-mask indexing (stereodiffusion_nodes.py:654-660, :667);
  decode_to_codes plus the Pillow-exact resize back to 1080p and 4K, against torch's (x / 2 + 0.5).clamp(0, 1), the copy to the
  host, nan_to_num, * 255, uint8 there (:673-677) and the copy back for the same resize.

  python tools/standard_bench.py [--iters 200]
It prints a table and judges nothing: there is no threshold in it.  DESIGN.md section 2 holds the numbers of whoever ran it.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # microseconds per call


def torch_gather(left, src_col):
    idx = src_col.clamp(min=0).long()[:, None].expand(-1, left.shape[1], -1, -1)
    return torch.where((src_col >= 0)[:, None], torch.gather(left, 3, idx), torch.zeros((), dtype=left.dtype, device=left.device))


def torch_first(latents, src_col, noise):
    ts = torch_gather(latents[:1], src_col)
    latents = torch.cat([latents[:1], ts], 0)
    mask = (ts[:, 0] != 0)[:, None].repeat(1, latents.shape[1], 1, 1)
    latents[1:][~mask] = noise[~mask]
    latents[1:][mask] = ts[mask]
    return latents, mask


def torch_reshift(latents, src_col, mask):
    ts = torch_gather(latents[:1], src_col)
    latents[1:][mask] = ts[mask]
    return latents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "standard_bench.py needs a GPU"
    rows = []
    g = torch.Generator().manual_seed(0)
    for side in (64, 128):
        for dtype in (torch.float32, torch.float16):
            disp = torch.rand((1, side, side), generator=g).cuda()
            src = engine.latent_shift_plan(disp, 8.0)
            lat = torch.randn((2, 4, side, side), generator=g).to(dtype).cuda()
            noise = torch.randn((1, 4, side, side), generator=g).to(dtype).cuda()
            mask = torch.zeros((1, side, side), dtype=torch.uint8, device="cuda")
            name = f"[2,4,{side},{side}] {str(dtype).split('.')[-1]}"
            rows.append((f"plan (once per image) {name}", timed(lambda: engine.latent_shift_plan(disp, 8.0), args.iters), None))
            ours = timed(lambda: engine.latent_shift_apply(lat[:1], lat[1:], src, mask, "first", noise=noise), args.iters)
            ref = timed(lambda: torch_first(lat, src, noise), args.iters)
            rows.append((f"FIRST {name}", ours, ref))
            _, bmask = torch_first(lat.clone(), src, noise)
            ours = timed(lambda: engine.latent_shift_apply(lat[:1], lat[1:], src, mask, "reshift"), args.iters)
            ref = timed(lambda: torch_reshift(lat, src, bmask), args.iters)
            rows.append((f"RESHIFT {name}", ours, ref))
    image = (torch.randn((2, 3, 512, 512), generator=g)).cuda()
    for label, (w, h) in (("1080p", (1920, 1080)), ("4K", (3840, 2160))):
        stereo = torch.empty((1, h, 2 * w, 3), dtype=torch.float32, device="cuda")

        def ours_fn():
            codes = engine.decode_to_codes(image)
            engine.pil_resize(codes[:1], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
            engine.pil_resize(codes[1:], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])

        def ref_fn():
            x = (image / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
            codes = torch.from_numpy((np.nan_to_num(x, nan=0.0, posinf=1.0, neginf=0.0) * 255).astype(np.uint8)).cuda()
            engine.pil_resize(codes[:1], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
            engine.pil_resize(codes[1:], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])

        rows.append((f"decode_to_codes + resize back to {label}", timed(ours_fn, max(1, args.iters // 10)),
                     timed(ref_fn, max(1, args.iters // 10))))
    print(f"{'what':58s} {'HIP us':>10s} {'torch us':>10s} {'ratio':>7s}")
    for what, ours, ref in rows:
        print(f"{what:58s} {ours:10.1f} " + (f"{ref:10.1f} {ref / ours:7.2f}" if ref is not None else f"{'-':>10s} {'-':>7s}"))


if __name__ == "__main__":
    main()
