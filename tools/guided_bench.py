"""Times the image-guided depth upsampling (engine.guided_depth: one launch per batch, the plan made once outside the timed region)
against two alternatives on the same device batch, 64 frames at 1080p and at 4K from depth maps of 518 on the short side:
  stock     the stock-torch composition of the same arithmetic, tap by tap with shifted index gathers (results compared);
  bilinear  F.interpolate(mode="bilinear"), the resize the pass replaces (another result: every silhouette a ramp).
Prints per configuration the times (best of --reps between HIP events), the device kernels each side launches (counted with
torch.profiler, memory copies and memsets left out), the bytes the HIP pass moves per output pixel (12 of the guide, 4 of the
result; the low-resolution samples a tile stages come on top and are counted separately) and the achieved GB/s, and one JSON line.

    python tools/guided_bench.py [--frames 64] [--reps 5] [--radius 2] [--channels 1]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine   # noqa: E402

TILE_W, TILE_H = 64, 16   # cs_guideddepth.hip GD_TW, GD_TH


def codes(image):
    return (torch.nan_to_num(image, nan=0.0).clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).to(torch.int32)


def stock(image, depth, plan):
    """The same arithmetic in stock torch ops: K * K trips of gathers, products and sums over the whole batch.  -> out."""
    r, k = plan.radius, plan.taps
    g = ((0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2]) if depth.shape[3] == 3 else depth[..., 0]
    cx, cy, wx, wy, wr = plan.cx.long(), plan.cy.long(), plan.wx, plan.wy, plan.wr
    pc = codes(image)
    qc = pc[:, plan.gy.long()][:, :, plan.gx.long()]
    num, den, ns, ds = (torch.zeros(image.shape[:3], device=image.device) for _ in range(4))
    for i in range(k):
        qy = (cy + (i - r)).clamp(0, plan.dh - 1)
        for j in range(k):
            qx = (cx + (j - r)).clamp(0, plan.dw - 1)
            ws = (wy[:, i, None] * wx[None, :, j])[None]
            d = (pc - qc[:, qy][:, :, qx]).abs().sum(dim=3)
            wg = ws * wr[d]
            v = g[:, qy][:, :, qx]
            num = num + wg * v
            den = den + wg
            ns = ns + ws * v
            ds = ds + ws
    return torch.where(den > 0, num / den, ns / ds)


def bilinear(depth, h, w):
    g = depth[..., 0] if depth.shape[3] != 3 else (0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2]
    return F.interpolate(g[:, None], size=(h, w), mode="bilinear", align_corners=False)[:, 0]


def count_kernels(fn):
    """The device kernels one call of fn launches, as torch.profiler sees them (memory copies and memsets are not kernels)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()
                and "memset" not in ev.name.lower()])


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def scene(n, h, w, dh, dw, c):
    """Frames of flat patches with noise on them, and smooth depth with noise: colour edges with and without a depth edge."""
    coarse = torch.rand((n, 3, h // 40 + 1, w // 40 + 1), device="cuda")
    image = (F.interpolate(coarse, size=(h, w), mode="nearest") + 0.04 * torch.rand((n, 3, h, w), device="cuda")).permute(0, 2, 3, 1).contiguous()
    depth = F.interpolate(torch.rand((n, 1, dh // 30 + 1, dw // 30 + 1), device="cuda"), size=(dh, dw), mode="bilinear")[:, 0]
    return image, depth[..., None].expand(n, dh, dw, c).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--channels", type=int, default=1)
    args = ap.parse_args()
    rows = []
    n, c = args.frames, args.channels
    for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        dh, dw = 518, round(518 * w / h)
        image, depth = scene(n, h, w, dh, dw, c)
        plan = engine.guided_depth_plan(h, w, dh, dw, args.radius)
        tiles = -(-w // TILE_W) * -(-h // TILE_H)
        staged = tiles * (TILE_W * dw / w + 2 * args.radius + 1) * (TILE_H * dh / h + 2 * args.radius + 1) * (4 * c + 12) / (h * w)
        row = dict(size=name, frames=n, c=c, radius=args.radius, depth=[dh, dw], bytes_per_pixel=16, staged_bytes_per_pixel=round(staged, 2))
        ms = timed(lambda: engine.guided_depth(image, depth, plan), args.reps)
        row["hip_ms"], row["hip_gb_s"] = round(ms, 3), round(n * h * w * 16 / ms / 1e6, 1)
        row["plan_ms"] = round(timed(lambda: engine.guided_depth_plan(h, w, dh, dw, args.radius), args.reps), 3)
        row["bilinear_ms"] = round(timed(lambda: bilinear(depth, h, w), args.reps), 3)
        y_hip, y_stock = engine.guided_depth(image, depth, plan), stock(image, depth, plan)
        row["max_abs_diff"] = float((y_hip - y_stock).abs().max())
        row["differing_pixels"] = int((y_hip != y_stock).sum())
        del y_hip, y_stock
        row["stock_ms"] = round(timed(lambda: stock(image, depth, plan), args.reps), 3)
        row["hip_launches"] = count_kernels(lambda: engine.guided_depth(image, depth, plan))
        row["stock_launches"] = count_kernels(lambda: stock(image, depth, plan))
        row["bilinear_launches"] = count_kernels(lambda: bilinear(depth, h, w))
        row["speedup_vs_stock"] = round(row["stock_ms"] / ms, 2)
        rows.append(row)
        print(f"{n} x {name} from {dh} x {dw}, C={c}, R={args.radius}: HIP {ms:.3f} ms ({row['hip_gb_s']} GB/s over 16 B/px + "
              f"{row['staged_bytes_per_pixel']} B/px staged, {row['hip_launches']} kernel), plan {row['plan_ms']:.3f} ms   stock torch "
              f"{row['stock_ms']:.3f} ms ({row['stock_launches']} kernels, x{row['speedup_vs_stock']})   bilinear resize "
              f"{row['bilinear_ms']:.3f} ms ({row['bilinear_launches']} kernels)   max |y - y_stock| {row['max_abs_diff']:.3g} "
              f"({row['differing_pixels']} pixels differ)", flush=True)
        del image, depth, plan
        torch.cuda.empty_cache()
    print(json.dumps({"guided_bench": rows}))


if __name__ == "__main__":
    main()
