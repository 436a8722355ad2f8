"""Times the foreground depth edge dilation (engine.depth_dilate: one launch per batch) against the stock-torch composition of the
same arithmetic on the same device batch: 64 frames at 1080p and at 4K, C = 1 and C = 3, R = 2 and R = 8, both shapes.
  stock, square   F.max_pool2d(kernel 2R + 1, stride 1, padding R) (it pads with -inf: the clipped window), the gate with torch.where
  stock, disc     the maximum over the disc's 2R + 1 chords: per distinct half-width a one F.max_pool2d(kernel (1, 2a + 1)), shifted by
                  the chord's dy with -inf rows, then the same gate
The results are checked identical (every bit) before anything is timed; the input is finite and has no zeros, where max_pool2d's
order is the specification's.  Prints per configuration the times (best of --reps between HIP events, after a warm-up call), the
device kernels each side launches (counted with torch.profiler, memory copies and memsets left out), the achieved TB/s over the
bytes the pass must move (4 C read + 4 written per pixel), and one JSON line.  A row where the HIP pass is slower says **slower**.

    python tools/dilate_bench.py [--frames 64] [--reps 5]
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
import dilate_oracle as oracle   # noqa: E402

INF = float("inf")


def gray(depth):
    return ((0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2]) if depth.shape[3] == 3 else depth[..., 0]


def stock(depth, radius, shape, threshold):
    """near = bright in stock torch ops over the whole batch -> y [N,H,W]."""
    g = gray(depth)
    x = g[:, None]
    if shape == "square":
        m = F.max_pool2d(x, 2 * radius + 1, stride=1, padding=radius)
    else:
        h = g.shape[1]
        rows, m = {}, None
        for dy, a in oracle.chords(radius).items():
            if a not in rows:
                rows[a] = x if a == 0 else F.max_pool2d(x, (1, 2 * a + 1), stride=1, padding=(0, a))
            r = rows[a]
            if dy:                                             # row y of the result reads row y + dy; rows outside the frame are -inf
                r = F.pad(r, (0, 0, max(-dy, 0), max(dy, 0)), value=-INF)[:, :, max(dy, 0):max(dy, 0) + h]
            m = r if m is None else torch.maximum(m, r)
    m = m[:, 0]
    return torch.where(m - g >= threshold, m, g)


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


def scene(n, h, w, c):
    """Smooth depth in 0.05..0.95 with near patches that have soft rims, and a little noise: slopes and silhouettes, no zeros."""
    base = F.interpolate(torch.rand((n, 1, h // 120 + 2, w // 120 + 2), device="cuda"), size=(h, w), mode="bilinear")
    patches = F.interpolate((torch.rand((n, 1, h // 200 + 2, w // 200 + 2), device="cuda") > 0.7).float(), size=(h, w), mode="bilinear")
    g = (0.05 + 0.5 * base + 0.35 * ((patches - 0.4) * 40).clamp(0, 1) + 0.01 * torch.rand((n, 1, h, w), device="cuda"))[:, 0]
    if c == 1:
        return g[..., None].contiguous()
    return torch.stack([g, g * 0.97, g * 1.02], dim=-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.04)
    args = ap.parse_args()
    rows = []
    n, thr = args.frames, args.threshold
    for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        for c in (1, 3):
            depth = scene(n, h, w, c)
            assert bool(torch.isfinite(depth).all()) and bool((depth > 0).all())
            for radius in (2, 8):
                for shape in ("square", "disc"):
                    hip = lambda: engine.depth_dilate(depth, radius, shape, "bright", thr)   # noqa: E731
                    ref = lambda: stock(depth, radius, shape, thr)                            # noqa: E731
                    y_hip, y_stock = hip(), ref()
                    same = torch.equal(y_hip.view(torch.int32), y_stock.view(torch.int32))
                    moved = float((y_hip != gray(depth)).float().mean())
                    del y_hip, y_stock
                    if not same:
                        raise SystemExit(f"{name} C={c} R={radius} {shape}: the HIP pass and the stock composition differ; nothing timed")
                    ms, stock_ms = timed(hip, args.reps), timed(ref, args.reps)
                    nbytes = n * h * w * (4 * c + 4)
                    row = dict(size=name, frames=n, c=c, radius=radius, shape=shape, threshold=thr, identical=same, pixels_moved=round(moved, 4),
                               hip_ms=round(ms, 3), stock_ms=round(stock_ms, 3), hip_tb_s=round(nbytes / ms / 1e9, 3),
                               bytes_per_pixel=4 * c + 4, hip_launches=count_kernels(hip), stock_launches=count_kernels(ref),
                               speedup_vs_stock=round(stock_ms / ms, 2))
                    rows.append(row)
                    verdict = f"x{row['speedup_vs_stock']}" if ms <= stock_ms else f"**slower** (x{row['speedup_vs_stock']})"
                    print(f"{n} x {name} C={c} R={radius} {shape:6s}: HIP {ms:.3f} ms ({row['hip_tb_s']} TB/s over {4 * c + 4} B/px, "
                          f"{row['hip_launches']} kernel)   stock torch {stock_ms:.3f} ms ({row['stock_launches']} kernels)   {verdict}   "
                          f"identical, {100 * moved:.2f} % of the pixels moved", flush=True)
            del depth
            torch.cuda.empty_cache()
    print(json.dumps({"dilate_bench": rows}))


if __name__ == "__main__":
    main()
