"""Times the temporal depth filter (engine.temporal_depth: three HIP launches) against the stock-torch composition of the same
arithmetic -- a Python loop over the frames of abs, mean, where -- on the same device batch: 64 x 1080p and 64 x 4K, C of 1 and 3.
Prints per configuration the times, the device kernels each side launches (counted with torch.profiler, memory copies left
out), the bytes per pixel and frame the kernels move (the count in
comfystereo_amd/csrc/cs_temporal.hip) and the achieved GB/s, and one JSON line with all of it.

    python tools/temporal_bench.py [--frames 64] [--reps 5]

The stock composition decides its cuts on the device as well (torch.where on the flag), so neither side waits for the host.
The filter's state is made once, outside the timed region: a timed call is the three kernels and its output allocations.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine   # noqa: E402

# bytes per pixel and frame: statistic pass (frame t, frame t - 1 again, the gray map written for C != 1) + recurrence (read, write)
BYTES_PER_PIXEL = {1: 4 + 4 + 4 + 4, 3: 12 + 12 + 4 + 4 + 4}


def stock(depth, alpha, motion_threshold, cut_threshold):
    """The same arithmetic in stock torch ops, frame by frame; the first frame has no predecessor.  -> y."""
    if depth.shape[3] == 3:
        g = (0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2]
    else:
        g = depth[..., 0].contiguous()
    y = torch.empty_like(g)
    y[0] = g[0]
    for t in range(1, g.shape[0]):
        cut = (g[t] - g[t - 1]).abs().mean() > cut_threshold
        delta = g[t] - y[t - 1]
        keep = cut | ~(delta.abs() < motion_threshold)
        y[t] = torch.where(keep, g[t], y[t - 1] + alpha * delta)
    return y


def count_kernels(fn):
    """The device kernels one call of fn launches, as torch.profiler sees them (memory copies are not kernels)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        for c in (1, 3):
            n = args.frames
            depth = torch.rand((n, h, w, c), device="cuda") * 0.02 + torch.rand((1, h, w, 1), device="cuda")
            prm = (0.5, 0.1, 0.08)
            y_hip = engine.temporal_depth(depth, None, *prm)[0]
            y_stock = stock(depth, *prm)
            state = engine.TemporalState(h, w, depth.device)

            def hip():   # (a later sub-batch of a clip: frame 0 has a predecessor in the state; the same kernels, the same bytes)
                return engine.temporal_depth(depth, state, *prm)
            ms_hip = timed(hip, args.reps)
            ms_stock = timed(lambda: stock(depth, *prm), args.reps)
            hip_launches, launches = count_kernels(hip), count_kernels(lambda: stock(depth, *prm))
            moved = n * h * w * BYTES_PER_PIXEL[c]
            row = dict(size=name, frames=n, c=c, hip_ms=round(ms_hip, 3), stock_ms=round(ms_stock, 3), hip_launches=hip_launches,
                       stock_launches=launches, bytes_per_pixel=BYTES_PER_PIXEL[c], hip_gb_s=round(moved / ms_hip / 1e6, 1),
                       speedup=round(ms_stock / ms_hip, 2), max_abs_diff=float((y_hip - y_stock).abs().max()))
            rows.append(row)
            print(f"{n} x {name} C={c}: HIP {ms_hip:.3f} ms ({row['hip_gb_s']} GB/s over {BYTES_PER_PIXEL[c]} B/px, {hip_launches} launches)   "
                  f"stock torch {ms_stock:.3f} ms ({launches} launches)   x{row['speedup']}   max |y - y_stock| {row['max_abs_diff']:.3g}")
            del depth, y_hip, y_stock
            torch.cuda.empty_cache()
    print(json.dumps({"temporal_bench": rows}))


if __name__ == "__main__":
    main()
