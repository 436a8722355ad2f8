"""Times the depth range clipping (engine.depth_range: seven launches, one of them a memset) against the stock-torch composition
of the same result -- per frame torch.kthvalue for both ranks, then the clamp -- on the same device batch: 64 x 1080p and 64 x 4K,
C of 1 and 3.  Prints per configuration the times, the device kernels each side launches (counted with torch.profiler, memory
copies and memsets left out), the bytes per pixel and frame the kernels move (the count in comfystereo_amd/csrc/cs_depthrange.hip)
and the achieved GB/s, and one JSON line with all of it.  Bin contention is the risk of a histogram, so the HIP side is timed on
three contents: a noise map, 8-bit depth (256 distinct values) and a constant frame.

    python tools/range_bench.py [--frames 64] [--reps 5]

beta is 1 on both sides (the stock side has no state to carry), so the results are comparable value for value.  The state is made
once, outside the timed region: a timed call is the launches and its output allocations.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine   # noqa: E402

# bytes per pixel and frame: three digit passes (the first reads the input and writes the gray map for C != 1) + apply (read, write)
BYTES_PER_PIXEL = {1: 4 + 4 + 4 + 4 + 4, 3: 12 + 4 + 4 + 4 + 4 + 4}
CLIP = (0.005, 0.005)


def stock(depth, rank_lo, rank_hi):
    """The same result in stock torch ops, frame by frame.  -> y."""
    if depth.shape[3] == 3:
        g = (0.2989 * depth[..., 0] + 0.5870 * depth[..., 1]) + 0.1140 * depth[..., 2]
    else:
        g = depth[..., 0].contiguous()
    y = torch.empty_like(g)
    for t in range(g.shape[0]):
        flat = g[t].reshape(-1)
        lo = torch.kthvalue(flat, rank_lo + 1).values
        hi = torch.kthvalue(flat, rank_hi + 1).values
        y[t] = torch.clamp(g[t], lo, hi)
    return y


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


def content(kind, n, h, w, c):
    if kind == "noise":
        return torch.rand((n, h, w, c), device="cuda")
    if kind == "8bit":
        return (torch.randint(0, 256, (n, h, w, 1), device="cuda").float() / 255.0).expand(n, h, w, c).contiguous()
    return torch.full((n, h, w, c), 0.625, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rows = []
    for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        for c in (1, 3):
            n = args.frames
            ranks = engine.clip_ranks(*CLIP, h * w)
            state = engine.RangeState(h, w, "cuda")
            row = dict(size=name, frames=n, c=c, bytes_per_pixel=BYTES_PER_PIXEL[c])
            for kind in ("noise", "8bit", "const"):
                depth = content(kind, n, h, w, c)

                def hip():   # (a later sub-batch of a clip: the same kernels, the same bytes)
                    return engine.depth_range(depth, state, *CLIP, 1.0)
                ms = timed(hip, args.reps)
                row[f"hip_ms_{kind}"] = round(ms, 3)
                if kind == "noise":
                    y_hip, y_stock = hip()[0], stock(depth, *ranks)
                    row["max_abs_diff"] = float((y_hip - y_stock).abs().max())
                    del y_hip, y_stock
                    row["stock_ms"] = round(timed(lambda: stock(depth, *ranks), args.reps), 3)
                    row["hip_launches"], row["stock_launches"] = count_kernels(hip), count_kernels(lambda: stock(depth, *ranks))
                    row["hip_gb_s"] = round(n * h * w * BYTES_PER_PIXEL[c] / ms / 1e6, 1)
                    row["speedup"] = round(row["stock_ms"] / ms, 2)
                del depth
                torch.cuda.empty_cache()
            rows.append(row)
            print(f"{n} x {name} C={c}: HIP noise {row['hip_ms_noise']:.3f} ms ({row['hip_gb_s']} GB/s over {BYTES_PER_PIXEL[c]} B/px, "
                  f"{row['hip_launches']} kernels), 8-bit {row['hip_ms_8bit']:.3f} ms, constant {row['hip_ms_const']:.3f} ms   "
                  f"stock torch {row['stock_ms']:.3f} ms ({row['stock_launches']} kernels)   x{row['speedup']}   "
                  f"max |y - y_stock| {row['max_abs_diff']:.3g}", flush=True)
    print(json.dumps({"range_bench": rows}))


if __name__ == "__main__":
    main()
