#!/usr/bin/env python3
"""Throughput of the Gaussian depth blurs (cs_gaussblur.hip) on one MI355X: 16 frames of 3840 x 2160 float32.

For each operation (plain, edge_selective, left, right) at sigma 1, 7 and 70: ms per call from device events (median of
--repeats timed batches of --iters calls after warm-up; the input buffers are re-used, so the first frames of a call may
come from the 256 MiB last-level cache), the algorithmic bytes -- 16 B per pixel for the two passes, plus 4 for the blending
operations' second read of the depth -- over the 8 TB/s HBM peak, and the float64 operations -- 2 passes x (2 * radius + 1)
taps x one multiply and one add -- over the part's vector float64 rate (78.6 TFLOP/s counts a fused multiply-add as two;
the kernels may not fuse, so they can reach half of it at most).
The taps upload and the workspace allocation of engine.gaussian_blur are inside the timed call, as a caller pays them.
Kernel-only time: `rocprofv3 --kernel-trace --stats -- python tools/gauss_bench.py --iters 3 --repeats 1`.

  python tools/gauss_bench.py [--frames 16] [--iters 10] [--repeats 5] [--warmup 3] [--reference]
--reference: instead, times the reference's own blur_depth_map on one 1080p map on the host, for scale (no GPU needed; build
machine only: loads the reference through tools/refload.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gauss_oracle as go  # noqa: E402

HBM_PEAK = 8.0e12
F64_PEAK = 78.6e12
H, W = 2160, 3840
OPS = ["plain", "edge_selective", "left", "right"]
SIGMAS = [1, 7, 70]


def timed(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.reference:
        return reference_on_host()
    from comfystereo_amd import engine
    n = a.frames
    g = torch.Generator(device="cuda").manual_seed(0)
    depth = (torch.rand((n, H // 40 + 1, W // 40 + 1), device="cuda", generator=g) * 255).round()
    depth = depth.repeat_interleave(40, 1).repeat_interleave(40, 2)[:, :H, :W]
    depth = (depth + torch.rand((n, H, W), device="cuda", generator=g) * 4).contiguous()
    px = n * H * W
    for sigma in SIGMAS:
        taps = 2 * int(3 * sigma) + 1
        for op in OPS:
            ms, lo, hi = timed(lambda: engine.gaussian_blur(depth, sigma, op, 6.0), a.iters, a.warmup, a.repeats)
            bpx = 16 if op == "plain" else 20
            flops = px * 2 * taps * 2
            print(json.dumps(dict(op=op, sigma=sigma, taps=taps, frames=n, ms_per_call=round(ms, 3), ms_min=round(lo, 3),
                                  ms_max=round(hi, 3), frames_per_s=round(n / ms * 1e3, 1), bytes_per_px=bpx,
                                  tb_per_s=round(bpx * px / (ms * 1e-3) / 1e12, 3),
                                  fraction_of_hbm_peak=round(bpx * px / (ms * 1e-3) / HBM_PEAK, 3),
                                  f64_tflops=round(flops / (ms * 1e-3) / 1e12, 2),
                                  fraction_of_f64_peak=round(flops / (ms * 1e-3) / F64_PEAK, 3))), flush=True)


def reference_on_host():
    """The reference's own blur_depth_map on one 1080p map (no GPU; needs the reference checkout of tools/refload.py)."""
    import refload
    refload.quiet()
    sig = refload.load_sig()
    d = go.depth_map("codes", 1080, 1920, 1080)
    for sigma in (1, 7, 70):
        t0 = time.perf_counter()
        want = sig.blur_depth_map(d, sigma)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(go.blur_depth_map(d, sigma).view(np.uint32), want.view(np.uint32)))
        print(json.dumps(dict(op="reference blur_depth_map on the host", sigma=sigma, frame="1920x1080", host_ms=round(dt * 1e3, 1),
                              restatement_bit_equal=same)), flush=True)


if __name__ == "__main__":
    main()
