#!/usr/bin/env python3
"""Time cs_pil_resize (engine.pil_resize) and the whole of stereodiffusion_nodes.generate_stereo_fast on the GPU, next to
F.interpolate(mode="bicubic", antialias=True) on the same batch in the same process.

  python tools/fastmode_bench.py [--iters 20] [--warmup 3]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/fastmode_bench.py --trace     (kernel times: k_pil_*)
Resizes: 16 x 4K -> 512 x 512, 16 x 512 x 512 -> 4K, 64 x 1080p -> 512 x 512, uint8 RGB in and out.  The torch call is not
bit-identical to Pillow and works on float32 NCHW, four times the bytes; it is the stock alternative a caller has, not a
restatement.  Times are HIP events around each call, the two paths alternated call by call (medians); GB/s is over the
algorithmic bytes of the HIP path (uint8 input + uint8 output).  generate_stereo_fast runs with an identity `inpaint` on float
frames with three-channel depth, all of its launches and its one host synchronisation included.  The last line is the JSON of
all of it.  --trace runs each HIP path a few times without timing, for a kernel trace of its own.
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
from comfystereo_amd import engine  # noqa: E402
from comfystereo_amd import stereodiffusion_nodes as sdn  # noqa: E402
from inpaint_bench import time_pair  # noqa: E402

RESIZES = [("4K->512 x16", 16, (2160, 3840), (512, 512)), ("512->4K x16", 16, (512, 512), (2160, 3840)),
           ("1080p->512 x64", 64, (1080, 1920), (512, 512))]
FAST = [("fast 1080p x16", 16, 1080, 1920), ("fast 4K x4", 4, 2160, 3840)]


def frames_u8(n, h, w):
    g = torch.Generator(device="cuda").manual_seed(h * 7 + w)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fastmode_bench needs a GPU")
    results = []
    for name, n, (h, w), (oh, ow) in RESIZES:
        x = frames_u8(n, h, w)
        hip = lambda: engine.pil_resize(x, (ow, oh))
        if a.trace:
            for _ in range(3):
                hip()
            torch.cuda.synchronize()
            continue
        xf = x.permute(0, 3, 1, 2).float().contiguous()   # (the conversion is not timed)
        stock = lambda: F.interpolate(xf, size=(oh, ow), mode="bicubic", antialias=True)
        diff = (hip().permute(0, 3, 1, 2).float() - stock().clamp(0, 255)).abs()
        ms_hip, ms_torch = time_pair(hip, stock, a.iters, a.warmup)
        nbytes = n * 3 * (h * w + oh * ow)
        r = dict(name=name, frames=n, src=[h, w], dst=[oh, ow], hip_ms=round(ms_hip, 4), torch_ms=round(ms_torch, 4),
                 ratio=round(ms_torch / ms_hip, 2), hip_gbps=round(nbytes / ms_hip / 1e6, 1),
                 max_abs_code_diff_to_torch=float(diff.max()), mean_abs_code_diff_to_torch=round(float(diff.mean()), 4))
        print(f"{name}: HIP {ms_hip:.3f} ms/batch ({r['hip_gbps']} GB/s algorithmic), torch float32 {ms_torch:.3f} ms/batch, "
              f"ratio {r['ratio']}x; codes differ from torch's by at most {r['max_abs_code_diff_to_torch']:.2f}")
        results.append(r)
        del x, xf, diff
    for name, n, h, w in FAST:
        g = torch.Generator(device="cuda").manual_seed(n + h)
        img = torch.rand((n, h, w, 3), device="cuda", generator=g)
        dep = torch.rand((n, h, w, 1), device="cuda", generator=g).expand(n, h, w, 3).contiguous()
        dep[:, :, w // 3: w // 2] *= 0.3   # (a step: something to inpaint)
        fast = lambda: sdn.generate_stereo_fast(img, dep, 5.0, lambda filled, mask, k: filled)
        if a.trace:
            fast()
            torch.cuda.synchronize()
            continue
        ms, _ = time_pair(fast, lambda: None, a.iters, a.warmup)
        r = dict(name=name, frames=n, src=[h, w], hip_ms=round(ms, 3), ms_per_frame=round(ms / n, 3))
        print(f"{name}: generate_stereo_fast {ms:.3f} ms/batch, {ms / n:.3f} ms/frame (identity inpaint)")
        results.append(r)
        del img, dep
    if not a.trace:
        print(json.dumps(dict(bench="fast_mode", iters=a.iters, results=results)))


if __name__ == "__main__":
    main()
