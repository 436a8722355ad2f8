#!/usr/bin/env python3
"""Times cs_stereo_attention on the four self-attention levels of SD 1.5 at 512 x 512 under CFG ([uncond, cond] x [left, right],
8 heads), 'uni' and 'bi', with HIP events, next to (a) a stock-torch composition of the reference's arithmetic on the same GPU
(its rearranges, einsum, softmax, einsum -- attn_batch, stereo_utils.py:124-132, per CFG chunk) and (b)
F.scaled_dot_product_attention in float32 on the rearranged tensors.  Prints one JSON line per level and direction; TFLOP/s
counts 4 * queries * keys * d per head (the two products), against the 157 TFLOP/s f32-matrix peak.

  python tools/attention_bench.py [--iters 20] [--warmup 3] [--sweep]
--sweep: the kernel alone with 1, 2 and 4 waves per workgroup forced (development switch attn_waves) next to the launcher's
choice: the measurement behind stereo_attention_waves() in cs_attention.hip.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comfystereo_amd import _native, engine  # noqa: E402

LEVELS = [(1, 4096, 40, 8), (2, 1024, 80, 8), (3, 256, 160, 8), (4, 64, 160, 8)]   # level, n, d, heads
PEAK_TFLOPS = 157.0


def views(q, k, v, mode, heads):
    """[(c s b h), n, d] -> per CFG chunk the reference's '(s b h) n d -> (b h) (s n) d' tensors (uni: the left view's k, v)."""
    out = []
    for qc, kc, vc in zip(q.chunk(2), k.chunk(2), v.chunk(2)):
        def seq(t, s):
            bh = t.shape[0] // s
            return t.reshape(s, bh, t.shape[1], t.shape[2]).permute(1, 0, 2, 3).reshape(bh, s * t.shape[1], t.shape[2])
        half = kc.shape[0] // 2
        out.append((seq(qc, 2), seq(kc, 2), seq(vc, 2)) if mode == "bi" else (seq(qc, 2), seq(kc[:half], 1), seq(vc[:half], 1)))
    return out


def back(o, heads):
    """'(b h) (s n) d -> (s b) n (h d)'"""
    bh, sn, d = o.shape
    b, n = bh // heads, sn // 2
    return o.reshape(b, heads, 2, n, d).permute(2, 0, 3, 1, 4).reshape(2 * b, n, heads * d)


def stock(q, k, v, mode, heads, scale):
    outs = []
    for qq, kk, vv in views(q, k, v, mode, heads):
        sim = torch.einsum("h i d, h j d -> h i j", qq, kk) * scale
        outs.append(back(torch.einsum("h i j, h j d -> h i d", sim.softmax(-1), vv), heads))
    return torch.cat(outs)


def sdpa(q, k, v, mode, heads, scale):
    return torch.cat([back(F.scaled_dot_product_attention(qq, kk, vv, scale=scale), heads) for qq, kk, vv in views(q, k, v, mode, heads)])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.sweep:
        for level, n, d, heads in LEVELS:
            q, k, v = (torch.randn(4 * heads, n, d, device="cuda") for _ in range(3))
            for mode in ("uni", "bi"):
                row = dict(level=level, n=n, d=d, mode=mode)
                for waves in (0, 1, 2, 4):
                    _native.debug_set("attn_waves", waves)
                    try:
                        row["auto_ms" if waves == 0 else f"waves{waves}_ms"] = round(timed(
                            lambda: engine.stereo_attention(q, k, v, heads, d ** -0.5, mode, chunks=2), args.iters, args.warmup)[0], 4)
                    finally:
                        _native.debug_set("attn_waves", 0)
                print(json.dumps(row), flush=True)
        return
    for level, n, d, heads in LEVELS:
        bh = 2 * 2 * heads
        q, k, v = (torch.randn(bh, n, d, device="cuda") for _ in range(3))
        scale = d ** -0.5
        for mode in ("uni", "bi"):
            want = stock(q, k, v, mode, heads, scale)
            got = engine.stereo_attention(q, k, v, heads, scale, mode, chunks=2)
            err = float((got - want).abs().max())
            t_k = timed(lambda: engine.stereo_attention(q, k, v, heads, scale, mode, chunks=2), args.iters, args.warmup)
            t_s = timed(lambda: stock(q, k, v, mode, heads, scale), args.iters, args.warmup)
            t_f = timed(lambda: sdpa(q, k, v, mode, heads, scale), args.iters, args.warmup)
            flop = 4.0 * bh * n * (2 * n if mode == "bi" else n) * d
            print(json.dumps(dict(level=level, n=n, d=d, heads=heads, mode=mode, kernel_ms=round(t_k[0], 4), kernel_min_ms=round(t_k[1], 4),
                                  stock_ms=round(t_s[0], 4), sdpa_ms=round(t_f[0], 4), kernel_tflops=round(flop / t_k[0] / 1e9, 2),
                                  of_peak=round(flop / t_k[0] / 1e9 / PEAK_TFLOPS, 3), speedup_vs_stock=round(t_s[0] / t_k[0], 2),
                                  speedup_vs_sdpa=round(t_f[0] / t_k[0], 2), max_abs_diff_vs_stock=err)), flush=True)


if __name__ == "__main__":
    main()
