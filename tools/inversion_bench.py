#!/usr/bin/env python3
"""Null-text inversion outside the UNet on one MI355X: per inner step of null_optimization (reference inversion.py:198-204),
everything between the UNet's output and the updated embedding -- guided step + loss + gradient + Adam -- fused
(engine.NullTextLoss + engine.adam_step) against the stock-torch composition of the same lines under autograd with
torch.optim.Adam; and the ddim_loop step alone (engine.ddim_step against next_step's expression).

The UNet is stood in for by `eps_uncond = embedding.sum() * 0 + eps`, the cheapest graph that carries a gradient back to the
[1,77,768] embedding, the same on both sides.  Latents [1,4,64,64].  Time: HIP events over `--iters` steps after `--warmup`;
launches: torch.profiler's device kernels of one step.  One JSON line per dtype.

  python tools/inversion_bench.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine  # noqa: E402

COEFFS = (0.8, 0.6, 0.7, 0.714)
GUIDANCE = 7.5


def stock_step(c, e, x):
    c1, c2, c3, c4 = c
    return c4 * ((x - c1 * e) / c2) + c3 * e


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3   # microseconds


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(0)
        lat = [torch.randn(1, 4, 64, 64, generator=g).to(dtype).cuda() for _ in range(4)]
        eps, eps_cond, cur, prev = lat
        c = tuple(torch.tensor(v) for v in COEFFS)

        emb_f = torch.randn(1, 77, 768, generator=g).to(dtype).cuda().requires_grad_(True)
        m, v = torch.zeros_like(emb_f), torch.zeros_like(emb_f)
        state = {"k": 0}

        def fused():
            state["k"] += 1
            e = emb_f.sum() * 0 + eps
            loss = engine.NullTextLoss.apply(e, eps_cond, cur, prev, GUIDANCE, COEFFS)
            (grad,) = torch.autograd.grad(loss, [emb_f])
            engine.adam_step(emb_f, grad.contiguous(), m, v, 1e-2, state["k"])

        emb_s = emb_f.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([emb_s], lr=1e-2)

        def stock():
            e = emb_s.sum() * 0 + eps
            pred = e + GUIDANCE * (eps_cond - e)
            loss = torch.nn.functional.mse_loss(stock_step(c, pred, cur), prev)
            opt.zero_grad()
            loss.backward()
            opt.step()

        out = torch.empty_like(cur)
        row = dict(dtype=str(dtype).split(".")[-1],
                   inner_step_fused_us=timed(fused, args.iters, args.warmup), inner_step_stock_us=timed(stock, args.iters, args.warmup),
                   inner_step_fused_launches=launches(fused), inner_step_stock_launches=launches(stock),
                   ddim_step_fused_us=timed(lambda: engine.ddim_step(cur, eps, None, 1.0, COEFFS, out=out), args.iters, args.warmup),
                   ddim_step_stock_us=timed(lambda: stock_step(c, eps, cur), args.iters, args.warmup),
                   ddim_step_fused_launches=launches(lambda: engine.ddim_step(cur, eps, None, 1.0, COEFFS, out=out)),
                   ddim_step_stock_launches=launches(lambda: stock_step(c, eps, cur)))
        print(json.dumps(row))


if __name__ == "__main__":
    main()
