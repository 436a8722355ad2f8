#!/usr/bin/env python3
"""Fast mode's inpainting loop outside the UNet on one MI355X: everything between two UNet calls of a 20-step run (21 PLMS
timesteps), float16, at the UNet inputs [2, 9, 64, 64] (one frame) and [32, 9, 64, 64] (sixteen frames in one batch).

  ours   comfystereo_amd.inpaint_runner.InpaintLoop.step: one cs_inpaint_plms_step launch on the persistent input
  stock  the stock-torch composition of reference model_wrappers.py:605-625 (tools/inpaintrun_stock.loop_step) with
         tools/plms_oracle.PLMSOracle as the scheduler: three cats, a .to, the guidance expression, the scheduler's step

The UNet is stood in for by a function that returns one fixed prediction, the same on both sides, so what is timed is the loop
around it.  The two sides alternate in one process, `--rounds` times each, a whole loop per measurement between two HIP events
(the events see the stream: where the host cannot launch fast enough the gaps count, as they do in a real run); the median per
step is reported.  Launches per step: torch.profiler's device kernels over one loop, divided by its steps.  One JSON line per
shape.

  python tools/inpaintrun_bench.py [--rounds 20] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inpaintrun_stock as stock  # noqa: E402
import plms_oracle  # noqa: E402
from comfystereo_amd import inpaint_runner as ir  # noqa: E402

GUIDANCE = 7.5


class FixedUNet(torch.nn.Module):
    in_channels = 9

    def __init__(self, pred):
        super().__init__()
        self.pred = pred

    def forward(self, x, t, context=None):
        return self.pred


def loop_time(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3   # microseconds


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
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    dtype, hl, wl = torch.float16, 64, 64
    for n in (1, 16):
        g = torch.Generator().manual_seed(0)
        pred = (0.1 * torch.randn(2 * n, 4, hl, wl, generator=g)).to(dtype).cuda()
        x0 = torch.randn(2 * n, 9, hl, wl, generator=g).to(dtype).cuda()
        x0[n:] = x0[:n]
        unet = FixedUNet(pred)
        runner = ir.InpaintRunner(unet, None, None, None)
        runner.num_inference_steps = args.steps
        timesteps = ir.plms_timesteps(args.steps)
        x = x0.clone()
        loop = ir.InpaintLoop(runner, x, None, timesteps, GUIDANCE)

        def ours():
            x.copy_(x0)
            for i in range(len(timesteps)):
                loop.step(i)

        scheduler = plms_oracle.PLMSOracle()
        mask_latent, masked_img_latent = x0[:n, 4:5].contiguous(), x0[:n, 5:].contiguous()
        ts = plms_oracle.plms_timesteps(args.steps)

        def stock_loop():
            scheduler.set_timesteps(args.steps)
            latents = x0[:n, :4]
            for t in ts:
                latents = stock.loop_step(unet, scheduler, latents, mask_latent, masked_img_latent, t, None, GUIDANCE, dtype)
            return latents

        # (stock.loop_step calls unet(x, t.expand(2)...): the stand-in ignores t, so the batch of 2n needs no other expand)
        for _ in range(3):
            ours()
            stock_loop()
        torch.cuda.synchronize()
        t_ours, t_stock = [], []
        for _ in range(args.rounds):
            t_ours.append(loop_time(ours))
            t_stock.append(loop_time(stock_loop))
        steps = len(timesteps)
        row = dict(shape=[2 * n, 9, hl, wl], dtype="float16", steps=args.steps, timesteps=steps, rounds=args.rounds,
                   ours_us_per_step=statistics.median(t_ours) / steps, stock_us_per_step=statistics.median(t_stock) / steps,
                   ours_launches_per_step=launches(lambda: [loop.step(i) for i in range(steps)]) / steps,
                   stock_launches_per_step=launches(stock_loop) / steps)
        row["ratio_stock_over_ours"] = row["stock_us_per_step"] / row["ours_us_per_step"]
        print(json.dumps(row))


if __name__ == "__main__":
    main()
