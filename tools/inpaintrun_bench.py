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

--sampler euler|lcm [--channels 4|9]: the few-step samplers instead (default --steps 4), without classifier-free guidance, at the
UNet inputs [1, C, 64, 64] and [16, C, 64, 64]:
  ours   comfystereo_amd.inpaint_runner.FewStepLoop.step: one cs_inpaint_fewstep_step launch
  stock  tools/fewstep_stock.loop_step: the cat (9 channels), the step of tools/fewstep_oracle.py, the blend (4 channels)
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
import fewstep_oracle  # noqa: E402
import fewstep_stock  # noqa: E402
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


def measure(ours, stock_loop, rounds):
    for _ in range(3):
        ours()
        stock_loop()
    torch.cuda.synchronize()
    t_ours, t_stock = [], []
    for _ in range(rounds):
        t_ours.append(loop_time(ours))
        t_stock.append(loop_time(stock_loop))
    return statistics.median(t_ours), statistics.median(t_stock)


def fewstep_main(args):
    """The few-step samplers without guidance: [n, C, 64, 64] float16, n = 1 and 16."""
    dtype, hl, wl, sampler, channels = torch.float16, 64, 64, args.sampler, args.channels
    steps = args.steps or 4
    acp = fewstep_oracle.alphas_cumprod()
    ts = fewstep_oracle.timesteps(sampler, steps)
    for n in (1, 16):
        g = torch.Generator().manual_seed(0)
        lat = lambda: torch.randn(n, 4, hl, wl, generator=g).to(dtype).cuda()   # noqa: E731
        pred = (0.1 * torch.randn(n, 4, hl, wl, generator=g)).to(dtype).cuda()
        x0 = torch.randn(n, channels, hl, wl, generator=g).to(dtype).cuda()
        state0, img_latent, noise0 = lat(), lat(), lat()
        step_noise = torch.stack([lat() for _ in range(max(steps - 1, 1))])
        mask_l = (torch.rand(n, 1, hl, wl, generator=g) < 0.5).to(dtype).cuda()
        unet = FixedUNet(pred)
        unet.in_channels = channels
        runner = ir.InpaintRunner(unet, None, None, None, sampler=sampler)
        x = x0.clone()
        loop = ir.FewStepLoop(runner, x, None, ts, 0.0, sampler, False, noise0=noise0, step_noise=step_noise)
        loop.img_latent = img_latent
        if loop.mask_l is not None:
            loop.mask_l.copy_(mask_l)

        def ours():
            x.copy_(x0)
            if loop.state is not None:
                loop.state.copy_(state0)
            for i in range(steps):
                loop.step(i)

        mask9, masked9 = (x0[:, 4:5].contiguous(), x0[:, 5:].contiguous()) if channels == 9 else (None, None)
        blend = (img_latent, noise0, mask_l) if channels == 4 else None
        plan = [fewstep_oracle.coeffs(sampler, acp, ts, i) for i in range(steps)]
        t_model = [torch.tensor(t) for t in ts]

        def stock_loop():
            x_lat, state = x0[:, :4], state0
            for i in range(steps):
                last = i == steps - 1
                out = fewstep_stock.loop_step(unet, sampler, state, x_lat, mask9, masked9, t_model[i], None, plan[i], 0.0, False, last, channels,
                                              z=step_noise[i] if sampler == "lcm" and not last else None, blend=blend)
                x_lat, state = out["x"], out["state"]
            return x_lat

        t_ours, t_stock = measure(ours, stock_loop, args.rounds)
        row = dict(sampler=sampler, shape=[n, channels, hl, wl], dtype="float16", steps=steps, rounds=args.rounds, cfg=False,
                   ours_us_per_step=t_ours / steps, stock_us_per_step=t_stock / steps,
                   ours_launches_per_step=launches(lambda: [loop.step(i) for i in range(steps)]) / steps,
                   stock_launches_per_step=launches(stock_loop) / steps)
        row["ratio_stock_over_ours"] = row["stock_us_per_step"] / row["ours_us_per_step"]
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--sampler", choices=("plms", "euler", "lcm"), default="plms")
    ap.add_argument("--channels", type=int, choices=(4, 9), default=9)
    args = ap.parse_args()
    if args.sampler != "plms":
        return fewstep_main(args)
    if args.channels != 9:
        ap.error("--sampler plms takes --channels 9")
    args.steps = args.steps or 20
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
