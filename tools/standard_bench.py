#!/usr/bin/env python3
"""Times the per-step kernels of StereoDiffusion's Standard mode next to the stock-torch composition of the same arithmetic on
the same GPU, with HIP events:

  FIRST and RESHIFT (engine.latent_shift_apply on a plan made once) at [2, 4, 64, 64] and [2, 4, 128, 128] latents, against a
  gather through the same table followed by the reference's boolean-mask indexing (stereodiffusion_nodes.py:654-660, :667);
  decode_to_codes plus the Pillow-exact resize back to 1080p and 4K, against torch's (x / 2 + 0.5).clamp(0, 1), the copy to the
  host, nan_to_num, * 255, uint8 there (:673-677) and the copy back for the same resize.

  python tools/standard_bench.py [--iters 200]
  python tools/standard_bench.py --scheduler ddim [--steps 50] [--rounds 20]
--scheduler ddim times the Standard loop's step outside the UNet instead (a UNet that returns a fixed tensor), three ways, in turn
in one process, `rounds` times, the median per step reported:
  fused    _StandardLoop.fused_step: one cs_standard_step launch on the persistent input
  unfused  the loop without the fused step: diffusion_step (cat, chunk, torch's guidance) over the same DDIMScheduler.step
           (cs_ddim_step), and cs_latent_shift_apply on the shift steps
  stock    the same arithmetic in stock torch: cat, guidance, the DDIM expression on 0-dim coefficients, gather and boolean masks
and counts the device kernels of one loop with torch.profiler, divided by its steps.  One JSON line per dtype.
It prints a table and judges nothing: there is no threshold in it.  DESIGN.md section 2 holds the numbers of whoever ran it.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfystereo_amd import engine  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # microseconds per call


def torch_gather(left, src_col):
    idx = src_col.clamp(min=0).long()[:, None].expand(-1, left.shape[1], -1, -1)
    return torch.where((src_col >= 0)[:, None], torch.gather(left, 3, idx), torch.zeros((), dtype=left.dtype, device=left.device))


def torch_first(latents, src_col, noise):
    ts = torch_gather(latents[:1], src_col)
    latents = torch.cat([latents[:1], ts], 0)
    mask = (ts[:, 0] != 0)[:, None].repeat(1, latents.shape[1], 1, 1)
    latents[1:][~mask] = noise[~mask]
    latents[1:][mask] = ts[mask]
    return latents, mask


def torch_reshift(latents, src_col, mask):
    ts = torch_gather(latents[:1], src_col)
    latents[1:][mask] = ts[mask]
    return latents


class FixedUNet(torch.nn.Module):
    in_channels = 4

    def __init__(self, pred):
        super().__init__()
        self.pred = pred

    def forward(self, x, t, encoder_hidden_states=None):
        return {"sample": self.pred}


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


def ddim_main(args):
    import json
    import types

    from comfystereo_amd import schedulers
    from comfystereo_amd import stereodiffusion_nodes as sdn
    steps, guidance = args.steps, 7.5
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float16, torch.float32):
        pred = torch.randn((4, 4, 64, 64), generator=g).to(dtype).cuda()
        start = torch.randn((2, 4, 64, 64), generator=g).to(dtype).cuda()
        noise = torch.randn((1, 4, 64, 64), generator=g).to(dtype).cuda()
        disp = torch.rand((1, 64, 64), generator=g).cuda()
        context = torch.zeros((4, 77, 8), dtype=dtype, device="cuda")
        sched = schedulers.DDIMScheduler(prediction_type=args.prediction)
        sched.set_timesteps(steps)
        model = types.SimpleNamespace(unet=FixedUNet(pred), scheduler=sched)
        loop = sdn._StandardLoop(model, disp, 8.0, True, steps, guidance, noise)
        ts = list(sched.timesteps)

        def fused():
            loop.shifted = False
            loop.begin(start, sched.timesteps)
            for i in range(steps):
                loop.fused_step(i, context)

        def unfused():   # what the loop ran before the fused step: loop.step over our scheduler's step
            loop.shifted = False
            lat = start
            for i, t in enumerate(ts):
                lat = loop.step(i, t, lat, context)

        acp, final = sched.alphas_cumprod.cuda(), sched.final_alpha_cumprod.cuda()
        src = loop.src_col

        def stock():
            lat, bmask = start, None
            for i, t in enumerate(ts):
                u, c = model.unet(torch.cat([lat, lat]), t)["sample"].chunk(2)
                e = u + guidance * (c - u)
                prev_t = int(t) - 1000 // steps
                a_t, a_p = acp[int(t)], (acp[prev_t] if prev_t >= 0 else final)
                if args.prediction == "v_prediction":   # e is the guided v
                    x0 = a_t ** 0.5 * lat - (1 - a_t) ** 0.5 * e
                    e = a_t ** 0.5 * e + (1 - a_t) ** 0.5 * lat
                    lat = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e
                else:
                    lat = a_p ** 0.5 * ((lat - (1 - a_t) ** 0.5 * e) / a_t ** 0.5) + (1 - a_p) ** 0.5 * e
                if i == loop.shift_step:
                    lat, bmask = torch_first(lat, src, noise)
                elif bmask is not None and i > loop.shift_step and i % loop.reshift_interval == 0:
                    lat = torch_reshift(lat, src, bmask)

        with torch.no_grad():
            for fn in (fused, unfused, stock):
                fn()
            times = {"fused": [], "unfused": [], "stock": []}
            for _ in range(args.rounds):   # alternating, so that drift falls on all three alike
                for name, fn in (("fused", fused), ("unfused", unfused), ("stock", stock)):
                    times[name].append(loop_time(fn) / steps)
            out = dict(bench="standard_loop_ddim", prediction=args.prediction, dtype=str(dtype).split(".")[-1], latents=[2, 4, 64, 64], steps=steps, rounds=args.rounds)
            for name, fn in (("fused", fused), ("unfused", unfused), ("stock", stock)):
                out[f"{name}_us_per_step"] = round(float(np.median(times[name])), 2)
                out[f"{name}_launches_per_step"] = round(launches(fn) / steps, 2)
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--scheduler", choices=["ddim"], default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--prediction", choices=["epsilon", "v"], default="epsilon",
                    help="what the model predicts (with --scheduler ddim): v = a v-prediction model, the SD 2.x 768-v checkpoints")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "standard_bench.py needs a GPU"
    args.prediction = {"epsilon": "epsilon", "v": "v_prediction"}[args.prediction]
    if args.prediction != "epsilon" and args.scheduler != "ddim":
        ap.error("--prediction v goes with --scheduler ddim (the shift kernels alone do not step)")
    if args.scheduler == "ddim":
        return ddim_main(args)
    rows = []
    g = torch.Generator().manual_seed(0)
    for side in (64, 128):
        for dtype in (torch.float32, torch.float16):
            disp = torch.rand((1, side, side), generator=g).cuda()
            src = engine.latent_shift_plan(disp, 8.0)
            lat = torch.randn((2, 4, side, side), generator=g).to(dtype).cuda()
            noise = torch.randn((1, 4, side, side), generator=g).to(dtype).cuda()
            mask = torch.zeros((1, side, side), dtype=torch.uint8, device="cuda")
            name = f"[2,4,{side},{side}] {str(dtype).split('.')[-1]}"
            rows.append((f"plan (once per image) {name}", timed(lambda: engine.latent_shift_plan(disp, 8.0), args.iters), None))
            ours = timed(lambda: engine.latent_shift_apply(lat[:1], lat[1:], src, mask, "first", noise=noise), args.iters)
            ref = timed(lambda: torch_first(lat, src, noise), args.iters)
            rows.append((f"FIRST {name}", ours, ref))
            _, bmask = torch_first(lat.clone(), src, noise)
            ours = timed(lambda: engine.latent_shift_apply(lat[:1], lat[1:], src, mask, "reshift"), args.iters)
            ref = timed(lambda: torch_reshift(lat, src, bmask), args.iters)
            rows.append((f"RESHIFT {name}", ours, ref))
    image = (torch.randn((2, 3, 512, 512), generator=g)).cuda()
    for label, (w, h) in (("1080p", (1920, 1080)), ("4K", (3840, 2160))):
        stereo = torch.empty((1, h, 2 * w, 3), dtype=torch.float32, device="cuda")

        def ours_fn():
            codes = engine.decode_to_codes(image)
            engine.pil_resize(codes[:1], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
            engine.pil_resize(codes[1:], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])

        def ref_fn():
            x = (image / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).float().numpy()
            codes = torch.from_numpy((np.nan_to_num(x, nan=0.0, posinf=1.0, neginf=0.0) * 255).astype(np.uint8)).cuda()
            engine.pil_resize(codes[:1], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, :w])
            engine.pil_resize(codes[1:], (w, h), f32="nhwc", codes=False, f32_out=stereo[:, :, w:])

        rows.append((f"decode_to_codes + resize back to {label}", timed(ours_fn, max(1, args.iters // 10)),
                     timed(ref_fn, max(1, args.iters // 10))))
    print(f"{'what':58s} {'HIP us':>10s} {'torch us':>10s} {'ratio':>7s}")
    for what, ours, ref in rows:
        print(f"{what:58s} {ours:10.1f} " + (f"{ref:10.1f} {ref / ours:7.2f}" if ref is not None else f"{'-':>10s} {'-':>7s}"))


if __name__ == "__main__":
    main()
