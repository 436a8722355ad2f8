#!/usr/bin/env python3
"""Null-text inversion outside the UNet on one MI355X: per inner step of null_optimization (reference inversion.py:198-204),
everything between the UNet's output and the updated embedding -- guided step + loss + gradient + Adam -- fused
(engine.NullTextLoss + engine.adam_step) against the stock-torch composition of the same lines under autograd with
torch.optim.Adam; and the ddim_loop step alone (engine.ddim_step against next_step's expression).

The UNet is stood in for by `eps_uncond = embedding.sum() * 0 + eps`, the cheapest graph that carries a gradient back to the
[1,77,768] embedding, the same on both sides.  Latents [1,4,64,64].  Time: HIP events over `--iters` steps after `--warmup`;
launches: torch.profiler's device kernels of one step.  One JSON line per dtype.

  python tools/inversion_bench.py [--iters 200] [--warmup 20]

--frames F: instead, null-text inversion of F frames on the stand-in model (tools/null_fake_model.py, form "exact", float32, 5 outer
steps of up to 10 inner steps): NullInversion.invert on the F frames one after the other against NullInversion.invert_frames on all
of them in one batch -- wall time of each (host clock around a device synchronise, the best of --repeats), device kernels and
device-to-host copies of one run each, from torch.profiler (the batched loop's one read per inner step is such a copy; the
single-frame loop's `loss.item()` does not always appear as one in the trace, so compare the kernels and the time, not the copies).  The stand-in's UNet costs next to nothing, so the time is
launches and waits: what the batch saves on a real UNet is not measured here.  One JSON line.
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


def stock_step(c, e, x, prediction="epsilon"):
    c1, c2, c3, c4 = c
    if prediction == "v_prediction":   # e is the model's v
        return c4 * (c2 * x - c1 * e) + c3 * (c2 * e + c1 * x)
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


def frames_bench(frames, repeats, prediction="epsilon"):
    import time

    from torch.profiler import ProfilerActivity, profile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import null_fake_model as nm
    from comfystereo_amd import inversion, stereo_utils
    steps, inner, guidance, epsilon = 5, 10, 7.5, 9.34e-3
    images = torch.stack([torch.from_numpy(nm.seeded_image(11 + f)) for f in range(frames)]).cuda()
    model = nm.NullModel("exact", "cuda")
    model.scheduler.config.prediction_type = prediction   # (NullInversion reads it from the scheduler)

    def one_by_one():
        for f in range(frames):
            inversion.NullInversion(model, steps, guidance).invert(images[f], "a photo", num_inner_steps=inner, early_stop_epsilon=epsilon)
        stereo_utils.restore_attention(model)

    def batched():
        inversion.NullInversion(model, steps, guidance).invert_frames(images, "a photo", num_inner_steps=inner, early_stop_epsilon=epsilon)
        stereo_utils.restore_attention(model)

    row = dict(frames=frames, prediction=prediction, outer_steps=steps, max_inner_steps=inner)
    for name, fn in (("one_by_one", one_by_one), ("batched", batched)):
        fn()
        best = float("inf")
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [ev.name.lower().replace(" ", "").replace("->", "to") for ev in prof.events()
                 if ev.device_type == torch.autograd.DeviceType.CUDA]
        copies = [n for n in names if "memcpy" in n or "copy" in n and "kernel" not in n]
        row[name] = dict(ms=best * 1e3, kernels=len(names) - len(copies),
                         device_to_host_copies=sum("dtoh" in n or "devicetohost" in n for n in copies))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="time F frames one after the other against the batched inversion")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prediction", choices=["epsilon", "v"], default="epsilon",
                    help="what the model predicts: v = a v-prediction model, the SD 2.x 768-v checkpoints")
    args = ap.parse_args()
    prediction = {"epsilon": "epsilon", "v": "v_prediction"}[args.prediction]
    if args.frames:
        if args.frames < 1:
            ap.error("--frames must be positive")
        return frames_bench(args.frames, args.repeats, prediction)
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
            loss = engine.NullTextLoss.apply(e, eps_cond, cur, prev, GUIDANCE, COEFFS, prediction)
            (grad,) = torch.autograd.grad(loss, [emb_f])
            engine.adam_step(emb_f, grad.contiguous(), m, v, 1e-2, state["k"])

        emb_s = emb_f.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([emb_s], lr=1e-2)

        def stock():
            e = emb_s.sum() * 0 + eps
            pred = e + GUIDANCE * (eps_cond - e)
            loss = torch.nn.functional.mse_loss(stock_step(c, pred, cur, prediction), prev)
            opt.zero_grad()
            loss.backward()
            opt.step()

        out = torch.empty_like(cur)
        def fused_step():
            return engine.ddim_step_pred(cur, eps, None, 1.0, COEFFS, out=out, prediction=prediction)

        row = dict(dtype=str(dtype).split(".")[-1], prediction=prediction,
                   inner_step_fused_us=timed(fused, args.iters, args.warmup), inner_step_stock_us=timed(stock, args.iters, args.warmup),
                   inner_step_fused_launches=launches(fused), inner_step_stock_launches=launches(stock),
                   ddim_step_fused_us=timed(fused_step, args.iters, args.warmup),
                   ddim_step_stock_us=timed(lambda: stock_step(c, eps, cur, prediction), args.iters, args.warmup),
                   ddim_step_fused_launches=launches(fused_step),
                   ddim_step_stock_launches=launches(lambda: stock_step(c, eps, cur, prediction)))
        print(json.dumps(row))


if __name__ == "__main__":
    main()
