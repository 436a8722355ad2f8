#!/usr/bin/env python3
"""Times cs_stereo_attention on the four self-attention levels of SD 1.5 at 512 x 512 under CFG ([uncond, cond] x [left, right],
8 heads), 'uni' and 'bi', with HIP events, next to (a) a stock-torch composition of the reference's arithmetic on the same GPU
(its rearranges, einsum, softmax, einsum -- attn_batch, stereo_utils.py:124-132, per CFG chunk) and (b)
F.scaled_dot_product_attention in float32 on the rearranged tensors.  Prints one JSON line per level and direction; TFLOP/s
counts 4 * queries * keys * d per head (the two products), against the 157 TFLOP/s f32-matrix peak.

  python tools/attention_bench.py [--iters 20] [--warmup 3] [--sweep] [--dtype f16|bf16] [--backward]
--backward: forward + backward of the plain attention that diffusion_utils.register_attention_control installs (batch 2 x 8 heads,
float32): self-attention at the four levels and cross-attention on 77 keys, engine.differentiable_attention next to (a) the
stock-torch composition of the reference's arithmetic (einsum, softmax, einsum; diffusion_utils.py:192-203) under autograd and
(b) F.scaled_dot_product_attention, all on the same GPU in one process, timed alternately.  Per row: median milliseconds of
forward + backward and the peak of torch.cuda.max_memory_allocated above the inputs, for each of the three.
--backward --dtype f16|bf16: the same rows on float16 / bfloat16 tensors for engine.differentiable_attention(..., native_half=True)
(cs_attention_half_fwd_lse / cs_attention_half_bwd), next to (a) the upcast path for the same tensors (native_half=False: three
casts, the float32 kernels, a cast back, and the same again in the backward), (b) the stock-torch composition in the dtype under
autograd and (c) F.scaled_dot_product_attention in the dtype; time and peak memory above the inputs for each of the four.
--sweep: the kernel alone with 1, 2 and 4 waves per workgroup forced (development switch attn_waves) next to the launcher's
choice: the measurement behind attention_waves() in cs_attention.hip (one rule for every dtype; --dtype sweeps the half kernels).
--dtype f16|bf16: cs_stereo_attention_half on random float16 / bfloat16 operands next to (a) the upcast path for the same
inputs (three casts to float32, the float32 kernel, one cast back: stereo_utils.HALF_ATTENTION = False) and (b)
F.scaled_dot_product_attention in that dtype on the routed keys.  The three are timed alternately, round by round, in one
process; the medians and the ratio to the upcast path are printed per level and direction.  TFLOP/s as above.
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


def timed_alternately(fns, iters, warmup):
    """{name: fn} -> {name: (median ms, min ms)}; one call of each per round, so that clock and cache state drift alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in ms.items()}


def half_rows(dtype, iters, warmup):
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    for level, n, d, heads in LEVELS:
        bh = 2 * 2 * heads
        q, k, v = (torch.randn(bh, n, d, device="cuda").to(dt) for _ in range(3))
        scale = d ** -0.5
        for mode in ("uni", "bi"):
            upcast = lambda: engine.stereo_attention(q.float(), k.float(), v.float(), heads, scale, mode, chunks=2).to(dt)  # noqa: E731
            got = engine.stereo_attention(q, k, v, heads, scale, mode, chunks=2)
            err = float((got.float() - upcast().float()).abs().max())
            t = timed_alternately({"kernel": lambda: engine.stereo_attention(q, k, v, heads, scale, mode, chunks=2),
                                   "upcast": upcast, "sdpa": lambda: sdpa(q, k, v, mode, heads, scale)}, iters, warmup)
            flop = 4.0 * bh * n * (2 * n if mode == "bi" else n) * d
            print(json.dumps(dict(dtype=dtype, level=level, n=n, d=d, heads=heads, mode=mode, kernel_ms=round(t["kernel"][0], 4),
                                  kernel_min_ms=round(t["kernel"][1], 4), upcast_ms=round(t["upcast"][0], 4),
                                  sdpa_ms=round(t["sdpa"][0], 4), kernel_tflops=round(flop / t["kernel"][0] / 1e9, 2),
                                  speedup_vs_upcast=round(t["upcast"][0] / t["kernel"][0], 2),
                                  speedup_vs_sdpa=round(t["sdpa"][0] / t["kernel"][0], 2), max_abs_diff_vs_upcast=err)), flush=True)


def backward_rows(iters, warmup, dtype="f32"):
    heads, batch = 8, 2
    bh = batch * heads
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]

    def fold(o):   # '(b h) n d -> b n (h d)'
        return o.reshape(batch, heads, o.shape[1], o.shape[2]).permute(0, 2, 1, 3).reshape(batch, o.shape[1], heads * o.shape[2])

    for level, n, d, _ in LEVELS:
        for kind, n_k in (("self", n), ("cross", 77)):
            scale = d ** -0.5
            q = torch.randn(bh, n, d, device="cuda").to(dt).requires_grad_(True)
            k, v = (torch.randn(bh, n_k, d, device="cuda").to(dt).requires_grad_(True) for _ in range(2))
            d_out = torch.randn(batch, n, heads * d, device="cuda").to(dt)

            def run(fwd):
                q.grad = k.grad = v.grad = None
                fwd().backward(d_out)

            fns = {
                "kernel": lambda: run(lambda: engine.differentiable_attention(q, k, v, heads, scale, native_half=True)),
                "stock": lambda: run(lambda: fold(torch.einsum("b i j, b j d -> b i d",
                                                               (torch.einsum("b i d, b j d -> b i j", q, k) * scale).softmax(dim=-1), v))),
                "sdpa": lambda: run(lambda: fold(F.scaled_dot_product_attention(q, k, v, scale=scale))),
            }
            if dtype != "f32":   # what the same tensors cost without the half kernels
                fns["upcast"] = lambda: run(lambda: engine.differentiable_attention(q, k, v, heads, scale))
            grads, peak = {}, {}
            for name, fn in fns.items():
                fn()
                grads[name] = (q.grad.clone(), k.grad.clone(), v.grad.clone())
                q.grad = k.grad = v.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.max_memory_allocated()
                fn()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() - base
            err = max(float((a.float() - b.float()).abs().max()) for a, b in zip(grads["kernel"], grads["stock"]))
            del grads
            t = timed_alternately(fns, iters, warmup)
            flop = (4.0 + 10.0) * bh * n * n_k * d   # forward 2 products, backward 5 (S, dP, dV, dK, dQ), 2 flop per multiply-add
            extra = {}
            if dtype != "f32":
                extra = dict(dtype=dtype, upcast_ms=round(t["upcast"][0], 4), upcast_peak_mib=round(peak["upcast"] / 2 ** 20, 2),
                             speedup_vs_upcast=round(t["upcast"][0] / t["kernel"][0], 2))
            print(json.dumps(dict(extra, backward=True, level=level, kind=kind, n=n, n_k=n_k, d=d, heads=heads, batch=batch,
                                  kernel_ms=round(t["kernel"][0], 4), kernel_min_ms=round(t["kernel"][1], 4),
                                  stock_ms=round(t["stock"][0], 4), sdpa_ms=round(t["sdpa"][0], 4),
                                  kernel_peak_mib=round(peak["kernel"] / 2 ** 20, 2), stock_peak_mib=round(peak["stock"] / 2 ** 20, 2),
                                  sdpa_peak_mib=round(peak["sdpa"] / 2 ** 20, 2), kernel_tflops=round(flop / t["kernel"][0] / 1e9, 2),
                                  speedup_vs_stock=round(t["stock"][0] / t["kernel"][0], 2),
                                  speedup_vs_sdpa=round(t["sdpa"][0] / t["kernel"][0], 2), max_abs_grad_diff_vs_stock=err)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--dtype", choices=("f32", "f16", "bf16"), default="f32")
    ap.add_argument("--backward", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.backward:
        backward_rows(args.iters, args.warmup, args.dtype)
        return
    if args.dtype != "f32" and not args.sweep:
        half_rows(args.dtype, args.iters, args.warmup)
        return
    if args.sweep:
        dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
        for level, n, d, heads in LEVELS:
            q, k, v = (torch.randn(4 * heads, n, d, device="cuda").to(dt) for _ in range(3))
            for mode in ("uni", "bi"):
                row = dict(dtype=args.dtype, level=level, n=n, d=d, mode=mode)
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
