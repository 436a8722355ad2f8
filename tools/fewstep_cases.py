"""Inputs of one few-step sampler step, made once for the fixture maker (tools/make_fewstep_goldens.py), the CPU tests and the
GPU tests: seeded tensors of a dtype, the coefficients of a step position of a 4-step plan, and the step's expected outputs from
tools/fewstep_oracle.py on the CPU.
"""
import torch

import fewstep_oracle as oracle

DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
POSITIONS = {"first": 0, "middle": 1, "last": 3}   # of the 4-step plan
PLAN_STEPS = 4


def specials(dtype):
    """+-0, +-inf, NaN, the largest finite value and the smallest subnormal of `dtype`, both signs."""
    fi = torch.finfo(dtype)
    tiny = fi.smallest_normal * fi.eps   # the smallest subnormal: 2^(emin - mantissa bits), exact
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), fi.max, -fi.max, tiny, -tiny]
    return torch.tensor(vals, dtype=torch.float64).to(dtype)


def make(sampler, dtype_name, cfg, channels, pos, n, hl, wl, seed=0, guidance=7.5, mask_kind="mixed", special=False):
    """-> dict of CPU tensors and scalars: pred [2n or n,4,hl,wl], s [n,4,hl,wl] (the sample: the Euler state, the LCM input),
    z (LCM, not last), img_latent, noise0, mask_l [n,1,hl,wl] (4 channels), k (the coefficients), last, guidance."""
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(1000 + seed)
    shape = (n, 4, hl, wl)
    rows = 2 * n if cfg else n
    c = dict(sampler=sampler, dtype=dtype, cfg=cfg, channels=channels, n=n, hl=hl, wl=wl, guidance=guidance)
    c["pred"] = torch.randn((rows, 4, hl, wl), generator=g).to(dtype)
    c["s"] = (3.0 * torch.randn(shape, generator=g)).to(dtype)
    ts = oracle.timesteps(sampler, PLAN_STEPS)
    i = POSITIONS[pos]
    c["last"] = i == len(ts) - 1
    c["k"] = oracle.coeffs(sampler, oracle.alphas_cumprod(), ts, i)
    c["z"] = torch.randn(shape, generator=g).to(dtype) if sampler == "lcm" and not c["last"] else None
    c["img_latent"] = torch.randn(shape, generator=g).to(dtype)
    c["noise0"] = torch.randn(shape, generator=g).to(dtype)
    if mask_kind == "mixed":
        m = (torch.rand((n, 1, hl, wl), generator=g) < 0.5)
        m[0, 0, 0, 0], m[-1, 0, -1, -1] = True, False
    else:
        m = torch.full((n, 1, hl, wl), mask_kind == "one")
    c["mask_l"] = m.to(dtype)
    if special:   # the special values in the sample and in the prediction (both halves), each against ordinary partners
        sp = specials(dtype)
        flat_s, flat_p = c["s"].view(-1), c["pred"].view(-1)
        flat_s[1:1 + len(sp)] = sp
        flat_p[12:12 + len(sp)] = sp
        if cfg:
            flat_p[n * 4 * hl * wl + 23:n * 4 * hl * wl + 23 + len(sp)] = sp
        # a NaN in the step's result under a zero mask: the select moves the kept value there, it does not multiply
        c["nan_at"] = (n - 1, 3, hl - 1, wl - 1)
        c["s"][c["nan_at"]] = float("nan")
        if mask_kind != "one":
            c["mask_l"][n - 1, 0, hl - 1, wl - 1] = 0
    return c


def want(c):
    """The oracle's dict(x, state, decode_in) for the inputs of make()."""
    blend = (c["img_latent"], c["noise0"], c["mask_l"]) if c["channels"] == 4 else None
    return oracle.step(c["sampler"], c["pred"], c["s"], c["k"], c["guidance"], c["cfg"], c["last"], z=c["z"], blend=blend)


def bits(t):
    """A tensor's bit patterns on the CPU, every NaN as one pattern (a NaN equals a NaN of any payload, as in the PLMS sweeps)."""
    t = t.detach().cpu().contiguous()
    raw = t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).clone()
    raw[torch.isnan(t)] = -1
    return raw


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))
