"""Edge inputs of the few-step sampler kernels (cs_fewstep.hip: k_inpaint_fewstep_init, k_inpaint_fewstep_step) and their CPU
reference, shared by tests/test_fewstep_edges_surface.py (which holds the reference side to its conditions) and
tests/test_gpu_fewstep_edges.py (which compares the kernels with it bit for bit).  Plain torch on the CPU; nothing in the package
imports it.

The value tables are those of the PLMS sweep (tools/inpaint_edge_inputs.py) under the step's own operand names: every float16 /
bfloat16 bit pattern in one operand against 16 finite special values in each of the other five, rolled against each other.  What is
new here are the masks of the RePaint select, the coefficient sets of plans a user can ask for, the plan that cycles guidance,
mask and instantiation over the crossing, and the inputs of the first latents.  The reference is tools/fewstep_oracle.py, called,
not restated.
"""
import torch

import fewstep_oracle as oracle
import inpaint_edge_inputs as ei
from inpaint_edge_inputs import every_half, finite_specials, fit, nonfinite_specials, random_patterns, widened_specials

SAMPLERS = oracle.SAMPLERS
OPERANDS = ("s", "u", "t", "z", "img_latent", "noise0")   # the sample, the prediction's two halves, LCM's noise, the blend's two
_THEIRS = dict(zip(OPERANDS, ei.OPERANDS))                # the PLMS tables have six operands too: theirs under our names
GUIDANCES = ei.GUIDANCES
INSTANTIATIONS = ((True, 9), (True, 4), (False, 9), (False, 4))   # (cfg, channels); with the sampler the kernel's eight
MASKS = ("pattern", "complement", "inside", "outside")
HL = WL = 512   # [1, 4, 512, 512]: the smallest latent shape of 16 x 65 536 elements per operand; it takes the 16-byte path


def _ours(theirs):
    return {name: theirs[_THEIRS[name]] for name in OPERANDS}


def live(sampler, cfg, channels, last):
    """The operands the step reads."""
    names = ["s", "u"] + (["t"] if cfg else []) + (["z"] if sampler == "lcm" and not last else [])
    if channels == 4:
        names += ["img_latent"] + ([] if last else ["noise0"])
    return tuple(names)


# ---- values ------------------------------------------------------------------------------------------------------------------------
def table(dtype, every="s"):
    """The six operands, 2^20 elements each: `every` holds the 65 536 patterns 16 times, each other operand one of the 16 finite
    specials per 65 536 elements."""
    return _ours(ei.table(dtype, "sample" if every == "s" else _THEIRS[every]))


def signed_zero_table(dtype, numel=64):
    """Every assignment of +0 / -0 to the six operands: 64 rows, continued from the first on up to `numel` elements."""
    return _ours(ei.signed_zero_table(dtype, numel))


def float32_table(seed=41, count=1 << 20):
    """The six operands in float32: the widened specials crossed, then `count` random bit patterns each."""
    return _ours(ei.float32_table(seed, count))


def layout(numel, wide):
    """(hl, wl) with 4 * hl * wl >= numel: a multiple of 8 elements per plane for the 16-byte path, an odd count for the other."""
    hwl = -(-numel // 4)
    return (8, -(-hwl // 8)) if wide else (1, hwl + 1 - hwl % 2)


def float32_case_table(wide):
    """(float32_table continued with its head up to a latent shape, hl, wl)."""
    ops = float32_table()
    hl, wl = layout(ops["s"].numel(), wide)
    return {name: fit(v, 4 * hl * wl) for name, v in ops.items()}, hl, wl


def nonfinite_tables(dtype, operands):
    """(bad operand, the six operands), 5 x 65 536 elements: per non-finite special a slice of the finite table that holds every
    sample once and all 16 rows of specials (17 is odd, so 17 j runs through every residue), with the operand replaced."""
    full, bad = table(dtype), nonfinite_specials(dtype)
    n = 1 << 16
    idx = torch.cat([(torch.arange(n) * 17 + 4099 * k) % (16 * n) for k in range(len(bad))])
    base = {name: v[idx].contiguous() for name, v in full.items()}
    for operand in operands:
        ops = dict(base)
        ops[operand] = bad.repeat_interleave(n)
        yield operand, ops


# ---- masks -------------------------------------------------------------------------------------------------------------------------
def mask_values(dtype):
    """(inside, outside): what the select `mask_l != 0` takes for the step and for the kept value."""
    fi = torch.finfo(dtype)
    sub = fi.smallest_normal * fi.eps
    inside = torch.tensor([1.0, -1.0, 2.0, sub, -sub, float("inf"), float("nan"), fi.max], dtype=torch.float64).to(dtype)
    return inside, torch.tensor([0.0, -0.0], dtype=torch.float64).to(dtype)


def mask_from(inside, dtype):
    """A bool pattern [hl, wl] as mask_l [1, 1, hl, wl]: the inside pixels cycle over the eight inside values in their own order,
    the outside ones over the two zeros in theirs."""
    flat = inside.reshape(-1)
    vin, vout = mask_values(dtype)
    rank_in, rank_out = flat.cumsum(0) - 1, (~flat).cumsum(0) - 1
    m = torch.where(flat, vin[rank_in.clamp(min=0) % len(vin)], vout[rank_out.clamp(min=0) % len(vout)])
    return m.view((1, 1) + tuple(inside.shape)).contiguous()


def mask_pattern(hl, wl, seed=7):
    """bool [hl, wl], seeded, half of the pixels inside (one more outside for an odd count)."""
    n = hl * wl
    return (torch.randperm(n, generator=torch.Generator().manual_seed(seed)) < n // 2).view(hl, wl)


def mask_tables(dtype, hl=HL, wl=WL):
    """MASKS: the seeded pattern, its complement -- so that every element of a table meets both sides of the select -- and the
    masks that are inside, and outside, everywhere."""
    p = mask_pattern(hl, wl)
    return {"pattern": mask_from(p, dtype), "complement": mask_from(~p, dtype), "inside": mask_from(torch.ones_like(p), dtype),
            "outside": mask_from(torch.zeros_like(p), dtype)}


def every_mask(dtype, hl=HL, wl=WL):
    """mask_l of every half bit pattern, tiled."""
    return fit(every_half(dtype), hl * wl).view(1, 1, hl, wl)


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
PLAN_SETS = (("4 first", 4, 1.0, 0), ("4 last", 4, 1.0, 3), ("1 only", 1, 1.0, 0), ("50 first", 50, 1.0, 0), ("50 last", 50, 1.0, 49),
             ("4 at strength 0.6", 4, 0.6, 0))


def synthetic_set(sampler):
    """Coefficients no plan gives (a plan's are all positive but Euler's k0): the first step of the 4-step plan with Euler's k0
    and k2, LCM's k2, k3 and k4 negated.  They reach results of -0.0 that no plan set reaches."""
    k = list(oracle.coeffs(sampler, oracle.alphas_cumprod(), oracle.timesteps(sampler, 4), 0))
    for j in ((0, 2) if sampler == "euler" else (2, 3, 4)):
        k[j] = -k[j]
    assert (k[0] > 0 and k[2] < 0) if sampler == "euler" else max(k[2:5]) < 0
    return tuple(k)


def coeff_sets(sampler):
    """(name, k, last): six sets from plans a user can ask for -- 50 steps is the longest plan LCM accepts, "1 only" a first step
    that is the last -- and the synthetic one."""
    acp = oracle.alphas_cumprod()
    sets = []
    for name, steps, strength, i in PLAN_SETS:
        ts = oracle.timesteps(sampler, steps, strength)
        sets.append((name, oracle.coeffs(sampler, acp, ts, i), i == len(ts) - 1))
    return sets + [("synthetic", synthetic_set(sampler), False)]


def sweep_plan(sampler):
    """The runs of the crossing, one per `every` operand and coefficient set under which the step reads that operand:
    dict(every, set, k, last, cfg, channels, guidance, mask).  The instantiation cycles over those that read the operand, the
    guidance over the runs with guidance, the mask table over the runs with a mask -- but for the mask that hides the operand
    everywhere: "outside" goes with the blend's operands only, "inside" with the step's."""
    plan, count = [], dict(inst=0, guidance=0, step=0, keep=0)
    for every in OPERANDS:
        for name, k, last in coeff_sets(sampler):
            allowed = [(cfg, ch) for cfg, ch in INSTANTIATIONS if every in live(sampler, cfg, ch, last)]
            if not allowed:
                continue
            cfg, channels = allowed[count["inst"] % len(allowed)]
            count["inst"] += 1
            guidance, mask = GUIDANCES[count["guidance"] % len(GUIDANCES)], None
            count["guidance"] += cfg
            if channels == 4:
                side, hidden = ("keep", "inside") if every in ("img_latent", "noise0") else ("step", "outside")
                shown = [m for m in MASKS if m != hidden]
                mask = shown[count[side] % len(shown)]
                count[side] += 1
            plan.append(dict(every=every, set=name, k=k, last=last, cfg=cfg, channels=channels, guidance=guidance, mask=mask))
    return plan


# ---- the step ----------------------------------------------------------------------------------------------------------------------
def case(sampler, ops, k, last, guidance, cfg, channels, mask=None, hl=HL, wl=WL):
    """Flat operands of 4 * hl * wl elements as the dict tools/fewstep_cases.make gives (one frame)."""
    shape = (1, 4, hl, wl)
    dtype = ops["u"].dtype
    v = {name: ops[name].view(shape) for name in OPERANDS}
    assert (mask is not None) == (channels == 4) and (mask is None or (mask.shape == (1, 1, hl, wl) and mask.dtype == dtype))
    return dict(sampler=sampler, dtype=dtype, cfg=cfg, channels=channels, n=1, hl=hl, wl=wl, guidance=guidance, k=tuple(k), last=last,
                pred=torch.cat([v["u"], v["t"]]) if cfg else v["u"], s=v["s"], z=v["z"] if sampler == "lcm" and not last else None,
                img_latent=v["img_latent"], noise0=v["noise0"], mask_l=mask)


def reference_step(c):
    """The oracle's dict(x, state, decode_in) for a case()."""
    blend = (c["img_latent"], c["noise0"], c["mask_l"]) if c["channels"] == 4 else None
    return oracle.step(c["sampler"], c["pred"], c["s"], c["k"], c["guidance"], c["cfg"], c["last"], z=c["z"], blend=blend)


# ---- the first latents -------------------------------------------------------------------------------------------------------------
INIT_OPERANDS = ("il", "noise")


def init_timesteps(sampler):
    """999, 499 and the smallest timestep a 50-step plan starts from under strength < 1: its last."""
    return (999, 499, oracle.timesteps(sampler, 50)[-1])


def init_inputs(dtype, every):
    """(il, noise), 2^20 elements: `every` holds every half value 16 times, the other one finite special per 65 536 elements;
    float32: both the widened specials crossed, then 2^20 random bit patterns."""
    if dtype == torch.float32:
        sp = widened_specials()
        return (torch.cat([sp.repeat(len(sp)), random_patterns(1 << 20, 51)]),
                torch.cat([sp.repeat_interleave(len(sp)), random_patterns(1 << 20, 52)]))
    ev, sp = every_half(dtype).repeat(16), finite_specials(dtype).repeat_interleave(1 << 16)
    return (ev, sp) if every == "il" else (sp, ev)


def reference_init(sampler, il, noise, t0):
    """-> (channels 0..3 of the first input, the state: for LCM the same).  noise None: no timestep is left, both are il."""
    if noise is None:
        return il, il
    x, state = oracle.first_latents(sampler, il, noise, oracle.alphas_cumprod(), t0)
    return x, x if state is None else state


# ---- what the surface test measures --------------------------------------------------------------------------------------------------
def is_subnormal(t):
    return (t != 0) & (t.abs() < torch.finfo(t.dtype).smallest_normal)


def is_negative_zero(t):
    return (t == 0) & torch.signbit(t)
