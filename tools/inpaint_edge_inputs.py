"""Edge inputs of the inpainting-loop kernels (cs_inpaintloop.hip) and their CPU reference, shared by
tests/test_inpaint_edges_surface.py (which holds the reference side to its conditions) and tests/test_gpu_inpaint_edges.py (which
compares the kernels with it bit for bit).  Plain torch on the CPU; nothing in the package imports it.

The operand table of the step crosses every float16 / bfloat16 bit pattern in one operand with 16 finite special values in each of
the other five, rolled against each other so that a row's operands differ.
"""
import itertools

import torch

import plms_oracle

KINDS = ("first", "second", "order2", "order3", "order4")
KIND_COUNTER = {"first": 0, "second": 1, "order2": 2, "order3": 3, "order4": 4}   # the oracle's counter at which the kind occurs
NEEDS = {"first": 0, "second": 1, "order2": 1, "order3": 2, "order4": 3}          # earlier predictions the kind reads
OPERANDS = ("sample", "u", "t", "e1", "e2", "e3")
GUIDANCES = (7.5, 7.3, 1.0, 0.0, -2.0)     # 7.3 has a full float32 mantissa; 1, 0 and a negative scale make exact and signed zeros
VAE_SCALE = 0.18215


def every_half(dtype):
    """The 65 536 bit patterns of a 16-bit float type."""
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


def finite_specials(dtype):
    fi = torch.finfo(dtype)
    sub, ulp, nrm = fi.smallest_normal * fi.eps, fi.eps, fi.smallest_normal
    return torch.tensor([0.0, -0.0, sub, -sub, 1.0, -1.0, 1.0 + ulp, 1.0 + 3 * ulp, nrm, -nrm / 2, 0.5, 3 * sub, 1e-3, -1e-3, 2.0, -0.75],
                        dtype=torch.float64).to(dtype)


def nonfinite_specials(dtype):
    """inf, -inf, NaN, and the two finite values whose products and sums leave the range."""
    fi = torch.finfo(dtype)
    return torch.tensor([float("inf"), float("-inf"), float("nan"), fi.max, -fi.max], dtype=torch.float64).to(dtype)


def table(dtype, every="sample"):
    """The six operands of the step, 2^20 elements each: `every` (the sample; "t": the conditional prediction, so that the guidance
    product and every combination meet all values too) holds every_half 16 times, the others one special per 65 536 elements."""
    ev, sp = every_half(dtype), finite_specials(dtype)
    n = ev.numel()
    ops = {"sample": ev.repeat(len(sp)), "u": sp.repeat_interleave(n), "t": sp.roll(5).repeat_interleave(n)}
    for name, shift in (("e1", 3), ("e2", 7), ("e3", 11)):
        ops[name] = sp.roll(shift).repeat_interleave(n)
    if every != "sample":
        ops["sample"], ops[every] = ops[every], ops["sample"]
    return ops


def signed_zero_table(dtype, numel=64):
    """Every assignment of +0 / -0 to the six operands: 64 rows, repeated from the first on up to `numel` elements."""
    rows = torch.tensor(list(itertools.product((0.0, -0.0), repeat=len(OPERANDS))), dtype=torch.float64).to(dtype)
    return {name: fit(rows[:, k].contiguous(), numel) for k, name in enumerate(OPERANDS)}


def fit(flat, numel):
    """`flat` continued with its own head up to `numel` elements (numel >= len(flat))."""
    assert numel >= flat.numel()
    reps = -(-numel // flat.numel())
    return flat.repeat(reps)[:numel].contiguous()


def seeded_oracle(kind, operands, num_steps, step_index):
    """(oracle, timestep): a PLMSOracle whose state is the one `kind` meets, set directly -- the counter, the kept predictions (the
    oldest first, as the oracle keeps them) and cur_sample -- at the timestep of `step_index`."""
    sch = plms_oracle.PLMSOracle()
    sch.set_timesteps(num_steps)
    sch.counter = KIND_COUNTER[kind]
    sch.ets = [operands[name] for name in ("e3", "e2", "e1")[3 - NEEDS[kind]:]]
    sch.cur_sample = operands["sample"] if kind == "second" else None
    return sch, sch.timesteps[step_index]


def reference_step(kind, operands, guidance, num_steps, step_index):
    """One step of the stock loop on the CPU -> (prev, e, prev / 0.18215).  The guidance expression is
    tools/inpaintrun_stock.loop_step's, the step PLMSOracle's from a seeded state."""
    sch, t = seeded_oracle(kind, operands, num_steps, step_index)
    noise_pred_uncond, noise_pred_text = operands["u"], operands["t"]
    noise_pred = noise_pred_uncond + guidance * (noise_pred_text - noise_pred_uncond)
    prev = sch.step(noise_pred, t, operands["sample"]).prev_sample
    return prev, noise_pred, prev / VAE_SCALE


def coeff_sets(kind):
    """(name, num_steps, step_index) of the coefficient sets every kind is run with: its own counter of a 6-step run; the same
    counter of a 50-step run (small da and denom); the last step of the 6-step run (timestep 0: prev_t < 0, the final alpha, so
    sc = 1 and da = 0 exactly -- every da * m is a zero, an infinite m a NaN; second goes over the interval before it instead);
    the last but one of the 50-step run (sc a few half ulp above 1)."""
    c = KIND_COUNTER[kind]
    return (("own", 6, c), ("fifty", 50, c), ("last", 6, 6), ("near one", 50, 49))


def widened_specials():
    """The finite and non-finite specials of all three dtypes as float32 values."""
    return torch.cat([torch.cat([finite_specials(d), nonfinite_specials(d)]).float() for d in (torch.float32, torch.float16, torch.bfloat16)])


def random_patterns(count, seed):
    """`count` float32 values of uniformly random bit patterns."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, (count,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)


def float32_table(seed=21, count=1 << 20):
    """The six operands in float32: the widened specials crossed (sample against u, the others rolled along u), then `count`
    random bit patterns each."""
    sp = widened_specials()
    k = len(sp)
    ops = {"sample": sp.repeat(k), "u": sp.repeat_interleave(k)}
    for name, shift in (("t", 7), ("e1", 3), ("e2", 11), ("e3", 17)):
        ops[name] = sp.roll(shift).repeat_interleave(k)
    return {name: torch.cat([ops[name], random_patterns(count, seed + j)]) for j, name in enumerate(OPERANDS)}


def latent_init_inputs(mean_dtype, dtype, seed=33):
    """(mean_img, mean_masked, noise) of one latent_init case, flat.  Half means: every value, 16 times; float32 means: the widened
    specials and 2^18 random patterns.  mean_masked is a rolled copy.  The noise runs through its 16 finite and 5 non-finite
    specials with period 21 -- coprime to 65 536, so that every mean meets 16 of them."""
    if mean_dtype == torch.float32:
        mean = torch.cat([widened_specials(), random_patterns(1 << 18, seed)])
    else:
        mean = every_half(mean_dtype).repeat(16)
    sp = torch.cat([finite_specials(dtype), nonfinite_specials(dtype)])
    return mean, mean.roll(4097), fit(sp, mean.numel())


def reference_latent_init(mean_img, mean_masked, noise, timestep, dtype):
    """The stock expressions (tools/inpaintrun_stock.run) on the CPU -> (img_latent, masked_latent, latents, latents / 0.18215);
    noise None: no timestep is left and the latents are the image's."""
    img_latent = (mean_img * VAE_SCALE).to(dtype)
    masked_latent = (mean_masked * VAE_SCALE).to(dtype)
    latents = img_latent if noise is None else plms_oracle.PLMSOracle().add_noise(img_latent, noise, torch.tensor([timestep]))
    return img_latent, masked_latent, latents, latents / VAE_SCALE


def class_of(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    t = t.detach().cpu().float()
    return torch.where(t.isnan(), 3, torch.where(t == float("inf"), 1, torch.where(t == float("-inf"), 2, 0)))


def all_codes_frame(h, w):
    """filled uint8 [1,h,w,3], mask uint8 [1,h,w] (h * w >= 512): pixel p holds code (p + 85 c) % 256 in channel c and lies under
    the mask when (p // 256) is odd, so every code occurs in every channel under both mask states."""
    assert h * w >= 512
    p = torch.arange(h * w)
    filled = torch.stack([(p + 85 * c) % 256 for c in range(3)], dim=1).to(torch.uint8).reshape(1, h, w, 3)
    mask = (((p // 256) % 2) * 255).to(torch.uint8).reshape(1, h, w)
    return filled.contiguous(), mask.contiguous()
