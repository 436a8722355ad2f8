"""The reference side of tests/test_gpu_fewstep_edges.py, without a GPU: the conditions under which a bit-for-bit comparison with
tools/fewstep_edge_inputs.reference_step says something.  The tables hold every value against every special; the reference's
outputs are rarely NaN and reach both zeros, the subnormals and both infinities; the masks and their complements put every
element on both sides of the select, with -0 outside and a subnormal, a negative and a NaN mask inside; the plans are the ones
they are named for; the synthetic coefficients reach a -0.0 of their own; and the plan of the crossing meets every instantiation,
guidance value and mask."""
import functools

import pytest
import torch

import fewstep_edge_inputs as fe
import fewstep_oracle as oracle
from fewstep_cases import bits, same_bits

HALF = ("float16", "bfloat16")
DTYPES = ("float32",) + HALF
NAN_CAP = 0.04   # a cap on the inputs, not a measurement: a NaN equals any NaN, so a NaN-heavy table is a weak test
# The least share of subnormals among the reference's x over the runs of one table, in percent, by (sampler, dtype, every): set
# from what the reference gives on the CPU (the measured shares are in DESIGN.md section 2, FE1), rounded down.  1 % where the
# table reaches it.  bfloat16 has 254 subnormal patterns in 65 536 (0.39 %) where float16 has 2 046 (3.1 %), and LCM's noise z
# reaches the output only as k5 * z beside k4 * den, which is tiny in few rows of specials: those tables stay below 1 %.
SUBNORMAL_FLOOR = {("euler", "float16"): dict(s=1, u=1, t=1, img_latent=1, noise0=1),
                   ("euler", "bfloat16"): dict(s=1, u=1, t=1, img_latent=1, noise0=1),
                   ("lcm", "float16"): dict(s=1, u=1, t=1, z=0.1, img_latent=1, noise0=1),
                   ("lcm", "bfloat16"): dict(s=1, u=1, t=1, z=0.01, img_latent=1, noise0=0.5)}


def raw(t):
    """The bit patterns themselves (fewstep_cases.bits makes every NaN one pattern)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def table(dtype_name, every):
    return fe.table(getattr(torch, dtype_name), every)


@functools.lru_cache(maxsize=None)
def masks(dtype_name):
    return fe.mask_tables(getattr(torch, dtype_name))


def run(sampler, dtype_name, p, mask=None):
    mask = p["mask"] if mask is None else mask
    c = fe.case(sampler, table(dtype_name, p["every"]), p["k"], p["last"], p["guidance"], p["cfg"], p["channels"],
                masks(dtype_name)[mask] if p["channels"] == 4 else None)
    return fe.reference_step(c)


@functools.lru_cache(maxsize=None)
def measured(sampler, dtype_name):
    """The reference over the crossing's plan, once: the largest NaN share of an output tensor, and per `every` table the count
    of x's elements, of its subnormals, and whether it holds +0, -0, +inf, -inf."""
    worst, per = 0.0, {}
    for p in fe.sweep_plan(sampler):
        want = run(sampler, dtype_name, p)
        worst = max([worst] + [float(v.isnan().float().mean()) for v in want.values() if v is not None])
        x = want["x"]
        m = per.setdefault(p["every"], dict(numel=0, subnormal=0, flags=set()))
        m["numel"] += x.numel()
        m["subnormal"] += int(fe.is_subnormal(x).sum())
        for name, hit in (("+0", (x == 0) & ~torch.signbit(x)), ("-0", fe.is_negative_zero(x)), ("+inf", x == float("inf")),
                          ("-inf", x == float("-inf"))):
            if bool(hit.any()):
                m["flags"].add(name)
    return worst, per


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
def test_every_table_holds_every_pattern_against_every_special(dtype_name):
    dtype = getattr(torch, dtype_name)
    special = set(raw(fe.finite_specials(dtype)).tolist())
    assert len(special) == 16
    for every in fe.OPERANDS:
        ops = table(dtype_name, every)
        assert all(v.numel() == 1 << 20 == 4 * fe.HL * fe.WL for v in ops.values())
        ev = raw(ops[every]).int() & 0xFFFF
        assert torch.equal(ev.view(16, -1).sort(dim=1).values, torch.arange(65536, dtype=torch.int32).expand(16, -1)), every
        for name in fe.OPERANDS:
            if name == every:
                continue
            rows = raw(ops[name]).view(16, -1)
            assert bool((rows == rows[:, :1]).all()) and set(rows[:, 0].tolist()) == special, (every, name)   # every pair occurs
        # a row's operands differ
        rows = torch.stack([raw(ops[name]).view(16, -1)[:, 0] for name in fe.OPERANDS if name != every])
        assert all(len(set(rows[:, r].tolist())) == rows.shape[0] for r in range(16)), every


@pytest.mark.parametrize("dtype_name", HALF)
def test_the_first_latents_tables_hold_every_pattern_against_every_special(dtype_name):
    dtype = getattr(torch, dtype_name)
    special = set(raw(fe.finite_specials(dtype)).tolist())
    for every in fe.INIT_OPERANDS:
        il, noise = fe.init_inputs(dtype, every)
        ev, sp = (il, noise) if every == "il" else (noise, il)
        pairs = set(((raw(ev).long() & 0xFFFF) * 65536 + (raw(sp).long() & 0xFFFF)).tolist())
        assert len(pairs) == 16 * 65536 and set(raw(sp).tolist()) == special


def test_the_every_pattern_mask_holds_every_pattern():
    for dtype in (torch.float16, torch.bfloat16):
        m = fe.every_mask(dtype)
        assert m.shape == (1, 1, fe.HL, fe.WL) and len(set(raw(m).reshape(-1).tolist())) == 65536


@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_the_plan_meets_every_instantiation_guidance_and_mask(sampler):
    plan = fe.sweep_plan(sampler)
    sets = fe.coeff_sets(sampler)
    assert len(sets) == 7
    # the crossing: every operand with every coefficient set under which the step reads it
    for every in fe.OPERANDS:
        readable = {name for name, _, last in sets if any(every in fe.live(sampler, cfg, ch, last) for cfg, ch in fe.INSTANTIATIONS)}
        assert {p["set"] for p in plan if p["every"] == every} == readable, every
        assert readable or (every == "z" and sampler == "euler")
    for p in plan:
        assert p["every"] in fe.live(sampler, p["cfg"], p["channels"], p["last"]), p
    # what is cycled: each instantiation meets an `every` table, each guidance value each instantiation with guidance, each mask
    # table each instantiation with a mask (the plan is the same for both half dtypes)
    assert {(p["cfg"], p["channels"]) for p in plan} == set(fe.INSTANTIATIONS)
    assert {(p["guidance"], p["channels"]) for p in plan if p["cfg"]} == {(g, ch) for g in fe.GUIDANCES for ch in (9, 4)}
    assert {(p["mask"], p["cfg"]) for p in plan if p["channels"] == 4} == {(m, cfg) for m in fe.MASKS for cfg in (True, False)}
    for p in plan:   # no run hides its `every` operand behind the mask
        if p["channels"] == 4:
            assert p["mask"] != ("inside" if p["every"] in ("img_latent", "noise0") else "outside"), p


# ---- the reference's outputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_nan_cap_and_edges_reached_over_the_crossing(sampler, dtype_name):
    worst, per = measured(sampler, dtype_name)
    print(sampler, dtype_name, "largest NaN share of an output tensor", worst)
    assert worst <= NAN_CAP, (sampler, dtype_name, worst)
    flags, numel, subnormal = set(), 0, 0
    for every, m in per.items():
        share = 100.0 * m["subnormal"] / m["numel"]
        print(sampler, dtype_name, every, "subnormal share of x in percent", round(share, 3), sorted(m["flags"]))
        assert share >= SUBNORMAL_FLOOR[sampler, dtype_name][every], (sampler, dtype_name, every, share)
        flags |= m["flags"]
        numel, subnormal = numel + m["numel"], subnormal + m["subnormal"]
    assert flags == {"+0", "-0", "+inf", "-inf"}, (sampler, dtype_name, flags)
    assert subnormal >= 0.01 * numel, (sampler, dtype_name, subnormal / numel)   # over the finite tables: at least 1 %


@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_nan_cap_of_the_narrower_tables(sampler):
    """The every-pattern mask, the float32 table and the first latents.  (The table of one non-finite operand at a time is under
    no cap: three fifths of that operand are infinite or NaN by construction; there the GPU test also asserts that the
    step's NaN is absent under an all-outside mask.)"""
    k, last = fe.coeff_sets(sampler)[0][1:]
    for dtype_name in HALF:
        c = fe.case(sampler, table(dtype_name, "s"), k, last, 7.3, True, 4, fe.every_mask(getattr(torch, dtype_name)))
        for name, v in fe.reference_step(c).items():
            assert v is None or float(v.isnan().float().mean()) <= NAN_CAP, (dtype_name, "every-pattern mask", name)
    ops, hl, wl = fe.float32_case_table(True)
    assert (hl * wl) % 4 == 0 and 4 * hl * wl >= 63 * 63 + (1 << 20)
    for name, v in fe.reference_step(fe.case(sampler, ops, k, last, 7.3, True, 9, None, hl, wl)).items():
        assert v is None or float(v.isnan().float().mean()) <= NAN_CAP, ("float32", name)
    for dtype_name in DTYPES:
        for every in fe.INIT_OPERANDS[:1 if dtype_name == "float32" else 2]:
            il, noise = fe.init_inputs(getattr(torch, dtype_name), every)
            for t0 in fe.init_timesteps(sampler):
                for name, v in zip(("x", "state"), fe.reference_init(sampler, il, noise, t0)):
                    share = float(v.isnan().float().mean())
                    assert share <= NAN_CAP, (dtype_name, every, t0, name, share)


# ---- the select ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_a_mask_and_its_complement_put_every_element_on_both_sides(sampler, dtype_name):
    dtype = getattr(torch, dtype_name)
    p = dict(every="s", k=fe.coeff_sets(sampler)[0][1], last=False, guidance=7.3, cfg=True, channels=4)
    x = {name: run(sampler, dtype_name, p, mask=name)["x"] for name in fe.MASKS}
    inside = fe.mask_pattern(fe.HL, fe.WL).view(1, 1, fe.HL, fe.WL).expand_as(x["inside"])
    assert int(inside[0, 0].sum()) * 2 == fe.HL * fe.WL
    for name, pattern in (("pattern", inside), ("complement", ~inside)):
        assert same_bits(x[name], torch.where(pattern, x["inside"], x["outside"])), name
    # the two sides differ where it matters: in most elements the step's value is not the kept one
    differ = (bits(x["inside"]) != bits(x["outside"]))
    assert float(differ.float().mean()) > 0.9
    # which mask values are which side: -0 is outside; a subnormal, a negative and a NaN mask are inside
    vin, vout = fe.mask_values(dtype)
    sub = torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps
    assert raw(vout).tolist() == [0, -32768] and bool((vout == 0).all())
    assert float(vin[3]) == sub and float(vin[4]) == -sub and float(vin[1]) == -1 and bool(vin[6].isnan()) and bool(vin[5].isinf())
    m = masks(dtype_name)["pattern"].expand_as(x["pattern"])
    got = bits(x["pattern"])
    for value in list(vin) + list(vout):
        at = (bits(m) == bits(value.reshape(1))) & differ
        side = x["outside"] if float(value) == 0 else x["inside"]
        assert int(at.sum()) > 1000 and torch.equal(got[at], bits(side)[at]), (sampler, dtype_name, float(value))


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_the_plans_are_what_they_are_named_for(sampler):
    sets = {name: (k, last) for name, k, last in fe.coeff_sets(sampler)}
    acp = oracle.alphas_cumprod()
    assert [last for _, last in sets.values()] == [False, True, True, False, True, False, False]
    k, last = sets["1 only"]
    assert oracle.timesteps(sampler, 1) == [999] and last
    if sampler == "euler":   # a final step: sigma_next = 0, so the next input's scale is 1 and the kept value has no noise
        assert k[1] == 1.0 and k[2] == 0.0 and k[0] == -oracle.sigma(acp, 999)
    else:                    # a_next = 1
        assert k[4] == 1.0 and k[5] == 0.0
    ts = oracle.timesteps(sampler, 50)
    assert len(ts) == 50 and ts[49] == min(ts) == fe.init_timesteps(sampler)[2]
    assert sets["50 last"][0] == oracle.coeffs(sampler, acp, ts, 49)
    if sampler == "lcm":     # the smallest origin timestep, and the longest plan
        assert ts[49] == oracle.TRAIN_STEPS // oracle.LCM_ORIGIN_STEPS - 1 == 19
        with pytest.raises(ValueError):
            oracle.timesteps(sampler, 51)
    sliced = oracle.timesteps(sampler, 4, strength=0.6)
    assert sliced == oracle.timesteps(sampler, 4)[1:] and sets["4 at strength 0.6"][0] == oracle.coeffs(sampler, acp, sliced, 0)
    for name, (k, _) in sets.items():   # what a plan gives is positive but Euler's k0; the synthetic set is not
        signs = [v < 0 for v in k]
        assert signs == ({"euler": [False, False, True], "lcm": [False, False, True, True, True, False]}[sampler] if name == "synthetic"
                         else {"euler": [True, False, False], "lcm": [False] * 6}[sampler]), name


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_the_synthetic_set_gives_a_negative_zero_no_plan_set_gives(sampler, dtype_name):
    """On the signed-zero table, without guidance (e = u): an element whose x is -0.0 under the synthetic coefficients and
    under no plan's, from the step (9 channels) and from the kept value (4 channels, outside the mask everywhere; there beside
    the plan sets that are no last step: a last step keeps img_latent itself, its sign with it)."""
    dtype = getattr(torch, dtype_name)
    ops = fe.signed_zero_table(dtype)
    assert len({tuple(raw(ops[n])[j].item() for n in fe.OPERANDS) for j in range(64)}) == 64
    outside = fe.mask_tables(dtype, 4, 4)["outside"]
    for channels in (9, 4):
        neg = {}
        for name, k, last in fe.coeff_sets(sampler):
            x = fe.reference_step(fe.case(sampler, ops, k, last, 0.0, False, channels, outside if channels == 4 else None, 4, 4))["x"]
            assert bool((x == 0).all())
            neg[name] = fe.is_negative_zero(x)
        lasts = {name for name, _, last in fe.coeff_sets(sampler) if last and channels == 4}
        plans = torch.stack([v for name, v in neg.items() if name != "synthetic" and name not in lasts]).any(0)
        assert bool(plans.any()) and bool((neg["synthetic"] & ~plans).any()), (sampler, dtype_name, channels)
