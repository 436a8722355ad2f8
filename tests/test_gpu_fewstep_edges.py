"""The few-step sampler kernels (cs_fewstep.hip: k_inpaint_fewstep_init, k_inpaint_fewstep_step) on the inputs their workload and
tests/test_gpu_fewstep.py never give them: every float16 / bfloat16 bit pattern in each operand against special values in the
others, masks that are -0, subnormal, negative, infinite and NaN, the coefficients of 1-step and 50-step plans and a synthetic
negative set, negative and zero guidance, signed zeros, one non-finite operand at a time, float32 specials and random bit patterns.

Every comparison is bit for bit (tools/fewstep_cases.same_bits: a NaN equals a NaN of any payload) against CPU torch running the
specification, tools/fewstep_oracle.py, through tools/fewstep_edge_inputs.py; tests/test_fewstep_edges_surface.py holds that
side to its conditions.  No tolerance and no value is left out."""
import functools
import itertools

import pytest
import torch

import fewstep_edge_inputs as fe
import fewstep_oracle as oracle
from comfystereo_amd import engine, inpaint_runner as ir
from fewstep_cases import bits, same_bits
from test_gpu_fewstep import GUARD, SENTINEL, Buffers

pytestmark = pytest.mark.gpu
HALF = ("float16", "bfloat16")
DTYPES = ("float32",) + HALF


def eq(got, want, what):
    if same_bits(got, want):
        return
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    bad = (bits(got).reshape(-1) != bits(want).reshape(-1)).nonzero().reshape(-1)
    at = int(bad[0])
    raise AssertionError((what, "elements that differ:", bad.numel(), "the first at", at, "got", float(got.reshape(-1)[at]), "want",
                          float(want.reshape(-1)[at])))


class Run(Buffers):
    """One engine.fewstep_step call on a case of tools/fewstep_edge_inputs.case, every tensor between guard words (Buffers), and
    every output the kernel writes against the reference."""

    def check(self, what, want=None):
        c, t = self.c, self.t
        want = fe.reference_step(c) if want is None else want
        eq(t["x"][:1, :4], want["x"], (what, "x, first half"))
        if c["cfg"]:
            eq(t["x"][1:, :4], want["x"], (what, "x, second half"))
        if c["sampler"] == "euler":
            eq(t["state"], want["state"], (what, "state"))
        if c["last"]:
            eq(t["decode_in"], want["decode_in"], (what, "decode_in"))
        if c["channels"] == 9:
            eq(t["x"][:, 4:], self.x0[:, 4:], (what, "channels 4..8 were touched"))
        for name in ("noise_pred", "step_noise", "img_latent", "noise0", "mask_l"):
            if name in t:
                eq(t[name], self.given[name], (what, name, "was written"))
        for name, (flat, off, count) in self.flat.items():
            assert bool((flat[:GUARD + off] == -SENTINEL).all()) and bool((flat[GUARD + off + count:] == -SENTINEL).all()), (what, name, "guard words")
        return want

    def outputs(self):
        return {name: self.t[name] for name in ("x", "state", "decode_in") if name in self.t}


@functools.lru_cache(maxsize=12)
def table(dtype_name, every):
    return fe.table(getattr(torch, dtype_name), every)


@functools.lru_cache(maxsize=None)
def masks(dtype_name, hl=fe.HL, wl=fe.WL):
    return fe.mask_tables(getattr(torch, dtype_name), hl, wl)


def sets(sampler):
    return {name: (k, last) for name, k, last in fe.coeff_sets(sampler)}


# ---- a. every half input of the step: sampler x dtype x `every` operand x coefficient set -------------------------------------------
CROSSING = [(s, d, e) for s in fe.SAMPLERS for d in HALF for e in fe.OPERANDS if any(p["every"] == e for p in fe.sweep_plan(s))]


@pytest.mark.parametrize("sampler, dtype_name, every", CROSSING)
def test_step_on_every_half_input(sampler, dtype_name, every):
    """Every bit pattern in one operand against 16 specials in each other one, under every coefficient set that reads the
    operand; guidance, mask table and instantiation cycle over the product (fewstep_edge_inputs.sweep_plan)."""
    for p in fe.sweep_plan(sampler):
        if p["every"] != every:
            continue
        mask = masks(dtype_name)[p["mask"]] if p["channels"] == 4 else None
        c = fe.case(sampler, table(dtype_name, every), p["k"], p["last"], p["guidance"], p["cfg"], p["channels"], mask)
        Run(c).run().check((sampler, dtype_name, every, p["set"], p["cfg"], p["channels"], p["guidance"], p["mask"]))


# ---- b. signed zeros -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_step_on_signed_zeros(sampler, dtype_name):
    """Every assignment of +0 / -0 to the operands under every coefficient set, guidance value and instantiation, inside and
    outside the mask, on both access paths."""
    dtype = getattr(torch, dtype_name)
    for hl, wl in ((4, 4), (1, 17)):   # 16 bytes at a time, one element at a time
        ops = fe.signed_zero_table(dtype, 4 * hl * wl)
        for (name, k, last), guidance, (cfg, channels) in itertools.product(fe.coeff_sets(sampler), fe.GUIDANCES, fe.INSTANTIATIONS):
            if not cfg and guidance != fe.GUIDANCES[0]:   # without guidance the scale is not read: once
                continue
            for mask in ("pattern", "complement") if channels == 4 else (None,):
                c = fe.case(sampler, ops, k, last, guidance, cfg, channels, masks(dtype_name, hl, wl)[mask] if mask else None, hl, wl)
                Run(c).run().check((sampler, dtype_name, name, guidance, cfg, channels, mask, hl, wl))


# ---- c. one non-finite operand at a time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_step_with_one_nonfinite_operand(sampler, dtype_name):
    """inf, -inf, NaN and the largest finite values in one operand against the finite table.  Outside the mask everywhere, a NaN
    of the step is not in the output: the select moves the kept value, nothing is multiplied by the mask."""
    dtype = getattr(torch, dtype_name)
    hl, wl = 256, 320
    k, last = sets(sampler)["4 first"]
    m = masks(dtype_name, hl, wl)
    for operand, ops in fe.nonfinite_tables(dtype, fe.live(sampler, True, 4, last)):
        assert ops[operand].numel() == 4 * hl * wl
        what = (sampler, dtype_name, "non-finite", operand)
        Run(fe.case(sampler, ops, k, last, 7.3, True, 4, m["pattern"], hl, wl)).run().check(what + ("pattern",))
        if operand in ("img_latent", "noise0"):
            continue
        inside = fe.reference_step(fe.case(sampler, ops, k, last, 7.3, True, 4, m["inside"], hl, wl))["x"]
        assert float(inside.isnan().float().mean()) > 0.19, what   # the step's result: a fifth of the operand is NaN
        run = Run(fe.case(sampler, ops, k, last, 7.3, True, 4, m["outside"], hl, wl)).run()
        run.check(what + ("outside",))
        assert not bool(run.t["x"].isnan().any()) and (sampler != "euler" or not bool(run.t["state"].isnan().any())), what


# ---- d. a mask of every bit pattern --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_step_under_a_mask_of_every_bit_pattern(sampler, dtype_name):
    """mask_l != 0 on all 65 536 patterns: the two zeros keep, everything else -- subnormals, negatives, NaNs -- steps."""
    mask = fe.every_mask(getattr(torch, dtype_name))
    for (name, cfg), every in zip((("4 first", True), ("4 last", False)), ("s", "img_latent")):
        k, last = sets(sampler)[name]
        c = fe.case(sampler, table(dtype_name, every), k, last, 7.3, cfg, 4, mask)
        want = Run(c).run().check((sampler, dtype_name, "every-pattern mask", name, cfg))
        kept = fe.reference_step(dict(c, mask_l=masks(dtype_name)["outside"]))["x"]
        zero = (mask == 0).expand_as(kept)
        assert int(zero[0, 0].sum()) == 2 * 4 and same_bits(want["x"][zero], kept[zero])


# ---- e. float32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_step_on_float32_specials_and_random_patterns(sampler):
    for wide in (True, False):
        ops, hl, wl = fe.float32_case_table(wide)
        assert (hl * wl) % 8 == 0 if wide else (hl * wl) % 2 == 1
        m = masks("float32", hl, wl)
        for j, (name, k, last) in enumerate(fe.coeff_sets(sampler)[:None if wide else 2]):
            cfg, channels = fe.INSTANTIATIONS[j % 4]
            mask = fe.MASKS[j % 2] if channels == 4 else None
            c = fe.case(sampler, ops, k, last, 7.3, cfg, channels, m[mask] if mask else None, hl, wl)
            Run(c).run().check((sampler, "float32", name, cfg, channels, mask, "16-byte" if wide else "one-element"))


# ---- f. the first latents ------------------------------------------------------------------------------------------------------------
class Init:
    """One engine.fewstep_latent_init call on flat il and noise of 4 * hl * wl elements, everything it may write pre-filled."""

    def __init__(self, sampler, il, noise, t0, cfg, channels, hl, wl):
        dtype, shape = il.dtype, (1, 4, hl, wl)
        self.sampler, self.cfg, self.channels = sampler, cfg, channels
        self.given = (il.view(shape), None if noise is None else noise.view(shape))
        self.want = fe.reference_init(sampler, self.given[0], self.given[1], t0)
        self.prep = torch.full((2, 9, hl, wl), SENTINEL, dtype=dtype)
        self.prep[:, 4] = fe.mask_from(fe.mask_pattern(hl, wl), dtype)[0]
        self.prep_d = self.prep.cuda()
        rows = 2 if cfg else 1
        self.x = self.prep_d[:rows] if channels == 9 else torch.full((rows, 4, hl, wl), SENTINEL, dtype=dtype, device="cuda")
        self.state = torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
        self.mask_l = torch.full((1, 1, hl, wl), SENTINEL, dtype=dtype, device="cuda") if channels == 4 else None
        self.inputs = (self.given[0].cuda(), None if noise is None else self.given[1].cuda())
        acp = oracle.alphas_cumprod()
        coeffs = None if noise is None else ir.euler_init_coeffs(acp, t0) if sampler == "euler" else ir.add_noise_coeffs(acp, t0, dtype)
        got = engine.fewstep_latent_init(self.inputs[0], self.inputs[1], coeffs, self.x, sampler, cfg, state=self.state,
                                         prep=self.prep_d if channels == 4 else None, mask_l=self.mask_l)
        assert got is self.x
        torch.cuda.synchronize()

    def check(self, what):
        want_x, want_state = self.want
        eq(self.x[:1, :4], want_x, (what, "x, first half"))
        if self.cfg:
            eq(self.x[1:, :4], want_x, (what, "x, second half"))
        eq(self.state, want_state, (what, "state"))
        if self.channels == 4:   # the mask as it stands in channel 4, NaN, -0 and subnormals included; prep is read only
            eq(self.mask_l, self.prep[:1, 4:5], (what, "mask_l"))
            eq(self.prep_d, self.prep, (what, "prep was written"))
        else:
            eq(self.prep_d[:, 4:], self.prep[:, 4:], (what, "channels 4..8 were touched"))
            if not self.cfg:
                eq(self.prep_d[1:], self.prep[1:], (what, "the second half was touched"))
        for got, given in zip(self.inputs, self.given):
            if given is not None:
                eq(got, given, (what, "an input was written"))


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_first_latents_on_every_input(sampler, dtype_name):
    """The image's latents and the noise each through every half value against the specials of the other (float32: specials
    crossed and random bit patterns, on both access paths), at the timesteps 999, 499 and 19, and without noise."""
    dtype = getattr(torch, dtype_name)
    count = itertools.count()
    for every in fe.INIT_OPERANDS[:1 if dtype_name == "float32" else 2]:
        il, noise = fe.init_inputs(dtype, every)
        layouts = [fe.layout(il.numel(), True), fe.layout(il.numel(), False)] if dtype_name == "float32" else [(fe.HL, fe.WL)]
        for hl, wl in layouts:
            a, b = fe.fit(il, 4 * hl * wl), fe.fit(noise, 4 * hl * wl)
            for t0 in fe.init_timesteps(sampler) + (None,):
                cfg, channels = fe.INSTANTIATIONS[next(count) % 4]
                Init(sampler, a, None if t0 is None else b, t0, cfg, channels, hl, wl).check((sampler, dtype_name, every, t0, cfg, channels, hl, wl))


def test_first_latents_take_one_dtype():
    """The dtype pairs the engine accepts are the equal ones: the image's latents, the noise and x share the model's dtype."""
    for a, b in itertools.permutations(DTYPES, 2):
        il = torch.zeros((1, 4, 8, 8), dtype=getattr(torch, a), device="cuda")
        other = torch.zeros((1, 4, 8, 8), dtype=getattr(torch, b), device="cuda")
        for kwargs in (dict(noise=other, x=torch.zeros_like(il)), dict(noise=torch.zeros_like(il), x=other)):
            with pytest.raises((TypeError, ValueError), match="dtype"):
                engine.fewstep_latent_init(il, kwargs["noise"], (1.0, 1.0), kwargs["x"], "lcm", False, state=torch.zeros_like(kwargs["x"]))


# ---- g. x one element off the 16-byte grid at a shape that allows 16-byte accesses ----------------------------------------------------
@pytest.mark.parametrize("dtype_name", HALF)
@pytest.mark.parametrize("sampler", fe.SAMPLERS)
def test_the_narrow_kernel_gives_the_wide_ones_bits(sampler, dtype_name):
    k, last = sets(sampler)["4 last"]   # (a last step: decode_in is written too)
    c = fe.case(sampler, table(dtype_name, "s"), k, last, 7.3, True, 4, masks(dtype_name)["pattern"])
    wide = Run(c).run()
    want = wide.check((sampler, dtype_name, "aligned"))
    narrow = Run(c, shift="x").run()
    assert narrow.t["x"].data_ptr() % 16 != 0 and wide.t["x"].data_ptr() % 16 == 0
    narrow.check((sampler, dtype_name, "x one element in"), want)
    for name, got in narrow.outputs().items():
        eq(got.cpu(), wide.outputs()[name].cpu(), (sampler, dtype_name, name, "narrow against wide"))
