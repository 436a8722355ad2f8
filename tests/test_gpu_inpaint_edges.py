"""The inpainting-loop kernels (cs_inpaintloop.hip: k_inpaint_image_prep, k_inpaint_latent_init, k_inpaint_plms_step) on the inputs
their workload and tests/test_gpu_inpaint_runner.py never give them: every float16 / bfloat16 bit pattern against special values,
signed zeros through every product, non-finite predictions, float32 specials and random bit patterns, all nine dtype pairs of the
latent initialisation, all 256 codes under both mask states, and pointers that forbid the 16-byte path at a shape that allows it.

Every comparison is bit for bit (a NaN equals a NaN of any payload) against CPU torch running the stock expressions
(tools/inpaint_edge_inputs.py; tests/test_inpaint_edges_surface.py holds that side to its conditions).  No tolerance and no value is
left out."""
import functools

import pytest
import torch

import inpaint_edge_inputs as ei
import inpaintrun_stock as stock
from comfystereo_amd import engine, inpaint_runner as ir
from test_gpu_stream_edges import same_bits

pytestmark = pytest.mark.gpu
HALF = ("float16", "bfloat16")
DTYPES = ("float32",) + HALF
PAIRS = [(m, t) for m in DTYPES for t in DTYPES]
SENTINEL = 7.0
ACP = ir.scaled_linear_alphas_cumprod()


def eq(got, want, what):
    ok, bad = same_bits(got.reshape(want.shape), want)
    assert ok, (what, "elements that differ:", bad)


def untouched(t, what):
    assert bool((t == SENTINEL).all()), (what, "written")


def coeffs_for(kind, num_steps, step_index, dtype):
    """What InpaintLoop hands the kernel for this kind at the timestep of `step_index` in a run of `num_steps`."""
    t = ir.plms_timesteps(num_steps)[step_index]
    return ir.plms_coeffs(ACP, ACP[0], ei.KIND_COUNTER[kind], t, 1000 // num_steps, dtype)


def layout(numel, wide):
    """(hl, wl) with 4 * hl * wl >= numel: a multiple of 8 elements per plane for the 16-byte path, an odd count for the other."""
    hwl = -(-numel // 4)
    if wide:
        return 8, -(-hwl // 8)
    return 1, hwl + 1 - hwl % 2


class Step:
    """One engine.plms_step call on flat CPU operands of 4 * hl * wl elements, everything it may write pre-filled."""

    def __init__(self, kind, ops, guidance, coeffs, hl, wl, place=None):
        place = place or (lambda name, t: t)
        shape = (1, 4, hl, wl)
        dtype = ops["u"].dtype
        self.kind, self.ops = kind, ops

        def full():
            return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")

        self.noise_pred = place("noise_pred", torch.cat([ops["u"], ops["t"]]).view(2, 4, hl, wl).cuda())
        x = torch.full((2, 9, hl, wl), SENTINEL, dtype=dtype, device="cuda")
        if kind != "second":   # second takes the sample from cur_sample: x keeps the sentinel
            x[0, :4] = ops["sample"].view(4, hl, wl).cuda()
        self.x = place("x", x)
        self.history = [place(name, ops[name].view(shape).cuda()) for name in ("e1", "e2", "e3")[:ei.NEEDS[kind]]]
        self.e_out = None if kind == "second" else place("e_out", full())
        self.cur_sample = place("cur_sample", full() if kind == "first" else ops["sample"].view(shape).cuda()) if kind in ("first", "second") else None
        self.decode_in = place("decode_in", full())
        assert engine.plms_step(self.noise_pred, self.x, kind, guidance, coeffs, e_out=self.e_out, history=self.history,
                                cur_sample=self.cur_sample, decode_in=self.decode_in) is self.x
        torch.cuda.synchronize()

    def outputs(self):
        out = {"x": self.x, "decode_in": self.decode_in}
        if self.e_out is not None:
            out["e_out"] = self.e_out
        if self.cur_sample is not None:
            out["cur_sample"] = self.cur_sample
        return out

    def check(self, want, what, classes=False):
        prev, e, dec = want
        pairs = [("x uncond half", self.x[0, :4], prev), ("x cond half", self.x[1, :4], prev), ("decode_in", self.decode_in, dec)]
        if self.kind != "second":
            pairs.append(("e_out", self.e_out, e))
        if self.cur_sample is not None:   # first writes the sample there, second only reads it
            pairs.append(("cur_sample", self.cur_sample, self.ops["sample"]))
        for name, got, w in pairs:
            if classes:
                cg, cw = ei.class_of(got).reshape(-1), ei.class_of(w).reshape(-1)
                assert torch.equal(cg, cw), (what, name, "class (finite, +inf, -inf, NaN) differs at", int((cg != cw).sum()))
            eq(got, w, (what, name))
        for name, got in zip(("e1", "e2", "e3"), self.history):
            eq(got, self.ops[name], (what, name, "read only"))
        eq(self.noise_pred, torch.cat([self.ops["u"], self.ops["t"]]), (what, "noise_pred", "read only"))
        untouched(self.x[:, 4:], (what, "channels 4..8"))


@functools.lru_cache(maxsize=4)
def table(dtype_name, every):
    return ei.table(getattr(torch, dtype_name), every)


# ---- a. every half input of the step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", ["sample", "t"])
@pytest.mark.parametrize("kind", ei.KINDS)
@pytest.mark.parametrize("dtype_name", HALF)
def test_step_on_every_half_input(dtype_name, kind, every):
    """Every bit pattern in the sample (and, second table, in the conditional prediction: the guidance product, the combination's
    constants and da * m / denom then meet every value) against 16 specials in each other operand, on both paths."""
    dtype = getattr(torch, dtype_name)
    ops = table(dtype_name, every)
    narrow = 4 * 513 * 513
    ops_narrow = {name: ei.fit(v, narrow) for name, v in ops.items()}   # the tail: the table's head again
    for guidance in ei.GUIDANCES:
        for name, num_steps, index in ei.coeff_sets(kind):
            want = ei.reference_step(kind, ops, guidance, num_steps, index)
            coeffs = coeffs_for(kind, num_steps, index, dtype)
            what = (dtype_name, kind, every, guidance, name)
            Step(kind, ops, guidance, coeffs, 512, 512).check(want, what + ("16-byte path",))
            Step(kind, ops_narrow, guidance, coeffs, 513, 513).check([ei.fit(w, narrow) for w in want], what + ("one-element path",))


# ---- b. one non-finite operand at a time ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ei.KINDS)
@pytest.mark.parametrize("dtype_name", HALF)
def test_step_with_one_nonfinite_operand(dtype_name, kind):
    dtype = getattr(torch, dtype_name)
    full, bad = table(dtype_name, "sample"), ei.nonfinite_specials(dtype)
    n = 1 << 16
    # per value a slice that holds every sample once and all 16 rows of specials: 17 is odd, so 17 j runs through every residue
    idx = torch.cat([(torch.arange(n) * 17 + 4099 * k) % (16 * n) for k in range(len(bad))])
    base = {name: v[idx].contiguous() for name, v in full.items()}
    hl, wl = 256, 320
    assert 4 * hl * wl == idx.numel()
    coeffs = coeffs_for(kind, 6, ei.KIND_COUNTER[kind], dtype)
    for operand in ("sample", "u", "t") + ("e1", "e2", "e3")[:ei.NEEDS[kind]]:
        ops = dict(base)
        ops[operand] = bad.repeat_interleave(n)
        want = ei.reference_step(kind, ops, 7.3, 6, ei.KIND_COUNTER[kind])
        Step(kind, ops, 7.3, coeffs, hl, wl).check(want, (dtype_name, kind, "non-finite", operand), classes=True)


# ---- c. signed zeros ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ei.KINDS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_step_on_signed_zeros(dtype_name, kind):
    dtype = getattr(torch, dtype_name)
    for hl, wl, path in ((4, 4, "16-byte path"), (1, 17, "one-element path")):
        ops = ei.signed_zero_table(dtype, 4 * hl * wl)
        for guidance in ei.GUIDANCES:
            for name, num_steps, index in ei.coeff_sets(kind):
                want = ei.reference_step(kind, ops, guidance, num_steps, index)
                Step(kind, ops, guidance, coeffs_for(kind, num_steps, index, dtype), hl, wl).check(want, (dtype_name, kind, guidance, name, path))


class LatentInit:
    """One engine.inpaint_latent_init call on flat CPU inputs of 4 * hl * wl elements."""

    def __init__(self, mean_img, mean_masked, noise, coeffs, dtype, hl, wl, place=None):
        place = place or (lambda name, t: t)
        shape = (1, 4, hl, wl)
        self.x = place("x", torch.full((2, 9, hl, wl), SENTINEL, dtype=dtype, device="cuda"))
        self.decode_in = place("decode_in", torch.full(shape, SENTINEL, dtype=dtype, device="cuda"))
        self.img_latent = place("img_latent", torch.full(shape, SENTINEL, dtype=dtype, device="cuda"))
        self.inputs = [place("mean_img", mean_img.view(shape).cuda()), place("mean_masked", mean_masked.view(shape).cuda()),
                       None if noise is None else place("noise", noise.view(shape).cuda())]
        self.given = [mean_img, mean_masked, noise]
        got = engine.inpaint_latent_init(self.inputs[0], self.inputs[1], self.inputs[2], coeffs, self.x, img_latent=self.img_latent,
                                         decode_in=self.decode_in)
        assert got is self.img_latent
        torch.cuda.synchronize()

    def outputs(self):
        return {"x": self.x, "decode_in": self.decode_in, "img_latent": self.img_latent}

    def check(self, want, what):
        il, ml, lat, dec = want
        for name, got, w in (("img_latent", self.img_latent, il), ("latents, uncond half", self.x[0, :4], lat), ("latents, cond half", self.x[1, :4], lat),
                             ("masked latents, uncond half", self.x[0, 5:], ml), ("masked latents, cond half", self.x[1, 5:], ml),
                             ("decode_in", self.decode_in, dec)):
            eq(got, w, (what, name))
        for got, w in zip(self.inputs, self.given):
            if w is not None:
                eq(got, w, (what, "read only"))
        untouched(self.x[:, 4], (what, "channel 4"))


@pytest.mark.parametrize("mean_name, dtype_name", PAIRS)
def test_latent_init_on_signed_zeros(mean_name, dtype_name):
    mean_dtype, dtype = getattr(torch, mean_name), getattr(torch, dtype_name)
    rows = ei.signed_zero_table(torch.float32)      # three of its columns: every sign of the two means and the noise
    coeffs = ir.add_noise_coeffs(ACP, 830, dtype)
    assert coeffs[0] > 0 and coeffs[1] > 0
    for hl, wl, path in ((1, 8, "16-byte path"), (1, 9, "one-element path")):
        a, b, nz = (ei.fit(rows[name][:8], 4 * hl * wl) for name in ("e1", "e2", "e3"))   # (the last columns: 8 rows hold every sign)
        a, b, nz = a.to(mean_dtype), b.to(mean_dtype), nz.to(dtype)
        want = ei.reference_latent_init(a, b, nz, 830, dtype)
        assert {int(v) for v in want[2].view(torch.uint8).reshape(-1, dtype.itemsize)[:, -1]} == {0, 128}    # both zeros among the latents
        LatentInit(a, b, nz, coeffs, dtype, hl, wl).check(want, (mean_name, dtype_name, path))
        LatentInit(a, b, None, None, dtype, hl, wl).check(ei.reference_latent_init(a, b, None, None, dtype), (mean_name, dtype_name, path, "no noise"))


# ---- d. float32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ei.KINDS)
def test_step_on_float32_specials_and_random_patterns(kind):
    table32 = ei.float32_table()
    numel = table32["u"].numel()
    assert numel == 63 * 63 + (1 << 20)
    for wide in (True, False):
        hl, wl = layout(numel, wide)
        ops = {name: ei.fit(v, 4 * hl * wl) for name, v in table32.items()}
        for name, num_steps, index in ei.coeff_sets(kind):
            want = ei.reference_step(kind, ops, 7.3, num_steps, index)
            Step(kind, ops, 7.3, coeffs_for(kind, num_steps, index, torch.float32), hl, wl).check(want, ("float32", kind, name, "16-byte" if wide else "one-element"))


# ---- e. the latent initialisation over its nine dtype pairs -------------------------------------------------------------------------
@pytest.mark.parametrize("mean_name, dtype_name", PAIRS)
def test_latent_init_on_every_mean(mean_name, dtype_name):
    """rnd<T>(mul_rnd<M>(mean, 0.18215)) at its edges -- subnormal products in M, means that overflow T, zeros negative in M -- and
    add_noise on finite and non-finite noise."""
    mean_dtype, dtype = getattr(torch, mean_name), getattr(torch, dtype_name)
    mean_img, mean_masked, noise = ei.latent_init_inputs(mean_dtype, dtype)
    if mean_dtype == torch.float32:
        layouts = [layout(mean_img.numel(), True), layout(mean_img.numel(), False)]
    else:
        layouts = [(512, 512), (513, 513)]
    for k, (hl, wl) in enumerate(layouts):
        assert (hl * wl) % 8 == 0 if k == 0 else (hl * wl) % 2 == 1
        a, b, nz = (ei.fit(v, 4 * hl * wl) for v in (mean_img, mean_masked, noise))
        for timestep in (999, 830, 0, None):
            want = ei.reference_latent_init(a, b, None if timestep is None else nz, timestep, dtype)
            coeffs = None if timestep is None else ir.add_noise_coeffs(ACP, timestep, dtype)
            LatentInit(a, b, None if timestep is None else nz, coeffs, dtype, hl, wl).check(want, (mean_name, dtype_name, timestep, (hl, wl)))


# ---- f. image_prep on all codes ------------------------------------------------------------------------------------------------------
def image_prep(filled, mask, dtype, latent_size, place=None):
    place = place or (lambda name, t: t)
    x = place("x", torch.full((2, 9) + tuple(latent_size), SENTINEL, dtype=dtype, device="cuda"))
    img, masked = engine.inpaint_image_prep(place("filled_u8", filled.cuda()), place("mask", mask.cuda()), x, latent_size)
    torch.cuda.synchronize()
    return {"img": img, "masked": masked, "x": x}


@pytest.mark.parametrize("h, w, path", [(16, 32, "P pixels"), (23, 23, "one pixel")])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_image_prep_on_all_codes(dtype_name, h, w, path):
    dtype = getattr(torch, dtype_name)
    assert (h * w) % 8 == (0 if path == "P pixels" else 1)
    filled, mask = ei.all_codes_frame(h, w)
    latent_size = (3, 5)
    got = image_prep(filled, mask, dtype, latent_size)
    w_img, w_masked, w_mask = stock.image_prep(filled[0], mask[0], dtype, latent_size)
    eq(got["img"], w_img, "img")
    eq(got["masked"], w_masked, "masked")
    eq(got["x"][0, 4], w_mask, "mask latent, uncond half")
    eq(got["x"][1, 4], w_mask, "mask latent, cond half")
    untouched(got["x"][:, :4], "channels 0..3")
    untouched(got["x"][:, 5:], "channels 5..8")
    # every code in every channel under both mask states; under the mask a code below 128 is -0.0, one from 128 up +0.0
    codes = filled[0].permute(2, 0, 1).reshape(3, -1).long()
    under = (mask[0].reshape(-1) != 0).expand(3, -1)
    for c in range(3):
        assert set(codes[c][under[c]].tolist()) == set(range(256)) == set(codes[c][~under[c]].tolist())
    masked, img = got["masked"][0].reshape(3, -1).cpu(), got["img"][0].reshape(3, -1).cpu()
    zeros = torch.where(codes < 128, torch.tensor(-0.0), torch.tensor(0.0)).to(dtype)
    eq(masked[under], zeros[under], "the sign of a masked pixel")
    eq(masked[~under], img[~under], "a pixel outside the mask")
    # 127 and 128 straddle zero: the two values nearest to it, of opposite signs
    by_code = img[0][:256].double()
    assert codes[0][:256].tolist() == list(range(256))
    assert by_code[127] < 0 < by_code[128]
    others = torch.cat([by_code[:127], by_code[129:]]).abs()
    assert float(others.min()) > max(-float(by_code[127]), float(by_code[128]))
    # a bool mask, and any non-zero byte, is the mask (engine.inpaint_image_prep: "non-zero: inpaint")
    for name, other in [("bool", mask.bool())] + [(v, mask // 255 * v) for v in (1, 128, 254)]:
        again = image_prep(filled, other, dtype, latent_size)
        for key in got:
            eq(again[key], got[key].cpu(), ("mask", name, key))


# ---- g. pointers that forbid the wide path at a shape that allows it ------------------------------------------------------------------
class OffByOne:
    """place(name, tensor): the tensor called `target` becomes a contiguous view that starts one element into a larger allocation
    filled with the sentinel -- its element type's alignment, never 16 bytes."""
    PAD = 8

    def __init__(self, target):
        self.target, self.buffer, self.numel = target, None, 0

    def __call__(self, name, t):
        if name != self.target:
            return t
        fill = SENTINEL if t.is_floating_point() else 7
        self.buffer = torch.full((t.numel() + 1 + self.PAD,), fill, dtype=t.dtype, device=t.device)
        self.numel = t.numel()
        view = self.buffer[1:1 + self.numel].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
        return view

    def check(self, what):
        assert self.buffer is not None, (what, "not an argument of this call")
        guards = torch.cat([self.buffer[:1], self.buffer[1 + self.numel:]])
        assert bool((guards == guards.new_tensor(7)).all()), (what, "wrote outside its view")


def compare_calls(got, want, what):
    assert got.keys() == want.keys()
    for key in want:
        eq(got[key], want[key].cpu(), (what, key))


def randn_ops(dtype, numel, seed):
    g = torch.Generator().manual_seed(seed)
    return {name: torch.randn(numel, generator=g).to(dtype) for name in ei.OPERANDS}


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_step_with_one_pointer_off_the_16_byte_grid(dtype_name):
    dtype = getattr(torch, dtype_name)
    hl, wl = 16, 24
    ops = randn_ops(dtype, 4 * hl * wl, 5)
    for kind in ("first", "second", "order4"):
        coeffs = coeffs_for(kind, 6, ei.KIND_COUNTER[kind], dtype)
        aligned = Step(kind, ops, 7.3, coeffs, hl, wl)
        want = ei.reference_step(kind, ops, 7.3, 6, ei.KIND_COUNTER[kind])
        aligned.check(want, (dtype_name, kind, "aligned"))
        names = ["noise_pred", "x", "decode_in"] + ["e1", "e2", "e3"][:ei.NEEDS[kind]]
        names += ["cur_sample"] if kind in ("first", "second") else []
        names += ["e_out"] if kind != "second" else []
        for name in names:
            place = OffByOne(name)
            step = Step(kind, ops, 7.3, coeffs, hl, wl, place)
            what = (dtype_name, kind, name, "one element in")
            step.check(want, what)
            compare_calls(step.outputs(), aligned.outputs(), what)
            place.check(what)


@pytest.mark.parametrize("mean_name, dtype_name", [("float16", "float32"), ("bfloat16", "float16"), ("float32", "bfloat16")])
def test_latent_init_with_one_pointer_off_the_16_byte_grid(mean_name, dtype_name):
    mean_dtype, dtype = getattr(torch, mean_name), getattr(torch, dtype_name)
    hl, wl = 16, 24
    g = torch.Generator().manual_seed(6)
    a, b = (torch.randn(4 * hl * wl, generator=g).to(mean_dtype) for _ in range(2))
    nz = torch.randn(4 * hl * wl, generator=g).to(dtype)
    coeffs = ir.add_noise_coeffs(ACP, 830, dtype)
    want = ei.reference_latent_init(a, b, nz, 830, dtype)
    aligned = LatentInit(a, b, nz, coeffs, dtype, hl, wl)
    aligned.check(want, (mean_name, dtype_name, "aligned"))
    for name in ("mean_img", "mean_masked", "noise", "x", "img_latent", "decode_in"):
        place = OffByOne(name)
        call = LatentInit(a, b, nz, coeffs, dtype, hl, wl, place)
        what = (mean_name, dtype_name, name, "one element in")
        call.check(want, what)
        compare_calls(call.outputs(), aligned.outputs(), what)
        place.check(what)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_image_prep_with_one_pointer_off_the_16_byte_grid(dtype_name):
    dtype = getattr(torch, dtype_name)
    filled, mask = ei.all_codes_frame(16, 40)
    aligned = image_prep(filled, mask, dtype, (2, 8))
    w_img, w_masked, w_mask = stock.image_prep(filled[0], mask[0], dtype, (2, 8))
    for name in ("filled_u8", "mask", "x"):
        place = OffByOne(name)
        got = image_prep(filled, mask, dtype, (2, 8), place)
        what = (dtype_name, name, "one element in")
        eq(got["img"], w_img, what)
        eq(got["masked"], w_masked, what)
        eq(got["x"][0, 4], w_mask, what)
        compare_calls(got, aligned, what)
        place.check(what)
