"""The few-step samplers of Fast mode on the GPU (cs_inpaint_fewstep_init, cs_inpaint_fewstep_step,
comfystereo_amd.inpaint_runner.FewStepLoop): every output bit for bit the CPU evaluation of tools/fewstep_oracle.py, the
specification, and the whole loop bit for bit tools/fewstep_stock.py on the CPU.  "Bit for bit" as in the PLMS sweeps: a NaN
equals a NaN of any payload (tools/fewstep_cases.bits).  The stand-in model's own arithmetic is treated as
tests/test_gpu_inpaint_runner.py treats it: built so that it rounds alike on both devices, and trusted to."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from comfystereo_amd import engine, inpaint_runner as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fewstep_cases as cases   # noqa: E402
import fewstep_fake_model as ffm   # noqa: E402
import fewstep_oracle as oracle   # noqa: E402
import fewstep_stock as stock   # noqa: E402
import inpaint_fake_model as fm   # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = list(cases.DTYPES)
SAMPLERS = ["euler", "lcm"]
SENTINEL = 5.0
GUARD = 64   # elements on either side of a buffer: a multiple of 16 bytes in every dtype
same_bits = cases.same_bits


class Buffers:
    """The device tensors of one step, each inside a flat allocation with guard words on both sides.  shift: the name of the one
    tensor that starts one element off the 16-byte grid."""

    def __init__(self, c, shift=None):
        self.c, self.flat, n, dtype = c, {}, c["n"], c["dtype"]
        rows, shape = (2 * n if c["cfg"] else n), (n, 4, c["hl"], c["wl"])
        x = torch.full((rows, c["channels"], c["hl"], c["wl"]), SENTINEL, dtype=dtype)
        if c["sampler"] == "lcm":   # the sample is read from the first half; the second half is only written
            x[:n, :4] = c["s"]
        self.x0 = x
        sentinel = torch.full(shape, SENTINEL, dtype=dtype)
        given = dict(noise_pred=c["pred"], x=x, state=c["s"] if c["sampler"] == "euler" else None, step_noise=c["z"],
                     img_latent=c["img_latent"] if c["channels"] == 4 else None, noise0=c["noise0"] if c["channels"] == 4 and not c["last"] else None,
                     mask_l=c["mask_l"] if c["channels"] == 4 else None, decode_in=sentinel if c["last"] else None)
        self.given = {k: v for k, v in given.items() if v is not None}
        self.t = {name: self.place(name, t, 1 if name == shift else 0) for name, t in self.given.items()}

    def place(self, name, t, off):
        flat = torch.full((t.numel() + 2 * GUARD + off,), -SENTINEL, dtype=t.dtype, device="cuda")
        view = flat[GUARD + off:GUARD + off + t.numel()].view(t.shape)
        view.copy_(t)
        self.flat[name] = (flat, off, t.numel())
        assert view.data_ptr() % 16 == (off * t.element_size()) % 16
        return view

    def run(self):
        c, t = self.c, self.t
        out = engine.fewstep_step(t["noise_pred"], t["x"], c["sampler"], c["guidance"], c["k"], c["cfg"], last=c["last"], state=t.get("state"),
                                  step_noise=t.get("step_noise"), img_latent=t.get("img_latent"), noise0=t.get("noise0"),
                                  mask_l=t.get("mask_l"), decode_in=t.get("decode_in"))
        assert out is t["x"]
        torch.cuda.synchronize()
        return self

    def check(self, what):
        c, t, n = self.c, self.t, self.c["n"]
        want = cases.want(c)
        assert same_bits(t["x"][:n, :4], want["x"]), (what, "x, first half")
        if c["cfg"]:
            assert same_bits(t["x"][n:, :4], want["x"]), (what, "x, second half")
        if c["channels"] == 9:
            assert same_bits(t["x"][:, 4:], self.x0[:, 4:]), (what, "channels 4..8 were touched")
        if c["sampler"] == "euler":
            assert same_bits(t["state"], want["state"]), (what, "state")
        if c["last"]:
            assert same_bits(t["decode_in"], want["decode_in"]), (what, "decode_in")
        for name in ("noise_pred", "step_noise", "img_latent", "noise0", "mask_l"):   # read only
            if name in t:
                assert same_bits(t[name], self.given[name]), (what, name, "was written")
        for name, (flat, off, count) in self.flat.items():
            assert bool((flat[:GUARD + off] == -SENTINEL).all()) and bool((flat[GUARD + off + count:] == -SENTINEL).all()), (what, name, "guard words")
        return want


# ---- the kernel grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_every_instantiation_at_every_step_position_on_both_access_paths(sampler, dtype_name):
    seed = 0
    for cfg, channels, pos, n, (hl, wl) in itertools.product((True, False), (9, 4), cases.POSITIONS, (1, 3), ((8, 8), (5, 7))):
        c = cases.make(sampler, dtype_name, cfg, channels, pos, n, hl, wl, seed=seed)
        Buffers(c).run().check((sampler, dtype_name, cfg, channels, pos, n, hl, wl))
        seed += 1


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_each_tensor_in_turn_one_element_off_the_16_byte_grid(sampler, dtype_name):
    for channels, pos in ((4, "middle"), (4, "last"), (9, "first")):
        c = cases.make(sampler, dtype_name, True, channels, pos, 2, 8, 8, seed=40)
        names = list(Buffers(c).given)
        assert {"noise_pred", "x"} <= set(names) and ("mask_l" in names) == (channels == 4)
        for name in names:
            Buffers(c, shift=name).run().check((sampler, dtype_name, channels, pos, "shifted", name))


@pytest.mark.parametrize("dtype_name, hl, wl", [("float16", 297, 297), ("float32", 592, 592)])
def test_a_second_pass_of_the_grid_stride_loop(dtype_name, hl, wl):
    """More items than the 4096 x 256 threads of the largest grid, at the smallest such shapes: 3 x 4 x 297 x 297 elements one
    at a time (an odd plane), 3 x 4 x 592 x 592 float32 elements four at a time."""
    n, width = 3, 16 // cases.DTYPES[dtype_name].itemsize if (hl * wl) % 8 == 0 else 1
    assert n * 4 * hl * wl // width > 4096 * 256 and n * 4 * (hl - 1) * (wl - 1) // width < 1.01 * 4096 * 256
    c = cases.make("lcm", dtype_name, True, 4, "middle", n, hl, wl, seed=41)
    Buffers(c).run().check((dtype_name, hl, wl))
    c = cases.make("euler", dtype_name, False, 9, "last", n, hl, wl, seed=42)
    Buffers(c).run().check((dtype_name, hl, wl))


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_guidance_scales_special_values_and_masks(sampler, dtype_name):
    """Guidance 7.5, 1.5, 1 and 0 through the guided instantiation; +-0, +-inf, NaN, the largest finite value and the smallest
    subnormal in the sample and the prediction; masks of all 0, all 1 and mixed.  Under a zero mask a NaN of the step's result is
    not in the output: the select moves the kept value."""
    for guidance, mask_kind, pos, (hl, wl) in itertools.product((7.5, 1.5, 1.0, 0.0), ("zero", "one", "mixed"), ("first", "last"), ((8, 8), (5, 7))):
        for channels, cfg in ((4, True), (9, True), (4, False)):
            c = cases.make(sampler, dtype_name, cfg, channels, pos, 2, hl, wl, seed=50, guidance=guidance, mask_kind=mask_kind, special=True)
            what = (sampler, dtype_name, guidance, mask_kind, pos, hl, wl, channels, cfg)
            b = Buffers(c).run()
            want = b.check(what)
            at = c["nan_at"]
            moved = channels == 4 and mask_kind != "one"
            assert bool(torch.isnan(want["x"][at])) != moved, what
            if moved:
                got = b.t["x"][:2, :4][at].cpu()
                assert bool(torch.isfinite(got)) and same_bits(got, want["x"][at]), what


# ---- the first latents -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_the_first_latents(sampler, dtype_name):
    dtype, acp = cases.DTYPES[dtype_name], oracle.alphas_cumprod()
    g = torch.Generator().manual_seed(60)
    for cfg, channels, n, (hl, wl), t0 in itertools.product((True, False), (9, 4), (1, 3), ((8, 8), (5, 7)), (999, 499)):
        il, nz = torch.randn((n, 4, hl, wl), generator=g).to(dtype), torch.randn((n, 4, hl, wl), generator=g).to(dtype)
        prep = torch.full((2 * n, 9, hl, wl), SENTINEL, dtype=dtype)
        prep[:, 4] = (torch.rand((n, hl, wl), generator=g) < 0.5).to(dtype).repeat(2, 1, 1)
        rows = 2 * n if cfg else n
        prep_d = prep.cuda()
        x = prep_d[:rows] if channels == 9 else torch.full((rows, 4, hl, wl), SENTINEL, dtype=dtype, device="cuda")
        state = torch.full((n, 4, hl, wl), SENTINEL, dtype=dtype, device="cuda")
        mask_l = torch.full((n, 1, hl, wl), SENTINEL, dtype=dtype, device="cuda") if channels == 4 else None
        coeffs = ir.euler_init_coeffs(acp, t0) if sampler == "euler" else ir.add_noise_coeffs(acp, t0, dtype)
        engine.fewstep_latent_init(il.cuda(), nz.cuda(), coeffs, x, sampler, cfg, state=state, prep=prep_d if channels == 4 else None, mask_l=mask_l)
        want_x, want_state = oracle.first_latents(sampler, il, nz, acp, t0)
        what = (sampler, dtype_name, cfg, channels, n, hl, wl, t0)
        assert same_bits(x[:n, :4], want_x) and (not cfg or same_bits(x[n:, :4], want_x)), what
        assert same_bits(state, want_x if want_state is None else want_state), what
        if channels == 4:
            assert same_bits(mask_l, prep[:n, 4:5]) and same_bits(prep_d, prep), what
        else:
            assert same_bits(prep_d[:, 4:], prep[:, 4:]) and (cfg or same_bits(prep_d[n:], prep[n:])), what
    # no timestep left: the latents are the image's
    x = torch.full((2, 4, 5, 7), SENTINEL, dtype=dtype, device="cuda")
    mask_l = torch.empty((2, 1, 5, 7), dtype=dtype, device="cuda")
    il = torch.randn((2, 4, 5, 7), generator=g).to(dtype)
    engine.fewstep_latent_init(il.cuda(), None, None, x, sampler, False, state=torch.empty_like(x), prep=torch.zeros((4, 9, 5, 7), dtype=dtype, device="cuda"), mask_l=mask_l)
    assert same_bits(x, il) and bool((mask_l == 0).all())


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
def frames(kind):
    if kind == "two 64 x 64":
        fs = [fm.seeded_frame(71, 64, 64, "mixed"), fm.seeded_frame(72, 64, 64, "mixed")]
    else:
        fs = [fm.seeded_frame(73, 40, 56, "mixed")]
    return torch.stack([f for f, _ in fs]), torch.stack([m for _, m in fs])


def generators(n, seed):
    return [torch.Generator().manual_seed(seed + k) for k in range(n)]


@pytest.mark.parametrize("channels", [9, 4])
@pytest.mark.parametrize("guidance", [7.5, 0.0])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_the_loop_equals_the_stock_composition_on_the_cpu(sampler, dtype_name, guidance, channels):
    dtype = cases.DTYPES[dtype_name]
    for kind, strength in itertools.product(("two 64 x 64", "one 40 x 56"), (1.0, 0.6)):
        filled, mask = frames(kind)
        n = filled.shape[0]
        want = stock.run(ffm.FewStepModel("cpu", dtype, in_channels=channels), sampler, "a photo", filled, mask, 4, guidance, strength, generators(n, 80))
        model = ffm.FewStepModel("cuda", dtype, in_channels=channels)
        model.unet.record = True
        runner = ir.InpaintRunner(*model.parts(), sampler=sampler)
        codes = runner.run("a photo", filled.cuda(), mask.cuda(), generators(n, 80), 4, guidance, strength)
        loop, what = runner.loop, (sampler, dtype_name, guidance, channels, kind, strength)
        rows = 2 * n if guidance > 1 else n
        assert isinstance(loop, ir.FewStepLoop) and loop.timesteps == oracle.timesteps(sampler, 4, strength) and loop.cfg == (guidance > 1), what
        assert len(model.unet.inputs) == len(want["unet_in"]) == len(loop.timesteps) == (4 if strength == 1.0 else 3), what
        assert tuple(loop.x.shape) == (rows, channels) + ((8, 8) if n == 2 else (5, 7)), what
        assert all(p == loop.x.data_ptr() for p in model.unet.pointers), what   # one persistent input
        for i, (x, wx) in enumerate(zip(model.unet.inputs, want["unet_in"])):
            assert same_bits(x, wx), (what, "UNet input", i)
        assert same_bits(loop.x[:n, :4], want["latents"]) and same_bits(loop.decode_in, want["decode_in"]), what
        assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), want["codes"]), what
        assert model.vae.encoded == (2 if channels == 9 else 1) and model.vae.decoded == 1


class FixedUNet(torch.nn.Module):
    """Returns one fixed prediction without a kernel of its own: what runs between two of its calls is the loop's."""

    def __init__(self, pred, in_channels):
        super().__init__()
        self.pred, self.in_channels = torch.nn.Parameter(pred, requires_grad=False), in_channels

    def forward(self, x, t, context=None):
        return self.pred


def fixed_loop(sampler, channels, cfg, n=2, steps=4, dtype=torch.float16):
    g = torch.Generator().manual_seed(90)
    rows = 2 * n if cfg else n
    pred = (0.1 * torch.randn((rows, 4, 8, 8), generator=g)).to(dtype).cuda()
    runner = ir.InpaintRunner(FixedUNet(pred, channels), None, None, None, sampler=sampler)
    lat = lambda: torch.randn((n, 4, 8, 8), generator=g).to(dtype).cuda()   # noqa: E731
    x = torch.randn((rows, channels, 8, 8), generator=g).to(dtype).cuda()
    loop = ir.FewStepLoop(runner, x, None, ir.fewstep_timesteps(sampler, steps), 7.5 if cfg else 0.0, sampler, cfg, noise0=lat(),
                          step_noise=torch.stack([lat() for _ in range(steps - 1)]))
    loop.img_latent = lat()
    if loop.state is not None:
        loop.state.copy_(lat())
    if loop.mask_l is not None:
        loop.mask_l.copy_((torch.rand((n, 1, 8, 8), generator=g) < 0.5).to(dtype))
    return loop


@pytest.mark.parametrize("sampler, channels, cfg", [("euler", 4, False), ("lcm", 4, False), ("euler", 9, True), ("lcm", 9, True)])
def test_one_launch_and_no_torch_kernel_between_two_unet_calls(sampler, channels, cfg):
    """The profiler's device kernels over a 4-step loop whose UNet launches nothing, as tools/inpaintrun_bench.py counts them:
    four, all of them k_inpaint_fewstep_step."""
    from torch.profiler import ProfilerActivity, profile
    loop = fixed_loop(sampler, channels, cfg)
    for i in range(4):
        loop.step(i)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(4):
            loop.step(i)
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()]
    assert len(names) == 4 and all("k_inpaint_fewstep_step" in name for name in names), names


@pytest.mark.parametrize("sampler, channels, cfg", [("euler", 4, False), ("lcm", 4, True), ("lcm", 9, False)])
def test_a_captured_step_replays_to_the_eager_bits(sampler, channels, cfg):
    loop = fixed_loop(sampler, channels, cfg)
    loop.step(0)
    torch.cuda.synchronize()
    keep = lambda: (loop.x.clone(), None if loop.state is None else loop.state.clone())   # noqa: E731

    def put(saved):
        loop.x.copy_(saved[0])
        if loop.state is not None:
            loop.state.copy_(saved[1])

    before = keep()
    loop.step(1)
    eager = keep()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop.step(1)   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    put(before)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop.step(1)
    put(before)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(loop.x, eager[0]) and not same_bits(loop.x, before[0])
    assert loop.state is None or same_bits(loop.state, eager[1])


# ---- PLMS is untouched -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [dict(), dict(sampler="plms")])
def test_plms_gives_the_bits_its_fixture_pins(kwargs):
    """InpaintRunner without a sampler, and with sampler="plms": the reference's CPU run of tests/golden/inpaint_runner.npz."""
    with np.load(os.path.join(ROOT, "tests", "golden", "inpaint_runner.npz")) as z:
        meta = json.loads(str(z["meta"]))
        golden = {name: z[name] for name in z.files}

    def as_tensor(a, dtype_name):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.view(torch.bfloat16) if dtype_name == "bfloat16" else t

    assert meta["cases"]
    for c in meta["cases"]:
        cid = c["id"]
        model = fm.FakeInpaintModel("cuda", getattr(torch, c["dtype"]))
        model.unet.record = True
        runner = ir.InpaintRunner(*model.parts(), **kwargs)
        codes = runner(c["prompt"], torch.from_numpy(golden[f"{cid}/filled"]).cuda(), torch.from_numpy(golden[f"{cid}/mask"]).cuda(),
                       num_inference_steps=c["steps"], guidance_scale=c["guidance"], strength=c["strength"],
                       generator=torch.Generator().manual_seed(c["seed"]))
        assert isinstance(runner.loop, ir.InpaintLoop) and runner.loop.timesteps == c["timesteps"], cid
        if c["timesteps"]:
            want_in = as_tensor(golden[f"{cid}/unet_in"], c["dtype"])
            for i, x in enumerate(model.unet.inputs):
                assert fm_same_bits(x, want_in[i]), (cid, "UNet input", i)
        assert fm_same_bits(runner.loop.decode_in, as_tensor(golden[f"{cid}/decode_in"], c["dtype"])), cid
        assert torch.equal(codes.cpu(), torch.from_numpy(golden[f"{cid}/codes"])), cid


def fm_same_bits(a, b):
    """Strictly bit for bit, as tests/test_gpu_inpaint_runner.py compares."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))
