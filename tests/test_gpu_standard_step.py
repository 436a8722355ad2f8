"""cs_standard_step -- guidance, the DDIM step and the latent shift in one launch -- against the pinned two-launch composition
(engine.ddim_step on the two halves, then engine.latent_shift_apply, then the copy), bit for bit; the Standard loop on it; the
StereoDiffusion node end to end on stand-in models (gpu)."""
import itertools
import types

import pytest
import torch
import torch.nn as nn

import inpaint_fake_model as ifm
import standard_fake_model as fm
from comfystereo_amd import engine, schedulers, stereo_utils
from comfystereo_amd import stereodiffusion_nodes as sdn

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
SHAPES = [(1, 4, 3, 5), (1, 4, 64, 64), (1, 4, 2, 65), (2, 5, 3, 257), (1, 1, 2, 1030), (1, 4, 1, 8192)]
GUIDANCES = (7.5, 1.0, 0.0)
GUARD = 64   # elements around every tensor the kernel writes or reads; GUARD + 1: one element off the 16-byte grid


def bits(t):
    return t.contiguous().view(INT_OF.get(t.dtype, t.dtype))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def step_coeffs(dtype):
    """The first, a middle and the last step of a 10-step schedule, and a set no schedule gives (c3, c4 < 0: the only way to a
    result of -0.0, since c3^2 + c4^2 = 1 keeps one product from underflowing and a -0.0 numerator needs e = +0.0)."""
    s = schedulers.DDIMScheduler()
    s.set_timesteps(10)
    return [s.coeffs(t, dtype) for t in (900, 500, 0)] + [(0.5, 0.5, -0.5, -0.5)]


def specials(dtype):
    """Triples (sample, uncond, cond) over +-0, subnormals, +-1, +-0.5, NaN and +-inf."""
    tiny = torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps
    v = [0.0, -0.0, tiny, -tiny, 3 * tiny, -3 * tiny, 1.0, -1.0, 0.5, -0.5, float("nan"), float("inf"), float("-inf")]
    return torch.tensor(list(itertools.product(v, v, v)), dtype=torch.float64).to(dtype)


def guarded(numel, dtype, off, fill):
    """-> (buffer, view of `numel` elements starting `off` elements in), the buffer filled with `fill`."""
    buf = torch.full((numel + 2 * off + 8,), fill, dtype=dtype, device="cuda")
    return buf, buf[off:off + numel]


def make_inputs(shape, dtype, seed, off=GUARD):
    b, c, h, w = shape
    n = 4 * b * c * h * w
    g = torch.Generator().manual_seed(seed)
    xbuf, x = guarded(n, dtype, off, 77.0)
    pbuf, pred = guarded(n, dtype, off, -55.0)
    x, pred = x.view(4 * b, c, h, w), pred.view(4 * b, c, h, w)
    x.copy_(torch.randn((4 * b, c, h, w), generator=g).to(dtype))           # the second half is NOT a copy: it is never read
    pred.copy_(torch.randn((4 * b, c, h, w), generator=g).to(dtype))
    sp = specials(dtype)[:h * w].cuda()
    k = sp.shape[0]
    x[0, 0].view(-1)[:k] = sp[:, 0]            # channel 0 of the left view: what the mask is made of
    pred[0, 0].view(-1)[:k] = sp[:, 1]
    pred[2 * b, 0].view(-1)[:k] = sp[:, 2]
    nbuf, noise = guarded(b * c * h * w, dtype, off, 11.0)
    noise = noise.view(b, c, h, w)
    noise.copy_(torch.randn((b, c, h, w), generator=g).to(dtype))
    mbuf, mask = guarded(b * h * w, torch.uint8, GUARD, 9)
    mask = mask.view(b, h, w)
    mask.copy_((torch.rand((b, h, w), generator=g) < 0.5).to(torch.uint8))
    return dict(x=x, xbuf=xbuf, pred=pred, pbuf=pbuf, noise=noise, nbuf=nbuf, mask=mask, mbuf=mbuf)


def tables(b, h, w):
    """The src_col tables: the reversed and the constant ones fail when a row's stores overtake its gathers."""
    cols = torch.arange(w, dtype=torch.int32, device="cuda").expand(b, h, w)
    ramp = (torch.arange(w, dtype=torch.float32, device="cuda") / max(w - 1, 1)).expand(b, h, w).contiguous()
    step = (torch.arange(w, device="cuda") >= w // 2).float().expand(b, h, w).contiguous()
    return {
        "identity": cols.contiguous(), "holes": torch.full_like(cols, -1), "reversed": (w - 1 - cols).contiguous(),
        "first_column": torch.zeros_like(cols), "last_column": torch.full_like(cols, w - 1),
        "plan_ramp": engine.latent_shift_plan(ramp, 9.0), "plan_step": engine.latent_shift_plan(step, -7.0),
    }


OPS = [("none", False), ("first", False), ("first", True), ("reshift", False)]


def composition(t, guidance, coeffs, op, src_col, with_noise):
    """-> (x [4B,C,h,w], mask) of the pinned kernels."""
    b2 = t["x"].shape[0] // 2
    b = b2 // 2
    new = engine.ddim_step(t["x"][:b2].clone(), t["pred"][:b2].contiguous(), t["pred"][b2:].contiguous(), guidance, coeffs)
    mask = t["mask"].clone()
    if op != "none":
        engine.latent_shift_apply(new[:b], new[b:], src_col, mask, op, noise=t["noise"].clone() if with_noise else None)
    return torch.cat([new, new]), mask


def run_and_compare(t, guidance, coeffs, op, src_col, with_noise, label):
    want_x, want_mask = composition(t, guidance, coeffs, op, src_col, with_noise)
    before = {k: t[k].clone() for k in ("xbuf", "pbuf", "nbuf", "mbuf")}
    x0 = t["x"].clone()
    out = engine.standard_step(t["pred"], t["x"], guidance, coeffs, op, None if op == "none" else src_col,
                               None if op == "none" else t["mask"], t["noise"] if with_noise else None)
    assert out is t["x"]
    b2 = t["x"].shape[0] // 2
    assert same_bits(t["x"][:b2], t["x"][b2:]), label            # both halves
    assert same_bits(t["x"], want_x), label
    assert torch.equal(t["mask"], want_mask), label
    if op != "first":
        assert torch.equal(t["mask"], before["mbuf"][GUARD:GUARD + t["mask"].numel()].view(t["mask"].shape)), label
    # nothing outside the tensors, and no input, is written
    n, off = t["x"].numel(), t["x"].storage_offset()
    assert same_bits(t["xbuf"][:off], before["xbuf"][:off]) and same_bits(t["xbuf"][off + n:], before["xbuf"][off + n:]), label
    assert same_bits(t["pbuf"], before["pbuf"]) and same_bits(t["nbuf"], before["nbuf"]), label
    m = t["mask"].numel()
    assert torch.equal(t["mbuf"][:GUARD], before["mbuf"][:GUARD]) and torch.equal(t["mbuf"][GUARD + m:], before["mbuf"][GUARD + m:]), label
    t["x"].copy_(x0)
    t["mask"].copy_(before["mbuf"][GUARD:GUARD + m].view(t["mask"].shape))
    return want_x


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_step_equals_the_two_launch_composition(shape, dtype):
    """Every op with every table at every shape and dtype.  Guidance and the coefficient sets are cycled over that product, not
    crossed with it (each of the twelve pairs meets some shift op at every shape); the full guidance x coefficients product runs
    on the plain step.  The shift moves values and never computes, so a pair that is right on one table is right on the others."""
    b, c, h, w = shape
    t = make_inputs(shape, dtype, seed=sum(shape))
    coeffs = step_coeffs(dtype)
    tabs = tables(b, h, w)
    zero_signs = set()
    for idx, ((op, with_noise), (tname, tab)) in enumerate(itertools.product(OPS, tabs.items())):
        guidance, cf = GUIDANCES[idx % 3], coeffs[(idx // 3) % 4]
        want = run_and_compare(t, guidance, cf, op, tab, with_noise, (op, with_noise, tname, guidance, cf))
        left0 = bits(want[0, 0]).view(-1)
        zero_signs |= {"+0"} if bool((left0 == 0).any()) else set()
        zero_signs |= {"-0"} if bool((left0 == torch.iinfo(left0.dtype).min).any()) else set()
    # every guidance with every coefficient set, on the plain step
    for guidance, cf in itertools.product(GUIDANCES, coeffs):
        run_and_compare(t, guidance, cf, "none", None, False, ("none", guidance, cf))
    if h * w >= 2197:   # the whole table of specials fits: channel 0 of the new left view was +0.0 and -0.0 somewhere
        assert zero_signs == {"+0", "-0"}


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_both_access_paths_at_the_workload_shape(dtype):
    """[1,4,64,64] allows 16-byte accesses; one element off the 16-byte grid the same shape takes the scalar path."""
    shape = (1, 4, 64, 64)
    coeffs = step_coeffs(dtype)
    tabs = tables(1, 64, 64)
    results = []
    for off in (GUARD, GUARD + 1):
        t = make_inputs(shape, dtype, seed=5, off=off)
        assert (t["x"].data_ptr() % 16 == 0) == (off == GUARD) and (t["pred"].data_ptr() % 16 == 0) == (off == GUARD)
        got = []
        for idx, ((op, with_noise), tname) in enumerate(itertools.product(OPS, ("reversed", "plan_ramp", "first_column"))):
            got.append(run_and_compare(t, GUIDANCES[idx % 3], coeffs[idx % 3], op, tabs[tname], with_noise, (off, op, tname)))
        results.append(got)
    assert all(same_bits(a, b) for a, b in zip(*results))


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
class NotOurs:
    """A DDIMScheduler behind a wrapper: isinstance fails, so the loop takes the unfused diffusion_step path over the same step."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)


def loop_inputs(dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    latent = torch.randn((1, 4, 64, 64), generator=g).to(dtype).cuda()
    noise = torch.randn((2, 4, 64, 64), generator=g).to(dtype).cuda()
    disp = (torch.arange(512, dtype=torch.float32) // 64 / 7).expand(1, 512, 512).contiguous().cuda()
    return torch.cat([latent, latent]), noise, disp


def run_loop(dtype, fused, direction, deblur, steps, uncond):
    model = fm.FakeModel("cuda", dtype)
    model.scheduler = schedulers.DDIMScheduler() if fused else NotOurs(schedulers.DDIMScheduler())
    model.unet.record = True
    latent, noise, disp = loop_inputs(dtype)
    unc = fm.fake_uncond_embeddings(steps, "cuda", dtype) if uncond else None
    seen = {}
    latents, mask = sdn._stereo_latents(model, ["", ""], unc, latent, disp, 8.0, direction, deblur, steps, 3.0, noise if deblur else None,
                                        None, on_step=lambda i, lat: seen.__setitem__(i, lat.clone()))
    return model, latents.clone(), mask, seen


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("direction,deblur,steps,uncond", [("uni", False, 5, False), ("bi", True, 10, True), ("uni", True, 10, False)])
def test_fused_loop_equals_the_unfused_loop(dtype, direction, deblur, steps, uncond):
    model, latents, mask, seen = run_loop(dtype, True, direction, deblur, steps, uncond)
    model_u, latents_u, mask_u, seen_u = run_loop(dtype, False, direction, deblur, steps, uncond)
    assert sorted(seen) == sorted(seen_u) == list(range(steps))
    for i in range(steps):
        assert same_bits(seen[i], seen_u[i]), i
    assert same_bits(latents, latents_u) and torch.equal(mask, mask_u) and bool(mask.any()) and not bool(mask.all())
    assert not latents.requires_grad
    # one UNet call per step, every one on the same tensor object: the persistent input [4,4,64,64]
    assert len(model.unet.calls) == steps and all(c is model.unet.calls[0] for c in model.unet.calls)
    assert tuple(model.unet.calls[0].shape) == (4, 4, 64, 64)
    assert same_bits(model.unet.calls[0][:2], model.unet.calls[0][2:])
    assert len(model_u.unet.calls) == steps and not all(c is model_u.unet.calls[0] for c in model_u.unet.calls)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_loop_equals_the_reference_on_every_fixture_case(fused):
    """tests/golden/standard_ddim.npz: the reference's own loop on the CPU under the host DDIM oracle.  The right view just after
    the first shift and after the re-shifts the file holds, the final latents, the mask and the codes, bit for bit, down both paths."""
    import json

    import numpy as np

    import make_standard_ddim_goldens as mk
    z = np.load(mk.OUT)
    meta = json.loads(str(z["meta"]))
    disp = torch.from_numpy(mk.disparity()).cuda()
    for c in meta["cases"]:
        cid, dtype = c["id"], getattr(torch, c["dtype"])
        model = fm.FakeModel("cuda", dtype)
        model.scheduler = schedulers.DDIMScheduler() if fused else NotOurs(schedulers.DDIMScheduler())
        x_t = mk.start_latent(dtype).cuda()
        unc = fm.fake_uncond_embeddings(c["steps"], "cuda", dtype) if c["uncond"] else None
        noise = mk.deblur_noise(dtype).cuda() if c["deblur"] else None
        first, _ = mk.shift_steps(c["steps"])
        seen = {}
        args = (model, ["", ""], unc, torch.cat([x_t, x_t]), disp, meta["scale_factor"], c["direction"], c["deblur"], c["steps"],
                meta["guidance_scale"], noise)
        latents, mask = sdn._stereo_latents(*args, None, on_step=lambda i, lat: seen.__setitem__(i, lat.clone()))
        assert np.array_equal(mask.cpu().numpy(), z[f"{cid}/mask"]), cid
        assert np.array_equal(bits(seen[first][1:]).cpu().numpy(), z[f"{cid}/latents_shift_right"].view(bits(latents).cpu().numpy().dtype)), cid
        kept = mk.stored_reshifts(c["dtype"], c["steps"])
        assert kept and all(f"{cid}/latents_reshift_right/{i}" in z.files for i in kept), cid
        for i in kept:   # the right view just after a re-shift
            want = z[f"{cid}/latents_reshift_right/{i}"]
            assert np.array_equal(bits(seen[i][1:]).cpu().numpy(), want.view(bits(latents).cpu().numpy().dtype)), (cid, i)
        assert np.array_equal(bits(latents).cpu().numpy(), z[f"{cid}/latents_final"].view(bits(latents).cpu().numpy().dtype)), cid
        codes = sdn.text2stereoimage(*args)
        assert np.array_equal(codes.cpu().numpy(), z[f"{cid}/codes"]), cid


def test_a_fused_step_is_captured_in_a_graph_and_replayed():
    """The shift step with deblur, on the loop's own buffers: a wait for the host or an allocation of ours would fail the capture."""
    dtype, steps = torch.float16, 10
    model = fm.FakeModel("cuda", dtype)
    model.scheduler = schedulers.DDIMScheduler()
    model.scheduler.set_timesteps(steps)
    latent, noise, disp = loop_inputs(dtype)
    disp_latent = sdn._disparity_to_latent(disp, (64, 64))
    context = torch.cat([model.text_encoder(torch.zeros((2, 77), dtype=torch.int64))[0]] * 2).contiguous()
    with torch.no_grad():
        loop = sdn._StandardLoop(model, disp_latent, 8.0, True, steps, 3.0, noise[1:].contiguous())
        loop.begin(latent, model.scheduler.timesteps)
        i = loop.shift_step
        for k in range(i):
            loop.fused_step(k, context)
        torch.cuda.synchronize()
        state = loop.x.clone()
        loop.fused_step(i, context)
        eager, eager_mask = loop.x.clone(), loop.mask.clone()
        assert bool(eager_mask.any()) and not same_bits(eager, state)

        def reset():
            loop.x.copy_(state)
            loop.mask.zero_()
            loop.shifted = False

        reset()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            loop.fused_step(i, context)   # warm-up on the side stream, as capture asks
        torch.cuda.current_stream().wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loop.fused_step(i, context)
        reset()
        graph.replay()
        torch.cuda.synchronize()
    assert same_bits(loop.x, eager) and torch.equal(loop.mask, eager_mask)


# ---- the node end to end ---------------------------------------------------------------------------------------------------------------
class ComfyDiffusion(nn.Module):
    """A fake UNet with ComfyUI's call: forward(x, timesteps, context=...) -> the noise prediction."""

    def __init__(self, inner, in_channels):
        super().__init__()
        self.inner, self.in_channels = inner, in_channels

    def forward(self, x, timesteps, context=None):
        out = self.inner(x, timesteps, encoder_hidden_states=context) if self.in_channels == 4 else self.inner(x, timesteps, context=context)
        return out["sample"] if isinstance(out, dict) else out


class ComfyVAE:
    """ComfyUI's VAE surface over a diffusers-style fake: NHWC [0,1] images on both sides."""

    def __init__(self, inner, dtype):
        self.inner, self.dtype = inner, dtype
        self.first_stage_model = nn.Linear(1, 1).to("cuda", dtype)

    def encode(self, pixels):
        x = (pixels.to("cuda", self.dtype).permute(0, 3, 1, 2) * 2.0 - 1.0).contiguous()
        return self.inner.encode(x)["latent_dist"].mean

    def decode(self, z):
        return ((self.inner.decode(z)["sample"] + 1.0) / 2.0).permute(0, 2, 3, 1)


class StandardVAE(fm.FakeVAE):
    def encode(self, x):
        lat = torch.stack([x[:, 0], x[:, 1], x[:, 2], x[:, 0] * 0.5], 1)[:, :, ::8, ::8].contiguous()
        return {"latent_dist": types.SimpleNamespace(mean=lat)}


class ComfyCLIP:
    def __init__(self, dtype, width):
        self.dtype, self.width, self.cond_stage_model = dtype, width, None

    def tokenize(self, text):
        return {"l": [[(49406, 1.0)] + [(1000 + ord(ch) % 97, 1.0) for ch in text] + [(49407, 1.0)]]}

    def encode_from_tokens(self, tokens, return_pooled=False):
        ids = torch.tensor([p[0] for p in tokens["l"][0]], dtype=torch.float32)
        g = torch.Generator().manual_seed(int(ids.sum()))
        cond = (torch.randint(-8, 9, (1, 77, self.width), generator=g).float() / 8).to("cuda", self.dtype)
        return (cond, None) if return_pooled else cond


class SD15:
    pass


def comfy_models(mode, dtype=torch.float16):
    if mode == sdn.FAST_MODE:
        fake = ifm.FakeInpaintModel("cuda", dtype)
        unet, vae, width = ComfyDiffusion(fake.unet, 9), ComfyVAE(fake.vae, dtype), ifm.WIDTH
    else:
        fake = fm.FakeModel("cuda", dtype)
        unet, vae, width = ComfyDiffusion(fake.unet, 4), ComfyVAE(StandardVAE(), dtype), fm.WIDTH
    unet = unet.to("cuda", dtype)
    model = types.SimpleNamespace(model=types.SimpleNamespace(diffusion_model=unet, model_config=SD15()))
    return model, ComfyCLIP(dtype, width), vae, fake


def frames(n, h, w, seed=6):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand((n, h, w, 3), generator=g)
    depth = ((torch.arange(w) * 4 // w).float() / 3)[None, None, :, None].expand(n, h, w, 3).contiguous()
    return image, depth


@pytest.mark.parametrize("h,w", [(17, 23), (64, 48)])
def test_node_fast_mode(h, w):
    image, depth = frames(1, h, w)
    node = sdn.StereoDiffusionNode()

    def run(seed):
        model, clip, vae, _ = comfy_models(sdn.FAST_MODE)
        return node.generate_stereo(image, depth, 8.0, "uni", False, sdn.FAST_MODE, 3.0, 4, seed, True, 0.6, model, clip, vae, "", "", "")

    stereo, left, right = run(1337)
    assert tuple(stereo.shape) == (1, h, 2 * w, 3) and stereo.dtype == torch.float32
    assert torch.equal(left, stereo[:, :, :w]) and torch.equal(right, stereo[:, :, w:])
    again = run(1337)
    assert all(torch.equal(a, b) for a, b in zip((stereo, left, right), again))
    assert not torch.equal(run(1338)[0], stereo)


@pytest.mark.parametrize("h,w", [(17, 23), (64, 48)])
@pytest.mark.parametrize("null_text", [False, True])
def test_node_standard_mode(h, w, null_text):
    image, depth = frames(1, h, w)
    node = sdn.StereoDiffusionNode()

    def run(seed):
        model, clip, vae, fake = comfy_models(sdn.STANDARD_MODE, torch.float32)
        out = node.generate_stereo(image, depth, 8.0, "bi", True, sdn.STANDARD_MODE, 3.0, 5, seed, null_text, 0.6, model, clip, vae)
        unet = model.model.diffusion_model
        assert not any(hasattr(m, stereo_utils._SAVED_FORWARD) for m in unet.modules())
        return out

    stereo, left, right = run(7)
    assert tuple(stereo.shape) == (1, h, 2 * w, 3) and stereo.dtype == torch.float32
    assert torch.equal(left, stereo[:, :, :w]) and torch.equal(right, stereo[:, :, w:])
    assert all(torch.equal(a, b) for a, b in zip((stereo, left, right), run(7)))


def test_node_removes_its_hooks_when_the_unet_raises():
    image, depth = frames(1, 17, 23)
    model, clip, vae, fake = comfy_models(sdn.STANDARD_MODE, torch.float32)
    fake.unet.fail_at = 7   # inside the Standard loop: 5 inversion calls come first
    with pytest.raises(RuntimeError, match="told to fail"):
        sdn.StereoDiffusionNode().generate_stereo(image, depth, 8.0, "uni", False, sdn.STANDARD_MODE, 3.0, 5, 7, False, 0.6, model, clip, vae)
    assert not any(hasattr(m, stereo_utils._SAVED_FORWARD) for m in model.model.diffusion_model.modules())
    assert stereo_utils._get_unet is not None
