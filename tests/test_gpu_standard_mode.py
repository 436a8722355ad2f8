"""StereoDiffusion's Standard mode on the GPU: cs_latent_shift_plan, cs_latent_shift_apply and cs_decode_to_codes against the
numpy restatement (tools/standard_oracle.py), and the loop and the whole mode around the stand-in model against the reference's
own values (tests/golden/standard_mode.npz).  Everything is compared bit for bit: values are moved or are single IEEE operations.
The one tolerance is the disparity bound of the end-to-end test, half the margin the fixture asserts."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import standard_fake_model as fm
import standard_oracle as so
from comfystereo_amd import engine, stereo_utils
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_standard_surface import bits, fixture_bits, fixture_tensor, load

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (5, 7), (33, 130), (64, 64), (64, 257)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def depth(kind, b, h, w, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((b, h, w), 0.25, dtype=np.float32)
    if kind == "ramp":
        return np.broadcast_to(np.linspace(0, 1, w, dtype=np.float32) + np.float32(0.01) * np.arange(h, dtype=np.float32)[:, None],
                               (b, h, w)).copy()
    if kind == "steps":
        return (rng.integers(0, 5, (b, h, (w + 7) // 8)).repeat(8, -1)[:, :, :w] / np.float32(4)).astype(np.float32)
    return rng.integers(0, 256, (b, h, w)).astype(np.float32) / np.float32(255.0)   # 8-bit noise: many collisions


@pytest.mark.parametrize("h,w", SHAPES)
def test_plan_equals_the_restatement(h, w):
    holes = 0
    for b in (1, 3):
        for kind in ("flat", "ramp", "steps", "noise"):
            d = depth(kind, b, h, w, seed=h * w + b)
            dev = torch.from_numpy(d).cuda()
            for e in (1.0, 0.5):
                for sf in (8.0, 0.5, 150.0):
                    got = engine.latent_shift_plan(dev, sf, e).cpu().numpy()
                    want = so.plan(d, sf, e)
                    assert got.dtype == np.int32 and np.array_equal(got, want), (b, kind, e, sf, int((got != want).sum()))
                    if kind == "flat" or (sf == 0.5 and w <= 130):
                        assert np.array_equal(got, np.broadcast_to(np.arange(w, dtype=np.int32), (b, h, w)))   # everything stays put
                    holes += int((got < 0).sum())
    assert holes > 0 or w < 5


def test_plan_on_the_widest_row():
    """8192 columns, the widest row the plan takes: a reach of |trunc(scale_px)| columns, and the whole row."""
    d = depth("noise", 1, 2, 8192, seed=3)
    dev = torch.from_numpy(d).cuda()
    for sf, e in ((8.0, 1.0), (150.0, 0.5)):
        got = engine.latent_shift_plan(dev, sf, e).cpu().numpy()
        assert np.array_equal(got, so.plan(d, sf, e)), (sf, e)
    with pytest.raises(ValueError):
        engine.latent_shift_plan(torch.zeros(1, 2, 8193, device="cuda"), 8.0)


def rand_latents(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("c", [1, 4, 5])
def test_apply_equals_the_restatement(dtype, c):
    for h, w in SHAPES:
        b = 2 if h * w < 4096 else 1
        d = depth("noise", b, h, w, seed=c + h)
        src = engine.latent_shift_plan(torch.from_numpy(d).cuda(), 8.0)
        src_np = src.cpu().numpy()
        assert np.array_equal(src_np, so.plan(d, 8.0))
        lat = rand_latents((2 * b, c, h, w), dtype, 11 * c + w)
        landed = np.argwhere(src_np >= 0)
        if len(landed) >= 2:   # a landed pixel whose channel 0 is +0.0, and one where it is -0.0: both count as holes
            for (bb, r, x), zero in ((landed[0], 0.0), (landed[-1], -0.0)):
                lat[bb, 0, r, src_np[bb, r, x]] = zero
        noise = rand_latents((b, c, h, w), dtype, 5 + w)
        for with_noise in (False, True):
            cur = lat.clone().cuda()                      # left and right are the two halves of one tensor
            mask = torch.full((b, h, w), 7, dtype=torch.uint8, device="cuda")
            out = engine.latent_shift_apply(cur[:b], cur[b:], src, mask, "first", noise=noise.cuda() if with_noise else None)
            assert out.data_ptr() == cur[b:].data_ptr()
            want, want_mask = so.apply_first(bits(lat[:b]), src_np, bits(noise) if with_noise else None)
            assert np.array_equal(bits(cur[:b]), bits(lat[:b])), "left was written"
            assert np.array_equal(mask.cpu().numpy(), want_mask), (h, w, with_noise)
            assert np.array_equal(bits(cur[b:]), want), (h, w, with_noise)
            if len(landed) >= 2:
                for bb, r, x in (landed[0], landed[-1]):
                    assert want_mask[bb, r, x] == 0
            # RESHIFT on a changed left: only the pixels of the STORED mask change (a mask recomputed from the new left would
            # differ: the new left has no zeros where the old one had them, and zeros elsewhere)
            new_left = rand_latents((b, c, h, w), dtype, 99 + w)
            new_left[:, 0, :, ::3] = 0
            before = bits(cur[b:]).copy()
            cur[:b] = new_left.cuda()
            engine.latent_shift_apply(cur[:b], cur[b:], src, mask, "reshift")
            assert np.array_equal(mask.cpu().numpy(), want_mask)
            assert np.array_equal(bits(cur[b:]), so.apply_reshift(bits(new_left), before, src_np, want_mask)), (h, w, with_noise)


def all_half_patterns(dtype):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_decode_equals_the_restatement(dtype):
    name = str(dtype).split(".")[-1]
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -1.0, 1.0, 0.0, -0.0, 3.0, -3.0,
                            2.0 ** -11, 3 * 2.0 ** -11, 2.0 ** -8, 3 * 2.0 ** -8,          # x / 2 + 0.5 on a float16 / bfloat16 tie
                            -1 + 2.0 ** -10, 1 - 2.0 ** -7, 2.0 ** -24, -2.0 ** -24, 1 - 2.0 ** -24, 0.999, -0.999, 1e-30, 65504.0])
    g = torch.Generator().manual_seed(4)
    pool = torch.cat([special, torch.rand(4096, generator=g) * 3 - 1.5, (torch.arange(512) - 256) / 256.0])
    if dtype == torch.float32:
        pool = torch.cat([pool, (torch.arange(256) + 0.5) / 255 * 2 - 1, torch.arange(256) / 255.0 * 2 - 1])
    images = [pool.to(dtype)]
    if dtype != torch.float32:
        images.append(all_half_patterns(dtype))          # every value of the dtype
    for flat in images:
        for n, c, h, w in ((1, 1, 1, flat.numel()), (3, 3, 5, 7), (2, 3, 9, 33), (1, 4, 17, 3)):
            k = n * c * h * w
            x = flat[torch.arange(k) % flat.numel()].reshape(n, c, h, w).contiguous() if k != flat.numel() else flat.reshape(n, c, h, w)
            got = engine.decode_to_codes(x.cuda()).cpu().numpy()
            want = so.decode_to_codes(x.double().numpy(), name)
            assert got.shape == (n, h, w, c) and got.dtype == np.uint8
            assert np.array_equal(got, want), (name, (n, c, h, w), int((got != want).sum()))
    # torch's own arithmetic on the same values, on the CPU as the reference runs it
    x = images[-1].reshape(1, 1, 1, -1)
    ref = (x / 2 + 0.5).clamp(0, 1).float().numpy()
    ref = (np.nan_to_num(ref, nan=0.0, posinf=1.0, neginf=0.0) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(engine.decode_to_codes(x.cuda()).cpu().numpy(), ref)


@pytest.fixture(scope="module")
def golden():
    return load()


def case_inputs(z, meta, c, dev="cuda"):
    """(model, x_t twice, uncond embeddings, noise [2,4,64,64] or None) of a fixture case on the device."""
    dtype = getattr(torch, c["dtype"])
    model = fm.FakeModel(dev, dtype)
    img512 = engine.pil_resize(torch.from_numpy(z["image"]).to(dev), (512, 512))[0]
    x_t, unc = fm.fake_invert(img512, dtype, meta["steps"] if c["uncond"] else None)
    noise = None
    if c["deblur"]:
        right = fixture_tensor(z[f"{c['id']}/noise_right"], dtype).to(dev)
        noise = torch.cat([torch.zeros_like(right), right])
    return model, torch.cat([x_t, x_t]), unc, noise


def test_loop_equals_the_reference_on_every_fixture_case(golden):
    z, meta = golden
    for c in meta["cases"]:
        cid = c["id"]
        model, latent, unc, noise = case_inputs(z, meta, c)
        disp = torch.from_numpy(z[f"disp512/{c['depth']}"]).cuda()
        seen = {}
        # the caller has autograd on (the reference's node enables it for the inversion) and the UNet has a weight that
        # requires grad: the loop switches autograd off itself, like the reference's (:575)
        assert torch.is_grad_enabled() and model.unet.gain.requires_grad
        latents, mask = sdn._stereo_latents(model, ["", ""], unc, latent, disp, c["scale_factor"], c["direction"], c["deblur"],
                                            meta["steps"], meta["guidance_scale"], noise, None,
                                            on_step=lambda i, lat: seen.__setitem__(i, lat.clone()))
        assert np.array_equal(mask.cpu().numpy(), z[f"{cid}/mask"]), cid
        assert not latents.requires_grad and latents.grad_fn is None and all(not t.requires_grad for t in seen.values())
        assert np.array_equal(bits(seen[meta["shift_step"]][1:]), fixture_bits(z[f"{cid}/latents_shift_right"])), cid
        assert np.array_equal(bits(latents), fixture_bits(z[f"{cid}/latents_final"])), cid
        codes = sdn.text2stereoimage(model, ["", ""], unc, latent, disp, c["scale_factor"], c["direction"], c["deblur"],
                                     meta["steps"], meta["guidance_scale"], noise=noise)
        assert codes.dtype == torch.uint8 and codes.is_cuda and tuple(codes.shape) == (2, 512, 512, 3)
        assert torch.is_grad_enabled()   # (and the caller's setting is back)
        assert np.array_equal(codes.cpu().numpy(), z[f"{cid}/codes"]), cid
        # the decode alone, on the reference's final latents
        ref_lat = fixture_tensor(z[f"{cid}/latents_final"], getattr(torch, c["dtype"])).cuda()
        again = engine.decode_to_codes(model.vae.decode(1 / 0.18215 * ref_lat)["sample"])
        assert np.array_equal(again.cpu().numpy(), z[f"{cid}/codes"]), cid


def test_whole_mode_equals_the_reference(golden):
    z, meta = golden
    image = torch.from_numpy(z["image"])
    for c in meta["cases"]:
        cid = c["id"]
        dep = torch.from_numpy(z[f"depth/{c['depth']}"])
        # the device's disparity at the latents' size against the reference's: within half the margin the fixture asserts
        depth_u8 = engine.pil_resize(dep.cuda(), (512, 512), gray=True)
        disp = sdn._norm_depth(depth_u8[..., 0].float() / 255.0)
        lat_disp = sdn._disparity_to_latent(disp, (64, 64)).cpu().numpy()
        scale_px = abs(c["scale_factor"] / 100.0 * 64)
        err = float(np.abs(lat_disp.astype(np.float64) - z[f"disp_latent/{c['depth']}"].astype(np.float64)).max()) * scale_px
        print(cid, "max |disp_gpu - disp_fixture| * |scale_px| =", err, "fixture margin", meta["margin"])
        assert meta["margin"] >= 1e-3
        assert err < 5e-4, (f"{cid}: the device's bicubic disparity differs from the reference's by {err} shift pixels, half the "
                            "fixture's margin of 1e-3 or more: a truncated shift could flip")
        model, _, _, noise = case_inputs(z, meta, c)
        dtype = getattr(torch, c["dtype"])
        invert = lambda u8, dtype=dtype, c=c: fm.fake_invert(u8, dtype, meta["steps"] if c["uncond"] else None)
        stereo, left, right = sdn.generate_stereo_standard(image, dep, c["scale_factor"], c["direction"], c["deblur"], meta["steps"],
                                                           meta["guidance_scale"], model, invert, noise=noise)
        want = z[f"{cid}/stereo"]
        w = want.shape[2] // 2
        assert not stereo.is_cuda and stereo.dtype == torch.float32     # host inputs: host results
        assert np.array_equal(stereo.numpy(), want), cid
        assert np.array_equal(left.numpy(), want[:, :, :w]) and np.array_equal(right.numpy(), want[:, :, w:]), cid
    # device inputs stay on the device; more than one frame: the first one only
    stereo2, _, _ = sdn.generate_stereo_standard(torch.cat([image, image * 0]).cuda(), torch.cat([dep, dep]).cuda(), c["scale_factor"],
                                                 c["direction"], c["deblur"], meta["steps"], meta["guidance_scale"], model, invert,
                                                 noise=noise)
    assert stereo2.is_cuda and np.array_equal(stereo2.cpu().numpy(), want)


def test_weights_that_require_grad_without_the_loops_no_grad_are_refused(golden):
    """What the loop's no_grad is for: one iteration called with autograd on hands the shift a tensor that requires grad."""
    z, meta = golden
    c = meta["cases"][0]
    model, latent, unc, noise = case_inputs(z, meta, c)
    loop = sdn._StandardLoop(model, torch.from_numpy(z[f"disp_latent/{c['depth']}"]).cuda(), 8.0, False, 2, 3.0, None)
    emb = model.text_encoder(torch.zeros(2, 77))[0]
    ctx = torch.cat([emb, emb])
    with torch.enable_grad():
        assert loop.step(0, 0, latent.cuda(), ctx).requires_grad
        with pytest.raises(ValueError, match="requires grad"):
            loop.step(1, 0, latent.cuda(), ctx)


def test_deblur_noise_drawn_from_a_generator(golden):
    z, meta = golden
    c = next(c for c in meta["cases"] if c["deblur"] and c["dtype"] == "float32")
    model, latent, unc, _ = case_inputs(z, meta, c)
    disp = torch.from_numpy(z[f"disp512/{c['depth']}"]).cuda()
    args = (model, ["", ""], unc, latent, disp, c["scale_factor"], c["direction"], True, meta["steps"], meta["guidance_scale"])
    for where in ("cuda", "cpu"):   # the noise is drawn on the generator's device
        runs = []
        for _ in range(2):
            seen = {}
            g = torch.Generator(device=where).manual_seed(77)
            latents, mask = sdn._stereo_latents(*args, None, g, on_step=lambda i, lat: seen.__setitem__(i, lat.clone()))
            runs.append((latents, mask, seen[meta["shift_step"]]))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        g = torch.Generator(device=where).manual_seed(77)
        drawn = torch.randn((2, 4, 64, 64), generator=g, device=where, dtype=torch.float32).cuda()
        mask, shifted = runs[0][1], runs[0][2]
        holes = (mask == 0)[:, None].expand(-1, 4, -1, -1)
        assert 0 < int(holes.sum()) < holes.numel()
        assert torch.equal(shifted[1:][holes], drawn[1:][holes])
        assert not torch.equal(shifted[1:][~holes], drawn[1:][~holes])
        assert np.array_equal(mask.cpu().numpy(), z[f"{c['id']}/mask"])
    # no latent and a CPU generator, the reference's kind: it serves init_latent and the noise in turn
    g = torch.Generator().manual_seed(5)
    codes = sdn.text2stereoimage(model, ["", ""], unc, None, disp, c["scale_factor"], c["direction"], True, meta["steps"],
                                 meta["guidance_scale"], generator=g)
    g = torch.Generator().manual_seed(5)
    want_latent = torch.randn((1, 4, 64, 64), generator=g)
    want_noise = torch.randn((2, 4, 64, 64), generator=g)
    again = sdn.text2stereoimage(model, ["", ""], unc, torch.cat([want_latent, want_latent]), disp, c["scale_factor"], c["direction"],
                                 True, meta["steps"], meta["guidance_scale"], noise=want_noise)
    assert torch.equal(codes, again)


def test_a_step_with_a_reshift_is_captured_in_a_graph_and_replayed(golden):
    with torch.no_grad():   # (the loop's own setting: an iteration is called directly here)
        _graph_capture_body(golden)


def _graph_capture_body(golden):
    z, meta = golden
    c = next(c for c in meta["cases"] if c["deblur"] and c["dtype"] == "float32")
    model, latent, unc, noise = case_inputs(z, meta, c)
    disp_latent = torch.from_numpy(z[f"disp_latent/{c['depth']}"]).cuda()
    loop = sdn._StandardLoop(model, disp_latent, c["scale_factor"], True, meta["steps"], meta["guidance_scale"], noise[1:].contiguous())
    emb = model.text_encoder(torch.zeros(2, 77))[0]
    model.scheduler.set_timesteps(meta["steps"])
    ts = model.scheduler.timesteps
    ctx = [torch.cat([unc[i].expand(*emb.shape), emb]) for i in range(meta["steps"])]
    latents = latent.cuda()
    i_re = meta["reshifts"][0]
    for i in range(i_re):
        latents = loop.step(i, ts[i], latents, ctx[i])
    assert loop.shifted
    static_in = latents.clone()
    eager = loop.step(i_re, ts[i_re], static_in, ctx[i_re]).clone()
    other_in = static_in.flip(-1).contiguous()
    eager_other = loop.step(i_re, ts[i_re], other_in, ctx[i_re]).clone()
    assert not torch.equal(eager, eager_other)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop.step(i_re, ts[i_re], static_in, ctx[i_re])   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # a wait for the host inside the step would make the capture fail
        out = loop.step(i_re, ts[i_re], static_in, ctx[i_re])
    graph.replay()
    assert torch.equal(out, eager)
    static_in.copy_(other_in)
    graph.replay()
    assert torch.equal(out, eager_other)


class DummyAttention(nn.Module):
    """A module the hook walk takes for an attention layer (its class name says so and it has children); the stand-in UNet never
    calls it."""
    scale, heads = 0.5, 1

    def __init__(self):
        super().__init__()
        self.to_q = nn.Linear(4, 4)


def test_hooks_are_removed_after_a_call_and_after_a_failing_call(golden):
    z, meta = golden
    c = meta["cases"][0]
    model, latent, unc, noise = case_inputs(z, meta, c)
    model.unet.down_blocks = nn.ModuleList([DummyAttention()])
    model.unet.mid_block = DummyAttention()
    layers = [model.unet.down_blocks[0], model.unet.mid_block]
    disp = torch.from_numpy(z[f"disp512/{c['depth']}"]).cuda()
    args = (model, ["", ""], unc, latent, disp, c["scale_factor"], c["direction"], c["deblur"], meta["steps"], meta["guidance_scale"])
    hooked = []
    real_step = model.scheduler.step

    def step(*a, **k):
        hooked.append(all("forward" in m.__dict__ for m in layers))
        return real_step(*a, **k)

    model.scheduler.step = step
    sdn.text2stereoimage(*args)
    assert hooked and all(hooked)                                 # installed during the loop ...
    assert all("forward" not in m.__dict__ and not hasattr(m, stereo_utils._SAVED_FORWARD) for m in layers)   # ... and gone after it
    model.unet.fail_at = model.unet.count + 3
    with pytest.raises(RuntimeError, match="told to fail"):
        sdn.text2stereoimage(*args)
    assert all("forward" not in m.__dict__ and not hasattr(m, stereo_utils._SAVED_FORWARD) for m in layers)
