"""Fast mode's inpainting loop on the GPU (cs_inpaint_image_prep, cs_inpaint_latent_init, cs_inpaint_plms_step,
comfystereo_amd.inpaint_runner): bit for bit the reference's CPU run recorded in tests/golden/inpaint_runner.npz, and at the
sizes the fixtures do not hold bit for bit the stock-torch composition of tools/inpaintrun_stock.py evaluated on the CPU inside the
test (tests/test_inpaint_runner_surface.py pins that composition to the fixtures)."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from comfystereo_amd import engine, inpaint_runner as ir, stereodiffusion_nodes as sdn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import inpaint_fake_model as fm   # noqa: E402
import inpaintrun_stock as stock   # noqa: E402
import plms_oracle   # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "float16", "bfloat16")

with np.load(os.path.join(ROOT, "tests", "golden", "inpaint_runner.npz")) as _z:
    META = json.loads(str(_z["meta"]))
CASE_IDS = [c["id"] for c in META["cases"]]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "inpaint_runner.npz"))


def as_tensor(a, dtype_name):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.bfloat16) if dtype_name == "bfloat16" else t


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def gpu_runner(dtype, **kwargs):
    model = fm.FakeInpaintModel("cuda", dtype, **kwargs)
    model.unet.record = True
    return model, ir.InpaintRunner(*model.parts())


def check_structure(model, loop, n):
    """One persistent input: the same pointer at every step, channels 4..8 untouched from the first step to the last, the two
    halves of channels 0..3 equal."""
    ins = model.unet.inputs
    assert len(set(model.unet.pointers)) <= 1 and all(p == loop.x.data_ptr() for p in model.unet.pointers)
    for x in ins + [loop.x]:
        assert same_bits(x[:n, :4], x[n:, :4])
        assert same_bits(x[:, 4:], (ins[0] if ins else loop.x)[:, 4:])
        assert same_bits(x[:n, 4:], x[n:, 4:])


# ---- against the goldens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_references_cpu_run_bit_for_bit(golden, cid):
    c = next(c for c in META["cases"] if c["id"] == cid)
    model, runner = gpu_runner(getattr(torch, c["dtype"]))
    filled, mask = torch.from_numpy(golden[f"{cid}/filled"]).cuda(), torch.from_numpy(golden[f"{cid}/mask"]).cuda()
    codes = runner(c["prompt"], filled, mask, num_inference_steps=c["steps"], guidance_scale=c["guidance"], strength=c["strength"],
                   generator=torch.Generator().manual_seed(c["seed"]))
    loop = runner.loop
    assert model.tokenizer.prompts == [[c["prompt"]], [""]] and model.vae.encoded == 2 and model.vae.decoded == 1
    assert loop.timesteps == c["timesteps"] and [p[0] for p in loop.plan] == c["kinds"] and model.unet.count == len(c["timesteps"])
    if c["timesteps"]:
        want_in = as_tensor(golden[f"{cid}/unet_in"], c["dtype"])
        for i, x in enumerate(model.unet.inputs):
            assert same_bits(x, want_in[i]), (cid, "UNet input", i)
        assert same_bits(torch.stack(model.unet.outputs), as_tensor(golden[f"{cid}/unet_out"], c["dtype"]))
        assert same_bits(loop.x[:1, :4], as_tensor(golden[f"{cid}/latents"], c["dtype"]))
    else:   # no step: the latents are the image's
        assert same_bits(loop.x[:1, :4], loop.img_latent)
    assert same_bits(loop.decode_in, as_tensor(golden[f"{cid}/decode_in"], c["dtype"]))
    assert codes.dtype == torch.uint8 and torch.equal(codes.cpu(), torch.from_numpy(golden[f"{cid}/codes"]))
    check_structure(model, loop, 1)


# ---- kernel edges at their smallest ------------------------------------------------------------------------------------------------
def against_stock(dtype, h, w, steps, guidance, strength, seed, mean_dtype=None, mask_kind="mixed"):
    filled, mask = fm.seeded_frame(seed, h, w, mask_kind)
    want = stock.run(fm.FakeInpaintModel("cpu", dtype, mean_dtype=mean_dtype), "a photo", filled, mask, steps, guidance, strength,
                     torch.Generator().manual_seed(seed))
    model, runner = gpu_runner(dtype, mean_dtype=mean_dtype)
    codes = runner("a photo", filled.cuda(), mask.cuda(), num_inference_steps=steps, guidance_scale=guidance, strength=strength,
                   generator=torch.Generator().manual_seed(seed))
    assert len(model.unet.inputs) == len(want["unet_in"]) > 0
    for i, (x, wx) in enumerate(zip(model.unet.inputs, want["unet_in"])):
        assert same_bits(x, wx), ("UNet input", i)
    assert same_bits(runner.loop.x[:1, :4], want["latents"]) and same_bits(runner.loop.decode_in, want["decode_in"])
    assert torch.equal(codes.cpu(), want["codes"])
    check_structure(model, runner.loop, 1)
    return runner


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_an_odd_latent_takes_the_one_element_path(dtype_name):
    """Latents 9 x 7: nothing after a channel offset is 16-byte aligned."""
    runner = against_stock(getattr(torch, dtype_name), 72, 56, 6, 7.5, 1.0, seed=7)
    assert tuple(runner.loop.x.shape) == (2, 9, 9, 7)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_an_aligned_latent_takes_the_16_byte_path(dtype_name):
    """Latents 8 x 8 (and a 64 x 64 frame: whole chunks per plane)."""
    runner = against_stock(getattr(torch, dtype_name), 64, 64, 6, 7.5, 0.6, seed=8)
    assert tuple(runner.loop.x.shape) == (2, 9, 8, 8)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_frame_that_is_no_multiple_of_the_latents(dtype_name):
    """20 x 30 under a VAE that answers 3 x 4: the mask's nearest index is F.interpolate's, evaluated on the CPU."""
    runner = against_stock(getattr(torch, dtype_name), 20, 30, 3, 7.5, 1.0, seed=9)
    assert tuple(runner.loop.x.shape) == (2, 9, 3, 4)


@pytest.mark.parametrize("model_dtype, mean_dtype", [("float16", "float32"), ("float32", "bfloat16"), ("bfloat16", "float16")])
def test_vae_means_in_another_dtype(model_dtype, mean_dtype):
    against_stock(getattr(torch, model_dtype), 16, 24, 3, 7.5, 1.0, seed=10, mean_dtype=getattr(torch, mean_dtype))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_nearest_index_of_the_mask_kernel_alone(dtype_name):
    dtype = getattr(torch, dtype_name)
    g = torch.Generator().manual_seed(3)
    for (h, w), (hl, wl) in (((37, 53), (5, 7)), ((20, 30), (3, 4)), ((9, 11), (9, 11)), ((5, 6), (11, 13)), ((64, 64), (8, 8))):
        n = 2
        filled = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        mask = (torch.rand((n, h, w), generator=g) < 0.5).to(torch.uint8) * 255
        x = torch.full((2 * n, 9, hl, wl), 5.0, dtype=dtype, device="cuda")
        img, masked = engine.inpaint_image_prep(filled.cuda(), mask.cuda(), x, (hl, wl))
        for k in range(n):
            w_img, w_masked, w_mask = stock.image_prep(filled[k], mask[k], dtype, (hl, wl))
            assert same_bits(img[k:k + 1], w_img) and same_bits(masked[k:k + 1], w_masked)
            assert same_bits(x[k:k + 1, 4:5], w_mask) and same_bits(x[n + k:n + k + 1, 4:5], w_mask)
            m01 = (mask[k] != 0).to(dtype)[None, None]
            assert same_bits(w_mask, F.interpolate(m01, size=(hl, wl), mode="nearest"))
        assert bool((x[:, :4] == 5).all()) and bool((x[:, 5:] == 5).all())   # nothing else of x is touched


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_a_second_pass_of_the_grid_stride_loop(dtype_name):
    """More elements than the 4096 x 256 threads of the largest grid, on the one-element path (odd hl * wl), through all five
    combinations; latent_init and image_prep at such a count too."""
    dtype = getattr(torch, dtype_name)
    n, hl, wl = 2, 367, 363
    assert n * 4 * hl * wl > 4096 * 256 and (hl * wl) % 2 == 1
    g = torch.Generator().manual_seed(4)
    shape = (n, 4, hl, wl)
    # latent_init
    mean_a, mean_b, noise = (torch.randn(shape, generator=g).to(dtype) for _ in range(3))
    acp = plms_oracle.PLMSOracle().alphas_cumprod
    x = torch.zeros((2 * n, 9, hl, wl), dtype=dtype, device="cuda")
    dec = torch.empty(shape, dtype=dtype, device="cuda")
    img_latent = engine.inpaint_latent_init(mean_a.cuda(), mean_b.cuda(), noise.cuda(), ir.add_noise_coeffs(acp, 830, dtype), x, decode_in=dec)
    sch = plms_oracle.PLMSOracle()
    w_il, w_ml = mean_a * 0.18215, mean_b * 0.18215
    w_lat = sch.add_noise(w_il, noise, torch.tensor([830]))
    assert same_bits(img_latent, w_il) and same_bits(x[:n, :4], w_lat) and same_bits(x[n:, :4], w_lat)
    assert same_bits(x[:n, 5:], w_ml) and same_bits(x[n:, 5:], w_ml) and same_bits(dec, w_lat / 0.18215)
    assert bool((x[:, 4] == 0).all())
    # seven steps: first, second, order2, order3, order4 and the ring's wrap
    runner = ir.InpaintRunner(*fm.FakeInpaintModel("cuda", dtype).parts())
    runner.num_inference_steps = 6
    loop = ir.InpaintLoop(runner, x, None, ir.plms_timesteps(6), 7.5)
    sch.set_timesteps(6)
    lat = w_lat
    for i, t in enumerate(sch.timesteps):
        pred = torch.randn((2 * n,) + shape[1:], generator=g).to(dtype)
        kind, reads, write, coeffs = loop.plan[i]
        engine.plms_step(pred.cuda(), x, kind, 7.5, coeffs, e_out=None if write is None else loop.history[write],
                         history=[loop.history[r] for r in reads], cur_sample=loop.cur_sample if i < 2 else None,
                         decode_in=dec if i == 6 else None)
        lat = sch.step(pred[:n] + 7.5 * (pred[n:] - pred[:n]), t, lat).prev_sample
        assert same_bits(x[:n, :4], lat) and same_bits(x[n:, :4], lat), (i, kind)
    assert same_bits(dec, lat / 0.18215) and same_bits(x[:n, 5:], w_ml) and bool((x[:, 4] == 0).all())
    # image_prep: an odd pixel count above the grid
    h, w = 1031, 1021
    filled = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8)
    mask = (torch.rand((1, h, w), generator=g) < 0.5).to(torch.uint8) * 255
    x1 = torch.zeros((2, 9, 4, 4), dtype=dtype, device="cuda")
    img, masked = engine.inpaint_image_prep(filled.cuda(), mask.cuda(), x1, (4, 4))
    w_img, w_masked, w_mask = stock.image_prep(filled[0], mask[0], dtype, (4, 4))
    assert same_bits(img, w_img) and same_bits(masked, w_masked) and same_bits(x1[:1, 4:5], w_mask)


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_run_on_two_frames_equals_two_calls(dtype_name):
    dtype = getattr(torch, dtype_name)
    frames = [fm.seeded_frame(21, 16, 24, "mixed"), fm.seeded_frame(22, 16, 24, "one")]
    filled = torch.stack([f for f, _ in frames]).cuda()
    mask = torch.stack([m for _, m in frames]).cuda()
    model, runner = gpu_runner(dtype)
    both = runner.run("a photo", filled, mask, [torch.Generator().manual_seed(31), torch.Generator().manual_seed(32)], 6, 7.5, 1.0)
    assert tuple(both.shape) == (2, 16, 24, 3) and model.unet.count == 7 and tuple(model.unet.inputs[0].shape) == (4, 9, 2, 3)
    check_structure(model, runner.loop, 2)
    x2 = runner.loop.x.clone()
    for k in range(2):
        _, single = gpu_runner(dtype)
        one = single("a photo", filled[k], mask[k].bool() if k else mask[k], 6, 7.5, 1.0, generator=torch.Generator().manual_seed(31 + k))
        assert torch.equal(one, both[k])
        assert same_bits(single.loop.x[0], x2[k]) and same_bits(single.loop.x[1], x2[2 + k])


def test_one_step_is_captured_in_a_graph_and_replayed():
    """The fake UNet and plms_step on one stream: a wait for the host or an allocation of ours inside the step would fail the capture."""
    dtype = torch.float16
    filled, mask = fm.seeded_frame(5, 64, 64, "mixed")
    model, runner = gpu_runner(dtype)
    model.unet.record = False
    loop = runner.prepare("a photo", filled[None].cuda(), mask[None].cuda(), [torch.Generator().manual_seed(5)], 6, 7.5, 1.0)
    for i in range(3):
        loop.step(i)
    torch.cuda.synchronize()
    state = (loop.x.clone(), loop.history.clone())
    eager = loop.step(3).clone()       # order3: reads two history slots, writes a third
    eager_history = loop.history.clone()
    other_x = state[0].flip(-1).contiguous()
    loop.x.copy_(other_x)
    loop.history.copy_(state[1])
    eager_other = loop.step(3).clone()
    assert not torch.equal(eager, eager_other)
    loop.x.copy_(state[0])
    loop.history.copy_(state[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loop.step(3)   # warm-up on the side stream, as capture asks
    torch.cuda.current_stream().wait_stream(side)
    loop.x.copy_(state[0])
    loop.history.copy_(state[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop.step(3)
    loop.x.copy_(state[0])
    loop.history.copy_(state[1])
    graph.replay()
    assert same_bits(loop.x, eager) and same_bits(loop.history, eager_history)
    loop.x.copy_(other_x)
    loop.history.copy_(state[1])
    graph.replay()
    assert same_bits(loop.x, eager_other)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_generate_stereo_fast_with_make_inpaint():
    """Two 17 x 23 frames; the first one's mask is empty and the model is not called for it."""
    g = torch.Generator().manual_seed(6)
    image = torch.rand((2, 17, 23, 3), generator=g)
    depth = torch.rand((2, 17, 23, 3), generator=g)
    # frame 0: a depth that falls smoothly from near on the left to far on the right -- the frame is squeezed, nothing is disoccluded
    depth[0] = ((255 - (torch.arange(23) * 255) // 22).float() / 255)[None, :, None]
    model, runner = gpu_runner(torch.float16)
    model.unet.record = False
    calls = []
    inner = ir.make_inpaint(runner, "", num_inference_steps=3, guidance_scale=7.5, strength=1.0, seed=11)

    def inpaint(filled_u8, mask, frame_index):
        calls.append(frame_index)
        return inner(filled_u8, mask, frame_index)

    stereo, left, right = sdn.generate_stereo_fast(image.cuda(), depth.cuda(), 5.0, inpaint)
    assert calls == [1] and model.vae.decoded == 1 and model.unet.count == 4
    assert model.tokenizer.prompts == [["high quality, detailed"], [""]]
    assert tuple(stereo.shape) == (2, 17, 46, 3) and stereo.dtype == torch.float32 and bool(torch.isfinite(stereo).all())
    assert tuple(runner.loop.x.shape) == (2, 9, 64, 64)
    # the same seed gives the same frame; another seed another one
    again = sdn.generate_stereo_fast(image.cuda(), depth.cuda(), 5.0, ir.make_inpaint(runner, "", 3, 7.5, 1.0, seed=11))[0]
    other = sdn.generate_stereo_fast(image.cuda(), depth.cuda(), 5.0, ir.make_inpaint(runner, "", 3, 7.5, 1.0, seed=12))[0]
    assert torch.equal(again, stereo) and not torch.equal(other[1], stereo[1]) and torch.equal(other[0], stereo[0])
