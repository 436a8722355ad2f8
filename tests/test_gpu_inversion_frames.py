"""Null-text optimisation on F frames at once, on the GPU: cs_null_loss_grad_frames and cs_adam_step_frames against the single-tensor
kernels on every frame alone, NullInversion.invert_frames against invert, generate_stereo_standard_frames against
generate_stereo_standard, and the node's STANDARD_ALL_FRAMES switch.

The yardstick is the single-frame path, which the fixtures pin to the reference -- never the batched code itself.  Bit for bit
wherever the model's own arithmetic does not depend on the batch (the kernels, the "exact" stand-in, the Standard loop's stand-in);
on the "attn" stand-in, whose linear layers run through the BLAS library, each frame's error against the float64 restatement
(tools/inversion_oracle.py) is held to 4 x the error the single-frame path shows on the same frame."""
import json
import math
import os

import numpy as np
import pytest
import torch

import inversion_oracle as io_
import null_fake_model as nm
import standard_fake_model as fm
from comfystereo_amd import engine, inversion, schedulers, stereo_utils
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_standard_surface import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "float16", "bfloat16")
COEFFS = (0.8, 0.6, 0.7, 0.714)
F = 3
# one thread's share, the edges of the 1024-thread stride, the block edge, the second stage with a one-element last block
PERS = (1, 1023, 1025, 32767, 32768, 32769, 65537)
POISON = 0x7fc01234   # a float32 NaN with a payload: what an untouched loss must still hold


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def loss_inputs(per, dtype, seed=5):
    """Four tensors [F, per]; frame 1 holds a NaN, frame 2 an infinity (where it has the room, next to finite values)."""
    g = torch.Generator().manual_seed(seed * 1000 + per % 997)
    t = [torch.randn((F, per), generator=g).to(dtype) for _ in range(4)]
    t[0][1, per // 2] = float("nan")
    t[2][2, per - 1] = float("inf")
    return [x.cuda() for x in t]


def flags(*values):
    return torch.tensor(values, dtype=torch.uint8, device="cuda")


def poisoned(like):
    rec = torch.full_like(like, -3.0)
    loss = torch.full((like.shape[0],), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return rec, loss


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("per", PERS)
def test_loss_frames_equal_the_single_tensor_kernel(per, dtype_name):
    dtype = getattr(torch, dtype_name)
    eu, ec, cur, prev = loss_inputs(per, dtype)
    for guidance in (7.5, 1.0):
        rec, loss, grad, out = engine.null_loss_grad_frames(eu, ec, cur, prev, guidance, COEFFS, flags(1, 1, 1), -math.inf)
        assert rec.dtype == grad.dtype == dtype and loss.dtype == torch.float32 and tuple(loss.shape) == (F,)
        assert out.tolist() == [1, 1, 1]
        for f in range(F):
            r1, l1, g1 = engine.null_loss_grad(eu[f], ec[f], cur[f], prev[f], guidance, COEFFS)
            assert same(rec[f], r1) and same(grad[f], g1) and same(loss[f:f + 1], l1.reshape(1)), (per, dtype_name, guidance, f)
        assert math.isnan(loss[1].item())
        assert per < 2 or not math.isnan(loss[0].item())   # the NaN of frame 1 stayed in frame 1


@pytest.mark.parametrize("per", (1025, 32769))
def test_inactive_frames_and_the_threshold(per):
    eu, ec, cur, prev = loss_inputs(per, torch.float32)
    full = engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, flags(1, 1, 1), -math.inf)
    for active in ((1, 1, 1), (0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        rec, loss = poisoned(eu)
        grad = torch.full_like(eu, 7.0)
        a_in, a_out = flags(*active), flags(9, 9, 9)
        got = engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, a_in, -math.inf, active_out=a_out, loss=loss, rec=rec, grad=grad)
        assert got[0] is rec and got[1] is loss and got[2] is grad and got[3] is a_out
        assert a_out.tolist() == list(active) and a_in.tolist() == list(active)
        for f in range(F):
            if active[f]:
                assert same(rec[f], full[0][f]) and same(loss[f:f + 1], full[1][f:f + 1]) and same(grad[f], full[2][f])
            else:   # a zero gradient; the reconstruction and the loss still hold what was there
                assert not bool(grad[f].any()) and bool((rec[f] == -3.0).all())
                assert int(loss[f:f + 1].view(torch.int32).item()) == POISON
    with pytest.raises(ValueError, match="active_out"):
        a = flags(1, 1, 1)
        engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, a, 0.0, active_out=a)
    # the stop: float64(loss) < threshold.  At the threshold a frame goes on, one float64 above it stops; a NaN loss never
    # stops; an inactive frame stays inactive whatever its stale loss says
    at = float(full[1][0].item())
    assert math.isfinite(at) and math.isnan(full[1][1].item())
    for threshold, want in ((at, 1), (math.nextafter(at, math.inf), 0)):
        _, loss, _, out = engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, flags(1, 1, 0), threshold,
                                                       loss=torch.full((F,), 0.5, device="cuda"))
        assert out.tolist() == [want, 1, 0] and loss[2].item() == 0.5, threshold
    _, _, _, out = engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, flags(1, 1, 0), math.inf, loss=torch.zeros(F, device="cuda"))
    assert out.tolist() == [0, 1, 0]


def nan_rows(shape, dtype, base):
    """NaNs of distinct payloads, one per element."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        return (torch.arange(n, dtype=torch.int32) % 4096 + 0x7fc00000 + base).view(torch.float32).reshape(shape).cuda()
    quiet = 0x7e00 if dtype == torch.float16 else 0x7fc0
    return (torch.arange(n, dtype=torch.int32) % 61 + quiet + base).to(torch.int16).view(dtype).reshape(shape).cuda()


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("m", (1, 255, 257, 77 * 768))
def test_adam_frames_equal_the_single_tensor_kernel(m, dtype_name):
    dtype = getattr(torch, dtype_name)
    g = torch.Generator().manual_seed(m)
    for step in (1, 10):
        for active in ((1, 1, 1), (0, 1, 0), (1, 0, 1)):
            p, gr, ea, es = (torch.randn((F, m), generator=g).to(dtype).cuda() for _ in range(4))
            es = es.abs()
            for f in range(F):
                if not active[f]:
                    p[f], gr[f], ea[f], es[f] = (nan_rows((m,), dtype, k + 1) for k in range(4))
            before = [t.clone() for t in (p, gr, ea, es)]
            assert engine.adam_step_frames(p, gr, ea, es, flags(*active), 1e-2, step) is p
            assert same(gr, before[1])
            for f in range(F):
                if active[f]:
                    want = [t[f].clone() for t in before]
                    engine.adam_step(want[0], want[1], want[2], want[3], 1e-2, step)
                    assert same(p[f], want[0]) and same(ea[f], want[2]) and same(es[f], want[3]), (m, dtype_name, step, f)
                    assert m == 1 or not same(p[f], before[0][f])
                else:   # not written at all: every bit pattern survives
                    assert all(same(t[f], b[f]) for t, b in zip((p, gr, ea, es), before)), (m, dtype_name, step, f)


def test_loss_frames_under_autograd():
    g = torch.Generator().manual_seed(9)
    eu, ec, cur, prev = (torch.randn((F, 1025), generator=g).cuda() for _ in range(4))
    w = torch.full_like(eu, 0.5, requires_grad=True)
    a_out = flags(0, 0, 0)
    loss = engine.NullTextLossFrames.apply(eu * w * 2, ec, cur, prev, 7.5, COEFFS, flags(1, 0, 1), 0.0, a_out)
    assert loss.requires_grad and tuple(loss.shape) == (F,) and a_out.tolist() == [1, 0, 1]
    (gw,) = torch.autograd.grad(loss.sum(), [w], retain_graph=True)
    _, _, grad, _ = engine.null_loss_grad_frames(eu, ec, cur, prev, 7.5, COEFFS, flags(1, 0, 1), 0.0)
    assert torch.equal(gw, grad * (eu * 2)) and not bool(gw[1].any()) and bool(gw[0].any())
    with pytest.raises(ValueError, match="ones"):
        torch.autograd.grad(loss, [w], grad_outputs=torch.full((F,), -2.5, device="cuda"))


# ---- the inversion ---------------------------------------------------------------------------------------------------------------
def frames_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "inversion_frames.json")) as f:
        return json.load(f)


def seeded_frames(seeds):
    return torch.stack([torch.from_numpy(nm.seeded_image(s)) for s in seeds]).cuda()


class Counted:
    """The UNet with a call counter."""

    def __init__(self, unet):
        self.unet, self.calls = unet, []

    def __getattr__(self, name):
        return getattr(self.unet, name)

    def __call__(self, x, t, encoder_hidden_states=None):
        self.calls.append(tuple(x.shape))
        return self.unet(x, t, encoder_hidden_states=encoder_hidden_states)


_single = {}


def single_runs(dtype_name, meta):
    """invert on every frame alone, once per dtype: the yardstick of the batched run."""
    if dtype_name not in _single:
        images, runs = seeded_frames(meta["seeds"]), []
        for f in range(len(meta["seeds"])):
            inv = inversion.NullInversion(nm.NullModel("exact", "cuda", getattr(torch, dtype_name)), meta["steps"], meta["guidance"])
            _, x_t, emb = inv.invert(images[f], meta["prompt"], num_inner_steps=meta["inner"], early_stop_epsilon=meta["epsilon"])
            runs.append((x_t, emb, inv.inner_steps_taken, inv.losses))
        _single[dtype_name] = runs
    return _single[dtype_name]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_invert_frames_equals_invert_on_every_frame(dtype_name):
    meta = frames_fixture()
    runs = single_runs(dtype_name, meta)
    counts = [[run[2][i] for run in runs] for i in range(meta["steps"])]   # [outer step][frame], from the single-frame runs
    print(dtype_name, "inner steps per outer step and frame", counts)
    # float32 carries the condition on the inputs.  On an MI355X the float16 run's losses are NaN (the moments underflow, as in the
    # reference's own float16 run) and no frame ever stops; the bfloat16 run's frames stop together: bit identity is asserted
    # for them all the same, the spread is float32's
    if dtype_name == "float32":
        assert counts == meta["inner_steps"]   # what the float64 restatement takes (tools/inversion_oracle.py), checked on the CPU
        # a run whose frames all stop together proves nothing about the flags: in one outer step the frames take different
        # numbers of inner steps and one of them runs to the last
        assert any(len(set(row)) >= 2 and max(row) == meta["inner"] for row in counts)
    model = nm.NullModel("exact", "cuda", getattr(torch, dtype_name))
    model.unet = Counted(model.unet)
    inv = inversion.NullInversion(model, meta["steps"], meta["guidance"])
    try:
        x_t, emb = inv.invert_frames(seeded_frames(meta["seeds"]), meta["prompt"], num_inner_steps=meta["inner"],
                                     early_stop_epsilon=meta["epsilon"])
    finally:
        stereo_utils.restore_attention(model)
    n = len(meta["seeds"])
    assert tuple(x_t.shape) == (n, 4, 64, 64) and len(emb) == meta["steps"] and all(tuple(e.shape) == (n, 77, nm.WIDTH) for e in emb)
    assert inv.inner_steps_taken == counts
    for f, (x1, emb1, _, losses1) in enumerate(runs):
        assert same(x_t[f:f + 1], x1), f
        for i in range(meta["steps"]):
            assert same(emb[i][f:f + 1], emb1[i]), (f, i)
            assert np.array_equal(np.array(inv.losses[i][f], np.float64).view(np.int64), np.array(losses1[i], np.float64).view(np.int64)), (f, i)
    # UNet calls: the DDIM loop's, then per outer step one conditional, one per inner step of the slowest frame, one guided
    want = [(n, 4, 64, 64)] * meta["steps"]
    for row in counts:
        want += [(n, 4, 64, 64)] * (1 + max(row)) + [(2 * n, 4, 64, 64)]
    assert model.unet.calls == want


def test_one_loss_launch_one_adam_launch_and_one_read_per_inner_step():
    from torch.profiler import ProfilerActivity, profile
    meta = frames_fixture()
    model = nm.NullModel("exact", "cuda")
    inv = inversion.NullInversion(model, meta["steps"], meta["guidance"])
    inv.init_prompt(meta["prompt"])
    ddim = inv.ddim_loop_frames(inv._images2latent(seeded_frames(meta["seeds"])))
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        inv.null_optimization_frames(ddim, meta["inner"], meta["epsilon"])
        torch.cuda.synchronize()
    names = [ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
    inner = sum(max(row) for row in inv.inner_steps_taken)
    assert inv.inner_steps_taken == meta["inner_steps"]
    assert sum("k_null_loss_grad_frames" in n for n in names) == inner
    assert sum("k_adam_step_frames" in n for n in names) == inner
    assert not any("k_null_loss_final" in n for n in names)   # 16 384 elements per frame: one stage
    flat = [n.lower().replace(" ", "").replace("->", "to") for n in names]
    reads = [n for n in flat if ("memcpy" in n or "copy" in n) and ("dtoh" in n or "devicetohost" in n)]
    print("device-to-host copies", len(reads), "inner steps", inner)
    assert len(reads) == inner


def test_attn_form_stays_within_four_times_the_single_frame_error():
    seeds, steps, inner, guidance, epsilon, prompt = (11, 12), 5, 3, 7.5, 6.4e-3, "a photo"
    images = seeded_frames(seeds)
    model = nm.NullModel("attn", "cuda")
    inv = inversion.NullInversion(model, steps, guidance)
    try:
        x_t, emb = inv.invert_frames(images, prompt, num_inner_steps=inner, early_stop_epsilon=epsilon)
        hooked = [hasattr(m, stereo_utils._SAVED_FORWARD) for m in model.unet.modules() if m.__class__.__name__ == "CrossAttention"]
        assert hooked == [True]
    finally:
        stereo_utils.restore_attention(model)
    model64 = nm.NullModel("attn", "cpu", torch.float64)
    model64.scheduler.set_timesteps(steps)
    ctx64 = inv.context.detach().cpu().double()
    for f in range(len(seeds)):
        one = inversion.NullInversion(nm.NullModel("attn", "cuda"), steps, guidance)
        _, x1, emb1 = one.invert(images[f], prompt, num_inner_steps=inner, early_stop_epsilon=epsilon)
        lat64 = one.image2latent(images[f]).detach().cpu().double()
        ddim64 = io_.ddim_loop(model64, lat64, ctx64[1:], steps)
        emb64, _ = io_.null_optimization(model64, ddim64, ctx64, steps, guidance, inner, epsilon)
        assert inv.inner_steps_taken and [row[f] for row in inv.inner_steps_taken] == one.inner_steps_taken
        for what, got, alone, want in (("x_t", x_t[f:f + 1], x1, ddim64[-1]),
                                       ("embeddings", torch.stack([e[f:f + 1] for e in emb]), torch.stack(emb1), torch.stack(emb64))):
            e_batch, e_single = io_.err(got.detach().cpu().double().numpy(), want.numpy()), io_.err(alone.detach().cpu().double().numpy(), want.numpy())
            print(f"attn frame {f} {what}: batched error {e_batch:.3e}, single-frame error {e_single:.3e}, "
                  f"ratio {e_batch / e_single if e_single else math.inf:.3f}")
            assert e_batch <= 4 * e_single, (f, what, e_batch, e_single)


# ---- Standard mode on every frame ------------------------------------------------------------------------------------------------
def standard_inputs(n=3, h=24, w=40, seed=8):
    g = torch.Generator().manual_seed(seed)
    image = torch.rand((n, h, w, 3), generator=g)
    # a depth of its own range and slope per frame: a range taken over the batch would change every frame's disparity
    ramp = (torch.arange(w) * 4 // w).float() / 3
    depth = torch.stack([(0.2 * k + (1 - 0.3 * k) * (ramp if k % 2 == 0 else ramp.flip(0)))[None, :, None].expand(h, w, 3) for k in range(n)])
    noise = torch.randn((n, 4, 64, 64), generator=g)
    return image, depth.contiguous(), noise


def standard_model():
    model = fm.FakeModel("cuda", torch.float32)
    model.scheduler = schedulers.DDIMScheduler()
    return model


STEPS = 5


def frame_embeddings(k, device):
    """Frame k's own null-text embeddings: the stand-in's, scaled by a power of two."""
    return [e * 2.0 ** -k for e in fm.fake_uncond_embeddings(STEPS, device, torch.float32)]


def invert_one(k):
    return lambda image_u8: (fm.fake_invert(image_u8)[0], frame_embeddings(k, image_u8.device))


def invert_many():
    """fake_invert on a group of frames; the groups arrive in frame order, so a counter knows which frames they are."""
    seen = [0]

    def invert_frames(images_u8):
        first, seen[0] = seen[0], seen[0] + len(images_u8)
        x_t = torch.cat([fm.fake_invert(u8)[0] for u8 in images_u8])
        per_frame = [frame_embeddings(first + f, images_u8.device) for f in range(len(images_u8))]
        return x_t, [torch.cat([emb[i] for emb in per_frame]) for i in range(STEPS)]

    return invert_frames


@pytest.mark.parametrize("direction,deblur", [("uni", True), ("bi", True), ("uni", False), ("bi", False)])
def test_standard_frames_equal_frame_by_frame(direction, deblur):
    image, depth, noise = standard_inputs()
    n = image.shape[0]
    want = []
    for k in range(n):
        one = sdn.generate_stereo_standard(image[k:k + 1].cuda(), depth[k:k + 1].cuda(), 8.0, direction, deblur, STEPS, 3.0, standard_model(),
                                           invert_one(k), torch.cat([noise[k:k + 1]] * 2) if deblur else None)
        want.append(one[0])
    want = torch.cat(want)
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    for per_batch in (1, 2, 4):   # 2: a short last group
        model = standard_model()
        model.unet.record = True
        stereo, left, right = sdn.generate_stereo_standard_frames(image.cuda(), depth.cuda(), 8.0, direction, deblur, STEPS, 3.0, model,
                                                                  invert_many(), per_batch, noise if deblur else None)
        assert tuple(stereo.shape) == (n, 24, 80, 3) and torch.equal(stereo, want), (direction, deblur, per_batch)
        assert torch.equal(left, stereo[:, :, :40]) and torch.equal(right, stereo[:, :, 40:])
        sizes = [c.shape[0] // 4 for c in model.unet.calls]
        assert sizes == [b for k in range(0, n, per_batch) for b in [min(per_batch, n - k)] * STEPS]


def test_standard_frames_draw_the_deblur_noise_as_successive_calls_do():
    image, depth, _ = standard_inputs(n=2)
    g = torch.Generator().manual_seed(21)
    want = torch.cat([sdn.generate_stereo_standard(image[k:k + 1].cuda(), depth[k:k + 1].cuda(), 8.0, "uni", True, STEPS, 3.0, standard_model(),
                                                   invert_one(k), generator=g)[0] for k in range(2)])
    g = torch.Generator().manual_seed(21)
    got = sdn.generate_stereo_standard_frames(image.cuda(), depth.cuda(), 8.0, "uni", True, STEPS, 3.0, standard_model(), invert_many(),
                                              generator=g)[0]
    assert torch.equal(got, want)
    # a scheduler that is not ours: frame by frame through generate_stereo_standard, on the same generator
    g = torch.Generator().manual_seed(21)
    plain = fm.FakeModel("cuda", torch.float32)
    got = sdn.generate_stereo_standard_frames(image.cuda(), depth.cuda(), 8.0, "uni", True, STEPS, 3.0, plain, invert_many(), generator=g)[0]
    g = torch.Generator().manual_seed(21)
    want = torch.cat([sdn.generate_stereo_standard(image[k:k + 1].cuda(), depth[k:k + 1].cuda(), 8.0, "uni", True, STEPS, 3.0,
                                                   fm.FakeModel("cuda", torch.float32), invert_one(k), generator=g)[0] for k in range(2)])
    assert torch.equal(got, want)


def test_node_switch(capsys, monkeypatch):
    from test_gpu_standard_step import comfy_models, frames
    image, depth = frames(2, 17, 23)
    node = sdn.StereoDiffusionNode()

    def run():
        model, clip, vae, _ = comfy_models(sdn.STANDARD_MODE, torch.float32)
        return node.generate_stereo(image, depth, 8.0, "bi", True, sdn.STANDARD_MODE, 3.0, 5, 7, True, 0.6, model, clip, vae)

    assert sdn.STANDARD_ALL_FRAMES is False
    first = run()[0]
    assert tuple(first.shape) == (1, 17, 46, 3) and "processes only the first frame" in capsys.readouterr().out
    monkeypatch.setattr(sdn, "STANDARD_ALL_FRAMES", True)
    stereo, left, right = run()
    assert tuple(stereo.shape) == (2, 17, 46, 3) and "first frame" not in capsys.readouterr().out
    assert torch.equal(left, stereo[:, :, :23]) and torch.equal(right, stereo[:, :, 23:])
    assert torch.equal(stereo[:1], first) and not torch.equal(stereo[1], stereo[0])
