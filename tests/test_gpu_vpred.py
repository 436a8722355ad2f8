"""v-prediction (SD 2.x 768-v) through the four fused kernels -- cs_ddim_step_pred, cs_null_loss_grad_pred,
cs_null_loss_grad_frames_pred, cs_standard_step_pred -- against the CPU torch expression of tools/vpred_oracle.py, bit for bit; the
same entry points with CS_PRED_EPSILON against their namesakes; Standard mode and DDIM inversion end to end on the stand-in models
at small work sizes (gpu).

The optimisation end to end is held to the float64 host loop of the oracle by the epsilon suite's rule (inner-step counts, losses,
embeddings); invert_frames to invert, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import inversion_oracle as io
import null_fake_model as nm
import standard_fake_model as fm
import vpred_oracle as vo
from comfystereo_amd import _native, engine, inversion, schedulers
from comfystereo_amd import stereodiffusion_nodes as sdn

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = lambda d: str(d).split(".")[-1]   # noqa: E731
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
V = "v_prediction"


def bits(t):
    return t.detach().cpu().contiguous().view(INT_OF[t.dtype])


def same(got, want):
    """Equal bits wherever neither is a NaN, and NaNs at the same positions."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype or not torch.equal(got.isnan(), want.isnan()):
        return False
    keep = ~want.isnan()
    return torch.equal(bits(got)[keep], bits(want)[keep])


def coeff_sets(dtype, prediction=V):
    s = schedulers.DDIMScheduler(prediction_type=prediction)
    s.set_timesteps(10)
    return [s.coeffs(t, dtype) for t in (900, 500, 0)]


def specials(dtype):
    info = torch.finfo(dtype)
    tiny = info.smallest_normal * info.eps
    return torch.tensor([0.0, -0.0, tiny, -tiny, info.max, -info.max, float("nan"), 1.0], dtype=torch.float64)


def step_inputs(n, dtype, seed):
    """(sample, a, b) on the host; with room, the specials meet each other in the first elements."""
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3)]
    sp = specials(dtype)
    for k, t in enumerate(ts):
        m = min(n, 8)
        t[:m] = sp.roll(k)[:m]
    return [t.to(dtype) for t in ts]


def on_device(t, off=0):
    buf = torch.empty(t.numel() + off + 8, dtype=t.dtype, device="cuda")
    view = buf[off:off + t.numel()]
    view.copy_(t)
    return view


# ---- cs_ddim_step_pred, CS_PRED_V ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ddim_step_v_equals_the_torch_expression(dtype):
    cs = coeff_sets(dtype)
    guidances = (7.5, 1.0, 0.0, -2.0)
    k = 0
    for n in (1, 7, 8, 32768, 32769):
        s, a, b = step_inputs(n, dtype, n)
        ds, da, db = on_device(s), on_device(a), on_device(b)
        for g in guidances if n == 32769 else guidances[k % 4:k % 4 + 1]:
            c = cs[k % 3]
            k += 1
            assert same(engine.ddim_step_pred(ds, da, db, g, c, prediction=V), vo.torch_step(s, a, b, g, c)), (n, g, c)
        assert same(engine.ddim_step_pred(ds, da, None, 1.0, cs[k % 3], prediction=V), vo.torch_step(s, a, None, 1.0, cs[k % 3])), n
    # every tensor one element off the 16-byte grid; out aliasing sample
    s, a, b = step_inputs(263, dtype, 5)
    ds, da, db = on_device(s, 1), on_device(a, 1), on_device(b, 1)
    out = on_device(torch.zeros_like(s), 1)
    assert all(t.data_ptr() % 16 for t in (ds, da, db, out))
    want = vo.torch_step(s, a, b, 7.5, cs[1])
    assert same(engine.ddim_step_pred(ds, da, db, 7.5, cs[1], out=out, prediction=V), want)
    assert engine.ddim_step_pred(ds, da, db, 7.5, cs[1], out=ds, prediction=V) is ds and same(ds, want)
    # c2 = 0 divides nothing
    ds = on_device(s)
    assert same(engine.ddim_step_pred(ds, on_device(a), None, 1.0, (1.0, 0.0, 0.5, 0.5), prediction=V), vo.torch_step(s, a, None, 1.0, (1.0, 0.0, 0.5, 0.5)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_fixture_is_what_the_kernel_gives(dtype):
    import json

    import make_vpred_goldens as mk
    z = np.load(mk.OUT)
    name = IDS(dtype)
    s, a, b, _ = mk.inputs(dtype)
    for c in json.loads(str(z["meta"]))["cases"]:
        if c["dtype"] != name:
            continue
        got = engine.ddim_step_pred(s.cuda(), a.cuda(), b.cuda(), c["guidance"], c["coeffs"], prediction=V)
        want = torch.from_numpy(z[c["id"] + "/step"].view({2: np.int16, 4: np.int32}[s.element_size()])).view(dtype)
        assert same(got, want), c["id"]


# ---- CS_PRED_EPSILON equals the namesake, all four pairs ----------------------------------------------------------------------------------
def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(fn, *args):
    _native.check(fn(*args, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_epsilon_through_the_new_entry_points_equals_the_old_ones(dtype):
    L, code = _native.lib(), _native.LATENT_DTYPE[IDS(dtype)]
    c, g, n = coeff_sets(dtype, "epsilon")[1], 7.5, 32769
    s, a, b = (on_device(t) for t in step_inputs(n, dtype, 9))
    prev = on_device(step_inputs(n, dtype, 10)[0])
    torch.cuda.synchronize()
    # cs_ddim_step
    outs = [torch.empty_like(s) for _ in range(2)]
    call(L.cs_ddim_step, ptr(s), ptr(a), ptr(b), ptr(outs[0]), code, n, g, *c)
    call(L.cs_ddim_step_pred, ptr(s), ptr(a), ptr(b), ptr(outs[1]), code, n, g, *c, 0)
    assert same(outs[1], outs[0])
    # cs_null_loss_grad (finite inputs: the loss of the specials is a NaN either way)
    fs, fa, fb, fp = (t[8:].clone() for t in (s, a, b, prev))
    m = n - 8
    res = []
    for pred in (None, 0):
        rec, grad, loss = torch.empty_like(fs), torch.empty_like(fs), torch.empty((), dtype=torch.float32, device="cuda")
        ws = torch.empty(max(L.cs_null_loss_workspace_bytes(m), 256), dtype=torch.uint8, device="cuda")
        head = (ptr(fa), ptr(fb), ptr(fs), ptr(fp), ptr(rec), ptr(loss), ptr(grad), code, m, g, *c)
        tail = (ptr(ws), ws.numel())
        call(L.cs_null_loss_grad, *head, *tail) if pred is None else call(L.cs_null_loss_grad_pred, *head, pred, *tail)
        res.append((rec, grad, loss))
    assert same(res[1][0], res[0][0]) and same(res[1][1], res[0][1]) and torch.equal(res[1][2], res[0][2])
    # cs_null_loss_grad_frames: 3 frames of 10 920 elements
    frames, per = 3, 10920
    f4 = [t[:frames * per].clone() for t in (fa, fb, fs, fp)]
    res = []
    for pred in (None, 0):
        rec, grad = torch.zeros_like(f4[0]), torch.empty_like(f4[0])
        loss = torch.zeros(frames, dtype=torch.float32, device="cuda")
        a_in, a_out = torch.ones(frames, dtype=torch.uint8, device="cuda"), torch.zeros(frames, dtype=torch.uint8, device="cuda")
        head = (*(ptr(t) for t in f4), ptr(rec), ptr(loss), ptr(grad), ptr(a_in), ptr(a_out), code, frames, per, g, *c)
        tail = (1e-3, None, 0)
        call(L.cs_null_loss_grad_frames, *head, *tail) if pred is None else call(L.cs_null_loss_grad_frames_pred, *head, pred, *tail)
        res.append((rec, grad, loss, a_out))
    assert same(res[1][0], res[0][0]) and same(res[1][1], res[0][1]) and torch.equal(res[1][2], res[0][2]) and torch.equal(res[1][3], res[0][3])
    # cs_standard_step, the shift with noise
    bsz, ch, h, w = 1, 4, 2, 8
    cnt = 4 * bsz * ch * h * w
    x0, pred_t = s[:cnt].clone().view(4, ch, h, w), a[:cnt].clone().view(4, ch, h, w)
    noise = b[8:8 + cnt // 4].clone().view(1, ch, h, w)
    src = table(bsz, h, w)
    res = []
    for pred in (None, 0):
        x, mask = x0.clone(), torch.zeros((bsz, h, w), dtype=torch.uint8, device="cuda")
        head = (ptr(x), ptr(pred_t), code, bsz, ch, h, w, g, *c)
        tail = (_native.STANDARD_OP["first"], ptr(src), ptr(mask), ptr(noise))
        call(L.cs_standard_step, *head, *tail) if pred is None else call(L.cs_standard_step_pred, *head, pred, *tail)
        res.append((x, mask))
    assert same(res[1][0], res[0][0]) and torch.equal(res[1][1], res[0][1])
    # an unknown prediction is refused before any launch
    assert L.cs_ddim_step_pred(ptr(s), ptr(a), ptr(b), ptr(outs[1]), code, n, g, *c, 2, None) == _native.CS_EINVAL
    assert b"prediction" in L.cs_last_error()


# ---- cs_null_loss_grad_pred, CS_PRED_V ---------------------------------------------------------------------------------------------------
def loss_inputs(n, dtype, seed, far=False):
    """(v_uncond, v_cond, latent_cur, latent_prev).  near: latent_prev a twentieth of a standard deviation from latent_cur, the
    scale of an inversion.  far: 4096 .. 16384 away from it, either side, so that every element's gradient -- of order
    (2 / n) * diff * 0.6 -- is at least 0.15 at n = 32 769: large enough for float16's Adam, whose second moment 0.001 * g * g is
    zero below |g| = 8e-3 and whose eps of 1e-8 rounds to 0 (torch.optim.Adam then divides 0 by 0)."""
    g = torch.Generator().manual_seed(seed)
    cur = torch.randn(n, generator=g, dtype=torch.float64)
    u, c = 0.5 * torch.randn(n, generator=g, dtype=torch.float64), 0.5 * torch.randn(n, generator=g, dtype=torch.float64)
    if far:
        sign = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
        prev = cur + sign * (4096 + 12288 * torch.rand(n, generator=g, dtype=torch.float64))
    else:
        prev = cur + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    return [t.to(dtype) for t in (u, c, cur, prev)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [5, 32768, 32769])
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_null_loss_grad_v(far, n, dtype):
    """rec: the bits of the step.  Loss, gradient and the Adam step that follows: within 4 x the error of the CPU torch-autograd
    composition (or one ulp) of the float64 restatement -- the rule the epsilon inversion is held to (tools/inversion_oracle.py).
    The Adam step is compared on the `far` inputs, at every count in every dtype (loss_inputs says why not on the near ones: the
    reference's float16 Adam is NaN there); loss and gradient on both."""
    name, g, cf = IDS(dtype), 7.5, coeff_sets(dtype)[1]
    u, c, cur, prev = loss_inputs(n, dtype, n, far)
    du, dc, dcur, dprev = (t.cuda() for t in (u, c, cur, prev))
    rec, loss, grad = engine.null_loss_grad(du, dc, dcur, dprev, g, cf, prediction=V)
    assert same(rec, engine.ddim_step_pred(dcur, du, dc, g, cf, prediction=V)) and same(rec, vo.torch_step(cur, u, c, g, cf))
    rec2, loss2, grad2 = engine.null_loss_grad(du, dc, dcur, dprev, g, cf, prediction=V)
    assert same(rec2, rec) and same(grad2, grad) and torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    f64 = lambda t: t.detach().cpu().double().numpy()   # noqa: E731
    _, want_loss, want_grad = vo.null_loss_grad64(f64(u), f64(c), f64(cur), f64(prev), g, cf)
    _, ref_loss, ref_grad = vo.torch_null_loss(u, c, cur, prev, g, cf)
    figures = {"loss": (io.err(f64(loss), want_loss), io.bound(io.err(f64(ref_loss), want_loss), "float32", want_loss)),
               "grad": (io.err(f64(grad), want_grad), io.bound(io.err(f64(ref_grad), want_grad), name, want_grad))}
    if far:   # Adam on the gradient, from zero moments
        p0 = (0.25 * torch.randn(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).to(dtype)
        want_p = io.adam(f64(p0), [want_grad], 1e-2)[0][0]
        ref_p = torch.nn.Parameter(p0.clone())
        ref_p.grad = ref_grad.clone()
        torch.optim.Adam([ref_p], lr=1e-2).step()
        assert bool(torch.isfinite(ref_p.detach()).all())   # (the inputs' purpose)
        dp = p0.cuda()
        engine.adam_step(dp, grad, torch.zeros_like(dp), torch.zeros_like(dp), 1e-2, 1)
        figures["adam"] = (io.err(f64(dp), want_p), io.bound(io.err(f64(ref_p), want_p), name, want_p))
    print(n, name, "far" if far else "near", figures)
    for key, (got, bound) in figures.items():
        assert got <= bound, (key, got, bound)


# ---- cs_null_loss_grad_frames_pred, CS_PRED_V -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("per", [5, 32769])
def test_null_loss_grad_frames_v(per, dtype):
    g, cf, frames = 7.5, coeff_sets(dtype)[1], 3
    rows = [[t.cuda() for t in loss_inputs(per, dtype, 40 + f)] for f in range(frames)]
    rows[2][3] = rows[2][2] + (rows[2][3] - rows[2][2]) * 4   # frame 2 lies farther from its target: a larger loss
    stacked = [torch.stack([rows[f][k] for f in range(frames)]).contiguous() for k in range(4)]
    alone = {f: engine.null_loss_grad(*rows[f], g, cf, prediction=V) for f in (0, 2)}
    l0, l2 = float(alone[0][1]), float(alone[2][1])
    assert l0 < l2
    threshold = (l0 + l2) / 2
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    poison = 77.0
    rec = torch.full_like(stacked[0], poison)
    grad = torch.full_like(stacked[0], poison)
    loss = torch.full((frames,), poison, dtype=torch.float32, device="cuda")
    _, _, _, out = engine.null_loss_grad_frames(*stacked, g, cf, active, threshold, loss=loss, rec=rec, grad=grad, prediction=V)
    for f in (0, 2):
        assert same(rec[f], alone[f][0]) and same(grad[f], alone[f][2]), f
        assert torch.equal(loss[f].view(torch.int32), alone[f][1].view(torch.int32)), f
    assert out.tolist() == [0, 0, 1]                      # frame 0 is below the threshold and stops, frame 2 goes on
    assert bool((rec[1] == poison).all()) and float(loss[1]) == poison and bool((grad[1] == 0).all())


# ---- cs_standard_step_pred, CS_PRED_V ----------------------------------------------------------------------------------------------------
def table(b, h, w):
    """Every row: a hole, a column gathered twice, the rest reversed."""
    cols = (w - 1 - torch.arange(w, dtype=torch.int32)).clone()
    cols[0] = -1
    cols[1] = cols[2]
    return cols.expand(b, h, w).contiguous().cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("hw", [(2, 5), (2, 8)], ids=["scalar", "wide"])
def test_standard_step_v_equals_the_composition(hw, b, dtype):
    (h, w), ch = hw, 4
    cs = coeff_sets(dtype)
    g = torch.Generator().manual_seed(h * w + b)
    x0 = torch.randn((4 * b, ch, h, w), generator=g).to(dtype).cuda()
    pred = torch.randn((4 * b, ch, h, w), generator=g).to(dtype).cuda()
    sp = specials(dtype).to(dtype).cuda()
    x0[0, 0].view(-1)[:8] = sp
    pred[0, 0].view(-1)[:8] = sp.roll(1)
    noise = torch.randn((b, ch, h, w), generator=g).to(dtype).cuda()
    stored = (torch.rand((b, h, w), generator=g) < 0.5).to(torch.uint8).cuda()
    src = table(b, h, w)
    for k, (op, with_noise) in enumerate([("none", False), ("first", False), ("first", True), ("reshift", False)]):
        guidance, cf = (7.5, 1.0, 0.0, -2.0)[k], cs[k % 3]
        new = engine.ddim_step_pred(x0[:2 * b].clone(), pred[:2 * b].contiguous(), pred[2 * b:].contiguous(), guidance, cf, prediction=V)
        want_mask = stored.clone()
        if op != "none":
            engine.latent_shift_apply(new[:b], new[b:], src, want_mask, op, noise=noise if with_noise else None)
        x, mask = x0.clone(), stored.clone()
        engine.standard_step(pred, x, guidance, cf, op, None if op == "none" else src, None if op == "none" else mask,
                             noise if with_noise else None, prediction=V)
        assert same(x, torch.cat([new, new])) and torch.equal(mask, want_mask), (op, with_noise)


# ---- end to end on the stand-in models ---------------------------------------------------------------------------------------------------
def disparity(size):
    return (torch.arange(size, dtype=torch.float32) // (size // 4) / 3).clamp(0, 1).expand(1, size, size).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("size,prediction", [(64, V), (72, V), (64, "epsilon")])
def test_standard_mode_at_a_small_work_size(size, prediction, dtype, monkeypatch):
    monkeypatch.setattr(sdn, "STANDARD_WORK_SIZE", size)
    steps, guidance, scale = 5, 3.0, 8.0
    hl = size // 8
    gen = torch.Generator().manual_seed(size)
    latent = torch.randn((1, 4, hl, hl), generator=gen).to(dtype)
    noise = torch.randn((2, 4, hl, hl), generator=gen).to(dtype)
    model = fm.FakeModel("cuda", dtype)
    model.scheduler = schedulers.DDIMScheduler(prediction_type=prediction)
    model.unet.record = True
    disp = disparity(size).cuda()
    args = (model, ["", ""], None, torch.cat([latent, latent]).cuda(), disp, scale, "uni", True, steps, guidance, noise.cuda())
    latents, mask = sdn._stereo_latents(*args, None)
    assert len(model.unet.calls) == steps and all(c is model.unet.calls[0] for c in model.unet.calls)   # one persistent input
    src = engine.latent_shift_plan(sdn._disparity_to_latent(disp, (hl, hl)), scale).cpu()
    host = fm.FakeModel("cpu", dtype)
    alphas = schedulers.DDIMScheduler().alphas_cumprod
    want, want_mask = vo.standard_loop(host, alphas, torch.cat([latent, latent]), src, steps, guidance, None, noise[1:], prediction)
    assert same(latents, want) and torch.equal(mask.cpu(), want_mask) and bool(want_mask.any())
    codes = sdn.text2stereoimage(*args)
    assert tuple(codes.shape) == (2, size, size, 3)
    assert torch.equal(codes, engine.decode_to_codes(model.vae.decode(1 / 0.18215 * want.cuda())["sample"].contiguous()))


INV = dict(steps=5, guidance=7.5, inner=10, epsilon=5e-4)
# On the float64 restatement (tools/vpred_oracle.py null_optimization, run on the CPU) the first outer step stops at its 4th inner
# step at both sizes and no other stops, every loss at least 11 % from its threshold: a stop in mid-loop, far from the rounding.
INNER_STEPS = [4, 10, 10, 10, 10]


def inversion_image(size, seed):
    return torch.randint(0, 256, (size, size, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def host_inversion(image, dtype):
    """DDIM inversion and null-text optimisation of the oracle on a CPU model of `dtype` -> (ddim latents, embeddings, losses)."""
    host = nm.NullModel("exact", "cpu", dtype)
    x = (image.float() / 127.5 - 1).permute(2, 0, 1).unsqueeze(0).to(dtype)
    start = host.vae.encode(x)["latent_dist"].mean * 0.18215
    ddim = vo.ddim_inversion_loop(host, start, INV["steps"])
    e = host.text_encoder(host.tokenizer([""]).input_ids)[0]
    emb, losses = vo.null_optimization(host, ddim, torch.cat([e, e]), INV["steps"], INV["guidance"], INV["inner"], INV["epsilon"])
    return ddim, emb, losses


_single = {}


def single_run(size, seed):
    """NullInversion.invert under a v-prediction scheduler, once per (size, seed) -> (x_t, embeddings, inner steps, losses)."""
    if (size, seed) not in _single:
        model = nm.NullModel("exact", "cuda", torch.float32)
        model.scheduler.config.prediction_type = V
        inv = inversion.NullInversion(model, INV["steps"], INV["guidance"])
        inv.work_size = size
        (_, _), x_t, emb = inv.invert(inversion_image(size, seed).cuda(), "", num_inner_steps=INV["inner"], early_stop_epsilon=INV["epsilon"])
        _single[size, seed] = (x_t, emb, list(inv.inner_steps_taken), [list(r) for r in inv.losses])
    return _single[size, seed]


@pytest.mark.parametrize("size", [64, 72])
def test_inversion_at_a_small_work_size_under_v_prediction(size):
    """x_t: the bits of the host loop.  The optimisation: the inner-step counts of the float64 restatement (a stop in mid-loop),
    every inner step's loss and the embeddings within 4 x the CPU float32 torch-autograd loop's own error of it -- the rule and
    the quantities of the epsilon suite (test_gpu_inversion.py)."""
    f64 = lambda t: t.detach().cpu().double().numpy()   # noqa: E731
    x_t, emb, taken, losses = single_run(size, size)
    image = inversion_image(size, size)
    ddim64, emb64, loss64 = host_inversion(image, torch.float64)
    ddim32, emb32, loss32 = host_inversion(image, torch.float32)
    assert tuple(x_t.shape) == (1, 4, size // 8, size // 8) and same(x_t, ddim32[-1])
    assert [len(r) for r in loss64] == INNER_STEPS and [len(r) for r in loss32] == INNER_STEPS
    assert io.margins(loss64, INV["epsilon"]) > 0.1
    assert taken == INNER_STEPS                                    # the stop falls where the restatement's falls
    flat = lambda rows: np.array([x for r in rows for x in r])     # noqa: E731
    worst = io.err(flat(losses), flat(loss64))
    bound = io.bound(io.err(flat(loss32), flat(loss64)), "float32", flat(loss64))
    print(size, "loss error", worst, "bound", bound)
    assert worst <= bound
    assert len(emb) == INV["steps"] and all(tuple(e.shape) == (1, 77, nm.WIDTH) for e in emb)
    worst = max(io.err(f64(a), f64(b)) for a, b in zip(emb, emb64))
    bound = io.bound(max(io.err(f64(a), f64(b)) for a, b in zip(emb32, emb64)), "float32", np.concatenate([f64(e).ravel() for e in emb64]))
    print(size, "embeddings error", worst, "bound", bound)
    assert worst <= bound
    # ... and under an epsilon scheduler the same inputs give other losses: the scheduler's prediction type reaches the loss
    model = nm.NullModel("exact", "cuda", torch.float32)
    inv = inversion.NullInversion(model, INV["steps"], INV["guidance"])
    inv.work_size = size
    inv.invert(image.cuda(), "", num_inner_steps=1, early_stop_epsilon=INV["epsilon"])
    assert abs(inv.losses[0][0] - losses[0][0]) > 0.1 * losses[0][0]


def test_invert_frames_under_v_prediction_equals_invert_on_every_frame():
    """Two frames in one batch at work size 64: x_t, embeddings, every loss and the inner-step counts of each frame are the bits of
    invert on that frame alone, one of which stops in mid-loop."""
    size, seeds = 64, (64, 65)
    runs = [single_run(size, seed) for seed in seeds]
    model = nm.NullModel("exact", "cuda", torch.float32)
    model.scheduler.config.prediction_type = V
    inv = inversion.NullInversion(model, INV["steps"], INV["guidance"])
    inv.work_size = size
    images = torch.stack([inversion_image(size, seed) for seed in seeds]).cuda()
    x_t, emb = inv.invert_frames(images, "", num_inner_steps=INV["inner"], early_stop_epsilon=INV["epsilon"])
    assert runs[0][2] == INNER_STEPS
    assert inv.inner_steps_taken == [[run[2][i] for run in runs] for i in range(INV["steps"])]
    for f, (x1, emb1, _, losses1) in enumerate(runs):
        assert same(x_t[f:f + 1], x1), f
        for i in range(INV["steps"]):
            assert same(emb[i][f:f + 1], emb1[i]), (f, i)
            assert inv.losses[i][f] == losses1[i], (f, i)
