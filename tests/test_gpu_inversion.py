"""Null-text inversion on the GPU: cs_ddim_step, cs_null_loss_grad and cs_adam_step on every kernel case of
tests/golden/inversion_*.npz, and comfystereo_amd.inversion.NullInversion end to end on the two stand-ins of
tools/null_fake_model.py against the reference's own run.

Bit for bit: the step in every dtype, the reconstructed latent, and the DDIM latents / x_t / image_rec on the "exact" stand-in.
Within a bound: loss, gradient, Adam and what follows from them -- error(ours, float64 restatement) <= max(4 * error(reference,
the same restatement), one ulp of the dtype at the tensor's largest magnitude); the reference's error is the fixture's."""
import numpy as np
import pytest
import torch

import inversion_oracle as io_
import make_inversion_goldens as mk
import null_fake_model as nm
from comfystereo_amd import engine, inversion, stereo_utils
from comfystereo_amd import stereodiffusion_nodes as sdn
from test_inversion_surface import load, load_steps, values
from test_standard_surface import bits, fixture_bits

pytestmark = pytest.mark.gpu
DTYPES = ("float32", "float16", "bfloat16")


def f64(t):
    return t.detach().cpu().double().numpy()


def within(got, want64, ref_err, dtype_name, what):
    e, b = io_.err(f64(got) if isinstance(got, torch.Tensor) else got, want64), io_.bound(ref_err, dtype_name, want64)
    print(what, "error", e, "bound", b, "reference error", ref_err)
    assert e <= b, (what, e, b)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_step_loss_and_gradient_cases(dtype_name):
    z, cases, steps = load_steps(dtype_name)
    dtype = getattr(torch, dtype_name)
    inv = inversion.NullInversion(nm.NullModel("exact"), steps, 7.5)
    for case in cases:
        cid = case["id"]
        x = {k: v.cuda() for k, v in mk.case_inputs(case["seed"], case["count"], dtype_name, ("sample", "eps_a", "eps_b", "noise")).items()}
        coeffs = inv._step_coeffs(case["kind"], case["t"], dtype)
        if dtype_name == "float32":
            assert list(coeffs) == case["coeffs"], cid
        want = fixture_bits(z[f"{cid}/out"])
        eps_b = x["eps_b"] if case["with_b"] else None
        out = engine.ddim_step(x["sample"], x["eps_a"], eps_b, case["guidance"], coeffs)
        assert out.dtype == dtype and np.array_equal(bits(out), want), (cid, int((bits(out) != want).sum()))
        same = x["sample"].clone()
        assert engine.ddim_step(same, x["eps_a"], eps_b, case["guidance"], coeffs, out=same) is same   # in place
        assert np.array_equal(bits(same), want), (cid, "in place")
        if case["loss"] is None:
            continue
        prev = (torch.from_numpy(values(z[f"{cid}/out"], dtype_name)) + 0.1 * x["noise"].cpu().double()).to(dtype).cuda()
        runs = [engine.null_loss_grad(x["eps_a"], x["eps_b"], x["sample"], prev, case["guidance"], coeffs) for _ in range(3)]
        rec, loss, grad = runs[0]
        assert loss.dtype == torch.float32 and loss.shape == () and grad.dtype == dtype
        assert np.array_equal(bits(rec), want), (cid, "rec")
        for r2, l2, g2 in runs[1:]:   # a fixed summation order: the same bits on every launch
            assert np.array_equal(bits(l2.reshape(1)), bits(loss.reshape(1))) and np.array_equal(bits(g2), bits(grad)) and np.array_equal(bits(r2), want)
        _, oloss, ograd = io_.null_loss_grad(f64(x["eps_a"]), f64(x["eps_b"]), f64(x["sample"]), f64(prev), case["guidance"], case["coeffs"])
        within(np.float64(loss.item()), np.float64(oloss), case["ref_err"]["loss"], dtype_name, f"{dtype_name} {cid} loss")
        within(grad, ograd, case["ref_err"]["grad"], dtype_name, f"{dtype_name} {cid} grad")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_adam_cases(dtype_name):
    z, meta = load(f"adam_{dtype_name}")
    for case in meta["cases"]:
        p0 = mk.case_inputs(case["seed"], case["count"], dtype_name, ("param",))["param"]
        grads = mk.adam_grads(case["seed"] + 1, case["count"], dtype_name)
        want = io_.adam(f64(p0), [f64(g) for g in grads], case["lr"])
        p = p0.cuda()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for k, g in enumerate(grads, 1):
            assert engine.adam_step(p, g.cuda(), m, v, case["lr"], k) is p
            if str(k) in case["ref_err"]:
                for j, (name, got) in enumerate((("param", p), ("exp_avg", m), ("exp_avg_sq", v))):
                    within(got, want[k - 1][j], case["ref_err"][str(k)][name], dtype_name, f"{dtype_name} {case['id']} step {k} {name}")


def test_null_text_loss_under_autograd():
    """NullTextLoss as a node of a graph: the gradient reaches what eps_uncond was computed from, scaled by grad_output."""
    z, cases, _ = load_steps("float32")
    case = next(c for c in cases if c["loss"] is not None and c["count"] == 140)
    x = {k: v.cuda() for k, v in mk.case_inputs(case["seed"], 140, "float32", ("sample", "eps_a", "eps_b", "noise")).items()}
    shape = (1, 4, 5, 7)
    prev = (x["sample"] + 0.1 * x["noise"]).reshape(shape)
    w = torch.full(shape, 0.5, device="cuda", requires_grad=True)
    eps_uncond = x["eps_a"].reshape(shape) * w * 2      # = eps_a, through a graph
    loss = engine.NullTextLoss.apply(eps_uncond, x["eps_b"].reshape(shape), x["sample"].reshape(shape), prev, case["guidance"], case["coeffs"])
    assert loss.requires_grad and loss.dtype == torch.float32
    (gw,) = torch.autograd.grad(loss, [w], grad_outputs=torch.tensor(-2.5, device="cuda"))
    _, _, grad = engine.null_loss_grad(x["eps_a"].reshape(shape), x["eps_b"].reshape(shape), x["sample"].reshape(shape), prev,
                                       case["guidance"], case["coeffs"])
    assert torch.equal(gw, (grad * -2.5) * (x["eps_a"].reshape(shape) * 2))
    _, oloss, ograd = io_.null_loss_grad(f64(x["eps_a"]), f64(x["eps_b"]), f64(x["sample"]), f64(prev).ravel(), case["guidance"], case["coeffs"])
    assert abs(loss.item() - oloss) <= 4 * io_.ulp("float32", oloss)
    assert io_.err(f64(grad).ravel(), ograd) <= 4 * io_.ulp("float32", np.abs(ograd).max())


def hooked(model):
    found = [m for m in model.unet.modules() if m.__class__.__name__ == "CrossAttention"]
    return [hasattr(m, stereo_utils._SAVED_FORWARD) for m in found]


@pytest.mark.parametrize("form", ["exact", "attn"])
def test_invert_equals_the_reference(form):
    z, meta = load(f"e2e_{form}")
    model = nm.NullModel(form, "cuda")
    inv = inversion.NullInversion(model, meta["steps"], meta["guidance"])
    image = torch.from_numpy(z["image"]).cuda()
    seen, real_loop = {}, inv.ddim_loop

    def loop(latent):   # invert keeps only the last DDIM latent: look at all of them, computed with the hook installed
        seen["ddim"] = real_loop(latent)
        return seen["ddim"]

    inv.ddim_loop = loop
    try:
        (image_gt, image_rec), x_t, embeddings = inv.invert(image, meta["prompt"], num_inner_steps=meta["inner"],
                                                            early_stop_epsilon=meta["epsilon"])
        assert hooked(model) == ([True] if form == "attn" else [])
    finally:
        stereo_utils.restore_attention(model)
    assert hooked(model) == ([False] if form == "attn" else [])
    assert image_gt is image and len(embeddings) == meta["steps"] and all(e.shape == (1, 77, nm.WIDTH) for e in embeddings)
    assert inv.inner_steps_taken == meta["inner_steps"]          # the breaks fall where the reference's fall
    assert np.array_equal(image_rec, z["image_rec"])
    ddim = seen["ddim"]
    assert len(ddim) == meta["steps"] + 1 and ddim[-1] is x_t
    model64 = nm.NullModel(form, "cpu", torch.float64)
    model64.scheduler.set_timesteps(meta["steps"])
    ctx64 = inv.context.detach().cpu().double()
    ref_ddim = [torch.from_numpy(z[f"ddim/{i}"]) for i in range(meta["steps"] + 1)]
    if form == "exact":
        for i, d in enumerate(ddim):
            assert np.array_equal(bits(d), fixture_bits(z[f"ddim/{i}"])), i
        assert np.array_equal(bits(x_t), fixture_bits(z["x_t"]))
    else:
        ddim64 = io_.ddim_loop(model64, ref_ddim[0].double(), ctx64[1:], meta["steps"])
        assert np.array_equal(bits(ddim[0]), fixture_bits(z["ddim/0"]))
        worst = max(io_.err(f64(a), f64(b)) for a, b in zip(ddim, ddim64))
        b = io_.bound(meta["ref_err"]["ddim"], "float32", np.concatenate([f64(d).ravel() for d in ddim64]))
        print("attn ddim error", worst, "bound", b)
        assert worst <= b
    emb64, loss64 = io_.null_optimization(model64, [d.double() for d in ref_ddim], ctx64, meta["steps"], meta["guidance"],
                                          meta["inner"], meta["epsilon"])
    # The embeddings' bound is loose: Adam steps every element by about lr whatever its gradient's size, so where a gradient is
    # rounding noise its sign decides and the reference itself ends 0.16 ("exact") / 0.058 ("attn") from the float64 run -- more
    # than the optimisation moves an element.  What pins the optimisation is the inner-step counts above and the loss of every
    # inner step below (each follows from all the updates before it); this bound only catches an embedding gone astray.
    worst = max(io_.err(f64(a), f64(b)) for a, b in zip(embeddings, emb64))
    b = io_.bound(meta["ref_err"]["emb"], "float32", np.concatenate([f64(e).ravel() for e in emb64]))
    print(form, "embeddings error", worst, "bound", b)
    assert worst <= b
    # ... and Adam did step: the first update moves every element with a non-zero gradient by lr (|m / sqrt(v)| = 1 after the
    # bias corrections), a second one by at most lr * (1 - beta1) / sqrt(1 - beta2) = 3.2 lr
    moved = io_.err(f64(embeddings[0]), f64(inv.context[:1]))
    print(form, "first outer step moved an element by", moved)
    assert 0.5 * 1e-2 <= moved <= meta["inner_steps"][0] * 3.2 * 1e-2
    worst = max(abs(x - y) for ra, rb in zip(inv.losses, loss64) for x, y in zip(ra, rb))
    b = io_.bound(meta["ref_err"]["loss"], "float32", np.array([x for r in loss64 for x in r]))
    print(form, "loss error", worst, "bound", b)
    assert worst <= b


def test_optimisation_disabled_and_the_standard_mode_around_it():
    z, meta = load("e2e_exact")
    model = nm.NullModel("exact", "cuda")
    inv = inversion.NullInversion(model, meta["steps"], meta["guidance"])
    array = z["image"]   # an array comes back as the array it is, as from the reference
    (image_gt, _), x_t, embeddings = inv.invert(array, meta["prompt"], null_text_optimization=False)
    assert image_gt is array
    (small, _), _, _ = inv.invert(np.ascontiguousarray(array[:40, :56]), meta["prompt"], null_text_optimization=False)
    assert isinstance(small, np.ndarray) and small.shape == (512, 512, 3) and small.dtype == np.uint8   # resized: the resized array
    assert np.array_equal(bits(x_t), fixture_bits(z["x_t"]))
    assert len(embeddings) == meta["steps"] and all(torch.equal(e, inv.context[:1]) and e.data_ptr() != inv.context.data_ptr() for e in embeddings)
    # the whole Standard mode with the inversion in its place, on the stand-in WITH an attention layer: invert installs the
    # fused attention on it and removes it, then the loop installs BNAttention on the same module and removes it
    attn = nm.NullModel("attn", "cuda")
    g = torch.Generator().manual_seed(3)
    image, depth = torch.rand(1, 40, 56, 3, generator=g), torch.rand(1, 40, 56, 3, generator=g)
    seen = []
    make = inversion.make_invert(attn, 5, 7.5, num_inner_steps=2, early_stop_epsilon=6.4e-3)

    def invert(image_u8):
        out = make(image_u8)
        seen.append((hooked(attn), out[0].shape, len(out[1])))
        return out

    stereo, left, right = sdn.generate_stereo_standard(image, depth, 8.0, "uni", False, 5, 7.5, attn, invert)
    assert seen == [([False], (1, 4, 64, 64), 5)]     # the inversion ran, and left no hook for the loop to stack on
    assert hooked(attn) == [False]                    # nor did the loop
    assert stereo.shape == (1, 40, 112, 3) and torch.equal(left, stereo[:, :, :56]) and torch.equal(right, stereo[:, :, 56:])
    assert bool(torch.isfinite(stereo).all())


@pytest.mark.parametrize("dtype_name", ["float16", "bfloat16"])
def test_half_ddim_latents_equal_a_reference_run(dtype_name):
    z, meta = load(f"e2e_exact_{dtype_name}")
    model = nm.NullModel("exact", "cuda", getattr(torch, dtype_name))
    inv = inversion.NullInversion(model, meta["steps"], 7.5)
    image = torch.from_numpy(nm.seeded_image(meta["image_seed"])).cuda()
    (_, image_rec), x_t, embeddings = inv.invert(image, meta["prompt"], num_inner_steps=meta["inner"], early_stop_epsilon=meta["epsilon"])
    with torch.no_grad():
        ddim = inv.ddim_loop(inv.image2latent(image))
    for i, d in enumerate(ddim):
        assert d.dtype == model.dtype and np.array_equal(bits(d), fixture_bits(z[f"ddim/{i}"])), i
    assert np.array_equal(bits(x_t), fixture_bits(z[f"ddim/{meta['steps']}"]))
    # the optimisation ran on the half kernels; its embeddings are finite exactly where the reference's run in the dtype is
    # (float16: (1 - beta2) * g * g underflows to 0 and eps is 0, so Adam divides by zero there as torch.optim.Adam does)
    assert bool(all(torch.isfinite(e).all() for e in embeddings)) == meta["embeddings_finite"]
    assert image_rec.shape == (512, 512, 3) and len(embeddings) == meta["steps"]
    assert all(e.dtype == model.dtype and e.shape == (1, 77, nm.WIDTH) for e in embeddings)
