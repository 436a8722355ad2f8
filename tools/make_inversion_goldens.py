#!/usr/bin/env python3
"""Fixtures of null-text inversion: tests/golden/inversion_*.npz.

Build-machine only, like tools/make_standard_goldens.py: loads the reference's inversion.py through tools/refload.py and runs
NullInversion itself on the CPU -- its prev_step / next_step and guidance expression, nnf.mse_loss + backward, torch.optim.Adam,
and invert() end to end on the two stand-ins of tools/null_fake_model.py.  Nothing of the reference's arithmetic is replaced;
nnf.mse_loss and ddim_loop are wrapped to look at what passes through them.

  python tools/make_inversion_goldens.py
Files (each below the 1 MiB a committed file may have); `meta` is JSON, bfloat16 arrays are stored as their int16 bit patterns:
  inversion_surface.npz       meta: the reference's signatures (names, parameters, defaults) of NullInversion and EmptyControl
  inversion_step_<dtype>.npz, inversion_step_<dtype>_b.npz  kernel cases (two files for the size limit): inputs are seeded (`case_inputs`), arrays '<id>/out' (the step), '<id>/grad' (loss cases);
                              meta.cases[*]: count, kind, t, guidance, with_b, coeffs, seed, and for loss cases loss (the
                              reference's), ref_err {loss, grad} against tools/inversion_oracle.py
  inversion_adam_<dtype>.npz  '<id>/param|exp_avg|exp_avg_sq@<step>' after steps 1, 2 and 10 of ten consecutive ones (the largest
                              count: the arrays of step 10 only, the errors of all three); meta.cases[*]: count, seed, lr, ref_err {step: {param, exp_avg, exp_avg_sq}}
  inversion_e2e_<form>.npz    invert() on a stand-in, float32: image, ddim/<i>, image_rec, emb/<i>, x_t; meta: losses, inner_steps,
                              epsilon, margin, ref_err {emb, loss, ddim}
  inversion_e2e_exact_<half>.npz  the DDIM latents of a reference run in float16 / bfloat16 on the "exact" stand-in; meta:
                              embeddings_finite, whether the reference's optimisation in that dtype stays finite
Asserted while making them: at least one outer step breaks early and one runs all its inner steps, and every loss the loop compares
lies at least 20 % of its threshold away from it.
"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import inversion_oracle as io_  # noqa: E402
import null_fake_model as nm  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = ("float32", "float16", "bfloat16")
STEP_COUNTS = (1, 63, 140, 16384, 16387, 32768 + 5)   # the last: past one workgroup's share of the loss kernel
ADAM_COUNTS = (1, 77 * 8, 77 * 768 + 5)
STEPS, INNER, GUIDANCE, PROMPT = 5, 10, 7.5, "a photo"
EPSILON = {"exact": 6.4e-3, "attn": 6.4e-3}   # between the losses of the stand-ins: see the margin assertion
MARGIN = 0.2
# (kind, timestep, with eps_b, guidance, a loss case too)
STEP_CASES = (("next", 1, False, 1.0, False), ("prev", 1, True, 7.5, True), ("prev", 401, True, 1.0, True), ("next", 401, False, 1.0, False),
              ("prev", 401, True, 7.5, True))
STEP_FILES = ((0, 1, 2, 3), (4,))   # the cases of inversion_step_<dtype>.npz and of inversion_step_<dtype>_b.npz (the size limit)


def to_np(t):
    import torch
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().copy() if t.dtype == torch.bfloat16 else t.numpy().copy()


def f64(t):
    return t.detach().cpu().double().numpy()


def case_inputs(seed, count, dtype_name, names):
    """The seeded inputs of a kernel case: standard normals (NumPy's default_rng, float64) rounded to the dtype -> torch tensors."""
    import torch
    rng = np.random.default_rng(seed)
    return {n: torch.from_numpy(rng.standard_normal(count)).to(getattr(torch, dtype_name)) for n in names}


def adam_grads(seed, count, dtype_name):
    """Ten gradients; the second has exact zeros in every third element."""
    import torch
    rng = np.random.default_rng(seed)
    out = []
    for k in range(10):
        # no magnitude below 0.025: float16 keeps (1 - beta2) * g * g above zero, so no step divides by a zero second moment
        g = rng.standard_normal(count)
        g = (g + np.copysign(0.05, g)) * 2.0 ** -rng.integers(0, 2)
        if k == 1:
            g[::3] = 0.0
        out.append(torch.from_numpy(g).to(getattr(torch, dtype_name)))
    return out


def signatures(mod):
    out = {}
    for cls in (mod.NullInversion, mod.EmptyControl):
        for name, fn in inspect.getmembers(cls, predicate=inspect.isfunction):
            if name.startswith("_") and name != "__init__" and name != "__call__":
                continue
            out[f"{cls.__name__}.{name}"] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                             for p in inspect.signature(fn).parameters.values()]
        out[f"{cls.__name__}.<properties>"] = sorted(n for n, v in vars(cls).items() if isinstance(v, property))
    return out


def make_steps(torch, mod):
    model = nm.NullModel("exact")
    inv = mod.NullInversion(model, STEPS, GUIDANCE)
    for dtype_name, (suffix, wanted) in ((d, f) for d in DTYPES for f in zip(("", "_b"), STEP_FILES)):
        arrays, cases = {}, []
        for count in STEP_COUNTS:
            for k, (kind, t, with_b, guidance, loss_too) in enumerate(STEP_CASES):
                if k not in wanted:
                    continue
                if count == STEP_COUNTS[-1] and not loss_too:
                    continue
                cid = f"{kind}{t}_{'cfg' if with_b else 'single'}_g{guidance}_n{count}"
                seed = 1000 * k + count
                x = case_inputs(seed, count, dtype_name, ("sample", "eps_a", "eps_b", "noise"))
                e = x["eps_a"] + guidance * (x["eps_b"] - x["eps_a"]) if with_b else x["eps_a"]   # (:88)
                out = (inv.prev_step if kind == "prev" else inv.next_step)(e, t, x["sample"])
                ratio = 1000 // STEPS
                sch = model.scheduler
                if kind == "prev":
                    a_t, a_o = sch.alphas_cumprod[t], sch.alphas_cumprod[t - ratio] if t - ratio >= 0 else sch.final_alpha_cumprod
                else:
                    a_t, a_o = (sch.alphas_cumprod[t - ratio] if t - ratio >= 0 else sch.final_alpha_cumprod), sch.alphas_cumprod[t]
                coeffs = [float((1 - a_t) ** 0.5), float(a_t ** 0.5), float((1 - a_o) ** 0.5), float(a_o ** 0.5)]
                case = dict(id=cid, count=count, kind=kind, t=t, with_b=with_b, guidance=guidance, seed=seed, coeffs=coeffs,
                            final_branch=bool(t - ratio < 0), loss=None)
                arrays[f"{cid}/out"] = to_np(out)
                assert out.dtype == x["sample"].dtype
                if loss_too:
                    # latent_prev: the reconstruction plus a tenth of a normal (a loss around 1e-2); the reference's own lines :198-203
                    latent_prev = (out.double() + 0.1 * x["noise"].double()).to(out.dtype)
                    eu = x["eps_a"].clone().requires_grad_(True)
                    pred = eu + guidance * (x["eps_b"] - eu)
                    rec = inv.prev_step(pred, t, x["sample"])
                    loss = mod.nnf.mse_loss(rec, latent_prev)
                    loss.backward()
                    assert np.array_equal(to_np(rec), arrays[f"{cid}/out"])
                    orec, oloss, ograd = io_.null_loss_grad(f64(x["eps_a"]), f64(x["eps_b"]), f64(x["sample"]), f64(latent_prev),
                                                            guidance, coeffs)
                    arrays[f"{cid}/grad"] = to_np(eu.grad)
                    case["loss"] = float(loss)
                    case["ref_err"] = dict(loss=abs(float(loss) - oloss), grad=io_.err(f64(eu.grad), ograd), rec=io_.err(f64(rec), orec))
                cases.append(case)
        path = os.path.join(GOLDEN, f"inversion_step_{dtype_name}{suffix}.npz")
        np.savez_compressed(path, meta=json.dumps(dict(cases=cases, steps=STEPS)), **arrays)
        print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes", len(cases), "cases")


def make_adam(torch):
    from torch.optim.adam import Adam
    for dtype_name in DTYPES:
        arrays, cases = {}, []
        for count in ADAM_COUNTS:
            seed, lr = 50 + count, 1e-2 * (1. - 3 / 100.)
            p0 = case_inputs(seed, count, dtype_name, ("param",))["param"]
            grads = adam_grads(seed + 1, count, dtype_name)
            want = io_.adam(f64(p0), [f64(g) for g in grads], lr)
            p = p0.clone().requires_grad_(True)
            opt = Adam([p], lr=lr)
            cid, ref_err = f"adam_n{count}", {}
            for k, g in enumerate(grads, 1):
                opt.zero_grad()
                p.grad = g.clone()
                opt.step()
                if k in (1, 2, 10):
                    st = opt.state[p]
                    got = dict(param=p, exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])
                    ref_err[str(k)] = {}
                    for j, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
                        if count != ADAM_COUNTS[-1] or k == 10:   # the largest count: the error of every step, the arrays of the last
                            arrays[f"{cid}/{name}@{k}"] = to_np(got[name])
                        ref_err[str(k)][name] = io_.err(f64(got[name]), want[k - 1][j])
            cases.append(dict(id=cid, count=count, seed=seed, lr=lr, ref_err=ref_err))
        path = os.path.join(GOLDEN, f"inversion_adam_{dtype_name}.npz")
        np.savez_compressed(path, meta=json.dumps(dict(cases=cases)), **arrays)
        print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


def run_reference(torch, mod, form, dtype, epsilon, optimise=True):
    model = nm.NullModel(form, "cpu", dtype)
    inv = mod.NullInversion(model, STEPS, GUIDANCE)
    seen = {"losses": [], "ddim": None}
    real_mse, real_loop = mod.nnf.mse_loss, inv.ddim_loop

    class Functional:
        def __getattr__(self, name):
            return getattr(real_nnf, name)

        @staticmethod
        def mse_loss(a, b):
            out = real_mse(a, b)
            seen["losses"].append(float(out))
            return out

    def loop(latent):
        seen["ddim"] = real_loop(latent)
        return seen["ddim"]

    real_nnf = mod.nnf
    mod.nnf, inv.ddim_loop = Functional(), loop
    try:
        (image, image_rec), x_t, embeddings = inv.invert(nm.seeded_image(11), PROMPT, num_inner_steps=INNER,
                                                         early_stop_epsilon=epsilon, null_text_optimization=optimise)
    finally:
        mod.nnf = real_nnf
    # cut the flat list of losses into outer steps: a step ends at its break or after INNER losses (:206)
    rows, flat, i = [], list(seen["losses"]), 0
    while flat:
        row = []
        while flat and len(row) < INNER:
            row.append(flat.pop(0))
            if row[-1] < epsilon + i * 2e-5:
                break
        rows.append(row)
        i += 1
    return model, inv, seen["ddim"], image_rec, x_t, embeddings, rows


def make_e2e(torch, mod):
    for form in ("exact", "attn"):
        eps = EPSILON[form]
        model, inv, ddim, image_rec, x_t, embeddings, rows = run_reference(torch, mod, form, torch.float32, eps)
        counts = [len(r) for r in rows]
        margin = io_.margins(rows, eps)
        print(form, "inner steps", counts, "margin", margin)
        for r in rows:
            print("   ", " ".join(f"{x:.3e}" for x in r))
        assert len(rows) == STEPS and torch.equal(x_t, ddim[-1])
        assert any(c < INNER for c in counts) and any(c == INNER for c in counts), counts
        assert margin >= MARGIN, margin
        model64 = nm.NullModel(form, "cpu", torch.float64)
        model64.scheduler.set_timesteps(STEPS)
        ctx64 = inv.context.double()
        ddim64 = io_.ddim_loop(model64, ddim[0].double(), ctx64[1:], STEPS)
        emb64, loss64 = io_.null_optimization(model64, [d.double() for d in ddim], ctx64, STEPS, GUIDANCE, INNER, eps)
        assert [len(r) for r in loss64] == counts
        ref_err = dict(emb=max(io_.err(f64(a), f64(b)) for a, b in zip(embeddings, emb64)),
                       loss=max(abs(a - b) for ra, rb in zip(rows, loss64) for a, b in zip(ra, rb)),
                       ddim=max(io_.err(f64(a), f64(b)) for a, b in zip(ddim, ddim64)))
        arrays = {"image": nm.seeded_image(11), "image_rec": image_rec, "x_t": to_np(x_t)}
        for i, d in enumerate(ddim):
            arrays[f"ddim/{i}"] = to_np(d)
        for i, e in enumerate(embeddings):
            arrays[f"emb/{i}"] = to_np(e)
        meta = dict(form=form, steps=STEPS, inner=INNER, guidance=GUIDANCE, prompt=PROMPT, epsilon=eps, losses=rows, inner_steps=counts,
                    margin=margin, ref_err=ref_err, image_seed=11)
        path = os.path.join(GOLDEN, f"inversion_e2e_{form}.npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes", ref_err)
    for dtype_name in ("float16", "bfloat16"):
        # the DDIM latents alone: null_text_optimization off (bfloat16 has no numpy form for the reference's latent2image: its
        # ddim_loop is run directly on its image2latent)
        model = nm.NullModel("exact", "cpu", getattr(torch, dtype_name))
        inv = mod.NullInversion(model, STEPS, GUIDANCE)
        inv.init_prompt(PROMPT)
        ddim = inv.ddim_loop(inv.image2latent(nm.seeded_image(11)))
        arrays = {f"ddim/{i}": to_np(d) for i, d in enumerate(ddim)}
        # the reference's optimisation in the dtype, two inner steps: are its embeddings finite?  (float16 moments underflow)
        embeddings = inv.null_optimization(ddim, 2, EPSILON["exact"])
        finite = bool(all(torch.isfinite(e).all() for e in embeddings))
        print(dtype_name, "embeddings finite:", finite)
        path = os.path.join(GOLDEN, f"inversion_e2e_exact_{dtype_name}.npz")
        np.savez_compressed(path, meta=json.dumps(dict(form="exact", steps=STEPS, prompt=PROMPT, image_seed=11, dtype=dtype_name,
                                                       inner=2, epsilon=EPSILON["exact"], embeddings_finite=finite)), **arrays)
        print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


def main():
    import torch
    import refload
    refload.quiet()
    mod = refload.load_inversion()
    which = sys.argv[1:] or ["surface", "steps", "adam", "e2e"]
    if "surface" in which:
        path = os.path.join(GOLDEN, "inversion_surface.npz")
        np.savez_compressed(path, meta=json.dumps(dict(signatures=signatures(mod), torch=torch.__version__)))
    if "steps" in which:
        make_steps(torch, mod)
    if "adam" in which:
        make_adam(torch)
    if "e2e" in which:
        make_e2e(torch, mod)


if __name__ == "__main__":
    main()
