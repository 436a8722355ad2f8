#!/usr/bin/env python3
"""Fixture of the attention gradients in float16 and bfloat16: tests/golden/attention_half_grad.npz.

Build-machine only, like tools/make_attention_grad_goldens.py (whose loader, torch_grads and record it uses): imports the
reference's diffusion_utils.py and installs its register_attention_control(model, None) on the toy stack.

  python tools/make_attention_half_grad_goldens.py
Layout (attention_grad.npz's): `meta` = JSON {cases, toy, factor}; a case is one (shape, dtype).  Inputs are seeds
(attention_half_grad_oracle.case_inputs / case_d_out: the float32 streams rounded to the dtype); of every gradient the fixture
holds a seeded sample of at most SAMPLE elements, `<id>/<t>/idx` and `<id>/<t>/ref64` (float64 gradients ON THE ROUNDED INPUTS), and
in meta e_ref[t] = max |grad_half - grad64| over the WHOLE tensor, grad_half being torch autograd on CPU through the reference's
arithmetic (its einsum / softmax / einsum strings, diffusion_utils.py:192-204) in the half dtype for loss = sum(out * d_out).
The toy: per dtype, the reference's own installed forward on the half-rounded weights and inputs in that dtype and in float64;
`toy_<dt>/<t>/idx|ref64` and meta toy[dt].e_ref.  The weights are attention_grad.npz's (rounded by the reader), not stored again.

The script asserts that the restatement in the kernels' arithmetic (grads_kernel) stays within FACTOR x e_ref of float64 for every
case, tensor and dtype, and records its ratio as tile_ratio[t]; where it alone exceeds FACTOR the tests use
max(FACTOR, 2 x tile_ratio[t]) and the script prints the tensor.  With a single key the reference's dq and dk are exactly zero
(e_ref = 0): the restatement is held to attention_half_grad_oracle.single_key_bounds instead.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_grad_oracle as go  # noqa: E402
import attention_half_grad_oracle as hgo  # noqa: E402
import make_attention_grad_goldens as mgg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE = mgg.SAMPLE
FACTOR = 4.0
# heads, batch entries, n, n_k, d
SHAPES = [(2, 4, 70, 70, 40), (2, 4, 70, 77, 40), (3, 4, 9, 9, 160), (5, 2, 100, 100, 80), (2, 1, 64, 64, 64), (1, 1, 33, 1, 8)]


def plan():
    cases, seed = [], 900
    base = dict(mode="self", chunks=1)
    for h, b, n, n_k, d in SHAPES:
        cases.append(dict(base, id=f"hgrad_{h}x{b}x{n}x{n_k}x{d}", kind="value", heads=h, samples=b, n=n, n_k=n_k, d=d, seed=seed))
        seed += 1
    cases.append(dict(base, id="hgrad_sharp_2x4x70x70x40", kind="sharp", heads=2, samples=4, n=70, n_k=70, d=40, seed=seed,
                      gain=mgg.SHARP_GAIN))
    seed += 1
    cases.append(dict(base, id="hgrad_small_2x4x70x77x40", kind="small", heads=2, samples=4, n=70, n_k=77, d=40, seed=seed,
                      d_out_mul=2.0 ** -12))
    return [dict(c, id=c["id"] + "_" + hgo.SHORT[dt], dtype=dt) for c in cases for dt in hgo.DTYPES]


def main():
    ref = mgg.load_ref()
    arrays, cases, over = {}, [], []
    for case in plan():
        tdt = getattr(torch, case["dtype"])
        q, k, v = hgo.case_inputs(case)
        d_out = hgo.case_d_out(case)
        for t in (q, k, v, d_out):   # the numpy rounding is torch's
            assert torch.equal(torch.from_numpy(t), torch.from_numpy(t).to(tdt).float())
        gh = tuple(g.float().numpy() for g in torch_grads_t(case, q, k, v, d_out, tdt))
        assert all(g.dtype == tdt for g in torch_grads_t(case, q, k, v, d_out, tdt))
        g64 = mgg.torch_grads(case, q, k, v, d_out, torch.float64)
        mine = hgo.grads64(case, q, k, v, d_out)
        kern = hgo.grads_kernel(case, q, k, v, d_out)
        case["e_ref"], case["tile_ratio"], case["shape"] = {}, {}, {}
        for j, t in enumerate(("dq", "dk", "dv")):
            assert g64[j].dtype == np.float64
            tol = 1e-12 * max(1.0, np.abs(g64[j]).max())
            assert np.abs(mine[j] - g64[j]).max() <= tol, (case["id"], t, np.abs(mine[j] - g64[j]).max())
            e_ref = float(np.abs(np.asarray(gh[j], np.float64) - g64[j]).max())
            err = float(np.abs(kern[j].astype(np.float64) - g64[j]).max())
            case["e_ref"][t] = e_ref
            case["shape"][t] = list(g64[j].shape)
            if e_ref > 0:
                case["tile_ratio"][t] = err / e_ref
                if err > FACTOR * e_ref:
                    over.append((case["id"], t, err / e_ref))
            else:   # a single key: dq and dk are zero in the reference's arithmetic
                assert case["n_k"] == 1 and t in ("dq", "dk") and np.abs(g64[j]).max() == 0, (case["id"], t)
                bound = hgo.single_key_bounds(case, q, k, v, d_out)[j]
                assert (np.abs(kern[j].astype(np.float64)) <= bound).all(), (case["id"], t)
                case["tile_ratio"][t] = 0.0
            mgg.record(arrays, f"{case['id']}/{t}", g64[j], case["seed"] + 1 + j)
        lse = hgo.lse64(case, q, k)
        assert np.abs(kern[4].astype(np.float64) - lse).max() <= 1e-5 * np.abs(lse).max(), case["id"]
        cases.append(case)

    # the toy stack through the reference's register_attention_control(model, None), per dtype
    grad_fix = np.load(os.path.join(OUT, "attention_grad.npz"))
    weights = json.loads(str(grad_fix["meta"]))["toy"]["weights"]
    toy = dict(go.TOY, weights=weights)
    for dt in hgo.DTYPES:
        state = hgo.toy_state({k_: grad_fix["toy/w/" + k_] for k_ in weights}, dt)
        res = {}
        for name, compute in (("half", getattr(torch, dt)), ("f64", torch.float64)):
            m = go.toy_model(state, compute)
            ref.register_attention_control(m, None)
            res[name] = hgo.toy_grads(m, dt, compute)
        entry = dict(e_ref={}, shape={})
        for j, t in enumerate(("out", "d_context", "d_x")):
            entry["e_ref"][t] = float(np.abs(res["half"][j] - res["f64"][j]).max())
            entry["shape"][t] = list(res["f64"][j].shape)
            mgg.record(arrays, f"toy_{hgo.SHORT[dt]}/{t}", res["f64"][j], go.TOY["seed"] + 20 + j)
        toy[dt] = entry

    meta = dict(cases=cases, toy=toy, factor=FACTOR, sample=SAMPLE, numpy=np.__version__, torch=torch.__version__)
    path = os.path.join(OUT, "attention_half_grad.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("attention_half_grad.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")
    for c in cases:
        for t in ("dq", "dk", "dv"):
            print(f"  {c['id']:34s} {t} e_ref {c['e_ref'][t]:.3e}  kernel-order ratio {c['tile_ratio'][t]:.2f}")
    for dt in hgo.DTYPES:
        for t, e in toy[dt]["e_ref"].items():
            print(f"  toy {dt:9s} {t:10s} e_ref {e:.3e}")
    print("restatement above FACTOR:", over or "none")


def torch_grads_t(case, q, k, v, d_out, dtype):
    """make_attention_grad_goldens.torch_grads in a half dtype (numpy has no bfloat16): the gradients stay torch tensors."""
    tq, tk, tv = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in (q, k, v))
    h = case["heads"]
    sim = torch.einsum("b i d, b j d -> b i j", tq, tk) * (case["d"] ** -0.5)
    attn = sim.softmax(dim=-1)
    out = torch.einsum("b i j, b j d -> b i d", attn, tv)
    bh, n, d = out.shape
    out = out.reshape(bh // h, h, n, d).permute(0, 2, 1, 3).reshape(bh // h, n, h * d)   # reshape_batch_dim_to_heads
    (out * torch.from_numpy(d_out).to(dtype)).sum().backward()
    return tq.grad, tk.grad, tv.grad


if __name__ == "__main__":
    main()
