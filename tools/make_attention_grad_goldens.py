#!/usr/bin/env python3
"""Fixture of the attention gradients: tests/golden/attention_grad.npz.

Build-machine only, like tools/make_attention_goldens.py: imports the reference's diffusion_utils.py (it needs einops) and
installs its register_attention_control(model, None) on the toy stack of tools/attention_grad_oracle.py.

  python tools/make_attention_grad_goldens.py
Layout: `meta` = JSON {cases, toy, factor}; arrays per case id and tensor.  Inputs are seeds (attention_grad_oracle.case_inputs /
case_d_out); of every gradient the fixture holds a seeded sample of at most SAMPLE elements: `<id>/<t>/idx` (flat indices) and
`<id>/<t>/ref64` (float64 values), and in meta e_ref[t] = max |grad32 - grad64| over the WHOLE tensor, where grad32 / grad64 are
torch autograd on CPU through the reference's arithmetic (its einsum / softmax / einsum strings, diffusion_utils.py:192-203) in
float32 / float64 for loss = sum(out * d_out).  For the toy: the reference's own installed forward, MSE loss, the gradients with
respect to the context embedding and the input.

This script also asserts that the float32 restatement in the kernels' tile order (grads_tiled) stays within FACTOR x e_ref of
float64 for every case and tensor -- that the tests' condition can be met at all; a tensor for which it cannot gets its own
ratio recorded as tile_ratio[t] and the tests use max(FACTOR, 2 x tile_ratio[t]) for it.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attention_grad_oracle as go  # noqa: E402
import refload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SAMPLE = 1024
FACTOR = 4.0
SHARP_GAIN = 3.0   # the `gain` of bn_attention.npz's sharp cases (tools/make_attention_goldens.py)
# heads, batch entries, n, n_k, d
SHAPES = [(2, 4, 70, 70, 40), (2, 4, 70, 77, 40), (3, 4, 9, 9, 160), (5, 2, 100, 100, 80), (2, 1, 64, 64, 64), (1, 1, 33, 1, 4)]


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_diffusion_utils", refload.REF + "/diffusion_utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan():
    cases, seed = [], 700
    for h, b, n, n_k, d in SHAPES:
        cases.append(dict(id=f"grad_{h}x{b}x{n}x{n_k}x{d}", kind="value", mode="self", chunks=1, heads=h, samples=b, n=n, n_k=n_k, d=d,
                          seed=seed))
        seed += 1
    cases.append(dict(id="grad_sharp_2x4x70x70x40", kind="sharp", mode="self", chunks=1, heads=2, samples=4, n=70, n_k=70, d=40, seed=seed,
                      gain=SHARP_GAIN))
    return cases


def torch_grads(case, q, k, v, d_out, dtype):
    """autograd through the reference's arithmetic (diffusion_utils.py:192-204) for loss = sum(out * d_out)."""
    tq, tk, tv = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in (q, k, v))
    h = case["heads"]
    sim = torch.einsum("b i d, b j d -> b i j", tq, tk) * (case["d"] ** -0.5)
    attn = sim.softmax(dim=-1)
    out = torch.einsum("b i j, b j d -> b i d", attn, tv)
    bh, n, d = out.shape
    out = out.reshape(bh // h, h, n, d).permute(0, 2, 1, 3).reshape(bh // h, n, h * d)   # reshape_batch_dim_to_heads
    (out * torch.from_numpy(d_out).to(dtype)).sum().backward()
    return tq.grad.numpy(), tk.grad.numpy(), tv.grad.numpy()


def record(arrays, key, g64, seed):
    rs = np.random.RandomState(seed)
    idx = np.sort(rs.choice(g64.size, min(g64.size, SAMPLE), replace=False)).astype(np.int32)
    arrays[key + "/idx"] = idx
    arrays[key + "/ref64"] = g64.reshape(-1)[idx]


def main():
    ref = load_ref()
    arrays, cases = {}, []
    for case in plan():
        q, k, v = go.case_inputs(case)
        d_out = go.case_d_out(case)
        scale = case["d"] ** -0.5
        g32 = torch_grads(case, q, k, v, d_out, torch.float32)
        g64 = torch_grads(case, q, k, v, d_out, torch.float64)
        mine = go.grads(q, k, v, d_out, case["heads"], scale)
        tiled = go.grads_tiled(q, k, v, d_out, case["heads"], scale)
        case["e_ref"], case["tile_ratio"], case["shape"] = {}, {}, {}
        for j, t in enumerate(("dq", "dk", "dv")):
            assert g32[j].dtype == np.float32 and g64[j].dtype == np.float64
            tol = 1e-12 * max(1.0, np.abs(g64[j]).max())
            assert np.abs(mine[j] - g64[j]).max() <= tol, (case["id"], t, np.abs(mine[j] - g64[j]).max())
            e_ref = float(np.abs(g32[j].astype(np.float64) - g64[j]).max())
            err = float(np.abs(tiled[j].astype(np.float64) - g64[j]).max())
            case["e_ref"][t] = e_ref
            case["shape"][t] = list(g64[j].shape)
            # (a single key: softmax = 1, dq and dk are exactly zero in every arithmetic; the restatement must agree)
            assert e_ref > 0 or err == 0, (case["id"], t, err)
            case["tile_ratio"][t] = err / e_ref if e_ref > 0 else 0.0
            assert case["tile_ratio"][t] <= FACTOR, (case["id"], t, case["tile_ratio"][t])
            record(arrays, f"{case['id']}/{t}", g64[j], case["seed"] + 1 + j)
        lse_err = np.abs(tiled[4].astype(np.float64) - go.lse2(q, k, scale)).max()
        assert lse_err <= 1e-5 * np.abs(go.lse2(q, k, scale)).max(), (case["id"], lse_err)
        cases.append(case)

    # the toy stack through the reference's register_attention_control(model, None)
    net = go.toy_model()
    state = {k_: v_.numpy().copy() for k_, v_ in net.state_dict().items()}
    for k_, a in state.items():
        arrays["toy/w/" + k_] = a
    res = {}
    for name, dtype in (("f32", None), ("f64", torch.float64)):
        m = go.toy_model(state, dtype)
        ref.register_attention_control(m, None)
        res[name] = go.toy_grads(m, dtype=dtype)
    toy = dict(go.TOY, weights=sorted(state), e_ref={}, shape={})
    for j, t in enumerate(("out", "d_context", "d_x")):
        g32, g64 = res["f32"][j], res["f64"][j]
        assert g32.dtype == np.float32 and g64.dtype == np.float64
        toy["e_ref"][t] = float(np.abs(g32.astype(np.float64) - g64).max())
        toy["shape"][t] = list(g64.shape)
        record(arrays, "toy/" + t, g64, go.TOY["seed"] + 10 + j)
    # the module's own forward computes the same thing: what restore_attention brings back
    own = go.toy_grads(go.toy_model(state, torch.float64), dtype=torch.float64)
    assert np.abs(own[0] - res["f64"][0]).max() <= 1e-12

    meta = dict(cases=cases, toy=toy, factor=FACTOR, sample=SAMPLE, numpy=np.__version__, torch=torch.__version__)
    path = os.path.join(OUT, "attention_grad.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("attention_grad.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")
    worst = 0.0
    for c in cases:
        for t in ("dq", "dk", "dv"):
            print(f"  {c['id']:28s} {t} e_ref {c['e_ref'][t]:.3e}  tile-order ratio {c['tile_ratio'][t]:.2f}")
            worst = max(worst, c["tile_ratio"][t])
    for t in toy["e_ref"]:
        print(f"  toy {t:10s} e_ref {toy['e_ref'][t]:.3e}")
    print("worst tile-order ratio", worst, "(FACTOR", FACTOR, ")")


if __name__ == "__main__":
    main()
