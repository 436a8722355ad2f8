"""Writes tests/golden/vpred.npz: the v-prediction DDIM step and the null-text loss on it as CPU torch computes them, per dtype
(python tools/make_vpred_goldens.py).

The reference is epsilon-only: these are NOT captures of it.  The expression is tools/vpred_oracle.py's torch_step -- Salimans & Ho
2022 in the operation order of diffusers' DDIMScheduler.step with prediction_type="v_prediction" -- evaluated by CPU torch on
seeded inputs, with the coefficients of comfystereo_amd.schedulers.DDIMScheduler(prediction_type="v_prediction").  The tests
reproduce the file on their CPU bit for bit, check it against the oracle's own per-dtype restatement (step_rounded) and hold the
kernels to it.  Tensors are stored as the unsigned integers of their bits.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpred_oracle as vo   # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "vpred.npz")
DTYPES = ("float32", "float16", "bfloat16")
COUNT, STEPS, TIMESTEPS, GUIDANCES = 263, 10, (900, 500, 0), (7.5, 1.0, 0.0, -2.0)
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def as_bits(t):
    return t.contiguous().view(BITS[t.dtype]).numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


def inputs(dtype):
    """(sample, v_a, v_b, latent_prev): seeded normals with the dtype's special values written over the first elements."""
    g = torch.Generator().manual_seed(20221)
    info = torch.finfo(dtype)
    special = torch.tensor([0.0, -0.0, info.smallest_normal * info.eps, -info.smallest_normal * info.eps, info.max, -info.max,
                            float("nan"), 1.0], dtype=torch.float64)
    out = []
    for k in range(4):
        t = torch.randn(COUNT, generator=g, dtype=torch.float64)
        t[:8] = special.roll(k)
        out.append(t.to(dtype))
    return out


def build():
    from comfystereo_amd import schedulers
    arrays, cases = {}, []
    for name in DTYPES:
        dtype = getattr(torch, name)
        sch = schedulers.DDIMScheduler(prediction_type="v_prediction")
        sch.set_timesteps(STEPS)
        sample, v_a, v_b, prev = inputs(dtype)
        for k, t in enumerate(("sample", "v_a", "v_b", "latent_prev")):
            arrays[f"{name}/{t}"] = as_bits((sample, v_a, v_b, prev)[k])
        for t in TIMESTEPS:
            c = sch.coeffs(t, dtype)
            for gi, g in enumerate(GUIDANCES):
                cid = f"{name}/t{t}/g{gi}"
                arrays[f"{cid}/step"] = as_bits(vo.torch_step(sample, v_a, v_b, g, c))
                cases.append({"id": cid, "dtype": name, "t": t, "guidance": g, "coeffs": list(c)})
            arrays[f"{name}/t{t}/step_single"] = as_bits(vo.torch_step(sample, v_a, None, 1.0, c))
            # the loss on finite inputs (the specials overflow it): elements 8..
            rec, loss, grad = vo.torch_null_loss(v_a[8:], v_b[8:], sample[8:], prev[8:], 7.5, c)
            arrays[f"{name}/t{t}/rec"], arrays[f"{name}/t{t}/grad"] = as_bits(rec), as_bits(grad)
            arrays[f"{name}/t{t}/loss"] = np.array(float(loss), dtype=np.float64)
    arrays["meta"] = np.array(json.dumps({"count": COUNT, "steps": STEPS, "cases": cases,
                                          "source": "restated from Salimans & Ho 2022 and diffusers' operation order; no reference capture"}))
    return arrays


if __name__ == "__main__":
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT))
